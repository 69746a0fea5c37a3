// Static execution plan ("tape") of the SDXL UNet training step.
//
// Engine  = configuration + packed parameters (bf16 weight arena, fp32 gradient arena) shared by all plans.
// Plan    = one bucket shape (B, H, W): every activation, gradient, statistic and scratch buffer has a fixed
//           offset in one workspace arena, every op holds resolved offsets, and forward / backward are plain
//           in-order / reverse-order walks that only launch kernels (no allocation, no host sync, no autograd).
// Gradient buffers are assigned while walking the tape in reverse: the first writer of a tensor's gradient
// overwrites, later writers accumulate, and a residual connection's gradient is an alias of its output's.
#pragma once
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/sdxlstep.h"
#include "../../include/sdxlstep_diag.h"
#include "kernels.h"

static const size_t NONE = (size_t)-1;

struct Act {           // bf16 activation [rows][cols] in the workspace
  size_t off = NONE;   // byte offset of data
  size_t goff = NONE;  // byte offset of gradient (assigned in reverse planning)
  long rows = 0;
  int cols = 0;
  int pad_rows = 0;    // rows allocated beyond `rows` in the data and the gradient buffer (a weight-gradient GEMM over the rows can
                       // then run a whole number of 64-row reduction steps: the op zeroes them before it reads them)
  bool need_grad = true;
  // column-slice view of a wider tensor (one block's K | V columns of the grouped cross-attention projection):
  // data / gradient live inside the parent's buffers, row stride = the parent's width
  Act* parent = nullptr;
  int col0 = 0;
  long ld() const { return parent ? parent->cols : cols; }
};

struct PRef {  // native parameter: element offset into the bf16 weight arena and the fp32 grad arena
  size_t off = NONE;
  size_t numel = 0;
};

struct SrcParam {  // one diffusers state-dict tensor and where it lives in the native arena
  std::string name;
  int ndim;
  long shape[4];
  PRef native;
  int kind;  // 0: rows copied at elem_off ; 1: conv3x3 [co][ci][3][3] -> [co][9][ci_pad]
  size_t elem_off;
  int ci_pad;
};

struct Engine;
struct Plan;

// The additional skip residuals of one micro-step (sdxl_residuals): a copy of the caller's host arrays, taken at the forward call and kept
// (StepState) for that micro-step's backward.  Index = the skip in forward order; a null entry = nothing at that skip.
struct ResidualReq {
  bool present = false;      // the call carried a sdxl_residuals: its forward and backward launch kernel by kernel, also in graph mode
  int dtype = 0;             // of down / mid: 0 fp32, 1 bf16
  std::vector<const void*> down;
  const void* mid = nullptr;
  std::vector<float*> d_down;
  float* d_mid = nullptr;
  bool wants_grads() const {
    if (d_mid) return true;
    for (float* d : d_down) if (d) return true;
    return false;
  }
};

struct Op {
  int seg = 0;
  bool hoist_fwd = false;   // forward depends on the inputs only (cross-attention K/V projections of the prompt
                            // embeddings): launched on the side stream at the start of the forward
  bool needs_hoisted = false;  // consumes a hoisted op's output: main stream waits for the side stream first
  virtual ~Op() {}
  virtual int fwd(Plan& p, hipStream_t st) = 0;
  virtual void plan_bwd(Plan& p) = 0;
  virtual int bwd(Plan& p, hipStream_t st, bool first_micro) = 0;
  // the plan map (sdxl_debug_plan_op): what this op reads and writes, from the fields it already holds; launches nothing.  `d` arrives cleared
  // (every offset NONE, every tensor role absent) with seg / hoist_fwd filled in.
  virtual void describe(const Plan& p, sdxl_plan_op_desc* d) const = 0;
};

struct Plan {
  Engine* eng = nullptr;
  int B = 0, H = 0, W = 0, ctx = 0;
  size_t ws_bytes = 0;   // bytes needed
  size_t cursor = 0;
  std::vector<std::unique_ptr<Act>> acts;
  std::vector<std::unique_ptr<Op>> ops;
  std::vector<int> seg_first_op, seg_last_op;  // op index ranges per segment (forward order)
  size_t tp32_off = NONE, tp32_bytes = 0;   // fp32 [B][sum Cout] time-embedding-projection gradient (zeroed at the start of a backward;
                                            // every resnet's conv1 backward adds its per-sample column sums into its slice)
  // well-known buffers
  Act *x_in = nullptr, *pred = nullptr, *ehs = nullptr, *aug_in = nullptr, *te_sin = nullptr, *tid_emb = nullptr;
  size_t t_off = NONE, tid_off = NONE, loss_off = NONE, loss_part_off = NONE;
  size_t in_lat_off = NONE, in_noise_off = NONE, in_sig_off = NONE, in_tag_off = NONE;   // staged copies of the step's inputs (fixed
                                                                                          // addresses for the captured graphs)
  size_t in_sw_off = NONE, in_hc_off = NONE;   // ... of the optional per-sample weights and per-sample Huber c ([B] each)
  size_t ps_loss_off = NONE;                   // [B] per-sample losses, copied to the caller's pointer after the loss kernels
  size_t in_mask_off = NONE, in_nin_off = NONE; // staged copies of the optional loss mask [B*H*W] and input noise [B*4*H*W]
  size_t in_cond_off = NONE;                   // staged copy of the extra input channels [B][in_channels - 4][H*W] (in_channels > 4 only)
  size_t mask_norm_off = NONE;                 // [B] masked_mean normaliser M_b: loss_finalize_kernel -> loss_bwd_kernel
  size_t samp_part_off = NONE;                 // sampler_part_floats(B, HW): the guidance-rescale partial sums of a sampler step
  size_t gn_ws_off = NONE, gn_ws_floats = 0;  // GroupNorm scratch shared by all (stream-ordered) norm ops
  size_t slab_off = NONE, slab_floats = 0;    // split-K partial slabs of the wgrad GEMMs (shared, stream-ordered)
  size_t slab_main_off = NONE, slab_main_floats = 0;   // the same for split forward / dgrad launches (caller's stream)
  size_t apart_off = NONE, apart_floats = 0;  // query-split partials of the self-attention dK / dV kernel (caller's stream)
  size_t apart_side_off = NONE, apart_side_floats = 0;   // ... of the cross-attention dK / dV kernel (side stream): never shared
  // LayerNorm backward inside the dgrad epilogue of the linear layer its output feeds (GemmP::ln_x): the tagged per-row partial sums the
  // column tiles of a row block exchange; shared, stream-ordered; zeroed at the start of a backward, whose fused launches count the epoch up
  size_t ln_part_off = NONE, ln_part_floats = 0;
  int ln_epoch = 0;
  // conditioning gradients (cond_dgrad.hip): d ehs = sum over the K | V projections of dKV . Wkv, d pooled = dA1 . W_add1[:, :pooled_dim], fp32.
  // Buffers and slab are always reserved (behind every other allocation); the kernels run only in a backward whose micro-step asked
  // (Engine::cond_ehs / cond_pool), at the end of the last segment, on the caller's stream, behind the join with the side stream.
  struct CondSrc { size_t dy_off = NONE; long lda = 0; PRef w; long ldb = 0; int K = 0; };
  CondSrc cond_kv[2], cond_add;        // the hoisted K | V projections in forward order (at most one per attention width); add_embedding.linear_1
  int cond_nkv = 0;
  CondSrc din_src;                     // conv_in's output gradient and weight, the operands of the input gradient (K = its output width); recorded by its plan_bwd
  size_t dehs_off = NONE, dpool_off = NONE, cond_slab_off = NONE;
  // direct adapter gradients (lora_grad.hip, Engine::lora): scratch of the widest targeted op, shared and stream-ordered (every launch
  // is on the side stream, or all on the caller's); nothing is reserved -- no offset of the plan moves -- without adapters
  size_t lg_tu_elems = 0, lg_part_floats = 0, lg_tu_off = NONE, lg_part_off = NONE;

  Act* new_act(long rows, int cols, bool need_grad = true, int pad_rows = 0);
  Act* view(Act* parent, int col0, int cols);   // columns [col0, col0 + cols) of parent
  size_t alloc(size_t bytes);
  // reverse planning.  Gradient buffers are WRITE-ONCE: the first writer of a tensor's gradient gets a fresh buffer,
  // every later writer gets another fresh buffer plus the previous one as addend (out = addend + contribution), so a
  // buffer is never modified after it has been produced -- deferred / concurrent readers (the wgrad GEMMs on the
  // side stream) need no ordering against later accumulations.
  struct GradDst { size_t out = NONE, addend = NONE; };
  GradDst grad_dst(Act* a);
  bool grad_alias(Act* x, Act* y);  // x.g := y.g when x has none yet (residual pass-through, no copy)
  bf16* GP(size_t off) const;       // workspace pointer of a gradient offset (nullptr for NONE)
  template <class T, class... A>
  T* add(A&&... a);
  // pointers (valid once a workspace is bound)
  bf16* P(const Act* a) const;
  bf16* G(const Act* a) const;
  float* F(size_t off) const;
};

struct Engine {
  sdxl_unet_config cfg;
  int device = 0;
  // parameters
  std::vector<PRef> natives;  // in creation (= forward) order
  std::vector<SrcParam> src;
  std::map<std::string, int> src_index;
  size_t param_elems = 0;
  bf16* weights = nullptr;
  float* grads = nullptr;
  bool own_weights = false, own_grads = false;
  // segments: contiguous native-parameter ranges (forward order)
  int nseg = 1;
  std::vector<size_t> seg_begin, seg_end;
  // plans
  std::map<std::tuple<int, int, int, int>, std::unique_ptr<Plan>> plans;
  Plan* cur = nullptr;
  char* ws = nullptr;
  size_t ws_cap = 0;
  bool own_ws = false;
  // backward concurrency: weight-gradient GEMMs (and bias column sums) run on a side stream, off the dgrad chain
  hipStream_t side = nullptr;
  hipEvent_t ev_join = nullptr, ev_hoist = nullptr;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  bool use_side = true;
  bf16* emit_base = nullptr;     // sdxl_set_grad_emit: weight-gradient GEMMs write their final value as bf16 into this arena (same
  float emit_scale = 1.f;        // element offsets as `grads`) instead of the fp32 arena -- the exchange micro-step under data parallelism
  bool join_last_only = false;   // sdxl_set_join_mode 1 / 2: main waits for the side stream at the last segment only
  bool seg_on_side = false;      // sdxl_set_join_mode 2: at every segment end the SIDE stream waits for main instead; the caller
                                 // enqueues the segment's cast + collective on the side stream (sdxl_side_stream)
  hipEvent_t ev_seg = nullptr;
  hipEvent_t next_event();
  std::vector<std::vector<GemmP>> wg_pending;   // weight gradients waiting for a grouped launch, one bucket per shape
  int defer_wgrad(Plan& p, hipStream_t main, const GemmP& g, int grp);
  int flush_wgrads(Plan& p, hipStream_t main);
  // leaf launches for the side stream that may start any time after the point they were queued at (their inputs are write-once
  // buffers produced by launches already enqueued on the caller's stream): they ride on the NEXT fork event instead of paying for
  // one of their own (LayerNorm parameter gradients, cross-attention dK / dV: 280 events per step)
  std::vector<std::function<int(hipStream_t)>> side_leaves;
  std::vector<LnRedEntry> ln_pending;     // LayerNorm backward launches whose dgamma | dbeta partials are not reduced yet
  std::vector<LnRedEntry> cs_pending;     // per-sample column sums (time-embedding row vectors) whose partial rows are not reduced yet: the consumer's cast flushes them
  int flush_ln_params(Plan& p, hipStream_t main);
  // Everything queued for a later launch holds raw workspace pointers of the plan and step it was queued in: dropped at the start of a
  // forward / of a backward, when a backward segment fails half way, and when the current plan changes (never launched against another
  // step's or plan's buffers).
  void drop_pending() { side_leaves.clear(); wg_pending.clear(); ln_pending.clear(); cs_pending.clear(); }
  bool side_dirty = false;       // the side stream has work the caller's stream has not joined yet
  bool cond_ehs = false, cond_pool = false;   // this micro-step's backward also produces d prompt_embeds / d pooled (set by the C ABI)
  bool cond_gated = false;                    // ... behind a loss (its gate scalar is read), not behind sdxl_unet_backward
  int launch_cond_grads(Plan& p, hipStream_t st);
  // additional skip residuals (residual.hip), consulted by ConcatOp: res_fwd is set by the C ABI for the duration of a forward that carries
  // them (the backward never reads the residuals), res_bwd before a backward whose micro-step asked for their gradients; res_gated as cond_gated
  const ResidualReq* res_fwd = nullptr;
  const ResidualReq* res_bwd = nullptr;
  bool res_gated = false;
  int num_skips() const { return 3 * cfg.layers_per_block + 3; }
  // input gradient (input_dgrad.hip), consulted by the ConvOp that reads the plan's x_in (conv_in): the caller's fp32 [B, in_channels, H, W]
  // buffer of the micro-step whose backward runs (sdxl_batch_din), set by the C ABI beside res_bwd; null = none; din_gated as cond_gated
  float* din = nullptr;
  bool din_gated = false;
  // Gradient selection (SDXL_DTYPE_GRAD_SELECT of sdxl_export_grad, OFF after sdxl_create): one flag per state-dict tensor, 1 = the backward
  // produces its gradient.  A native parameter is frozen when EVERY tensor that maps into it is (fused q | k | v, the grouped K | V and
  // time-embedding projections: a tensor is a row range of the native weight), and an op skips its weight-gradient work -- the launch with
  // its bias column sums, the zero-row memsets in front of it, the norm-parameter reduce -- when every native parameter it owns is frozen:
  // nothing is written into the fp32 arena or the emit arena for it.  The dgrad side never looks at the selection.  Read at launch time
  // (it holds for every plan); a change drops the captured graphs.
  // Adapters whose gradients the backward writes itself (sdxl_grad_select.lora): the targets of one LinearOp, keyed by its weight's arena
  // offset; that op launches lora_grad.hip's kernels in place of its weight gradient.  Plans reserve the scratch in plan_bwd, so the
  // plans are dropped when this changes.
  struct LoraOpSel { std::vector<LoraGradTarget> host; const LoraGradTarget* dev = nullptr; int tiles = 0, reds = 0; size_t part_unit = 0; };
  struct LoraSel {
    std::vector<int> params;
    int rank = 0; float scale = 0.f;
    const bf16* adapters = nullptr; float* grads = nullptr;
    std::map<size_t, LoraOpSel> ops;
    LoraGradTarget* dev = nullptr;           // one device table, the ops' targets back to back
  } lora;
  const LoraOpSel* lora_op(PRef w) const {
    if (lora.ops.empty()) return nullptr;
    auto it = lora.ops.find(w.off);
    return it == lora.ops.end() ? nullptr : &it->second;
  }
  std::vector<unsigned char> trainable;      // [src.size()], empty = every tensor trainable
  std::set<size_t> frozen_offs;              // PRef::off of the frozen native parameters (empty without a selection: one test per op)
  void set_trainable(const unsigned char* flags);      // nullptr = all trainable
  bool frozen(PRef a, PRef b) const {        // an op owning a (and b, unless NONE): skip its parameter gradients?
    if (frozen_offs.empty()) return false;
    return (a.off == NONE || frozen_offs.count(a.off)) && (b.off == NONE || frozen_offs.count(b.off));
  }
  // hipGraph replay of the step (sdxl_set_graph_mode, OFF by default): forward (+ loss) and backward are captured once per
  // (plan, configuration) -- both streams, every event edge -- and replayed with one hipGraphLaunch, on an engine-owned
  // stream (the caller's may be the legacy default stream, which cannot be captured) fenced by two events.  Measured on
  // ROCm 7.2 / MI355X (r02, same box): B=4 1024^2 eager 124.1 ms/step, forward graph only 124.6, backward graph 142.8, both
  // 143.9; B=1 512^2 (3,400 launches in 61 ms) eager 61.5, forward only 62.5, both 67.5 -- the runtime replays a
  // two-branch graph with LESS overlap between the branches than two streams give, and no cheaper per kernel.  Kept as an
  // opt-in for runtimes where that changes; the step's gaps are the dispatcher's, not this host loop's.
  bool use_graphs = false;
  hipStream_t gstream = nullptr;
  hipEvent_t ev_gin = nullptr, ev_gout = nullptr;
  struct GraphKey {
    const void* plan; int kind, k, first, join; unsigned scale_bits, cfg;
    unsigned cfg2, huber_bits;      // element loss + which per-sample arrays are present; the scalar huber_c (capi.hip: loss_cfg_bits2)
    bool operator<(const GraphKey& o) const {
      return std::tie(plan, kind, k, first, join, scale_bits, cfg, cfg2, huber_bits) <
             std::tie(o.plan, o.kind, o.k, o.first, o.join, o.scale_bits, o.cfg, o.cfg2, o.huber_bits);
    }
  };
  struct GraphEntry { hipGraphExec_t exec = nullptr; int seen = 0; };
  std::map<GraphKey, GraphEntry> graphs;
  void clear_graphs() {
    for (auto& kv : graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    graphs.clear();
  }
  // builder state
  bool registering = true;
  size_t native_cursor = 0;
  Plan* bp = nullptr;  // plan being built (nullptr while registering parameters)

  PRef param(size_t numel, bool small = false);   // small: bias / norm vectors, accumulated with atomics -> zeroed per cycle
  std::vector<std::pair<size_t, size_t>> small_ranges;   // (elem offset, elems) of the small parameters
  unsigned long long* small_ranges_dev = nullptr;         // same list on the device (pairs), for the zeroing kernel
  void map_src(const std::string& name, std::vector<long> shape, PRef p, int kind, size_t elem_off, int ci_pad);
  int seg_of(size_t elem_off) const;
  void build(Plan* plan);  // registers parameters (plan == nullptr) or builds a plan
  bf16* Wp(PRef p) const { return weights + p.off; }
  float* Gp(PRef p) const { return grads + p.off; }
};

inline bf16* Plan::P(const Act* a) const { return (bf16*)(eng->ws + a->off); }
inline bf16* Plan::G(const Act* a) const { return a->goff == NONE ? nullptr : (bf16*)(eng->ws + a->goff); }
inline float* Plan::F(size_t off) const { return (float*)(eng->ws + off); }
inline bf16* Plan::GP(size_t off) const { return off == NONE ? nullptr : (bf16*)(eng->ws + off); }
template <class T, class... A>
T* Plan::add(A&&... a) {
  T* o = new T(std::forward<A>(a)...);
  ops.emplace_back(o);
  return o;
}

void plan_describe_tensor(sdxl_plan_tensor& t, const Act* a);      // the plan map's view of one activation (a == nullptr: absent)
int engine_load_weight(Engine& e, const char* name, const void* src, int dtype, hipStream_t st);
int engine_export(Engine& e, const char* name, void* dst, int dtype, bool grad, hipStream_t st);
int probe_layout(void* out, hipStream_t st);
