// extern "C" surface of libsdxlstep (see include/sdxlstep.h for the contract of every entry point).
#include "capi.h"
#include <functional>
#include <mutex>

extern "C" {

const char* sdxl_last_error(void) { return sdxl_get_error(); }
int sdxl_version(void) { return 1; }

int sdxl_default_config(sdxl_unet_config* c) {
  ARG_CHECK(c, "null config");
  c->in_channels = 4; c->out_channels = 4;
  c->block_out_channels[0] = 320; c->block_out_channels[1] = 640; c->block_out_channels[2] = 1280;
  c->layers_per_block = 2;
  c->transformer_layers[0] = 0; c->transformer_layers[1] = 2; c->transformer_layers[2] = 10;
  c->head_dim = 64; c->cross_attention_dim = 2048; c->norm_num_groups = 32;
  c->addition_time_embed_dim = 256; c->pooled_dim = 1280;
  c->resnet_eps = 1e-5f; c->tf_gn_eps = 1e-6f; c->ln_eps = 1e-5f;
  return 0;
}

int sdxl_create(const sdxl_unet_config* cfg, int device, sdxl_handle** out) {
  ARG_CHECK(cfg && out, "null argument");
  ARG_CHECK(cfg->head_dim == 64, "head_dim must be 64 (got %d)", cfg->head_dim);
  ARG_CHECK(cfg->in_channels >= 4 && cfg->in_channels <= 16, "in_channels must be 4 .. 16 (got %d)", cfg->in_channels);
  ARG_CHECK(cfg->out_channels == 4, "out_channels must be 4 (got %d)", cfg->out_channels);
  ARG_CHECK(cfg->transformer_layers[0] == 0, "level 0 must not have attention");
  for (int i = 0; i < 3; ++i) {
    int c = cfg->block_out_channels[i];
    ARG_CHECK(c % cfg->norm_num_groups == 0 && c % 8 == 0, "block_out_channels[%d]=%d unsupported", i, c);
    if (cfg->transformer_layers[i] > 0) ARG_CHECK(c % 128 == 0, "attention level width %d must be a multiple of 128", c);
  }
  ARG_CHECK(cfg->cross_attention_dim % 8 == 0 && cfg->pooled_dim % 8 == 0 && cfg->addition_time_embed_dim % 8 == 0,
            "conditioning widths must be multiples of 8");
  int ndev = 0;
  HIP_CHECK_RET(hipGetDeviceCount(&ndev));
  ARG_CHECK(device >= 0 && device < ndev, "device %d out of range (have %d)", device, ndev);
  HIP_CHECK_RET(hipSetDevice(device));
  sdxl_handle* h = new sdxl_handle();
  h->e.cfg = *cfg;
  h->e.device = device;
  h->e.build(nullptr);
  const char* ns = getenv("SDXL_NO_SIDE_STREAM");     // measurement mode: everything on the caller's stream (clean per-kernel
  h->e.use_side = !(ns && ns[0] == '1');              // durations for the serialized rocprof summaries under profiles/)
  if (h->e.use_side) {
    if (const char* sp = getenv("SDXL_SIDE_PRIO")) {   // measurement only: queue priority of the side stream (1 low, 0 normal, -1 high)
      HIP_CHECK_RET(hipStreamCreateWithPriority(&h->e.side, hipStreamNonBlocking, atoi(sp)));
    } else
    HIP_CHECK_RET(hipStreamCreateWithFlags(&h->e.side, hipStreamNonBlocking));   // (stream priorities: measured, neutral)
    HIP_CHECK_RET(hipStreamCreateWithFlags(&h->e.gstream, hipStreamNonBlocking));
    HIP_CHECK_RET(hipEventCreateWithFlags(&h->e.ev_gin, hipEventDisableTiming));
    HIP_CHECK_RET(hipEventCreateWithFlags(&h->e.ev_gout, hipEventDisableTiming));
    HIP_CHECK_RET(hipEventCreateWithFlags(&h->e.ev_join, hipEventDisableTiming | hipEventDisableSystemFence));
    HIP_CHECK_RET(hipEventCreateWithFlags(&h->e.ev_seg, hipEventDisableTiming | hipEventDisableSystemFence));
    HIP_CHECK_RET(hipEventCreateWithFlags(&h->e.ev_hoist, hipEventDisableTiming | hipEventDisableSystemFence));
  }
  *out = h;
  return 0;
}

int sdxl_destroy(sdxl_handle* h) {
  if (!h) return 0;
  if (h->e.own_weights && h->e.weights) (void)hipFree(h->e.weights);
  if (h->e.own_grads && h->e.grads) (void)hipFree(h->e.grads);
  if (h->e.own_ws && h->e.ws) (void)hipFree(h->e.ws);
  h->e.clear_graphs();
  if (h->e.gstream) (void)hipStreamDestroy(h->e.gstream);
  if (h->e.ev_gin) (void)hipEventDestroy(h->e.ev_gin);
  if (h->e.ev_gout) (void)hipEventDestroy(h->e.ev_gout);
  for (hipEvent_t ev : h->e.ev_pool) (void)hipEventDestroy(ev);
  if (h->e.ev_join) (void)hipEventDestroy(h->e.ev_join);
  if (h->e.ev_seg) (void)hipEventDestroy(h->e.ev_seg);
  if (h->e.ev_hoist) (void)hipEventDestroy(h->e.ev_hoist);
  if (h->e.side) (void)hipStreamDestroy(h->e.side);
  if (h->e.small_ranges_dev) (void)hipFree(h->e.small_ranges_dev);
  lora_cache_free(h->lora);
  if (h->e.lora.dev) (void)hipFree(h->e.lora.dev);
  delete h;
  return 0;
}

int sdxl_param_bytes(sdxl_handle* h, size_t* wb, size_t* gb) {
  H_CHECK(h);
  if (wb) *wb = h->e.param_elems * sizeof(bf16);
  if (gb) *gb = h->e.param_elems * sizeof(float);
  return 0;
}

int sdxl_bind_params(sdxl_handle* h, void* w, void* g) {
  H_CHECK(h);
  Engine& e = h->e;
  e.clear_graphs();                                   // captured kernels hold the old arena addresses
  if (w) { e.weights = (bf16*)w; e.own_weights = false; }
  else {
    HIP_CHECK_RET(hipMalloc((void**)&e.weights, e.param_elems * sizeof(bf16)));
    HIP_CHECK_RET(hipMemset(e.weights, 0, e.param_elems * sizeof(bf16)));
    e.own_weights = true;
  }
  if (g) { e.grads = (float*)g; e.own_grads = false; }
  else {
    HIP_CHECK_RET(hipMalloc((void**)&e.grads, e.param_elems * sizeof(float)));
    HIP_CHECK_RET(hipMemset(e.grads, 0, e.param_elems * sizeof(float)));
    e.own_grads = true;
  }
  ARG_CHECK(((uintptr_t)e.weights & 255) == 0 && ((uintptr_t)e.grads & 255) == 0, "arenas must be 256-byte aligned");
  return 0;
}

int sdxl_num_params(sdxl_handle* h) { return h ? (int)h->e.src.size() : -1; }

int sdxl_param_info(sdxl_handle* h, int i, char* name, int cap, int* ndim, long shape[4]) {
  H_CHECK(h);
  ARG_CHECK(i >= 0 && i < (int)h->e.src.size(), "parameter index %d out of range", i);
  const SrcParam& s = h->e.src[i];
  if (name && cap > 0) snprintf(name, cap, "%s", s.name.c_str());
  if (ndim) *ndim = s.ndim;
  if (shape) for (int k = 0; k < 4; ++k) shape[k] = s.shape[k];
  return 0;
}

int sdxl_param_range(sdxl_handle* h, int i, size_t* elem_off, size_t* elems) {
  H_CHECK(h);
  ARG_CHECK(i >= 0 && i < (int)h->e.src.size(), "parameter index %d out of range", i);
  const SrcParam& s = h->e.src[i];
  size_t n = 1;
  for (int k = 0; k < s.ndim; ++k) n *= (size_t)s.shape[k];
  if (s.kind == 1) n = (size_t)s.shape[0] * 9 * (size_t)s.ci_pad;   // conv: [cout][tap][cin padded]
  if (elem_off) *elem_off = s.native.off + s.elem_off;
  if (elems) *elems = n;
  return 0;
}

// ---- LoRA by merge and project (SDXL_DTYPE_LORA): checks, the cached device table, the launches of csrc/lora.hip ----
// the checks every user of a sdxl_lora_op shares (merge, project, the backward's own adapter gradients), before anything is launched
static int lora_check_op(const sdxl_lora_op* op, bool need_base, bool need_grads) {
  ARG_CHECK(op && op->n >= 1 && op->param, "lora: empty target list");
  ARG_CHECK(op->rank >= 1 && op->rank <= 128, "lora: rank %d outside 1 .. 128", op->rank);
  ARG_CHECK(isfinite(op->scale), "lora: scale is not finite");
  ARG_CHECK(aligned16(op->adapters), "lora: adapters must be a 16-byte aligned device pointer");
  if (need_base) ARG_CHECK(aligned16(op->base), "lora: base must be a 16-byte aligned device pointer");
  if (need_grads) ARG_CHECK(aligned16(op->adapter_grads), "lora: adapter_grads must be a 16-byte aligned device pointer");
  return 0;
}
// the targets of `params` in order, every one checked, with what every family's table shares of a target: its place in the weight arena and in
// the packed W0 (w_off, base_off), out, in, kind, cg, nrows.  The adapter offsets and the first tiles are the family's placement step's (below).
// layouts (every dtype but SDXL_DTYPE_LORA): also the tensors held in a packed layout, by their kind; *mapped_ = some target needs the kind-aware kernels
static int lora_targets(Engine& e, const std::vector<int>& params, int rank, bool layouts, std::vector<LoraTarget>& tab, int* mapped_ = nullptr) {
  tab.assign(params.size(), LoraTarget());
  int mapped = 0;
  std::vector<char> seen(e.src.size(), 0);
  long b = 0;
  for (size_t i = 0; i < params.size(); ++i) {
    const int pi = params[i];
    ARG_CHECK(pi >= 0 && pi < (int)e.src.size(), "lora: parameter index %d out of range", pi);
    const SrcParam& sp = e.src[pi];
    if (!layouts)
      ARG_CHECK(sp.ndim == 2 && sp.kind == 0, "lora: '%s' is not a 2-D weight in plain row layout (convolutions and the interleaved "
                "ff.net.0.proj cannot be targets)", sp.name.c_str());
    else
      ARG_CHECK(sp.ndim == 2 || sp.ndim == 4, "lora: '%s' is not a weight (a bias or a norm parameter cannot be a target)", sp.name.c_str());
    ARG_CHECK(!seen[pi], "lora: '%s' is listed twice", sp.name.c_str());
    seen[pi] = 1;
    const int out = (int)sp.shape[0], in = (int)(sp.shape[1] * sp.shape[2] * sp.shape[3]);      // (shape is 1 past ndim)
    CHK(lora_check_shape(sp.name.c_str(), out, in, rank));
    LoraTarget& t = tab[i];
    t.kind = LORA_KIND_PLAIN; t.cg = 0; t.nrows = out;
    if (layouts && sp.kind == 1) {
      ARG_CHECK(sp.shape[2] == 3 && sp.shape[3] == 3 && sp.ci_pad == (int)sp.shape[1], "lora: '%s' is stored with its input channels padded "
                "from %ld to %d: it cannot be a target", sp.name.c_str(), sp.shape[1], sp.ci_pad);
      t.kind = LORA_KIND_CONV3; t.cg = sp.ci_pad; mapped = 1;
    } else if (layouts && sp.kind == 2) {
      ARG_CHECK(sp.ndim == 2 && out % 2 == 0 && sp.ci_pad >= 1 && (out / 2) % sp.ci_pad == 0, "lora: '%s' [%d][%d] is not interleaved in whole "
                "groups of %d", sp.name.c_str(), out, in, sp.ci_pad);
      t.kind = LORA_KIND_GEGLU; t.cg = sp.ci_pad; mapped = 1;
    } else if (layouts) {
      ARG_CHECK(sp.kind == 0, "lora: '%s' is stored in a layout (%d) the adapter kernels do not know", sp.name.c_str(), sp.kind);
    }
    t.w_off = (long)(sp.native.off + sp.elem_off);
    ARG_CHECK(t.w_off % 8 == 0, "lora: '%s' does not start on a 16-byte boundary of the arena", sp.name.c_str());
    t.base_off = b; b += (long)out * in;
    t.out = out; t.in = in;
  }
  if (mapped_) *mapped_ = mapped;
  return 0;
}

// ---- the placement step: where a family puts one target's factors, scratch and workgroups, given the targets before it ----
struct Placed {      // the running totals of a table
  long at = 0;               // adapter (and adapter-gradient) arena, elements
  long tiles[3] = {0, 0, 0}; // workgroups of the family's three launches (LoraTarget::tile_m, tile_b, tile_a)
  size_t scratch = 0;        // sdxl_lokr_op.scratch, floats
  long norm = 0;             // sdxl_dora_op.norm0 / norm, floats
};
// The walk over the adapter arena, the C twin of lora.py's adapter_layout: a target's factor sizes in arena order (lora.py's target_factors),
// each padded to 8 elements; off[i] = where factor i starts.
static void arena_place(Placed& pl, std::initializer_list<long> sizes, long* off) {
  for (long n : sizes) { *off++ = pl.at; pl.at += (n + 7) / 8 * 8; }
}
// ... and over the launches: the target's first workgroup in each, from the number it takes of each
static int tiles_place(Placed& pl, LoraTarget& t, long m, long b, long a, const char* who) {
  t.tile_m = (int)pl.tiles[0]; t.tile_b = (int)pl.tiles[1]; t.tile_a = (int)pl.tiles[2];
  pl.tiles[0] += m; pl.tiles[1] += b; pl.tiles[2] += a;
  ARG_CHECK(pl.tiles[0] < (1L << 31) && pl.tiles[1] < (1L << 31) && pl.tiles[2] < (1L << 31), "%s: too many tiles", who);
  return 0;
}
// LoRA: A [rank][in], B [out][rank]; also the direct backward's (grad_select) and, with mu behind them, DoRA's
static int lora_place(Placed& pl, LoraTarget& t, int rank) {
  long off[2];
  arena_place(pl, {(long)rank * t.in, (long)t.out * rank}, off);
  t.a_off = t.ga_off = off[0]; t.b_off = t.gb_off = off[1];
  return tiles_place(pl, t, lora_tiles_m(t.out, t.in), lora_tiles_b(t.out, t.in), lora_tiles_a(t.out, t.in), "lora");
}

// ---- the four families of sdxl_load_weight / sdxl_export_grad: what adapter_prepare (below) asks of each ----
//   who, dtype_name, list   the message prefix, the dtype and the struct field that lists the targets, as the messages name them
//   check                   the op, field and pointer checks, in the family's own order
//   lora, factor, full      the sdxl_lora_op inside the family's struct; the rest of the cache key
//   place                   the placement step of one target
//   fill                    the launch struct from the cached table and the call's pointers (and the checks that need the table)
struct TargetsKey {      // the cache key of a family whose table follows from (dtype, rank, target list) alone
  static int factor(const void*) { return 0; }
  static int full(const void*) { return 0; }
};
struct LoraFamily : TargetsKey {      // SDXL_DTYPE_LORA, SDXL_DTYPE_LORA_LAYOUTS: the launches of csrc/lora.hip
  typedef sdxl_lora_op Op; typedef LoraTarget Target; typedef LoraP P;
  static constexpr const char *who = "lora", *dtype_name = "SDXL_DTYPE_LORA", *list = "sdxl_lora_op.param";
  static int check(const Op* op, bool merge) { return lora_check_op(op, merge, !merge); }
  static const sdxl_lora_op* lora(const Op* op) { return op; }
  static int place(Placed& pl, Target& x, const LoraTarget& t, const char*, const Op* op) { x = t; return lora_place(pl, x, op->rank); }
  static int fill(const Engine& e, const LoraCache& c, const Op* op, bool, P& q) {
    q.table = (const Target*)c.dev; q.n = op->n; q.rank = op->rank; q.scale = op->scale;
    q.tiles_m = c.tiles_m; q.tiles_b = c.tiles_b; q.tiles_a = c.tiles_a; q.mapped = c.mapped;
    q.w = e.weights; q.base = (const bf16*)op->base; q.a = q.b = (const bf16*)op->adapters;
    q.dw = e.grads; q.ga = q.gb = op->adapter_grads;
    return 0;
  }
};
struct LohaFamily : TargetsKey {      // SDXL_DTYPE_LOHA: SDXL_DTYPE_LORA_LAYOUTS' checks and targets, the rank cap, four factors per target
  typedef sdxl_lora_op Op; typedef LohaTarget Target; typedef LohaP P;
  static constexpr const char *who = "loha", *dtype_name = "SDXL_DTYPE_LOHA", *list = "sdxl_lora_op.param";
  static int check(const Op* op, bool merge) {
    ARG_CHECK(op != nullptr, "loha: empty target list");
    CHK(loha_check_rank(op->rank));
    return lora_check_op(op, merge, !merge);
  }
  static const sdxl_lora_op* lora(const Op* op) { return op; }
  static int place(Placed& pl, Target& x, const LoraTarget& t, const char*, const Op* op) {
    x.t = t;
    const long na = (long)op->rank * t.in, nb = (long)t.out * op->rank;
    long off[4];
    arena_place(pl, {na, nb, na, nb}, off);      // A1, B1, A2, B2
    x.t.a_off = x.t.ga_off = off[0]; x.t.b_off = x.t.gb_off = off[1];
    x.a2_off = x.ga2_off = off[2]; x.b2_off = x.gb2_off = off[3];
    return tiles_place(pl, x.t, loha_tiles_m(t.out, t.in), loha_tiles_b(t.out, t.in), loha_tiles_a(t.out, t.in), who);
  }
  static int fill(const Engine& e, const LoraCache& c, const Op* op, bool, P& q) {
    q.table = (const Target*)c.dev; q.n = op->n; q.rank = op->rank; q.scale = op->scale;
    q.tiles_m = c.tiles_m; q.tiles_b = c.tiles_b; q.tiles_a = c.tiles_a;
    q.w = e.weights; q.base = (const bf16*)op->base; q.a1 = q.b1 = q.a2 = q.b2 = (const bf16*)op->adapters;
    q.dw = e.grads; q.ga1 = q.gb1 = q.ga2 = q.gb2 = op->adapter_grads;
    return 0;
  }
};
// SDXL_DTYPE_LOKR: SDXL_DTYPE_LORA_LAYOUTS' checks and targets; per target the factorisation, the form (the rule, or sdxl_lokr_op.full) in the
// table; the scale by the form per call (1 for a full target, op.scale for a factored one; op.scale == 0 zeroes both: the restoring merge)
struct LokrFamily {
  typedef sdxl_lokr_op Op; typedef LokrTarget Target; typedef LokrP P;
  static constexpr const char *who = "lokr", *dtype_name = "SDXL_DTYPE_LOKR", *list = "sdxl_lokr_op.op.param";
  static int check(const Op* lop, bool merge) {
    ARG_CHECK(lop != nullptr, "lokr: empty target list");
    CHK(lokr_check_fields(lop->op.rank, lop->factor, lop->full));
    return lora_check_op(&lop->op, merge, !merge);
  }
  static const sdxl_lora_op* lora(const Op* lop) { return &lop->op; }
  static int factor(const Op* lop) { return lop->factor; }
  static int full(const Op* lop) { return lop->full; }
  static int place(Placed& pl, Target& x, const LoraTarget& t, const char* name, const Op* lop) {
    const int rank = lop->op.rank;
    memset(&x, 0, sizeof(x));
    x.t = t;
    lokr_geometry(x, t.kind == LORA_KIND_CONV3 ? t.cg : t.in, lop->factor, 0);
    CHK(lokr_check_size(name, x, rank));
    x.full = lop->full || lokr_rule_full(x.out_k, x.in_n, rank);
    long off[3];
    if (x.full) {      // C, W2
      arena_place(pl, {(long)x.out_l * x.in_m, (long)x.out_k * x.n2}, off);
      x.t.a_off = x.t.ga_off = 0;
    } else {           // C, B, A
      arena_place(pl, {(long)x.out_l * x.in_m, (long)x.out_k * rank, (long)rank * x.n2}, off);
      x.t.a_off = x.t.ga_off = off[2];
    }
    x.c_off = off[0]; x.t.b_off = x.t.gb_off = off[1];
    x.part_off = (long)pl.scratch; pl.scratch += lokr_part_floats(x);
    x.dw2_off = (long)pl.scratch; pl.scratch += lokr_dw2_floats(x);
    return tiles_place(pl, x.t, lokr_tiles_m(x), x.ptiles, lokr_tiles_q(x, rank), who);
  }
  static int fill(const Engine& e, const LoraCache& c, const Op* lop, bool merge, P& q) {
    const sdxl_lora_op* op = &lop->op;
    if (!merge) CHK(lokr_check_scratch(lop->scratch, lop->scratch_floats, c.scratch_floats));
    q.table = (const Target*)c.dev; q.n = op->n; q.rank = op->rank;
    q.scale = op->scale; q.scale_full = op->scale == 0.f ? 0.f : 1.f;      // (scale 0: the restoring merge zeroes both forms)
    q.tiles_m = c.tiles_m; q.tiles_p = c.tiles_b; q.tiles_q = c.tiles_a;
    q.w = e.weights; q.base = (const bf16*)op->base; q.c = q.b = q.a = (const bf16*)op->adapters;
    q.dw = e.grads; q.gc = q.gb = q.ga = op->adapter_grads; q.scratch = lop->scratch;
    return 0;
  }
};
// SDXL_DTYPE_DORA: SDXL_DTYPE_LORA_LAYOUTS' checks and targets; per target A, B, mu in the adapter arena, LoRA's tiles and its rows of norm0 / norm
struct DoraFamily : TargetsKey {
  typedef sdxl_dora_op Op; typedef DoraTarget Target; typedef DoraP P;
  static constexpr const char *who = "dora", *dtype_name = "SDXL_DTYPE_DORA", *list = "sdxl_dora_op.op.param";
  static int check(const Op* dop, bool merge) {
    ARG_CHECK(dop != nullptr, "dora: empty target list");
    CHK(dora_check_fields(dop->op.rank, merge ? dop->mode : 0));
    CHK(lora_check_op(&dop->op, true, !merge));
    return dora_check_norms(dop->norm0, dop->norm);
  }
  static const sdxl_lora_op* lora(const Op* dop) { return &dop->op; }
  static int place(Placed& pl, Target& x, const LoraTarget& t, const char*, const Op* dop) {
    x.t = t;
    CHK(lora_place(pl, x.t, dop->op.rank));      // A, B
    arena_place(pl, {(long)t.out}, &x.mu_off);   // mu
    x.n_off = pl.norm; pl.norm += dora_pad4(t.out);
    return 0;
  }
  static int fill(const Engine& e, const LoraCache& c, const Op* dop, bool, P& q) {
    const sdxl_lora_op* op = &dop->op;
    q.table = (const Target*)c.dev; q.n = op->n; q.rank = op->rank; q.scale = op->scale;
    q.tiles_m = c.tiles_m; q.tiles_b = c.tiles_b; q.tiles_a = c.tiles_a; q.mapped = c.mapped;
    q.w = e.weights; q.base = (const bf16*)op->base; q.a = q.b = q.mu = (const bf16*)op->adapters;
    q.dw = e.grads; q.ga = q.gb = q.gmu = op->adapter_grads;
    q.norm0 = dop->norm0; q.norm = dop->norm;
    return 0;
  }
};

// The launch struct of a merge (sdxl_load_weight) or a projection (sdxl_export_grad) of family F: the checks, then the device table of the
// targets, built when the cached one (LoraCache) has another key.  The host table is complete before the cached one is freed -- a refused
// call leaves the cache as it was -- and the free comes before the allocation: hipFree waits for the launches that still read the old table.
extern "C++" template <class F>
static int adapter_prepare(sdxl_handle* h, const char* name, const typename F::Op* fop, bool merge, int dtype, typename F::P& q) {
  ARG_CHECK(name == nullptr, "%s: `name` must be NULL with %s (the targets are listed in %s)", F::who, F::dtype_name, F::list);
  CHK(F::check(fop, merge));
  const sdxl_lora_op* op = F::lora(fop);
  Engine& e = h->e;
  ARG_CHECK(merge ? e.weights != nullptr : e.grads != nullptr, "%s: %s are not bound", F::who, merge ? "weights" : "grads");
  LoraCache& c = h->lora;
  std::vector<int> params(op->param, op->param + op->n);
  const int factor = F::factor(fop), full = F::full(fop);
  if (!(c.dev && c.dtype == dtype && c.rank == op->rank && c.factor == factor && c.full == full && c.params == params)) {
    std::vector<LoraTarget> tab;
    int mapped = 0;
    CHK(lora_targets(e, params, op->rank, dtype != SDXL_DTYPE_LORA, tab, &mapped));
    std::vector<typename F::Target> ftab(tab.size());
    Placed pl;
    for (size_t i = 0; i < tab.size(); ++i) CHK(F::place(pl, ftab[i], tab[i], e.src[params[i]].name.c_str(), fop));
    lora_cache_free(c);
    HIP_CHECK_RET(hipMalloc(&c.dev, ftab.size() * sizeof(ftab[0])));
    HIP_CHECK_RET(hipMemcpy(c.dev, ftab.data(), ftab.size() * sizeof(ftab[0]), hipMemcpyHostToDevice));
    c.params = params; c.rank = op->rank; c.dtype = dtype; c.factor = factor; c.full = full; c.mapped = mapped;
    c.scratch_floats = pl.scratch;
    c.tiles_m = (int)pl.tiles[0]; c.tiles_b = (int)pl.tiles[1]; c.tiles_a = (int)pl.tiles[2];
  }
  memset(&q, 0, sizeof(q));
  return F::fill(e, c, fop, merge, q);
}
static int dora_launch_load(const DoraP& q, int mode, hipStream_t st) {
  return mode == 0 ? launch_dora_merge(q, st) : mode == 1 ? launch_dora_init(q, st) : launch_dora_restore(q, st);
}

int sdxl_load_weight(sdxl_handle* h, const char* name, const void* src, int dtype, void* st) {
  if (dtype == SDXL_DTYPE_DORA_ONE) {      // (a test hook that is a dtype: include/sdxlstep_diag.h)
    ARG_CHECK(h == nullptr && name == nullptr, "dora: SDXL_DTYPE_DORA_ONE takes no handle and no name");
    return dora_one_load((const sdxl_dora_one*)src, st);
  }
  if (dtype == SDXL_DTYPE_LOKR_ONE) {      // (a test hook that is a dtype: include/sdxlstep_diag.h)
    ARG_CHECK(h == nullptr && name == nullptr, "lokr: SDXL_DTYPE_LOKR_ONE takes no handle and no name");
    return lokr_one_merge((const sdxl_lokr_one*)src, st);
  }
  H_CHECK(h);
  if (dtype == SDXL_DTYPE_DORA) {
    DoraP q;
    CHK(adapter_prepare<DoraFamily>(h, name, (const sdxl_dora_op*)src, true, dtype, q));
    return dora_launch_load(q, ((const sdxl_dora_op*)src)->mode, (hipStream_t)st);
  }
  if (dtype == SDXL_DTYPE_LOKR) {
    LokrP q;
    CHK(adapter_prepare<LokrFamily>(h, name, (const sdxl_lokr_op*)src, true, dtype, q));
    return launch_lokr_merge(q, (hipStream_t)st);
  }
  if (dtype == SDXL_DTYPE_LOHA) {
    LohaP q;
    CHK(adapter_prepare<LohaFamily>(h, name, (const sdxl_lora_op*)src, true, dtype, q));
    return launch_loha_merge(q, (hipStream_t)st);
  }
  if (dtype == SDXL_DTYPE_LORA || dtype == SDXL_DTYPE_LORA_LAYOUTS) {
    LoraP q;
    CHK(adapter_prepare<LoraFamily>(h, name, (const sdxl_lora_op*)src, true, dtype, q));
    return launch_lora_merge(q, (hipStream_t)st);
  }
  ARG_CHECK(name && src, "null argument");
  return engine_load_weight(h->e, name, src, dtype, (hipStream_t)st);
}
int sdxl_export_weight(sdxl_handle* h, const char* name, void* dst, int dtype, void* st) {
  H_CHECK(h);
  ARG_CHECK(name && dst, "null argument");
  return engine_export(h->e, name, dst, dtype, false, (hipStream_t)st);
}
// ---- gradient selection (SDXL_DTYPE_GRAD_SELECT): host flags in, Engine::set_trainable; nothing is launched ----
static int grad_select(sdxl_handle* h, const char* name, const sdxl_grad_select* sel) {
  ARG_CHECK(name == nullptr, "grad select: `name` must be NULL with SDXL_DTYPE_GRAD_SELECT (the tensors are flagged in sdxl_grad_select.trainable)");
  H_CHECK(h);
  Engine& e = h->e;
  std::vector<unsigned char> want;      // normal form: empty = every tensor trainable
  if (sel) {
    ARG_CHECK(sel->n == (int)e.src.size(), "grad select: n = %d, but the model has %d state-dict tensors (sdxl_num_params)", sel->n, (int)e.src.size());
    ARG_CHECK(sel->trainable != nullptr, "grad select: trainable is NULL (pass a NULL struct for `every tensor trainable`)");
    bool all = true;
    for (int i = 0; i < sel->n; ++i) {
      ARG_CHECK(sel->trainable[i] <= 1, "grad select: trainable[%d] ('%s') is %d (0 = frozen, 1 = trainable)", i, e.src[i].name.c_str(), (int)sel->trainable[i]);
      all = all && sel->trainable[i] == 1;
    }
    if (!all) want.assign(sel->trainable, sel->trainable + sel->n);
  }
  // adapters whose gradients the backward writes itself: the same checks and messages as SDXL_DTYPE_LORA, then the targets by op
  Engine::LoraSel L;
  std::vector<LoraGradTarget> flat;
  if (sel && sel->lora) {
    const sdxl_lora_op* op = sel->lora;
    CHK(lora_check_op(op, false, true));
    ARG_CHECK(e.emit_base == nullptr, "lora: adapter gradients from the backward cannot be combined with a bf16 emit arena (sdxl_set_grad_emit)");
    L.params.assign(op->param, op->param + op->n);
    L.rank = op->rank; L.scale = op->scale; L.adapters = (const bf16*)op->adapters; L.grads = op->adapter_grads;
    std::vector<LoraTarget> tab;
    CHK(lora_targets(e, L.params, op->rank, false, tab));
    Placed pl;
    for (LoraTarget& t : tab) CHK(lora_place(pl, t, op->rank));
    for (size_t i = 0; i < tab.size(); ++i) {
      const SrcParam& sp = e.src[L.params[i]];
      ARG_CHECK(sp.elem_off % (size_t)tab[i].in == 0, "lora: '%s' does not start on a row of its native weight", sp.name.c_str());
      LoraGradTarget g;
      memset(&g, 0, sizeof(g));
      g.a_off = tab[i].a_off; g.b_off = tab[i].b_off; g.ga_off = tab[i].ga_off; g.gb_off = tab[i].gb_off;
      g.out = tab[i].out; g.in = tab[i].in; g.dy_col = (int)(sp.elem_off / (size_t)tab[i].in);
      L.ops[sp.native.off].host.push_back(g);
    }
    // every tensor of an op that holds a target is frozen: the op forms no dW, so it has no gradient to give them
    for (size_t i = 0; i < e.src.size(); ++i) {
      if (!sel->trainable[i]) continue;
      const SrcParam& sp = e.src[i];
      bool shares = L.ops.count(sp.native.off) != 0;
      const size_t dot = sp.name.rfind('.');
      if (!shares && dot != std::string::npos && sp.name.compare(dot, std::string::npos, ".bias") == 0) {      // the bias of a targeted layer
        auto it = e.src_index.find(sp.name.substr(0, dot) + ".weight");
        shares = it != e.src_index.end() && L.ops.count(e.src[it->second].native.off) != 0;
      }
      ARG_CHECK(!shares, "grad select: '%s' is flagged trainable but belongs to an op with adapter targets, whose dW is never formed: its flag must be 0",
                sp.name.c_str());
    }
    for (auto& kv : L.ops) {
      Engine::LoraOpSel& o = kv.second;
      long tiles = 0, reds = 0, unit = 0;
      for (LoraGradTarget& g : o.host) {
        g.tile0 = (int)tiles; g.red0 = (int)reds; g.part_off = unit;
        tiles += lora_grad_tiles(g.out, g.in); reds += lora_grad_reds(g.out, g.in, L.rank); unit += (long)L.rank * ((long)g.in + g.out);
      }
      ARG_CHECK(tiles < (1L << 24) && reds < (1L << 31), "lora: too many tiles");
      o.tiles = (int)tiles; o.reds = (int)reds; o.part_unit = (size_t)unit;
      flat.insert(flat.end(), o.host.begin(), o.host.end());
    }
  }
  const bool same_lora = L.params == e.lora.params && L.rank == e.lora.rank && L.scale == e.lora.scale && L.adapters == e.lora.adapters &&
                         L.grads == e.lora.grads;
  if (want == e.trainable && same_lora) return 0;      // unchanged: captured graphs stay valid
  ARG_CHECK(!h->step.awaiting_bwd, "grad select: the selection cannot change between sdxl_forward_loss and the end of its backward");
  e.clear_graphs();                       // captured backwards hold the old selection's launches
  if (!same_lora) {
    // the plans reserve the adapter-gradient scratch of their targeted ops: dropped, the caller plans again (sdxl_plan, sdxl_bind_workspace)
    HIP_CHECK_RET(hipDeviceSynchronize());
    e.drop_pending();
    e.plans.clear();
    e.cur = nullptr;
    if (e.lora.dev) { (void)hipFree(e.lora.dev); e.lora.dev = nullptr; }
    if (!flat.empty()) {
      HIP_CHECK_RET(hipMalloc((void**)&L.dev, flat.size() * sizeof(LoraGradTarget)));
      if (hipMemcpy(L.dev, flat.data(), flat.size() * sizeof(LoraGradTarget), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(L.dev);
        e.lora = Engine::LoraSel();      // (the old table is gone and the plans are dropped: no adapters until the next call)
        sdxl_set_error("grad select: copying the target table to the device failed");
        return 2;
      }
      size_t at = 0;
      for (auto& kv : L.ops) { kv.second.dev = L.dev + at; at += kv.second.host.size(); }
    }
    e.lora = std::move(L);
  }
  e.set_trainable(want.empty() ? nullptr : want.data());
  return 0;
}

int sdxl_export_grad(sdxl_handle* h, const char* name, void* dst, int dtype, void* st) {
  if (dtype == SDXL_DTYPE_GRAD_SELECT) return grad_select(h, name, (const sdxl_grad_select*)dst);
  if (dtype == SDXL_DTYPE_LOKR_ONE) {
    ARG_CHECK(h == nullptr && name == nullptr, "lokr: SDXL_DTYPE_LOKR_ONE takes no handle and no name");
    return lokr_one_project((const sdxl_lokr_one*)dst, st);
  }
  if (dtype == SDXL_DTYPE_DORA_ONE) {
    ARG_CHECK(h == nullptr && name == nullptr, "dora: SDXL_DTYPE_DORA_ONE takes no handle and no name");
    return dora_one_project((const sdxl_dora_one*)dst, st);
  }
  H_CHECK(h);
  if (dtype == SDXL_DTYPE_DORA) {
    DoraP q;
    CHK(adapter_prepare<DoraFamily>(h, name, (const sdxl_dora_op*)dst, false, dtype, q));
    return launch_dora_project(q, (hipStream_t)st);
  }
  if (dtype == SDXL_DTYPE_LOKR) {
    LokrP q;
    CHK(adapter_prepare<LokrFamily>(h, name, (const sdxl_lokr_op*)dst, false, dtype, q));
    return launch_lokr_project(q, (hipStream_t)st);
  }
  if (dtype == SDXL_DTYPE_LOHA) {
    LohaP q;
    CHK(adapter_prepare<LohaFamily>(h, name, (const sdxl_lora_op*)dst, false, dtype, q));
    return launch_loha_project(q, (hipStream_t)st);
  }
  if (dtype == SDXL_DTYPE_LORA || dtype == SDXL_DTYPE_LORA_LAYOUTS) {
    LoraP q;
    CHK(adapter_prepare<LoraFamily>(h, name, (const sdxl_lora_op*)dst, false, dtype, q));
    return launch_lora_project(q, (hipStream_t)st);
  }
  ARG_CHECK(name && dst, "null argument");
  return engine_export(h->e, name, dst, dtype, true, (hipStream_t)st);
}

int sdxl_plan(sdxl_handle* h, int B, int H, int W, int ctx, size_t* ws_bytes) {
  H_CHECK(h);
  ARG_CHECK(B > 0 && H > 0 && W > 0 && ctx > 0, "bad plan shape B=%d H=%d W=%d ctx=%d", B, H, W, ctx);
  ARG_CHECK(H % 4 == 0 && W % 4 == 0, "latent H=%d W=%d must be multiples of 4 (two stride-2 levels)", H, W);
  Engine& e = h->e;
  auto key = std::make_tuple(B, H, W, ctx);
  auto it = e.plans.find(key);
  if (it == e.plans.end()) {
    std::unique_ptr<Plan> p(new Plan());
    p->eng = &e;
    p->B = B; p->H = H; p->W = W; p->ctx = ctx;
    e.build(p.get());
    it = e.plans.emplace(key, std::move(p)).first;
  }
  if (e.cur != it->second.get()) e.drop_pending();
  e.cur = it->second.get();
  h->step.awaiting_bwd = false;      // (the caller's way to say that the last sdxl_forward_loss gets no backward: sdxlstep.h, gradient selection)
  if (ws_bytes) *ws_bytes = e.cur->ws_bytes;
  return 0;
}

int sdxl_bind_workspace(sdxl_handle* h, void* ws, size_t bytes) {
  H_CHECK(h);
  Engine& e = h->e;
  if (ws) {
    if (ws == (void*)e.ws && bytes == e.ws_cap) return 0;     // unchanged: captured graphs stay valid
    e.clear_graphs();
    if (e.own_ws && e.ws) (void)hipFree(e.ws);
    e.ws = (char*)ws; e.ws_cap = bytes; e.own_ws = false;
  } else {
    size_t need = bytes;
    for (auto& kv : e.plans) if (kv.second->ws_bytes > need) need = kv.second->ws_bytes;
    if (e.own_ws && e.ws && e.ws_cap >= need) return 0;
    e.clear_graphs();
    if (e.own_ws && e.ws) (void)hipFree(e.ws);
    HIP_CHECK_RET(hipMalloc((void**)&e.ws, need));
    e.ws_cap = need; e.own_ws = true;
  }
  ARG_CHECK(((uintptr_t)e.ws & 255) == 0, "workspace must be 256-byte aligned");
  return 0;
}

// zero the gradient ranges that are accumulated with += by every backward (bias / norm vectors: ~2.6 M of the 2.57 G elements; one writer per element and launch);
// the weight matrices are overwritten by the first micro-step's wgrad GEMMs (first_micro) and need no zeroing
static int small_ranges_on_device(Engine& e);
__global__ void zero_ranges_kernel(float* __restrict__ g, const unsigned long long* __restrict__ ranges) {
  const unsigned long long off = ranges[2 * blockIdx.x], n = ranges[2 * blockIdx.x + 1];
  for (unsigned long long i = threadIdx.x; i < n; i += blockDim.x) g[off + i] = 0.f;
}

int sdxl_zero_grads(sdxl_handle* h, void* st) {
  H_CHECK(h);
  Engine& e = h->e;
  ARG_CHECK(e.grads, "grads are not bound");
  CHK(small_ranges_on_device(e));
  hipLaunchKernelGGL(zero_ranges_kernel, dim3((unsigned)e.small_ranges.size()), dim3(256), 0, (hipStream_t)st, e.grads,
                     e.small_ranges_dev);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

static int check_batch(Engine& e, const sdxl_batch* b) {
  Plan& p = *e.cur;
  ARG_CHECK(b, "null batch");
  const int ctx = b->ctx_len & ~SDXL_BATCH_FLAGS;
  ARG_CHECK(b->B == p.B && b->H == p.H && b->W == p.W && ctx == p.ctx,
            "batch shape (B=%d,H=%d,W=%d,ctx=%d) does not match the current plan (B=%d,H=%d,W=%d,ctx=%d)", b->B, b->H,
            b->W, ctx, p.B, p.H, p.W, p.ctx);
  ARG_CHECK(b->timestep && b->prompt_embeds && b->pooled && b->time_ids, "batch is missing conditioning pointers");
  return 0;
}

// The conditioning-gradient request of a micro-step: sdxl_batch_ext's two fields, read only behind SDXL_BATCH_EXT (a caller without the
// flag passes a shorter struct).  The one error that needs no plan comes first, before the handle is looked at or anything is launched.
static int check_cond_request(const sdxl_batch* b) {
  if (!b || !(b->ctx_len & SDXL_BATCH_FLAGS)) return 0;
  const sdxl_batch_ext* x = (const sdxl_batch_ext*)b;
  ARG_CHECK(!(b->sampler && (x->d_prompt_embeds || x->d_pooled)), "d_prompt_embeds / d_pooled cannot be combined with a sampler step");
  return 0;
}
static int read_cond_request(Engine& e, const sdxl_batch* b, float** d_ehs, float** d_pool) {
  *d_ehs = *d_pool = nullptr;
  if (!(b->ctx_len & SDXL_BATCH_FLAGS)) return 0;
  const sdxl_batch_ext* x = (const sdxl_batch_ext*)b;
  if (x->d_prompt_embeds) {
    for (int g = 0; g < e.cur->cond_nkv; ++g)
      ARG_CHECK(e.cur->cond_kv[g].K % 64 == 0, "d_prompt_embeds: K | V width %d is not a multiple of 64", e.cur->cond_kv[g].K);
  }
  if (x->d_pooled) ARG_CHECK(e.cur->cond_add.K >= 64 && e.cur->cond_add.K % 64 == 0, "d_pooled: time-embedding width %d is not a multiple of 64", e.cur->cond_add.K);
  *d_ehs = x->d_prompt_embeds; *d_pool = x->d_pooled;
  return 0;
}
// The extra input channels of a batch (sdxl_batch_cond) against the handle's in_channels, before anything is copied or launched.
// reader: this call builds the UNet input itself (loss preparation, sampler step), so in_channels > 4 needs the array.
static int check_input_cond(const Engine& e, const sdxl_batch* b, bool reader, const float** cond) {
  const int n = e.cfg.in_channels - 4;
  int ch;
  read_input_cond(b, cond, &ch);
  ARG_CHECK(n > 0 || !*cond, "input_cond must be NULL: the UNet has in_channels = 4");
  ARG_CHECK(ch == 0 || ch == n, "input_cond: cond_channels %d does not match in_channels - 4 = %d", ch, n);
  ARG_CHECK(n == 0 || !reader || *cond, "input_cond is missing: the UNet has in_channels = %d, channels 4.. of its input come from input_cond", e.cfg.in_channels);
  return 0;
}
// which of them the backward of this micro-step produces: part of the capture key of its graphs (the launch sequence differs)
static unsigned cond_bits(const StepState& s) { return ((unsigned)(s.d_ehs != nullptr) << 8) | ((unsigned)(s.d_pool != nullptr) << 9); }
// ... and the copies from the plan's buffers to the caller's, behind the last segment (outside any captured graph: the caller's buffers may move)
static int copy_cond_grads(sdxl_handle* h, hipStream_t st) {
  Plan& p = *h->e.cur;
  const sdxl_unet_config& c = h->e.cfg;
  if (h->step.d_ehs)
    HIP_CHECK_RET(hipMemcpyAsync(h->step.d_ehs, p.F(p.dehs_off), sizeof(float) * (size_t)p.B * p.ctx * c.cross_attention_dim, hipMemcpyDeviceToDevice, st));
  if (h->step.d_pool)
    HIP_CHECK_RET(hipMemcpyAsync(h->step.d_pool, p.F(p.dpool_off), sizeof(float) * (size_t)p.B * c.pooled_dim, hipMemcpyDeviceToDevice, st));
  return 0;
}
static void set_cond_request(sdxl_handle* h, bool gated) {
  h->e.cond_ehs = h->step.d_ehs != nullptr; h->e.cond_pool = h->step.d_pool != nullptr; h->e.cond_gated = gated;
  h->e.res_bwd = h->step.res.wants_grads() ? &h->step.res : nullptr; h->e.res_gated = gated;      // (the residual gradients: ConcatOp::bwd)
  h->e.din = h->step.d_input; h->e.din_gated = gated;                                              // (the input gradient: conv_in's ConvOp::bwd)
}

static int upload_cond(Engine& e, const sdxl_batch* b, hipStream_t st) {
  Plan& p = *e.cur;
  const sdxl_unet_config& c = e.cfg;
  HIP_CHECK_RET(hipMemcpyAsync(p.P(p.ehs), b->prompt_embeds, (size_t)p.B * p.ctx * c.cross_attention_dim * sizeof(bf16),
                               hipMemcpyDeviceToDevice, st));
  HIP_CHECK_RET(hipMemcpyAsync(p.F(p.t_off), b->timestep, sizeof(float) * p.B, hipMemcpyDeviceToDevice, st));
  HIP_CHECK_RET(hipMemcpyAsync(p.F(p.tid_off), b->time_ids, sizeof(float) * p.B * 6, hipMemcpyDeviceToDevice, st));
  CHK(launch_copy_cols((const bf16*)b->pooled, c.pooled_dim, p.P(p.aug_in), c.pooled_dim + 6L * c.addition_time_embed_dim,
                       p.B, c.pooled_dim, st));
  return 0;
}

static void fill_loss(Engine& e, const sdxl_loss_config* lc, const sdxl_batch* b, float grad_scale, LossP& L) {
  Plan& p = *e.cur;
  memset(&L, 0, sizeof(L));
  L.method = lc->method; L.prediction_type = lc->prediction_type; L.use_min_snr = lc->use_min_snr;
  L.min_snr_gamma = lc->min_snr_gamma; L.use_ztsnr = lc->use_ztsnr;
  fill_loss_ext(lc, b, L);
  L.B = p.B; L.HW = p.H * p.W; L.C = 4;
  L.latents = b->latents; L.noise = b->noise; L.sigma = b->sigma_or_t; L.tag_w = b->tag_weights;
  L.unet_in = p.P(p.x_in); L.pred = p.P(p.pred); L.dpred = p.G(p.pred);
  L.grad_scale = grad_scale;
  L.out = p.F(p.loss_off);
  L.part = p.F(p.loss_part_off);
  L.mnorm = p.F(p.mask_norm_off);
}

// run `body(stream)` once eagerly (first call for a key: one-time function attributes), capture it on the second call, replay
// the instantiated graph from then on; everything on the engine's graph stream, fenced against the caller's stream
static int run_graphed(Engine& e, Engine::GraphKey key, hipStream_t user, const std::function<int(hipStream_t)>& body) {
  if (!e.use_graphs || !e.gstream || gemm_profiling()) return body(user);
  Engine::GraphEntry& g = e.graphs[key];
  hipStream_t gs = e.gstream;
  HIP_CHECK_RET(hipEventRecord(e.ev_gin, user));
  HIP_CHECK_RET(hipStreamWaitEvent(gs, e.ev_gin, 0));
  if (g.exec) {
    HIP_CHECK_RET(hipGraphLaunch(g.exec, gs));
  } else if (g.seen++ == 0) {
    CHK(body(gs));
  } else {
    HIP_CHECK_RET(hipStreamBeginCapture(gs, hipStreamCaptureModeThreadLocal));
    const int rc = body(gs);
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(gs, &graph);
    if (rc || ce != hipSuccess) {
      if (graph) (void)hipGraphDestroy(graph);
      if (rc) return rc;
      sdxl_set_error("hipStreamEndCapture: %s", hipGetErrorString(ce));
      return 2;
    }
    HIP_CHECK_RET(hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0));
    (void)hipGraphDestroy(graph);
    HIP_CHECK_RET(hipGraphLaunch(g.exec, gs));
  }
  HIP_CHECK_RET(hipEventRecord(e.ev_gout, gs));
  HIP_CHECK_RET(hipStreamWaitEvent(user, e.ev_gout, 0));
  return 0;
}
static unsigned loss_cfg_bits(const sdxl_loss_config& lc, bool tag) {
  unsigned g;
  memcpy(&g, &lc.min_snr_gamma, 4);
  return (unsigned)lc.method | ((unsigned)lc.prediction_type << 2) | ((unsigned)lc.use_min_snr << 4) | ((unsigned)lc.use_ztsnr << 5) |
         ((unsigned)tag << 6) | (g << 7);
}
// the second key word: element loss, which of the per-sample arrays, the mask and noise_in are present and the mask's normalisation
// (every one changes the captured kernels' arguments); lc is read_loss_config's copy, so loss_type is without the flag
static unsigned loss_cfg_bits2(const sdxl_loss_config& lc, const sdxl_batch& b) {
  return (unsigned)(lc.loss_type & 3) | ((unsigned)(b.sample_weights != nullptr) << 2) | ((unsigned)(b.huber_c != nullptr) << 3) |
         ((unsigned)(b.per_sample_loss != nullptr) << 4) | ((unsigned)(lc.loss_mask != nullptr) << 5) |
         ((unsigned)(lc.noise_in != nullptr) << 6) | ((unsigned)(lc.mask_norm & 1) << 7);
}
// the third: the scalar huber_c, a kernel argument baked into a captured graph (not read for l2 or with a per-sample array)
static unsigned loss_huber_bits(const sdxl_loss_config& lc, const sdxl_batch& b) {
  unsigned h = 0;
  if (lc.loss_type != 0 && !b.huber_c) memcpy(&h, &lc.huber_c, 4);
  return h;
}

static int run_forward_ops(Engine& e, hipStream_t st) {
  Plan& p = *e.cur;
  e.drop_pending();      // (leftovers of a backward that failed half way)
  const bool side = e.use_side && e.side && !gemm_profiling();
  if (side) {   // hoisted ops (inputs-only dependencies) run on the side stream, concurrently with the first layers
    HIP_CHECK_RET(hipEventRecord(e.ev_hoist, st));
    HIP_CHECK_RET(hipStreamWaitEvent(e.side, e.ev_hoist, 0));
    for (auto& op : p.ops) if (op->hoist_fwd) CHK(op->fwd(p, e.side));
    HIP_CHECK_RET(hipEventRecord(e.ev_hoist, e.side));
  }
  bool waited = false;
  for (auto& op : p.ops) {
    if (side && op->hoist_fwd) continue;
    if (side && op->needs_hoisted && !waited) {
      HIP_CHECK_RET(hipStreamWaitEvent(st, e.ev_hoist, 0));
      waited = true;
    }
    CHK(op->fwd(p, st));
  }
  if (side && e.side_dirty) {      // forward work put on the side stream (an upsampled image only a weight gradient reads): the caller's
    HIP_CHECK_RET(hipEventRecord(e.ev_join, e.side));      // stream owns everything the forward produced once this returns
    HIP_CHECK_RET(hipStreamWaitEvent(st, e.ev_join, 0));
    e.side_dirty = false;
  }
  return 0;
}

int sdxl_forward_loss(sdxl_handle* h, const sdxl_loss_config* lc, const sdxl_batch* b, void* stp) {
  CHK(check_cond_request(b));
  H_CHECK(h);
  Engine& e = h->e;
  hipStream_t st = (hipStream_t)stp;
  CHK(ready(e));
  ARG_CHECK(lc, "null loss config");
  ARG_CHECK(lc->method == 0 || lc->method == 1, "unknown method %d", lc->method);
  CHK(check_batch(e, b));
  ARG_CHECK(b->latents && b->noise && b->sigma_or_t, "batch is missing latents/noise/sigma");
  sdxl_loss_config full;
  CHK(read_loss_config(lc, &full));
  lc = &full;
  CHK(check_loss_ext(lc, b));
  const float* icond;
  CHK(check_input_cond(e, b, true, &icond));
  float *d_ehs, *d_pool;
  CHK(read_cond_request(e, b, &d_ehs, &d_pool));
  ResidualReq res;
  CHK(read_residuals(b, e.num_skips(), &res));
  float* d_input;
  CHK(read_input_grad(b, e.cfg.block_out_channels[0], &d_input));
  CHK(upload_cond(e, b, st));
  // the step's inputs are staged at fixed addresses inside the plan (the caller's tensors move from step to step; the captured
  // kernels must not)
  Plan& p = *e.cur;
  sdxl_batch sb;      // every field but the appended sampler pointer, which only sdxl_unet_forward reads (a caller of this entry point
  memcpy(&sb, b, offsetof(sdxl_batch, sampler));      // may hold the struct as it was before that field was appended)
  sb.sampler = nullptr; sb.ctx_len = p.ctx;
  if (e.use_graphs) {
    const size_t nlat = sizeof(float) * (size_t)p.B * 4 * p.H * p.W;
    HIP_CHECK_RET(hipMemcpyAsync(p.F(p.in_lat_off), b->latents, nlat, hipMemcpyDeviceToDevice, st));
    HIP_CHECK_RET(hipMemcpyAsync(p.F(p.in_noise_off), b->noise, nlat, hipMemcpyDeviceToDevice, st));
    HIP_CHECK_RET(hipMemcpyAsync(p.F(p.in_sig_off), b->sigma_or_t, sizeof(float) * p.B, hipMemcpyDeviceToDevice, st));
    if (b->tag_weights) HIP_CHECK_RET(hipMemcpyAsync(p.F(p.in_tag_off), b->tag_weights, sizeof(float) * p.B, hipMemcpyDeviceToDevice, st));
    sb.latents = p.F(p.in_lat_off); sb.noise = p.F(p.in_noise_off); sb.sigma_or_t = p.F(p.in_sig_off);
    sb.tag_weights = b->tag_weights ? p.F(p.in_tag_off) : nullptr;
    if (b->sample_weights) {
      HIP_CHECK_RET(hipMemcpyAsync(p.F(p.in_sw_off), b->sample_weights, sizeof(float) * p.B, hipMemcpyDeviceToDevice, st));
      sb.sample_weights = p.F(p.in_sw_off);
    }
    if (b->huber_c) {
      HIP_CHECK_RET(hipMemcpyAsync(p.F(p.in_hc_off), b->huber_c, sizeof(float) * p.B, hipMemcpyDeviceToDevice, st));
      sb.huber_c = p.F(p.in_hc_off);
    }
    if (full.loss_mask) {
      HIP_CHECK_RET(hipMemcpyAsync(p.F(p.in_mask_off), full.loss_mask, sizeof(float) * (size_t)p.B * p.H * p.W, hipMemcpyDeviceToDevice, st));
      full.loss_mask = p.F(p.in_mask_off);
    }
    if (full.noise_in) {
      HIP_CHECK_RET(hipMemcpyAsync(p.F(p.in_nin_off), full.noise_in, nlat, hipMemcpyDeviceToDevice, st));
      full.noise_in = p.F(p.in_nin_off);
    }
    if (icond) {
      HIP_CHECK_RET(hipMemcpyAsync(p.F(p.in_cond_off), icond, sizeof(float) * (size_t)p.B * (e.cfg.in_channels - 4) * p.H * p.W, hipMemcpyDeviceToDevice, st));
      icond = p.F(p.in_cond_off);
    }
  }
  // the per-sample losses are produced inside the plan (a fixed address for a captured graph) and copied out below
  if (b->per_sample_loss) sb.per_sample_loss = p.F(p.ps_loss_off);
  LossP L;
  fill_loss(e, lc, &sb, 1.f, L);
  const int ncond = icond ? e.cfg.in_channels - 4 : 0;      // (the preparation only: the backward never reads input_cond)
  Engine::GraphKey key{&p, 0, 0, 0, 0, 0u, loss_cfg_bits(*lc, b->tag_weights != nullptr), loss_cfg_bits2(*lc, *b) | ((unsigned)(icond != nullptr) << 10),
                      loss_huber_bits(*lc, *b)};
  auto body = [&](hipStream_t s) -> int {
    CHK(launch_loss_prepare(L, s, icond, ncond));
    CHK(run_forward_ops(e, s));
    CHK(launch_loss_fwd(L, s));
    return 0;
  };
  if (res.present) {      // additional residuals: kernel by kernel also in graph mode (the caller's tensors are read where they lie)
    e.res_fwd = &res;
    const int rc = body(st);
    e.res_fwd = nullptr;
    CHK(rc);
  } else {
    CHK(run_graphed(e, key, st, body));
  }
  if (b->per_sample_loss)
    HIP_CHECK_RET(hipMemcpyAsync(b->per_sample_loss, p.F(p.ps_loss_off), sizeof(float) * p.B, hipMemcpyDeviceToDevice, st));
  h->step.lc = full; h->step.b = sb; h->step.valid = true;
  h->step.d_ehs = d_ehs; h->step.d_pool = d_pool;
  h->step.res = std::move(res);
  h->step.d_input = d_input;
  h->step.awaiting_bwd = true;
  return 0;
}

int sdxl_num_segments(sdxl_handle* h) { return h ? h->e.nseg : -1; }
int sdxl_set_join_mode(sdxl_handle* h, int mode) {
  H_CHECK(h);
  ARG_CHECK(mode >= 0 && mode <= 2, "join mode %d (0, 1, 2)", mode);
  h->e.join_last_only = mode != 0;
  h->e.seg_on_side = mode == 2 && h->e.use_side && h->e.side;
  return 0;
}
int sdxl_side_stream(sdxl_handle* h, void** stream) {
  H_CHECK(h);
  ARG_CHECK(stream, "null output");
  *stream = h->e.use_side ? (void*)h->e.side : nullptr;
  return 0;
}

int sdxl_segment_range(sdxl_handle* h, int k, size_t* off, size_t* n) {
  H_CHECK(h);
  ARG_CHECK(k >= 0 && k < h->e.nseg, "segment %d out of range", k);
  int s = h->e.nseg - 1 - k;
  if (off) *off = h->e.seg_begin[s];
  if (n) *n = h->e.seg_end[s] - h->e.seg_begin[s];
  return 0;
}

static int run_backward_segment_body(Engine& e, int k, bool first, hipStream_t st);
static int run_backward_segment(Engine& e, int k, bool first, hipStream_t st) {
  if (k == 0) e.drop_pending();
  const int rc = run_backward_segment_body(e, k, first, st);
  if (rc) e.drop_pending();      // an op failed: its queued leaves / grouped weight gradients must not ride on a later step's fork event
  return rc;
}
static int run_backward_segment_body(Engine& e, int k, bool first, hipStream_t st) {
  Plan& p = *e.cur;
  int s = e.nseg - 1 - k;
  e.ev_used = 0;   // per-op events are consumed in order; a segment's waits are all enqueued before the pool is reused
  if (k == 0 && p.tp32_off != NONE) HIP_CHECK_RET(hipMemsetAsync(p.F(p.tp32_off), 0, p.tp32_bytes, st));
  if (k == 0 && p.ln_part_floats) {      // the fused LayerNorm backward's tagged partial sums: epochs count from 1 in every backward
    HIP_CHECK_RET(hipMemsetAsync(p.F(p.ln_part_off), 0, p.ln_part_floats * sizeof(float), st));
    p.ln_epoch = 0;
  }
  for (int i = p.seg_last_op[s]; i >= p.seg_first_op[s] && i >= 0; --i) CHK(p.ops[i]->bwd(p, st, first));
  // the segment's weight gradients are complete once `st` passes this point -- unless the caller declared (sdxl_set_join_mode)
  // that it only needs that of the whole backward (no per-segment gradient exchange): then the side stream runs free
  // until the last segment (nothing on the main stream reads a weight gradient, and no gradient buffer is reused)
  CHK(e.flush_wgrads(p, st));
  CHK(e.flush_ln_params(p, st));
  // the per-sample column sums are reduced only by the LinearOp that casts their fp32 buffer: one still queued after the last
  // segment was never folded into its gradient (a silent zero), so that is an error.  (wg_pending / ln_pending: flushed just above)
  ARG_CHECK(k != e.nseg - 1 || e.cs_pending.empty(), "backward: %zu per-sample column sums were never reduced", e.cs_pending.size());
  if (e.seg_on_side && !gemm_profiling()) {   // the side stream sees the segment's main-stream gradients (norm parameters, ...)
    HIP_CHECK_RET(hipEventRecord(e.ev_seg, st));
    HIP_CHECK_RET(hipStreamWaitEvent(e.side, e.ev_seg, 0));
    e.side_dirty = true;                       // (the caller's cast + collective follow on the side stream)
  }
  if (e.side_dirty && !(e.join_last_only && k != e.nseg - 1)) {
    HIP_CHECK_RET(hipEventRecord(e.ev_join, e.side));
    HIP_CHECK_RET(hipStreamWaitEvent(st, e.ev_join, 0));
    e.side_dirty = false;
  }
  // the conditioning gradients, when this micro-step asked: behind the last join (dK | dV come from the side stream), on the caller's stream
  if (k == e.nseg - 1 && (e.cond_ehs || e.cond_pool)) CHK(e.launch_cond_grads(p, st));
  return 0;
}

int sdxl_backward_segment(sdxl_handle* h, int k, float grad_scale, int first_micro, void* stp) {
  H_CHECK(h);
  Engine& e = h->e;
  hipStream_t st = (hipStream_t)stp;
  CHK(ready(e));
  ARG_CHECK(k >= 0 && k < e.nseg, "segment %d out of range", k);
  if (k == 0) ARG_CHECK(h->step.valid, "sdxl_backward_segment(0) needs a preceding sdxl_forward_loss");
  set_cond_request(h, true);
  auto body = [&](hipStream_t s) -> int {
    if (k == 0) {
      LossP L;
      fill_loss(e, &h->step.lc, &h->step.b, grad_scale, L);
      CHK(launch_loss_bwd(L, s));
    }
    return run_backward_segment(e, k, first_micro != 0, s);
  };
  // a segment can only be captured on its own when it ends with the side stream joined (per-segment join mode, or the last one)
  if (e.join_last_only || h->step.res.present || h->step.d_input) {      // (a micro-step that carried residuals: kernel by kernel, as its forward; one that asked for d_input: its kernel writes the caller's buffer)
    CHK(body(st));
  } else {
    unsigned sbits;
    memcpy(&sbits, &grad_scale, 4);
    Engine::GraphKey key{e.cur, 1, k, first_micro != 0, 0, sbits, loss_cfg_bits(h->step.lc, h->step.b.tag_weights != nullptr),
                        loss_cfg_bits2(h->step.lc, h->step.b) | cond_bits(h->step), loss_huber_bits(h->step.lc, h->step.b)};
    CHK(run_graphed(e, key, st, body));
  }
  if (k == e.nseg - 1) h->step.awaiting_bwd = false;
  return k == e.nseg - 1 ? copy_cond_grads(h, st) : 0;
}

int sdxl_backward_all(sdxl_handle* h, float grad_scale, int first_micro, void* stp) {
  H_CHECK(h);
  Engine& e = h->e;
  hipStream_t st = (hipStream_t)stp;
  CHK(ready(e));
  ARG_CHECK(h->step.valid, "sdxl_backward_all needs a preceding sdxl_forward_loss");
  unsigned sbits;
  memcpy(&sbits, &grad_scale, 4);
  set_cond_request(h, true);
  Engine::GraphKey key{e.cur, 2, 0, first_micro != 0, e.join_last_only, sbits, loss_cfg_bits(h->step.lc, h->step.b.tag_weights != nullptr),
                      loss_cfg_bits2(h->step.lc, h->step.b) | cond_bits(h->step), loss_huber_bits(h->step.lc, h->step.b)};
  auto body = [&](hipStream_t s) -> int {
    LossP L;
    fill_loss(e, &h->step.lc, &h->step.b, grad_scale, L);
    CHK(launch_loss_bwd(L, s));
    for (int k = 0; k < e.nseg; ++k) CHK(run_backward_segment(e, k, first_micro != 0, s));
    return 0;
  };
  if (h->step.res.present || h->step.d_input) CHK(body(st));      // (a micro-step that carried residuals or asked for d_input: kernel by kernel)
  else CHK(run_graphed(e, key, st, body));
  h->step.awaiting_bwd = false;
  return copy_cond_grads(h, st);
}
int sdxl_set_graph_mode(sdxl_handle* h, int on) {
  H_CHECK(h);
  h->e.use_graphs = on != 0 && h->e.use_side;
  if (!h->e.use_graphs) h->e.clear_graphs();
  return 0;
}

int sdxl_loss_fwd_bwd(sdxl_handle* h, const sdxl_loss_config* lc, const sdxl_batch* b, float grad_scale,
                      int first_micro, void* st) {
  CHK(sdxl_forward_loss(h, lc, b, st));
  return sdxl_backward_all(h, grad_scale, first_micro, st);
}

int sdxl_read_loss(sdxl_handle* h, float out[8], void* stp) {
  H_CHECK(h);
  CHK(ready(h->e));
  hipStream_t st = (hipStream_t)stp;
  HIP_CHECK_RET(hipMemcpyAsync(out, h->e.cur->F(h->e.cur->loss_off), 8 * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_CHECK_RET(hipStreamSynchronize(st));
  return 0;
}

int sdxl_unet_forward(sdxl_handle* h, const void* sample, const sdxl_batch* cond, void* pred, void* stp) {
  CHK(check_cond_request(cond));
  H_CHECK(h);
  Engine& e = h->e;
  hipStream_t st = (hipStream_t)stp;
  CHK(ready(e));
  CHK(check_batch(e, cond));
  Plan& p = *e.cur;
  const float* icond;
  CHK(check_input_cond(e, cond, cond->sampler != nullptr, &icond));
  float *d_ehs, *d_pool;
  CHK(read_cond_request(e, cond, &d_ehs, &d_pool));
  ResidualReq res;
  CHK(read_residuals(cond, e.num_skips(), &res));
  float* d_input;
  CHK(read_input_grad(cond, e.cfg.block_out_channels[0], &d_input));
  if (cond->sampler) {      // a sampling step: the forward runs on what the plan's input buffer holds, the step kernel writes the next input there
    SamplerP q;
    CHK(fill_sampler(cond->sampler, p.B, p.H * p.W, q));
    ARG_CHECK(sample == nullptr && pred == nullptr, "sampler: sample and pred must be NULL (the step reads and writes the plan's own buffers)");
    q.pred = p.P(p.pred); q.x_in = p.P(p.x_in); q.part = p.F(p.samp_part_off);
    if (!q.init) {
      CHK(upload_cond(e, cond, st));
      e.res_fwd = res.present ? &res : nullptr;
      const int rc = run_forward_ops(e, st);
      e.res_fwd = nullptr;
      CHK(rc);
    }
    return launch_sampler_step(q, st, icond, icond ? e.cfg.in_channels - 4 : 0);
  }
  CHK(upload_cond(e, cond, st));
  h->step.d_ehs = d_ehs; h->step.d_pool = d_pool;
  h->step.awaiting_bwd = false;      // (this forward replaced the loss step's activations: nothing waits for that backward any more)
  const size_t rows = (size_t)p.B * p.H * p.W;      // (input_cond is not read here: the caller's sample carries every channel)
  HIP_CHECK_RET(hipMemcpyAsync(p.P(p.x_in), sample, rows * input_cs(e.cfg.in_channels) * sizeof(bf16), hipMemcpyDeviceToDevice, st));
  e.res_fwd = res.present ? &res : nullptr;
  const int rc = run_forward_ops(e, st);
  e.res_fwd = nullptr;
  CHK(rc);
  h->step.res = std::move(res);
  h->step.d_input = d_input;
  if (pred) HIP_CHECK_RET(hipMemcpyAsync(pred, p.P(p.pred), rows * 8 * sizeof(bf16), hipMemcpyDeviceToDevice, st));
  return 0;
}

int sdxl_unet_backward(sdxl_handle* h, const void* dpred, int first_micro, void* stp) {
  H_CHECK(h);
  Engine& e = h->e;
  hipStream_t st = (hipStream_t)stp;
  CHK(ready(e));
  Plan& p = *e.cur;
  size_t bytes = (size_t)p.B * p.H * p.W * 8 * sizeof(bf16);
  HIP_CHECK_RET(hipMemcpyAsync(p.G(p.pred), dpred, bytes, hipMemcpyDeviceToDevice, st));
  set_cond_request(h, false);
  for (int k = 0; k < e.nseg; ++k) CHK(run_backward_segment(e, k, first_micro != 0, st));
  return copy_cond_grads(h, st);
}

int sdxl_grads_to_bf16(sdxl_handle* h, size_t off, size_t n, void* dst, float scale, void* st) {
  H_CHECK(h);
  ARG_CHECK(h->e.grads && off + n <= h->e.param_elems, "range out of bounds");
  return launch_f32_to_bf16(h->e.grads + off, (bf16*)dst, (long)n, scale, (hipStream_t)st);
}

// bf16 cast of the SMALL parameter ranges (biases, norm weights: the fp32 += accumulators) inside [off, off + n): what is
// left to cast when the weight-gradient GEMMs emit bf16 themselves (sdxl_set_grad_emit)
__global__ void cast_small_ranges_kernel(const float* __restrict__ g, bf16* __restrict__ dst, const unsigned long long* __restrict__ ranges,
                                         unsigned long long lo, unsigned long long hi, float scale) {
  const unsigned long long off = ranges[2 * blockIdx.x], n = ranges[2 * blockIdx.x + 1];
  if (off < lo || off + n > hi) return;
  for (unsigned long long i = threadIdx.x; i < n; i += blockDim.x) dst[off - lo + i] = (bf16)(g[off + i] * scale);
}
static int small_ranges_on_device(Engine& e) {
  if (!e.small_ranges_dev) {
    std::vector<unsigned long long> flat;
    for (auto& r : e.small_ranges) { flat.push_back(r.first); flat.push_back(r.second); }
    HIP_CHECK_RET(hipMalloc((void**)&e.small_ranges_dev, flat.size() * sizeof(unsigned long long)));
    HIP_CHECK_RET(hipMemcpy(e.small_ranges_dev, flat.data(), flat.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
  }
  return 0;
}
int sdxl_small_grads_to_bf16(sdxl_handle* h, size_t off, size_t n, void* dst, float scale, void* st) {
  H_CHECK(h);
  Engine& e = h->e;
  ARG_CHECK(e.grads && off + n <= e.param_elems && dst, "range out of bounds");
  CHK(small_ranges_on_device(e));
  if (e.small_ranges.empty()) return 0;
  hipLaunchKernelGGL(cast_small_ranges_kernel, dim3((unsigned)e.small_ranges.size()), dim3(256), 0, (hipStream_t)st, e.grads, (bf16*)dst,
                     e.small_ranges_dev, (unsigned long long)off, (unsigned long long)(off + n), scale);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
int sdxl_set_grad_emit(sdxl_handle* h, void* bf16_arena, float scale) {
  H_CHECK(h);
  ARG_CHECK(((uintptr_t)bf16_arena & 15) == 0, "bf16 gradient arena must be 16-byte aligned");
  ARG_CHECK(bf16_arena == nullptr || h->e.lora.ops.empty(), "lora: a bf16 emit arena cannot be combined with adapter gradients from the backward (sdxl_grad_select.lora)");
  if (h->e.emit_base != (bf16*)bf16_arena || h->e.emit_scale != scale) h->e.clear_graphs();   // captured wgrad launches hold the old target
  h->e.emit_base = (bf16*)bf16_arena;
  h->e.emit_scale = scale;
  return 0;
}

int sdxl_grad_sumsq(sdxl_handle* h, float* out, void* st) {
  H_CHECK(h);
  ARG_CHECK(h->e.grads, "grads are not bound");
  HIP_CHECK_RET(hipMemsetAsync(out, 0, sizeof(float), (hipStream_t)st));
  return launch_sumsq_f32(h->e.grads, (long)h->e.param_elems, out, (hipStream_t)st);
}

int sdxl_sumsq(const void* x, int dtype, size_t n, float* out, void* st) {
  ARG_CHECK(x && out && (dtype == 0 || dtype == 1), "sumsq: bad arguments");
  ARG_CHECK(((uintptr_t)x & 15) == 0, "sumsq: x must be 16-byte aligned");
  HIP_CHECK_RET(hipMemsetAsync(out, 0, sizeof(float), (hipStream_t)st));
  return dtype == 0 ? launch_sumsq_f32((const float*)x, (long)n, out, (hipStream_t)st)
                    : launch_sumsq_bf16((const bf16*)x, (long)n, out, (hipStream_t)st);
}
int sdxl_clip_coef(const float* sumsq_dev, float max_norm, float* coef_dev, void* st) {
  ARG_CHECK(sumsq_dev && coef_dev && max_norm > 0.f, "clip_coef: bad arguments");
  return launch_clip_coef(sumsq_dev, max_norm, coef_dev, (hipStream_t)st);
}

// ---- row f1: fused AdamW_BF16 ----
static float bf16_round_host(float x) {
  unsigned u;
  memcpy(&u, &x, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  u &= 0xFFFF0000u;
  memcpy(&x, &u, 4);
  return x;
}
int sdxl_adamw_default_config(sdxl_adamw_config* c) {
  ARG_CHECK(c, "null config");
  memset(c, 0, sizeof(*c));
  c->lr = 1e-4; c->beta1 = 0.9; c->beta2 = 0.999; c->eps = 1e-8;   // AdamWBF16.__init__ defaults (:31-36)
  c->step = 1.0;
  c->reference_ema = 1;
  return 0;
}
// what both algorithms of sdxl_adamw_bf16_step check, then fill in the same way (`who` in front of the hyper-parameter message):
// python doubles -> the float32 / bf16 scalars torch's ops on bf16 tensors use
static int fill_optim(OptimP& q, void* p, const void* grad, int grad_dtype, void* m, void* v, size_t n, const sdxl_adamw_config* c,
                      const float* grad_scale_dev, bool own_ok, const char* who) {
  ARG_CHECK(own_ok && c->beta1 >= 0.0 && c->beta1 < 1.0 && c->beta2 >= 0.0 && c->beta2 < 1.0 && c->eps >= 0.0,
            "%s: invalid hyper-parameters", who);
  q.p = (bf16*)p; q.m = (bf16*)m; q.v = (bf16*)v; q.n = n;
  if (grad_dtype == 0) q.grad_f32 = (const float*)grad; else q.grad_bf16 = (const bf16*)grad;
  q.beta1 = (float)c->beta1; q.beta2 = (float)c->beta2;
  q.one_minus_beta2 = (float)(1.0 - c->beta2);
  q.eps_bf16 = bf16_round_host((float)c->eps);
  q.grad_round_bf16 = c->grad_round_bf16;
  q.grad_scale = grad_scale_dev;
  q.ema = c->ema; q.ema_omd = c->ema_one_minus_decay;
  return 0;
}
// algorithm 1 of sdxl_adamw_bf16_step: every argument error is reported before anything touches the device
static int sf_kahan_step(void* p, const void* grad, int grad_dtype, void* m, void* v, void* kahan_comp, size_t n, const sdxl_adamw_config* c,
                         const float* grad_scale_dev, const unsigned short* rand_inject, hipStream_t st) {
  ARG_CHECK(rand_inject == nullptr, "schedule-free: rand_inject must be NULL (the update has no random rounding)");
  ARG_CHECK(c->kahan_sum == 0 || kahan_comp != nullptr, "schedule-free: kahan_sum needs the kahan_comp arena (shift argument)");
  SfkP q;
  memset(&q, 0, sizeof(q));
  CHK(fill_optim(q, p, grad, grad_dtype, m, v, n, c, grad_scale_dev,
                 c->weight_decay >= 0.0 && c->sf_step_size >= 0.0 && std::isfinite(c->sf_step_size), "schedule-free"));
  q.c = c->kahan_sum ? (bf16*)kahan_comp : nullptr;
  // the scalars of torch's ops as tests/_schedulefree_ref.py has them
  const double ss = c->sf_step_size, wd = c->weight_decay;
  q.one_minus_beta1_bf16 = bf16_round_host((float)(1.0 - c->beta1));
  q.has_wd = wd != 0.0;
  q.wd_alpha_bf16 = bf16_round_host((float)-wd);
  q.neg_step = (float)-ss;
  q.step = (float)ss;
  q.decay = (float)(ss * wd);
  return launch_sfk(q, c->sf_reference, st);
}
// algorithm 2 of sdxl_adamw_bf16_step (Prodigy): every argument error is reported before anything touches the device, and every
// message names the algorithm
static int prodigy_step(void* p, const void* grad, int grad_dtype, void* m, void* v, void* comp, size_t n, const sdxl_adamw_config* c,
                        const float* grad_scale_dev, const unsigned short* rand_inject, hipStream_t st) {
  const char* who = "prodigy (algorithm 2)";
  ARG_CHECK(rand_inject == nullptr, "%s: rand_inject must be NULL (the update has no random rounding)", who);
  ARG_CHECK(c->beta3 >= 0.0 && c->beta3 < 1.0, "%s: beta3 %g must lie in [0, 1)", who, c->beta3);
  ARG_CHECK(c->d0 > 0.0 && std::isfinite(c->d0), "%s: d0 %g must be finite and > 0", who, c->d0);
  ARG_CHECK(c->d_coef > 0.0 && std::isfinite(c->d_coef), "%s: d_coef %g must be finite and > 0", who, c->d_coef);
  ARG_CHECK(c->growth_rate >= 1.0, "%s: growth_rate %g must be >= 1", who, c->growth_rate);
  ARG_CHECK(std::isfinite(c->prodigy_bc) && c->prodigy_bc > 0.0, "%s: prodigy_bc %g must be finite and > 0", who, c->prodigy_bc);
  ARG_CHECK(c->lr >= 0.0 && std::isfinite(c->lr), "%s: lr %g must be finite and >= 0", who, c->lr);
  ARG_CHECK(c->weight_decay >= 0.0 && std::isfinite(c->weight_decay), "%s: weight_decay %g must be finite and >= 0", who, c->weight_decay);
  ProdigyP q;
  memset(&q, 0, sizeof(q));
  CHK(fill_optim(q, p, grad, grad_dtype, m, v, n, c, grad_scale_dev, true, who));
  q.m32 = (float*)m; q.v32 = (float*)v; q.s = c->s;
  q.c = (bf16*)comp; q.p0 = (const bf16*)c->p0; q.state = c->prodigy_state;
  // host doubles rounded to float once
  q.lr = (float)c->lr; q.bc = (float)c->prodigy_bc;
  q.one_minus_beta1 = (float)(1.0 - c->beta1);
  q.beta3 = (float)c->beta3; q.eps = (float)c->eps;
  q.d0 = (float)c->d0; q.d_coef = (float)c->d_coef; q.growth = (float)c->growth_rate;
  q.wd = (float)c->weight_decay;
  q.safeguard = c->safeguard_warmup != 0;
  return launch_prodigy(q, st);
}
// algorithm 3 of sdxl_adamw_bf16_step (Adafactor).  The device copy of the table (the caller's entries plus their places in the work-item
// prefix tables and in the scratch) is cached, keyed by the entries, the device and the two buffers the copy points into, as the
// LoRA table is per handle; this call has no handle, so one table per process, under a lock
struct AfCache {
  std::vector<sdxl_adafactor_tensor> key;
  int device = -1;
  float *state = nullptr, *scratch = nullptr;
  AfTensor* dev = nullptr;
  int tiles = 0, chunks = 0;
};
static AfCache af_cache;
static std::mutex af_mutex;
static_assert(AF_ROWS == SDXL_AF_ROWS && AF_COLS == SDXL_AF_COLS, "the geometry and the scratch formula of include/sdxlstep.h");
// the entries checked against n, then as the kernels read them; every message names the entry
static int adafactor_table(const sdxl_adafactor_tensor* in, int nt, size_t n, float* state, float* scratch, const char* who,
                           std::vector<AfTensor>& tab, long* tiles_, long* chunks_) {
  tab.assign((size_t)nt, AfTensor());
  size_t end = 0, sc = 4 * (size_t)nt;
  long tiles = 0, chunks = 0;
  for (int i = 0; i < nt; ++i) {
    const sdxl_adafactor_tensor& e = in[i];
    ARG_CHECK(e.rows >= 1 && e.cols >= 8 && e.cols % 8 == 0, "%s: entry %d is [%d][%d]: rows must be >= 1 and cols a positive multiple of 8", who, i,
              e.rows, e.cols);
    const size_t span = (size_t)e.rows * (size_t)e.cols;
    ARG_CHECK(e.elem_off % 8 == 0, "%s: entry %d starts at element %zu, not a multiple of 8", who, i, e.elem_off);
    ARG_CHECK(e.elem_off >= end, "%s: entry %d starts at element %zu, before the end %zu of entry %d: the entries must be sorted and must not overlap",
              who, i, e.elem_off, end, i - 1);
    ARG_CHECK(e.elem_off <= n && span <= n - e.elem_off, "%s: entry %d covers elements %zu .. %zu, past n = %zu", who, i, e.elem_off, e.elem_off + span, n);
    ARG_CHECK(e.numel >= 1 && e.numel <= span, "%s: entry %d has numel %zu outside 1 .. rows*cols = %zu", who, i, e.numel, span);
    ARG_CHECK(e.factored == 0 || e.factored == 1, "%s: entry %d has factored = %d (0 or 1)", who, i, e.factored);
    ARG_CHECK(e.state_off % 4 == 0, "%s: entry %d has state_off %zu, not a multiple of 4 floats", who, i, e.state_off);
    end = e.elem_off + span;
    AfTensor& t = tab[(size_t)i];
    t.elem_off = e.elem_off; t.numel = e.numel; t.rows = e.rows; t.cols = e.cols; t.factored = e.factored;
    t.ncb = (e.cols + AF_COLS - 1) / AF_COLS; t.nrb = (e.rows + AF_ROWS - 1) / AF_ROWS;
    t.nrc = e.factored ? (e.rows + 255) / 256 : 0; t.ncc = e.factored ? (e.cols + 255) / 256 : 0;
    t.tile0 = (int)tiles; t.chunk0 = (int)chunks;
    const size_t T = (size_t)t.nrb * t.ncb;
    tiles += (long)T; chunks += t.nrc + t.ncc;
    ARG_CHECK(tiles < (1L << 31) && chunks < (1L << 31), "%s: entry %d: too many tiles", who, i);
    t.R = state + e.state_off; t.C = t.R + e.rows;
    t.sx = scratch + sc; sc += T;
    t.su = scratch + sc; sc += T;
    if (e.factored) {
      t.rch = scratch + sc; sc += (size_t)t.nrc;
      t.rowp = scratch + sc; sc += (size_t)e.rows * t.ncb;
      t.colp = scratch + sc; sc += (size_t)t.nrb * e.cols;
    }
  }
  *tiles_ = tiles; *chunks_ = chunks;
  return 0;
}
static int adafactor_step(void* p, const void* grad, int grad_dtype, void* m, void* v, void* comp, size_t n, const sdxl_adamw_config* c,
                          const float* grad_scale_dev, const unsigned short* rand_inject, hipStream_t st) {
  const char* who = "adafactor (algorithm 3)";
  ARG_CHECK(v == nullptr, "%s: v must be NULL (the second moment is factored and lives in af_state: unlike algorithm 2 there is no arena-sized v)", who);
  ARG_CHECK(rand_inject == nullptr, "%s: rand_inject must be NULL (the update has no random rounding)", who);
  ARG_CHECK(c->clip_threshold > 0.0 && std::isfinite(c->clip_threshold), "%s: clip_threshold %g must be finite and > 0", who, c->clip_threshold);
  ARG_CHECK(c->beta2t >= 0.0 && c->beta2t < 1.0, "%s: beta2t %g must lie in [0, 1)", who, c->beta2t);
  ARG_CHECK(std::isfinite(c->rho), "%s: rho %g must be finite", who, c->rho);
  ARG_CHECK(c->eps1 >= 0.0 && std::isfinite(c->eps1) && c->eps2 >= 0.0 && std::isfinite(c->eps2), "%s: eps1 %g and eps2 %g must be finite and >= 0", who,
            c->eps1, c->eps2);
  ARG_CHECK(c->weight_decay >= 0.0 && std::isfinite(c->weight_decay), "%s: weight_decay %g must be finite and >= 0", who, c->weight_decay);
  ARG_CHECK(!c->use_beta1 || (c->beta1 >= 0.0 && c->beta1 < 1.0), "%s: beta1 %g must lie in [0, 1)", who, c->beta1);
  ARG_CHECK((c->use_beta1 != 0) == (m != nullptr), "%s: m must be the fp32 first moment with use_beta1 and NULL without it (missing or unexpected buffer)", who);
  ARG_CHECK(c->n_tensors >= 0 && (c->n_tensors == 0 || c->tensors != nullptr), "%s: missing buffers (tensors: %d entries)", who, c->n_tensors);
  ARG_CHECK(c->af_state && c->af_scratch, "%s: missing buffers (af_state, af_scratch)", who);
  ARG_CHECK((((uintptr_t)c->af_state | (uintptr_t)c->af_scratch) & 15) == 0, "%s: buffers must be 16-byte aligned", who);
  AdafactorP q;
  memset(&q, 0, sizeof(q));
  q.p = (bf16*)p; q.m = (bf16*)(m ? m : p); q.v = (bf16*)p; q.n = n;        // (m, v: addresses for the shared checks only)
  if (grad_dtype == 0) q.grad_f32 = (const float*)grad; else q.grad_bf16 = (const bf16*)grad;
  q.grad_round_bf16 = c->grad_round_bf16;
  q.grad_scale = grad_scale_dev;
  q.ema = c->ema; q.ema_omd = c->ema_one_minus_decay;
  q.c = (bf16*)comp; q.m32 = (float*)m; q.scal = c->af_scratch;
  // host doubles rounded to float once
  q.beta1 = (float)c->beta1; q.omb1 = (float)(1.0 - c->beta1);
  q.eps1 = (float)c->eps1; q.eps2 = (float)c->eps2; q.clip = (float)c->clip_threshold;
  q.b2t = (float)c->beta2t; q.omb2t = (float)(1.0 - c->beta2t); q.rho = (float)c->rho; q.wd = (float)c->weight_decay;
  q.scale_parameter = c->scale_parameter != 0;
  q.n_tensors = c->n_tensors;
  std::vector<AfTensor> tab;
  long tiles = 0, chunks = 0;
  CHK(adafactor_table(c->tensors, c->n_tensors, n, c->af_state, c->af_scratch, who, tab, &tiles, &chunks));
  q.tiles = (int)tiles; q.chunks = (int)chunks;
  {                                                                        // the buffer checks of the launch, with nothing to launch
    AdafactorP none = q;
    none.n_tensors = 0;
    CHK(launch_adafactor(none, st));
  }
  if (q.n_tensors == 0 || n == 0) return 0;
  std::lock_guard<std::mutex> lock(af_mutex);
  int device = -1;
  HIP_CHECK_RET(hipGetDevice(&device));
  AfCache& k = af_cache;
  const bool hit = k.dev && k.device == device && k.state == c->af_state && k.scratch == c->af_scratch && k.key.size() == (size_t)c->n_tensors &&
                   memcmp(k.key.data(), c->tensors, sizeof(sdxl_adafactor_tensor) * (size_t)c->n_tensors) == 0;
  if (!hit) {
    if (k.dev) (void)hipFree(k.dev);
    k.dev = nullptr;
    HIP_CHECK_RET(hipMalloc((void**)&k.dev, tab.size() * sizeof(AfTensor)));
    HIP_CHECK_RET(hipMemcpy(k.dev, tab.data(), tab.size() * sizeof(AfTensor), hipMemcpyHostToDevice));
    k.key.assign(c->tensors, c->tensors + c->n_tensors);
    k.device = device; k.state = c->af_state; k.scratch = c->af_scratch;
  }
  q.table = k.dev;
  return launch_adafactor(q, st);
}
int sdxl_adamw_bf16_step(void* p, const void* grad, int grad_dtype, void* m, void* v, void* shift, size_t n,
                         const sdxl_adamw_config* c, const float* grad_scale_dev, const unsigned short* rand_inject,
                         void* st) {
  ARG_CHECK(c, "null config");
  ARG_CHECK(grad_dtype == 0 || grad_dtype == 1, "adamw: grad_dtype %d (0 = fp32, 1 = bf16)", grad_dtype);
  ARG_CHECK(c->algorithm >= 0 && c->algorithm <= 3,
            "adamw: algorithm %d (0 = AdamW_BF16, 1 = schedule-free Kahan, algorithm 2 = Prodigy, algorithm 3 = Adafactor)", c->algorithm);
  ARG_CHECK(c->ema == nullptr || (c->ema_one_minus_decay >= 0.f && c->ema_one_minus_decay <= 1.f),
            "adamw: ema_one_minus_decay %g must lie in [0, 1]", (double)c->ema_one_minus_decay);
  if (c->algorithm == 1) return sf_kahan_step(p, grad, grad_dtype, m, v, shift, n, c, grad_scale_dev, rand_inject, (hipStream_t)st);
  if (c->algorithm == 2) return prodigy_step(p, grad, grad_dtype, m, v, shift, n, c, grad_scale_dev, rand_inject, (hipStream_t)st);
  if (c->algorithm == 3) return adafactor_step(p, grad, grad_dtype, m, v, shift, n, c, grad_scale_dev, rand_inject, (hipStream_t)st);
  AdamWP q;
  memset(&q, 0, sizeof(q));
  CHK(fill_optim(q, p, grad, grad_dtype, m, v, n, c, grad_scale_dev, c->step >= 1.0, "adamw"));
  q.shift = (bf16*)shift;
  // scalars exactly as the reference's python floats reach the torch kernels: double arithmetic, then float32
  q.one_minus_beta1 = (float)(1.0 - c->beta1);
  q.value = (float)(-c->lr * sqrt(1.0 - pow(c->beta2, c->step)));
  q.decay_alpha_bf16 = c->decay_this_iteration > 0.0 ? bf16_round_host((float)-c->decay_this_iteration) : 0.f;
  q.reference_ema = c->reference_ema;
  q.rand = rand_inject;
  q.seed_lo = (unsigned)c->seed; q.seed_hi = (unsigned)(c->seed >> 32);
  q.step_counter = (unsigned)c->step;
  q.elem_offset = (size_t)c->elem_offset;
  return launch_adamw_bf16(q, (hipStream_t)st);
}
int sdxl_adamw_decay(void* shift, const void* p, size_t n, float decay, void* st) {
  ARG_CHECK(shift && p, "adamw decay: missing buffers");
  if (decay <= 0.f) return 0;
  return launch_adamw_decay((bf16*)shift, (const bf16*)p, n, bf16_round_host(-decay), (hipStream_t)st);
}
}  // extern "C"
