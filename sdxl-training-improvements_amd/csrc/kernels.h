// Launcher declarations for every hand-written gfx950 kernel family of the SDXL training step.
// All tensors are bf16, token-major ("NHWC"): an activation is a row-major [rows = B*H*W, C] matrix.
// All launchers are stream-ordered and return 0 on success (non-zero + sdxl_last_error() otherwise).
#pragma once
#include "common.h"

// experiment knobs (sdxl_set_knob / bench.py --knob id=value; 0 = the shipped policy everywhere):
//   0 wave priority of the main-stream dgrad GEMMs in the backward, 1 of the attention backward kernels
//   2 = 1: no split of the one-round 3x3 convolutions' reduction; = 16: every side-stream leaf behind its own fork event;
//       = 4 / 8 / 12: the same split for the long linear dgrads / forward projections / both
//       = 64: upsampler convolutions on the upsampled image; = 128: only their weight gradient; = 256: stride-2 dgrad through the general
//       gather; = 512: stride-2 forward / weight gradient on phase planes (OFF by default: neutral in the step)
//   3, 4 split-K factor of the long linear dgrads and its N threshold; 5 = 80: GEGLU packed in groups of 80
//   6, 7 forced configuration of the linear / conv dgrads, 8 N threshold of knob 6
//   9 = 1: no wgrad256 kernel; 10 = 1: LayerNorm backward as lean dx kernel + parameter-gradient leaf pass (0 / 2: dx and parameter partials in one pass, shipped), 3: lean + the atomic column-sum pass; 11 = 1: the round-2 LayerNorm dx kernel
//   12 = 1: no three-tap conv weight gradient; 13 split-K workgroup target of conv_wgrad3 / wgrad256 (144); 14 = 2: its W = 32 form
//   15 = 1: no half-height tail workgroups in the 256 x 256 kernel
//   16 co-resident 256-row kernel for the level-2 linear weight gradients: 0 policy, 1 off, 2 / 3 = 128 / 160-column tiles wherever allowed;
//   17 its split-K workgroup target for long reductions (0: 256); 19 = 1: also the 16 384-row level's linear weight gradients on it; 20 = 1: self-attention backward as two launches (dQ, then dK / dV); 23: loop of the co-resident 256-row kernel's 128-column tiles: 0 / 1 lockstep (shipped), 5 phased everywhere (rounds 4-5), 2 phased only for >= 256 tiles, 3 / 4 phased + 160-column tiles for >= 8192 rows / wherever they divide; 22 configuration of the GEGLU (FF2) dgrad; 21 = 1: Delta always from its own pass; 18 = 1: no padding columns on the feed-forward hidden tensors
//   24 = 1: GroupNorm backward partial sums by the LDS-free row-lane kernel (neutral in the step: r04i_ab_gn_nolds.txt)
//   37 problems per grouped weight-gradient launch (0: 256 / tiles = 3 for the 1280 x 1280 ones; 1 = alone with their split-K, 2, 4)
//   36 workgroup target of the cross-attention dK / dV kernel's query split (0: the shipped 160; 640 = rounds 2 - 4)
//   25 LayerNorm backward knock-outs (timing only, wrong gradients): 1 no dgamma / dbeta pass, 2 no dx pass either, 3 no dx pass
//   26 LayerNorm backward in the consumer's dgrad epilogue (GemmP::ln_x): 0 separate passes (shipped), 1 fused (dx + dgamma | dbeta partials), 2 fused dx, dy stored and the parameter pass kept
//   27 timing knock-outs by op type (bit mask, wrong results): 1 GroupNorm backward, 2 GroupNorm forward, 4 LayerNorm forward, 8 cross-attention
//      backward, 16 self-attention backward, 32 self-attention forward, 64 cross-attention forward; 128 / 256 GroupNorm / LayerNorm forward replaced by ONE elementwise launch
//      (live data downstream: the skipped ops leave stale zeros behind, and a chip at its power cap runs zeros ~5 % faster -- profiles/r05t_knockouts_live_data.txt)
//   28 wave priority (s_setprio 0..3) of the LayerNorm backward dx kernel
//   30 pipelined one-wave-per-SIMD kernels, bit mask (0 = the shipped policy = 3; 64 = none): 1 = the forward's one-round linear problems on gemm_pl.hip, 2 = the one-round linear dgrads,
//      16 = every plain linear NT / NN problem whose tiles are whole rounds of 256, 1024 = the FORWARD ones of those with more than one round, 32 = every plain linear NT / NN problem;
//      4 = the one-round 3x3 convolutions forward on gemm.hip's configuration 5 / 6 (unsplit instead of two co-resident halves), 8 = their dgrads
//   31 = 1: gemm_pl.hip WITH its L2 prefetch wave (measured: no gain)
//   32 = 1: attention workgroups in plain (block, pair) order instead of the XCD-aware one
//   33 attention forward kernel (Nk >= 256): 0 = the tiled kernel of attention.hip (shipped), 2 = the software-pipelined kernel of attention_pl.hip
//      (4 waves, one per SIMD, 512 registers): parity-green, at parity in time (profiles/r06f_attn_ab.txt)
//   35 self-attention backward: 0 policy (attention_bwd_pl.hip for Nq, Nk >= 2048, attn_bwd_fused_kernel below), 1 = attn_bwd_fused_kernel everywhere, 2 = pipelined wherever it applies
//   34 = 1: no generic XCD order (xcd_seq_map) in the weight-gradient kernels: identity where no XCD rectangle fits, = 2: the generic order also where a rectangle fits (cr256)
//   38 LDS KiB requested per workgroup of the co-resident 256-row weight-gradient kernel (0: the shipped 84 = one per CU + room for the other stream; 1: its ring's own size = two per CU; N: N KiB)
//   39 = a + 1000 b: a KiB of LDS per workgroup of the 128-row kernel's NN (dgrad) launches, b KiB for its TN launches (one per CU; measured: +12 / +1.1 ms)
//   29 = 1: weight-gradient GEMMs that use no split-K slab and whose operands come from the caller's stream are launched any-order on the side stream
// The product library has NO knobs: KNOB(i) is the constant 0 (= the shipped policy) and every experiment branch below it folds away.
// The diagnostics build (`build.py --diag`: -DSDXL_DIAG -> libsdxlstep_diag.so, include/sdxlstep_diag.h) keeps the table, sdxl_set_knob,
// the stream-K kernel (gemm_sk.hip), the stride-2 forward / weight gradient on phase planes (GemmP::up2 == 3) and the W = 32 three-tap form:
// measured, parity-tested experiments the step does not run (DESIGN.md sections 10, 11).
#define SDXL_NKNOBS 40
#ifdef SDXL_DIAG
extern int g_knobs[SDXL_NKNOBS];
#define KNOB(i) (g_knobs[(i)])
constexpr bool SDXL_DIAG_BUILD = true;
constexpr bool SDXL_UP2_3 = true;
constexpr bool SDXL_LN_EPILOGUE = true;
#else
#define KNOB(i) 0
constexpr bool SDXL_DIAG_BUILD = false;
constexpr bool SDXL_UP2_3 = false;
constexpr bool SDXL_LN_EPILOGUE = false;      // GemmP::ln_x (LayerNorm backward in the dgrad epilogue): measured, not shipped
#endif

// ------------------------------------------------------------------------------------------------
// bf16 MFMA GEMM family (gemm.hip).  C[M,N] = sum_k A(m,k) * B(k,n), fp32 accumulate.
//   NT: A [M][K] K-contiguous (optionally rows gathered from an image = implicit-GEMM conv),
//       B [N][K] K-contiguous                     -> Linear forward, conv3x3 forward
//   NN: A as NT, B [K][N] N-contiguous            -> Linear dgrad, conv3x3 dgrad
//   TN: A [K][M] M-contiguous, B [K][N] N-contiguous (optionally rows gathered) -> wgrad
// ------------------------------------------------------------------------------------------------
enum { GEMM_NT = 0, GEMM_NN = 1, GEMM_TN = 2 };
// kernel launch of a GemmP problem: in stream order, or (GemmP::anyorder) without the barrier against the stream's earlier launches
#define GEMM_LAUNCH(kernel, grid, block, smem, st, p)                                                          \
  do {                                                                                                         \
    if ((p).anyorder) hipExtLaunchKernelGGL(kernel, grid, block, smem, st, nullptr, nullptr, hipExtAnyOrderLaunch, p); \
    else hipLaunchKernelGGL(kernel, grid, block, smem, st, p);                                                 \
  } while (0)

#define GEMM_MAX_GROUP 4
struct GemmP {
  int form;
  const bf16* A;
  const bf16* B;
  void* C;
  int M, N, K;      // K = reduction length per tap (channels for conv forms, pixels for TN)
  long lda, ldb, ldc;
  // implicit-GEMM 3x3 gather (taps == 9).  The gathered operand's rows are pixels (b,y,x) of an
  // Hm x Wm image; tap (dy,dx) reads source pixel ((y*sm+dy-1)/sd, (x*sm+dx-1)/sd) of an Hs x Ws
  // image when divisible and in range, else zero.
  int taps;
  int Hm, Wm, Hs, Ws, sm, sd;
  int flip;            // NT/NN: weight tap index = flip ? 8-tap : tap
  // up2 (NT / NN, same-size stride-1 gather): a nearest-2x upsampling folded into the 3x3 convolution that follows it.  Output pixel
  // (2i + a, 2j + b) = phase 2a + b sees a 2 x 2 stencil (u, v) of the LOW-resolution input at (i + u - (1 - a), j + v - (1 - b)) whose
  // weights are sums of the nine taps (elementwise.hip: launch_upconv_fold_weights): weight entry e = 4 phase + 2u + v of a
  // [Cout][16][Cin] matrix (ldb = 16 Cin, b_tap_stride = Cin).  NT (forward): taps = 4, M = 4 x up_plane rows in PLANAR phase-major order
  // (row m: phase m / up_plane, low-resolution pixel m % up_plane; rows >= up_rows of a plane are padding), A = the low-resolution image.  NN (dgrad):
  // taps = 16, M = up_rows low-resolution pixels, A = the planar phase-major output gradient [4][up_plane][K], gathered at the mirrored offsets.
  int up2;             // 1: as above.  3 (NT, TN): a STRIDE-2 3x3 convolution on the four phase planes of its input (A resp. B = [4][up_plane][Cin]): tap
                       // (ky, kx) reads plane (ky != 1, kx != 1) at row / column offset -1 (ky, kx = 0) or 0; M resp. K = up_rows output pixels.
                       //  2 (NN only): the input gradient of a STRIDE-2 3x3 convolution by output phase -- M = 4 x up_plane planar
                       // rows, A = the low-resolution output gradient, plain [Cout][9][Cin] weights, taps = 4 (1 / 2 / 2 / 4 used by phase)
  int up_plane, up_rows;      // up2: rows per phase plane of the planar matrix (a multiple of 128, >= up_rows) and low-resolution pixels B Hm Wm
  long b_tap_stride;   // NT/NN: elements added to B per weight tap
  long c_tap_stride;   // TN: elements added to C per tap
  // epilogue, bf16 output:  C = acc + bias[n] + rowvec[m / rows_per_batch][n] + resid[m][n]
  const bf16* bias;
  const bf16* resid;
  long ldr;
  const bf16* rowvec;
  long ldv;
  int rows_per_batch;
  // GEGLU fused into the feed-forward GEMMs (bf16 output forms, tile width = 2 * group).  The 2*C4 columns of the first
  // projection are stored interleaved in groups of G = 64 or 80: column (c/G)*2G + c%G is the value half of channel c,
  // +G its gate half (the weight rows are packed in the same order), so one tile holds both halves of 64 channels.
  //   geglu == 1 (NT, N = 2*C4):  C = u (pre-activation, kept for the backward), aux[m][c] = value * gelu(gate)
  //   geglu == 2 (NN, N = C4):    acc = dG;  C[m][2*C4] = dU from aux = u:  d value = dG * gelu(gate),
  //                                                                        d gate  = dG * value * gelu'(gate)
  int geglu;
  int geglu_group;   // 64 (128-column tiles) or 80 (160-column tiles); 0 = 64
  bf16* aux;
  long ldaux;
  // NT / NN (bf16 output), taps == 1, no GEGLU, K % 64 == 0: splitk > 1 -> fp32 partial tiles to slab[split], then
  // splitk_epilogue_kernel sums them in a fixed order and applies bias / row vector / residual (small-M problems).
  // fp32 output (wgrad): C_f32 (+)= acc.  splitk > 1: each split writes its partial [M][N*taps] tile set to
  // slab[split] (plain stores) and a reduce kernel sums the slabs in a fixed order (deterministic, no atomics);
  // the conv form requires C to be the dense [M][taps*N] weight-gradient matrix (ldc == N*taps).
  int out_f32;
  int accumulate;
  int splitk;
  float* slab;     // gemm_slab_floats(M, N, taps, splitk): splitk * M * N * taps partial tiles + a [splitk][M] tail (bias-gradient partials)
  long slab_ld;    // set by the launcher
  // TN only, optional: the FINAL value (acc [+ C when accumulate]) * cb_scale goes out as bf16 to Cb (same [M][ldc] geometry as C)
  // and C itself is not written -- the gradient-exchange micro-step under data parallelism wants the bf16 comm arena, and
  // a separate cast pass over the 10 GB fp32 arena costs 3.4 ms per step (grouped launches: gCb[i])
  bf16* Cb;
  float cb_scale;
  float* bias_grad;  // TN only, optional: bias_grad[m] += sum_k A(k, m)  (column sums of dY, computed on the matrix pipe
                     // by the n-tile-0 / tap-0 workgroups with an all-ones B fragment).  Bitwise reproducible: an unsplit launch adds ONE
                     // value per element; a split launch stores the splits' sums as rows of the slab's tail and splitk_reduce_kernel adds
                     // them in a fixed order (gemm_bias_out below)
  // NN (bf16 output), 128-column tiles of the 4-wave kernel only (a wave then owns whole 64-column heads): the output is an attention
  // layer's dO; also write Delta[b * delta_heads + head][q] = sum_d dO[m][64 head + d] * O[m][64 head + d] (m = b * delta_nq + q, O = delta_o,
  // row stride delta_ldo) from the bf16-rounded output -- what attn_delta_kernel would compute in a pass of its own
  const bf16* delta_o;
  long delta_ldo;
  float* delta_out;
  int delta_nq, delta_heads;
  // (Diagnostics build only -- SDXL_LN_EPILOGUE; the product kernel has no such path.)  NN, plain bf16 epilogue, configuration 1 (128 x 128 tiles): this dgrad's output IS the output gradient dy of a LayerNorm (y = LN(x) feeds only
  // this linear layer).  With ln_x set the epilogue also runs that LayerNorm's backward: per-row partial sums (sum dy g, sum dy g xhat) of
  // the workgroup's columns -> ln_part[column tile][row] as 8-byte (value, tag) granules, write-through -> every workgroup of the row block
  // gathers the granules of all its column tiles, polling until they carry this launch's tag (ln_epoch: unique among the launches that
  // share ln_part since it was last zeroed) -> dx = rstd (dy g - S1 / N - xhat S2 / N) + addend, bf16, to ln_dx; and -- ln_pcol set -- the
  // block's dgamma | dbeta column partial sums to ln_pcol[row block][2][N] (folded later by ln_param_reduce_kernel).  C == nullptr: dy itself
  // is not stored.  N = the LayerNorm width <= 1280; launches of <= 512 workgroups only (all resident at once: the meeting cannot starve).
  const bf16* ln_x;        // the LayerNorm's input [M][N], row stride ln_ldx
  long ln_ldx;
  const float* ln_stats;   // [M][2] mean, rstd (forward)
  const bf16* ln_gamma;    // [N]
  bf16* ln_dx;             // [M][N], row stride ln_ldo
  const bf16* ln_addend;   // or nullptr
  long ln_ldo;
  float* ln_part;          // gemm_ln_part_floats(M, N) floats of scratch, 16-byte aligned, zeroed before epoch 1
  int ln_epoch;            // > 0
  float* ln_pcol;          // or nullptr: [gridDim.y][2][N]
  int xcd_px;      // set by the launcher: XCD grid width over n-tiles (0 = identity order)
  int xcd_bh;      // set by the launcher: band height of the generic XCD order (gemm_tiles.h: xcd_seq_map) where no px x py rectangle fits; 0 = off
  int tail_n0;     // 256 x 256 kernel, set by its launcher: > 0 = the tile columns from tail_n0 on are computed by HALF-HEIGHT workgroups
                   // (128 x 256: waves 4-7 only stage data) so that a launch of 2.5 rounds of tiles takes ~2.6 rounds, not 3
  int anyorder;    // host side, experiment (knob 29): launch without the in-stream barrier (hipExtAnyOrderLaunch): the kernel depends on nothing the stream ran before it
  int cfg;         // > 0: this launch's configuration of the 128-row kernel (1, 2, 3, 13, 23), overriding the selection policy
  int prio;        // wave priority (s_setprio 0..3) of the whole kernel: the backward's critical-path launches (dgrad chain, caller's
                   // stream) outrank the co-resident weight-gradient workgroups of the side stream on every SIMD they share
  // grouped launch (TN, taps == 1, splitk == 1): `group` > 1 problems of one shape in one grid (blockIdx.z = problem i, which
  // uses gA[i], gB[i], gC[i], gbias_grad[i] in place of A, B, C, bias_grad).  Small weight gradients (1280 x 1280: 80 tiles)
  // fill the chip three at a time instead of each being cut into split-K slabs and reduced.
  int group;
  const bf16* gA[GEMM_MAX_GROUP];
  const bf16* gB[GEMM_MAX_GROUP];
  float* gC[GEMM_MAX_GROUP];
  float* gbias_grad[GEMM_MAX_GROUP];
  bf16* gCb[GEMM_MAX_GROUP];
};

// Bias-gradient value of row m from reduction split `split` (the kernels' epilogues call this from the one workgroup per row block and split
// that owns it).  Unsplit: the only writer of the element in this launch.  Split: row `split` of the slab's tail, folded by splitk_reduce_kernel.
__device__ __forceinline__ void gemm_bias_out(float* bias_grad, float* slab, long slab_ld, int splitk, int split, int M, int m, float v) {
  if (splitk > 1) slab[(long)splitk * M * slab_ld + (long)split * M + m] = v;
  else atomicAdd(bias_grad + m, v);
}
int gemm_pick_group(int M, int N, int taps, long red, int splitk);   // problems per grouped wgrad launch (1 = launch alone)
size_t gemm_slab_floats(int M, int N, int taps, int splitk);
void gemm_defaults(GemmP* p);
int launch_gemm(const GemmP& p, hipStream_t st);
// What launch_gemm runs for a problem: decided by gemm_route (gemm.hip), the one place the selection policy lives; the launcher only obeys it.
enum { GEMM_K128 = 0, GEMM_K256, GEMM_KCR256, GEMM_KPL, GEMM_KWGRAD256, GEMM_KCONV_WGRAD3, GEMM_KSK };      // gemm_kernel | gemm256 | cr256 | gemm_pl | wgrad256 | conv_wgrad3 | stream-K (diagnostics build)
enum { GEMM_POST_NONE = 0, GEMM_POST_REDUCE, GEMM_POST_EPILOGUE };      // the pass over the split-K slabs: fp32 sum (weight gradients) | sum + bf16 epilogue
struct GemmRoute {
  int kernel;
  int cfg;        // GEMM_K128: 1, 2, 3, 13, 23, 5, 6 (43); GEMM_KCR256: 31 .. 36; GEMM_KPL: 7, 8 (with the prefetch wave); else 0
  bool fast;      // GEMM_K128: the FAST staging instantiation
  int post;
};
GemmRoute gemm_route(const GemmP& p);                 // p checked and normalised (as launch_gemm does first); no HIP call
int gemm_route_checked(GemmP p, GemmRoute* r);        // the same checks and normalisation as a launch, then gemm_route: 0, or the launch's argument error
// 256 x 256 tile, 8-phase kernel (gemm256.hip): M, N multiples of 256, K of 64, no 3x3 gather
bool gemm256_applicable(const GemmP& p);
void gemm_set_mode(int mode);   // bits 0-1: 0 never / 1 policy / 2 wherever applicable; bits 2..: force a 128-row configuration
bool gemm_use256(int form, int M, int N, int K, int splitk);   // the policy of mode 1
int gemm_pick_splitk(int M, int N, int taps, long red);        // split-K factor the wgrad launchers should request
int gemm_pick_splitk_small(int M, int N, int K, int kind = -1);               // split-K factor for NT / NN (bf16 output) launches of small problems
// the plan-time choices of the layers' launches, once for the plan and the single-kernel entry points (gemm.hip): the split-K factor of each
// launch WITH the condition under which it applies (1 = unsplit), and the geometry of a 3x3 convolution's three problems
int linear_wgrad_splitk(int Mo, int No, long rows);
int conv3x3_fwd_splitk(int B, int H, int W, int Cin, int Cout, int stride);
int conv3x3_dgrad_splitk(int B, int H, int W, int Cin, int Cout, int stride);
int conv3x3_wgrad_splitk(int B, int H, int W, int Cin, int Cout, int stride);
int upconv3x3_fwd_splitk(int B, int H, int W, int Cin, int Cout);       // B, H, W: the LOW-resolution image
int upconv3x3_dgrad_splitk(int B, int H, int W, int Cin, int Cout);
GemmP conv3x3_fwd_problem(int B, int H, int W, int Cin, int Cout, int stride);
GemmP conv3x3_dgrad_problem(int B, int H, int W, int Cin, int Cout, int stride);
GemmP conv3x3_wgrad_problem(int B, int H, int W, int Cin, int Cout, int stride);
// ... and a linear layer's three problems (w [N][K] dense; ld*: row strides of the activations), the epilogues that attach to them and the grouped
// weight gradient: the one place a GemmP of the linear family is assembled (LinearOp and the single-kernel entry points call these).  Pure: no
// HIP call, no policy -- split-K, slab, group size, cfg and accumulate are the caller's.
GemmP linear_fwd_problem(const bf16* x, long ldx, const bf16* w, void* y, long ldy, int M, int N, int K, const bf16* bias, const bf16* resid, long ldr);
GemmP linear_dgrad_problem(const bf16* dy, long ldy, const bf16* w, void* dx, long ldx, int M, int N, int K, const bf16* addend, long ldr);      // dx [M][N] = dy [M][K] . w [K][N]
GemmP linear_wgrad_problem(const bf16* dy, long ldy, const bf16* x, long ldx, float* dw, int Mo, int No, int rows, float* bias_grad);      // dw [Mo][No] = dy [rows][Mo]^T . x [rows][No]
void gemm_attach_geglu_fwd(GemmP& g, int group, bf16* gact, long ldgact);      // GemmP::geglu == 1
void gemm_attach_geglu_bwd(GemmP& g, int group, bf16* u, long ldu);            // GemmP::geglu == 2: also ldc = ldu
void gemm_attach_delta(GemmP& g, const bf16* o, long ldo, float* delta, int nq, int heads);      // GemmP::delta_out: also cfg = 1
void gemm_attach_ln_bwd(GemmP& g, const bf16* x, long ldx, const float* stats, const bf16* gamma, bf16* dx, const bf16* addend, float* part, int epoch,
                        float* pcol);      // GemmP::ln_x: also cfg = 0 and no resid
void gemm_fill_group(GemmP& g, const GemmP* v, int n);      // GemmP::group: g (= v[0]) launches the n problems of v in one grid
int launch_gemm256(const GemmP& p, hipStream_t st);
void gemm256_set_tail(bool on);     // half-height workgroups for the last partial round (default on; A/B runs)
#ifdef SDXL_DIAG
// persistent stream-K kernel (gemm_sk.hip): up to 4 problems (M, N multiples of 256, K of 64, no gather) in ONE launch, their
// K-steps cut evenly over the CUs; partial tiles are handed to the tile's owner inside the launch (fixed order: reproducible)
bool gemm_sk_applicable(const GemmP& p);
int launch_gemm_sk(const GemmP* problems, int n, hipStream_t st);
int launch_gemm_multi(const GemmP* problems, int n, hipStream_t st);   // = launch_gemm_sk + the per-launch profiling of launch_gemm
void gemm_set_sk_mode(int mode);                      // 0 never / 1 policy (gemm_use_sk) / 2 wherever applicable
int gemm_sk_mode();
bool gemm_use_sk(const GemmP& p);
void gemm_sk_set_workers(int n);                      // > 0: force the worker count (microbenchmarks), 0: policy
int gemm_ln_error(unsigned* out);                         // != 0: a LayerNorm-backward epilogue (GemmP::ln_x) gave up waiting for its row block's other tiles; clears it
int gemm_sk_error(hipStream_t st, unsigned* out);     // != 0: an owner gave up waiting for a partial tile (results invalid)
#endif
// 3x3 weight gradient, three taps per workgroup (conv_wgrad3.hip): same-size stride-1 convolutions whose image width is a multiple of 64
bool conv_wgrad3_applicable(const GemmP& p);
bool conv_wgrad3_policy(int M, int N, long red, int Wm, int stride);   // the plan's choice (long reductions: the 128^2 / 64^2 levels)
int conv_wgrad3_pick_splitk(int M, int N, long red);
int launch_conv_wgrad3(const GemmP& p, hipStream_t st);
void conv_wgrad3_set_enabled(bool on);
// long-reduction linear weight gradient, 256 x 160 tiles, 8 waves (wgrad256.hip)
bool wgrad256_applicable(const GemmP& p);
bool wgrad256_policy(int M, int N, long red);
int wgrad256_pick_splitk(int M, int N, long red);
int launch_wgrad256(const GemmP& p, hipStream_t st);
void wgrad256_set_enabled(bool on);
// co-resident 256-row tile, 8 waves, <= 78 KiB LDS, <= 128 registers (gemm_cr256.hip): linear NT / NN / TN problems, K % 32 == 0
bool cr256_applicable(const GemmP& p);
int launch_cr256(const GemmP& p, int bn, hipStream_t st, bool deep = false, bool phased = false);      // bn = 160 / 128 / 0 (pick); deep: exclusive 6-deep ring (diagnostics build)
int cr256_wgrad_cfg(int M, int N, long red, bool bias);
// software-pipelined one-wave-per-SIMD kernel (gemm_pl.hip): 128 x 160 / 128 x 128 x 64 tiles, 4 waves, 4-deep ring; linear NT / NN, plain bf16 epilogue
bool pl_applicable(const GemmP& p);
int launch_pl(const GemmP& p, int bn, hipStream_t st, bool prefetch = false);
int launch_pl_prefetch_b(const GemmP& p, int parts, hipStream_t st);      // diagnostics build: L2 prefetch of B for a coming launch_pl (another stream)      // bn = 160 / 128 / 0 (160 where N % 160 == 0)
int gemm_ln_cfg(int M, int N, int K);                  // GemmP::ln_x: the configuration such a launch takes (GemmP::cfg), 0 = not possible for this shape
size_t gemm_ln_part_floats(int M, int N);
size_t gemm_ln_pcol_floats(int M, int N);
int gemm_ln_rowblocks(int M);
int cr256_pick_splitk(int M, int N, long red, int cfg);        // the plan's choice for a linear weight gradient [M][N] over `red` rows: 0 / 31 / 32 (GemmP::cfg)
// per-launch HIP-event timing of every GEMM launch between begin and end (end synchronises the device)
int gemm_profile_begin();
FILE* launch_log();      // SDXL_LAUNCH_LOG (gemm.hip)
bool gemm_profiling();   // true between begin and end: the engine then runs everything on one stream (clean durations)
int gemm_profile_end(double* flops, double* ms, int* launches);

// ------------------------------------------------------------------------------------------------
// flash attention, head_dim 64 (attention.hip).  Q rows [B*Nq], K/V rows [B*Nk]; head h lives in
// columns [h*64, h*64+64) of each; row strides ldq/ldk/ldv/ldo in elements.  softmax scale 1/8.
// ------------------------------------------------------------------------------------------------
struct AttnP {
  const bf16 *Q, *K, *V;
  bf16* O;
  float* LSE;          // [B*H][Nq]  log-sum-exp of the scaled scores (natural log)
  int B, H, Nq, Nk;
  long ldq, ldk, ldv, ldo;
  // backward
  const bf16* dO;
  long lddo;
  bf16 *dQ, *dK, *dV;
  long lddq, lddk, lddv;
  float* Delta;        // [B*H][Nq]  rowsum(dO * O)
  int accumulate;      // dQ/dK/dV += (else =)
  // dK/dV kernel, short key sequences (cross attention, Nk = 77): the query loop is split over grid.z so the
  // kernel fills the chip; each split writes fp32 partials to `part` and a reduce kernel sums them (fixed order)
  int qsplit;
  float* part;         // qsplit * B*H * kvtiles*64 * 64 * 2 floats
  int prio;            // wave priority of the backward kernels (see GemmP::prio)
  int delta_ready;     // fused backward: Delta is already in place (written by the epilogue of the GEMM that produced dO, GemmP::delta_out)
  int xcd;             // set by the launchers: XCD-aware (block, pair) order of the workgroups (attention.hip: attn_xcd_map)
};
size_t attn_part_floats(int B, int H, int Nk, int qsplit);
int attn_pick_qsplit(int B, int H, int Nq, int Nk);
int launch_attn_fwd(const AttnP& p, hipStream_t st);
int launch_attn_fwd_tiled(const AttnP& p, hipStream_t st); // attention.hip: 128-query workgroups, three per CU (what launch_attn_fwd runs)
bool attn_fwd_pl_applicable(const AttnP& p);               // diagnostics build (attention_pl.hip): software-pipelined forward, Nk >= 256
int launch_attn_fwd_pl(const AttnP& p, hipStream_t st);
bool attn_bwd_pl_applicable(const AttnP& p);               // attention_bwd_pl.hip: software-pipelined dQ | dK | dV in one grid (Nq, Nk >= 256; Delta in place)
int launch_attn_bwd_pl(const AttnP& p, hipStream_t st);
int launch_attn_bwd(const AttnP& p, hipStream_t st);       // = dq, then dkv
int launch_attn_bwd_dq(const AttnP& p, hipStream_t st);
int launch_attn_bwd_dkv(const AttnP& p, hipStream_t st);
int launch_attn_bwd_fused(const AttnP& p, hipStream_t st);   // self-attention: Delta pass + dK / dV and dQ workgroups in one grid

// ------------------------------------------------------------------------------------------------
// normalisation (norm.hip)
// ------------------------------------------------------------------------------------------------
// GroupNorm over [B][HW][C] with G groups (+ optional SiLU).  stats: [B][G][2] = mean, rstd.
// ws: groupnorm_ws_floats(B, C, G) floats of scratch (may be shared by stream-ordered calls)
size_t groupnorm_ws_floats(int B, int C, int G);
int launch_groupnorm_fwd(const bf16* x, bf16* y, const bf16* gamma, const bf16* beta, float* stats,
                         float* ws, int B, int HW, int C, int G, float eps, int silu,
                         hipStream_t st);
// dx (+)= ; dgamma/dbeta fp32 += .  ws: same scratch
// dx = (addend ? addend : 0) + grad   (addend may alias dx; a distinct addend keeps gradient buffers write-once)
int launch_groupnorm_bwd(const bf16* x, const bf16* dy, const bf16* gamma, const bf16* beta,
                         const float* stats, bf16* dx, const bf16* addend, float* dgamma, float* dbeta, float* ws,
                         int B, int HW, int C, int G, int silu, hipStream_t st, float* prow = nullptr);
// LayerNorm over rows of [M][C]; stats [M][2] = mean, rstd
int launch_layernorm_fwd(const bf16* x, bf16* y, const bf16* gamma, const bf16* beta, float* stats, int M,
                         int C, float eps, hipStream_t st);
// dx = (addend ? addend : 0) + grad; with `part` (layernorm_bwd_part_floats(M, C) floats) also the per-block partial sums of
// dgamma | dbeta, which launch_ln_param_reduce folds into the fp32 gradients (+=) for a whole batch of LayerNorms at once
size_t layernorm_bwd_part_floats(int M, int C);
int launch_layernorm_bwd(const bf16* x, const bf16* dy, const bf16* gamma, const float* stats, bf16* dx,
                         const bf16* addend, float* part, int* nblk_out, int M, int C, hipStream_t st);
int launch_layernorm_param_grads(const bf16* x, const bf16* dy, const float* stats, float* dgamma, float* dbeta, int M, int C, hipStream_t st);
// the same sums as layernorm_param_partial_rows(M, C) partial rows part[rows][2][C] (plain stores, inside layernorm_bwd_part_floats(M, C));
// an LnRedEntry with nblk = that row count folds them into the gradients (launch_ln_param_reduce)
int layernorm_param_partial_rows(int M, int C);
int launch_layernorm_param_partials(const bf16* x, const bf16* dy, const float* stats, float* part, int M, int C, hipStream_t st);
#define LN_RED_MAX 64
struct LnRedEntry { const float* part; float* dgamma; float* dbeta; int nblk, C; };
struct LnRedBatch { LnRedEntry e[LN_RED_MAX]; int n; };   // passed by value as the kernel argument (2 KiB)
int launch_ln_param_reduce(const LnRedBatch& b, hipStream_t st);

// ------------------------------------------------------------------------------------------------
// elementwise / small (elementwise.hip)
// ------------------------------------------------------------------------------------------------
int launch_silu_fwd(const bf16* x, bf16* y, long n, hipStream_t st);
int launch_silu_bwd(const bf16* x, const bf16* dy, bf16* dx, const bf16* addend, long n, hipStream_t st);
int launch_add(const bf16* a, const bf16* b, bf16* o, long n, hipStream_t st);           // o = a + b
size_t colsum_part_floats(int batches, int rows, int N);
int launch_colsum_f32_batched(const bf16* x, float* out, int batches, int rows, int N, long ldx, long ld_out, float* part, hipStream_t st);  // out[b][n] += sum_m, fixed order
int launch_colsum_partials(const bf16* x, float* out, int batches, int rows, int N, long ldx, long ld_out, float* part, LnRedEntry* entries, hipStream_t st);
int launch_concat(const bf16* a, int Ca, const bf16* b, int Cb, bf16* o, long rows, hipStream_t st);
int launch_split_add(const bf16* g, bf16* ga, int Ca, const bf16* add_a, bf16* gb, int Cb, const bf16* add_b,
                     long rows, hipStream_t st);                                                  // concat backward
// residual.hip: the concat with an NCHW residual ra [B][Ca][HW] / rb [B][Cb][HW] (rdtype 0 fp32, 1 bf16; either may be null, both null =
// launch_concat) added to its half, and the fp32 NCHW gradient of such a residual: columns of the concat's output gradient g [B * HW][Ca + Cb]
// (exact zeros when *gate == 0; gate may be null).  Every non-null pointer 16-byte aligned.
int launch_concat_residual(const bf16* a, int Ca, const bf16* b, int Cb, const void* ra, const void* rb, int rdtype, bf16* o, int B, int HW,
                           hipStream_t st);
int launch_residual_grad(const bf16* g, int Ca, int Cb, float* da, float* db, const float* gate, int B, int HW, hipStream_t st);
// input_dgrad.hip: the input gradient of conv_in (sdxl_batch_din), dx [B][in_channels][H][W] fp32 NCHW =
// sum over taps and o of dy [B * H * W][Cout] (pixel y + 1 - ky, x + 1 - kx) . w [Cout][9][Cs] (Cs = input_cs(in_channels), zero pad channels),
// fp32 sums in a fixed order (no atomics); exact zeros, dy not read, when *gate == 0 (gate may be null).  Cout % 32 == 0, in_channels 1 .. 16,
// any B, H, W >= 1; dy, w, dx 16-byte aligned.  Not a GEMM route: a kernel and a launcher of its own.
int launch_input_dgrad(const bf16* dy, const bf16* w, float* dx, const float* gate, int B, int H, int W, int in_channels, int Cout, hipStream_t st);
int launch_upsample2x(const bf16* x, bf16* y, int B, int H, int W, int C, hipStream_t st);
// GemmP::up2 companions: the [Cout][16][Cin] stencil weights of a [Cout][9][Cin] kernel; planar phase-major <-> high-resolution layout
int launch_upconv_fold_weights(const bf16* w, bf16* weff, int Cout, int Cin, hipStream_t st);
int launch_pixel_shuffle2(const bf16* src, bf16* dst, int B, int H, int W, int C, int to_hi, hipStream_t st, const bf16* addend = nullptr);   // plane stride = upconv_plane_rows
static inline long upconv_plane_rows(int B, int H, int W) { return ((long)B * H * W + 127) / 128 * 128; }
int launch_upconv3x3_fwd(const bf16* x, const bf16* w, const bf16* bias, bf16* weff, bf16* planar, bf16* y, int B, int H, int W, int Cin,
                         int Cout, int splitk, float* slab, hipStream_t st);          // gemm.hip
#ifdef SDXL_DIAG
int launch_conv3x3_s2_fwd(const bf16* x, const bf16* w, const bf16* bias, bf16* xplanar, bf16* y, int B, int H, int W, int Cin, int Cout,
                          hipStream_t st);      // gemm.hip (GemmP::up2 == 3)
int launch_conv3x3_s2_wgrad(const bf16* dy, const bf16* xplanar, float* dw, float* dbias, bf16* emit, float emit_scale, int accumulate, int B,
                            int H, int W, int Cin, int Cout, int splitk, float* slab, hipStream_t st);
#endif
int launch_conv3x3_s2_dgrad(const bf16* dy, const bf16* w, bf16* planar, bf16* dx, const bf16* addend, int B, int H, int W, int Cin,
                            int Cout, int prio, hipStream_t st);      // gemm.hip (GemmP::up2 == 2)
int launch_upconv_unfold_grads(const float* dweff, float* dw, bf16* emit, float emit_scale, int accumulate, int Cout, int Cin, hipStream_t st);
int launch_upconv3x3_wgrad(const bf16* planar, const bf16* x, float* dweff, float* dw, float* dbias, bf16* emit, float emit_scale,
                           int accumulate, int B, int H, int W, int Cin, int Cout, int splitk, float* slab, hipStream_t st);
int launch_upconv3x3_dgrad(const bf16* dy, const bf16* weff, bf16* planar, bf16* dx, const bf16* addend, int B, int H, int W, int Cin,
                           int Cout, int splitk, float* slab, int prio, hipStream_t st);
int launch_upsample2x_bwd(const bf16* dy, bf16* dx, const bf16* addend, int B, int H, int W, int C, hipStream_t st);
// sinusoidal embedding, cos first: out[r][0:half]=cos(t*f_i), out[r][half:]=sin ; out row stride ldo
int launch_sincos(const float* t, bf16* out, int rows, int dim, long ldo, hipStream_t st);
int launch_copy_cols(const bf16* src, long lds, bf16* dst, long ldd, int rows, int cols, hipStream_t st);
int launch_f32_to_bf16(const float* x, bf16* y, long n, float scale, hipStream_t st);
int launch_bf16_to_f32(const bf16* x, float* y, long n, hipStream_t st);
int launch_sumsq_f32(const float* x, long n, float* out /* += */, hipStream_t st);
int launch_sumsq_bf16(const bf16* x, long n, float* out /* += */, hipStream_t st);
int launch_clip_coef(const float* sumsq, float max_norm, float* coef, hipStream_t st);
int launch_scale_f32(float* x, long n, const float* scale_dev, hipStream_t st);
int launch_exchange_shadow(void* buf, size_t bytes, int workgroups, int lds_bytes, float busy_us, hipStream_t st);   // measurement hook

// ------------------------------------------------------------------------------------------------
// loss side (loss.hip) -- restates reference compute_loss arithmetic on device
// ------------------------------------------------------------------------------------------------
struct LossP {
  int method;             // 0 = ddpm, 1 = flow matching
  int prediction_type;    // ddpm: 0 = epsilon, 1 = v_prediction
  int use_min_snr;        // ddpm
  float min_snr_gamma;
  int use_ztsnr;          // clamp noisy latents to +-20000
  int B, HW, C;           // latents [B][C][HW] (NCHW, fp32), C = 4
  const float* latents;   // x (ddpm) / x1 (flow)
  const float* noise;     // noise (ddpm) / x0 (flow)
  const float* sigma;     // ddpm: [B] sigma ; flow: [B] t
  const float* tag_w;     // optional [B]
  bf16* unet_in;          // [B*HW][8] (channels 4..7 zero; wider and filled with ncond > 0, below)
  const bf16* pred;       // [B*HW][8]
  bf16* dpred;            // [B*HW][8]
  float grad_scale;       // multiplies d(loss)/d(pred) (1/grad_accum, 1/world)
  float* out;             // device: [0]=loss [1]=raw loss [2]=sum|pred| [3]=sum pred^2 [4]=sum|noise|
                          //         [5]=sum x0^2 [6]=sum x1^2 [7]=gate
  float* part;            // device scratch, loss_part_floats(B, HW): the blocks' partial sums (no atomics: the loss is bitwise reproducible)
  // ---- per-sample weights / losses and the selectable element loss (all zero / NULL = the reference's two objectives as above) ----
  int loss_type;          // 0 = l2: d^2 ; 1 = huber: 2c(sqrt(d^2+c^2)-c) ; 2 = smooth_l1: 2(sqrt(d^2+c^2)-c)
  float huber_c;          // c when huber_cb is NULL
  const float* sample_w;  // optional [B]: s_b, multiplied into each sample's loss and gradient
  const float* huber_cb;  // optional [B]: per-sample c_b
  float* ps_out;          // optional [B] OUT: L_b = s_b w_b mean_chw l(d), before the tag mean and the guard
  // ---- masked loss / input perturbation (NULL / 0 = every pixel counts, the input is built from `noise`) ----
  const float* noise_in;  // [B][4][HW]: what loss_prepare_kernel builds the UNet input from (the callers set it to `noise` when the
                          // batch has none); the target, the weights and out[4], out[5] always use `noise`
  const float* mask;      // optional [B][HW]: m >= 0 per latent pixel, multiplied into (s_b w_b) for all four channels
  int mask_norm;          // with mask: 0 = mean (divide by numel), 1 = masked_mean (per sample by 4 M_b, M_b = sum_hw m)
  float* mnorm;           // masked_mean: [B] scratch, M_b left by loss_finalize_kernel for loss_bwd_kernel
};
// ---- extra UNet input channels (in_channels > 4): what the COND instantiations of loss_prepare_kernel take; LossP itself, and with it
// every kernel of the 4-channel UNet, stays as it is.  Read by the preparation only (its gradient: input_dgrad.hip). ----
struct LossCondP : LossP {
  const float* cond;      // [B][ncond][HW] fp32 NCHW: channels 4 .. 4 + ncond - 1 of the UNet input, bf16(cond) round to nearest even
  int ncond;              // in_channels - 4, 1 .. 12; unet_in is [B*HW][Cs] with Cs = input_cs(4 + ncond), the channels behind zero
};
// stored width of an input pixel: one 16-byte vector up to 8 channels, two above (conv_in's Cin and the row stride of the plan's input buffer)
static inline __host__ __device__ int input_cs(int in_channels) { return in_channels <= 8 ? 8 : 16; }
// A 256-pixel block of the flat [B*HW] range touches at most loss_ps_slots samples (it straddles a sample boundary whenever
// HW % 256 != 0, several when HW < 256).  The scratch holds the blocks' six batch sums first, then one partial of the weighted
// element loss per (block, sample slot); slot j of block r belongs to sample (r * 256) / HW + j.  masked_mean adds a second such
// column behind it: the block's partial of the mask sum M_b per slot.
static inline __host__ __device__ int loss_ps_slots(int B, int HW) { const int s = 255 / HW + 2; return s < B ? s : B; }
static inline size_t loss_part_floats(int B, int HW) { return (6 + 2 * (size_t)loss_ps_slots(B, HW)) * (((size_t)B * HW + 255) / 256); }
int launch_loss_prepare(const LossP& p, hipStream_t st, const float* cond = nullptr, int ncond = 0);
int launch_loss_fwd(const LossP& p, hipStream_t st);
int launch_loss_bwd(const LossP& p, hipStream_t st);

// ---- one sampler step (sampler.hip): guidance + denoiser + solver step + the next UNet input, the fields of sdxl_sampler_step ----
struct SamplerP {
  float* x;               // [B][4][HW] fp32 NCHW state, in place
  const bf16* pred;       // [(cfg ? 2B : B) * HW][8]: conditional rows first, then the unconditional ones (not read with init)
  bf16* x_in;             // same shape: the next UNet input, both halves (channels 4..7 zero)
  int B, HW;              // B = samples (half the image's batch with cfg)
  int cfg, init;
  float a_skip, a_out, p, q, a_in_next, clamp, guidance, rescale;
  float* part;            // device scratch, sampler_part_floats(B, HW), read only when rescale != 0
  // ---- the extended step (sdxl_sampler_step_ext); ext = 0: none of these is read and the plain kernel runs ----
  int ext;
  float* hist;            // [B][4][HW] fp32: read with r != 0, written (den) with save & 1
  float* xsave;           // [B][4][HW] fp32: read with u != 0, written (x before the step) with save & 2
  const float* noise;     // [B][4][HW] fp32: read with s != 0
  float r, u, s;
  int save;
  const float* mask;      // [B][HW] fp32, 1 = generated, 0 = kept; NULL = no blend
  const float* known;     // [B][4][HW] fp32
  const float* knoise;    // [B][4][HW] fp32: read with k_b != 0
  float k_a, k_b;
};
// ---- extra UNet input channels (the COND instantiations of sampler_step_kernel): x_in is [rows][Cs], Cs = input_cs(4 + ncond); pred stays [rows][8] ----
struct SamplerCondP : SamplerP {
  const float* cond;      // [(cfg ? 2B : B)][ncond][HW] fp32 NCHW: row b goes to the conditional half, row b + B to the unconditional one
  int ncond;
};
static inline size_t sampler_part_floats(int B, int HW) { return 4 * (size_t)B * (((size_t)HW + 255) / 256); }
int launch_sampler_step(const SamplerP& p, hipStream_t st, const float* cond = nullptr, int ncond = 0);

// ---- the fused optimizer updates (optimizer.hip): one launch over an arena slice ----
// what both algorithms' kernels read
struct OptimP {
  bf16* p;
  const float* grad_f32;       // native fp32 gradient arena, or
  const bf16* grad_bf16;       //   bf16 gradients (exactly one of the two)
  bf16 *m, *v;                 // exp_avg, exp_avg_sq
  size_t n;                    // elements, multiple of 8
  float beta1, beta2;          // float32, as torch's mul_ by a python scalar uses them
  float one_minus_beta2;       // value of addcmul_
  float eps_bf16;              // eps rounded to bf16 (torch casts the scalar it adds to a bf16 tensor)
  int grad_round_bf16;         // round the (scaled) gradient to bf16 first, as the reference's bf16 autograd does
  const float* grad_scale;     // device scalar multiplied into the gradient (unscale / clip), or nullptr
  float* ema;                  // fp32 EMA of the weights, element 0 = p's element 0, or nullptr (no EMA)
  float ema_omd;               // 1 - decay of this update, float32: e <- e - omd * (e - p_new), three separately rounded ops
};
// AdamW_BF16 (adamw_bf16_kernel; reference adamw_bfloat16/__init__.py:146-197)
struct AdamWP : OptimP {
  bf16* shift;
  float one_minus_beta1;       // float32
  float value;                 // -lr * sqrt(1 - beta2^step)
  float decay_alpha_bf16;      // -decay_this_iteration rounded to bf16, 0 = no decay in this launch
  int reference_ema;           // 1: the reference's actual first-moment update  m <- SR(g + (1-b1) * b1*m)   (quirk D17)
                               // 0: the documented EMA                          m <- SR(b1*m + (1-b1) * g)
  const unsigned short* rand;  // [4][n] injected random 16-bit integers (parity tests), or nullptr = Philox
  unsigned seed_lo, seed_hi, step_counter;
  size_t elem_offset;          // arena index of element 0 of this launch (multiple of 8): the Philox counters are those of the
                               // full-arena launch, so a sharded (ZeRO-1) update is bit-identical to the unsharded one
};
int launch_adamw_bf16(const AdamWP& q, hipStream_t st);
// schedule-free Kahan AdamW (sfk_kernel)
struct SfkP : OptimP {
  bf16* c;                     // kahan_comp (nullptr without kahan_sum)
  float one_minus_beta1_bf16;  // alpha of exp_avg.add_(grad, alpha=1-beta1): rounded to bf16 as torch does
  int has_wd;                  // weight_decay != 0
  float wd_alpha_bf16;         // reference mode: alpha of p.add_(p, alpha=-weight_decay), rounded to bf16
  float neg_step;              // reference mode: -step_size (float32)
  float step;                  // compensated mode: step_size (float32)
  float decay;                 // compensated mode: step_size * weight_decay (float32)
};
int launch_sfk(const SfkP& q, int reference, hipStream_t st);
// Prodigy (prodigy_accumulate_kernel, prodigy_finalize_kernel, prodigy_apply_kernel): fp32 moments, so OptimP's bf16 m / v carry the
// addresses for check_arenas only and the kernels read m32 / v32; beta1, beta2, one_minus_beta2 are OptimP's, eps_bf16 is not read
struct ProdigyP : OptimP {
  float *m32, *v32, *s;        // exp_avg, exp_avg_sq, Prodigy's s
  bf16* c;                     // compensation: the true parameter is p + c
  const bf16* p0;              // the parameters at construction
  float* state;                // [8] d, d_max, num, Bs, d_hat, dlr, A, 0, then [2 * grid] the workgroups' partial sums (t, a) by index
  float lr, bc;                // float32 of the caller's doubles: the multiplier on d, this step's bias-correction factor
  float one_minus_beta1, beta3, eps, d0, d_coef, growth;
  float wd;                    // weight_decay (float32), 0 = none
  int safeguard;
};
int launch_prodigy(const ProdigyP& q, hipStream_t st);
// Adafactor (adafactor_*_kernel; include/sdxlstep.h, algorithm 3, is the contract).  One table entry per tensor, as the kernels read it:
// the caller's entry plus its place in the two work-item prefix tables and in the scratch
struct AfTensor {
  size_t elem_off, numel;
  float *R, *C;                // factored: the row and column statistics in af_state (C = R + rows); unfactored: R = v, C unused
  float *sx, *su;              // [tiles] the tiles' sums of x*x and of u*u
  float *rch, *rowp, *colp;    // factored: [ceil(rows/256)] chunk partials of R', [rows][ncb] row sums, [nrb][cols] column sums
  int rows, cols, factored;
  int ncb, nrb;                // column blocks of AF_COLS, row blocks of AF_ROWS
  int tile0;                   // tiles of the entries before this one (launches 1, 3, 5)
  int nrc, ncc, chunk0;        // chunks of 256 rows, of 256 columns, and the chunks of the entries before this one (launch 2)
};
constexpr int AF_ROWS = 128, AF_COLS = 256;
// OptimP's bf16 m / v carry addresses for check_arenas only (v is p's: the algorithm has no arena-sized second moment)
struct AdafactorP : OptimP {
  const AfTensor* table;       // device
  int n_tensors, tiles, chunks;
  bf16* c;                     // compensation: the true parameter is p + c
  float* m32;                  // first moment, or nullptr (use_beta1 == 0)
  float* scal;                 // [n_tensors][4] rho_t, eta_t, rms_u, rms_p
  float eps1, eps2, clip, b2t, omb2t, rho, omb1, wd;
  int scale_parameter;
};
int launch_adafactor(const AdafactorP& q, hipStream_t st);
int launch_adamw_decay(bf16* shift, const bf16* p, size_t n, float alpha_bf16, hipStream_t st);


// ---- conditioning gradients (cond_dgrad.hip): C32 [M][N] = sum_g A_g [M][K_g] . W_g [K_g][N], bf16 operands, fp32 sums and output ----
struct CondDgradP {
  int n;                  // groups, 1 or 2
  const bf16* A[2];       // [M][K_g], row stride lda (rows >= M are never read)
  const bf16* W[2];       // [K_g][N], row stride ldb >= N (a column slice of a wider weight)
  long lda[2], ldb[2];
  int K[2];               // multiples of 64
  float* C;               // [M][N] fp32, row stride ldc: overwritten
  long ldc;
  int M, N;               // N % 8 == 0
  float* slab;            // cond_dgrad_slab_floats(n, K, M, N) floats (may be null when that is 0)
  const float* gate;      // device scalar or null: when it reads 0 (closed gradient gate) the result is exact zeros
};
size_t cond_dgrad_slab_floats(int n, const int* K, int M, int N);
int launch_cond_dgrad(const CondDgradP& p, hipStream_t st);

// ---- LoRA by merge and project (lora.hip): table-driven, one launch of each kernel covers every target ----
#define LORA_M_ROWS 32    // merge tile
#define LORA_M_COLS 64
#define LORA_M_KC 32      // ranks staged per step
#define LORA_B_ROWS 32    // dB: rows per workgroup
#define LORA_B_COLS 256   //     columns staged per step
#define LORA_B_KC 16      //     ranks per pass over the rows
#define LORA_A_COLS 128   // dA: columns per workgroup
#define LORA_A_ROWS 32    //     rows staged per step
struct LoraTarget {       // one targeted weight [out][in]; element offsets from the launch's pointers
  long w_off;             // weight / gradient arena
  long base_off;          // packed W0
  long a_off, b_off;      // adapter arena: A [rank][in], B [out][rank]
  long ga_off, gb_off;    // adapter-gradient arena: dA, dB
  int out, in;            // of the state-dict tensor flattened to [shape[0]][prod(shape[1:])]; in % 8 == 0
  int tile_m, tile_b, tile_a;   // first workgroup of this target in the merge / dB / dA launch
  // where source element (o, i) lives (SDXL_DTYPE_LORA_LAYOUTS; the arena's packed layouts, repack_kernel in engine.hip).  Native rows are
  // `in` elements long for every kind, so the tiles walk native rows and columns and only the indices into A, B, dA, dB are mapped:
  int kind;               // LORA_KIND_PLAIN: native (o, i).  LORA_KIND_CONV3: i = c * 9 + tap at native (o, tap * cg + c).
                          // LORA_KIND_GEGLU: o = half * C4 + c at native row (c / cg) * 2 cg + half * cg + c % cg, C4 = out / 2
  int cg;                 // CONV3: cin (in == 9 cin);  GEGLU: the group G (C4 % G == 0);  PLAIN: unused
  int nrows;              // native rows, >= out: rows out .. nrows - 1 (CONV3 only) hold no source element; merge copies W0 there
};
#define LORA_KIND_PLAIN 0
#define LORA_KIND_CONV3 1
#define LORA_KIND_GEGLU 2
__host__ __device__ static inline int lora_src_col(int kind, int cg, int j) {      // native column -> column of A / dA
  return kind == LORA_KIND_CONV3 ? (j % cg) * 9 + j / cg : j;
}
__host__ __device__ static inline int lora_src_row(int kind, int cg, int c4, int r) {      // native row < out -> row of B / dB
  if (kind != LORA_KIND_GEGLU) return r;
  const int grp = r / (2 * cg), rem = r - grp * 2 * cg, half = rem / cg;
  return half * c4 + grp * cg + rem - half * cg;
}
struct LoraP {
  const LoraTarget* table;      // device [n], or nullptr: a table of one, passed by value in `one`
  LoraTarget one;
  int n, rank;                  // rank 1 .. 128
  float scale;
  int tiles_m, tiles_b, tiles_a;
  int mapped;                   // 0: every target is LORA_KIND_PLAIN with nrows == out, and the launch takes the kernels that never look at
                                // kind / cg / nrows; 1: the kind-aware instantiations (which also run the plain targets of a mixed table)
  bf16* w;                      // merge: out
  const bf16* base;             // merge
  const bf16 *a, *b;            // what a_off / b_off count from: the adapter arena twice, or the hook's A and B (offsets 0)
  const float* dw;              // project
  float *ga, *gb;               // project: out, overwritten; what ga_off / gb_off count from (the gradient arena twice, or dA and dB)
};
// the LoraTarget of a table row: the row itself, or the `t` a family's row (LohaTarget, LokrTarget, DoraTarget) wraps
__device__ __forceinline__ const LoraTarget& lora_of(const LoraTarget& t) { return t; }
template <class T> __device__ __forceinline__ const LoraTarget& lora_of(const T& x) { return x.t; }
// a workgroup's row of a launch struct P (LoraP, LohaP, LokrP, DoraP): the last target whose first tile FIRST is <= tile
template <int LoraTarget::*FIRST, class P>
__device__ __forceinline__ auto adapter_find(const P& p, int tile) -> decltype(p.one) {
  if (!p.table) return p.one;
  int lo = 0, hi = p.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (lora_of(p.table[mid]).*FIRST <= tile) lo = mid; else hi = mid - 1;
  }
  return p.table[lo];
}
static inline int lora_tiles_m(int out, int in) { return cdiv(out, LORA_M_ROWS) * cdiv(in, LORA_M_COLS); }
static inline int lora_tiles_b(int out, int in) { return cdiv(out, LORA_B_ROWS); }
static inline int lora_tiles_a(int out, int in) { return cdiv(in, LORA_A_COLS); }
int launch_lora_merge(const LoraP& p, hipStream_t st);
int launch_lora_project(const LoraP& p, hipStream_t st);     // two launches: dB, dA

// ---- LoHa by merge and project (loha.hip; SDXL_DTYPE_LOHA): dW = s (B1 A1) .* (B2 A2), table-driven like LoRA's, always kind-aware ----
#define LOHA_MAX_RANK 64
#define LOHA_M_ROWS 32    // merge tile
#define LOHA_M_COLS 64
#define LOHA_M_KC 32      // ranks staged per step
#define LOHA_P_ROWS 32    // project: the G .* P tile both launches walk
#define LOHA_P_COLS 32
struct LohaTarget {       // LoraTarget (its a / b offsets: the first pair) and the second pair's offsets; t.nrows is not used: only the
  LoraTarget t;           // rows < out of a target are read or written
  long a2_off, b2_off;    // adapter arena: A2 [rank][in], B2 [out][rank]
  long ga2_off, gb2_off;  // adapter-gradient arena: dA2, dB2
};
struct LohaP {
  const LohaTarget* table;      // device [n], or nullptr: a table of one, passed by value in `one`
  LohaTarget one;
  int n, rank;                  // rank 1 .. LOHA_MAX_RANK
  float scale;
  int tiles_m, tiles_b, tiles_a;
  bf16* w;                      // merge: out
  const bf16* base;             // merge
  const bf16 *a1, *b1, *a2, *b2;      // what the a / b offsets count from: the adapter arena four times, or the hook's factors (offsets 0)
  const float* dw;              // project
  float *ga1, *gb1, *ga2, *gb2;       // project: out, overwritten
};
static inline int loha_tiles_m(int out, int in) { return cdiv(out, LOHA_M_ROWS) * cdiv(in, LOHA_M_COLS); }
static inline int loha_tiles_b(int out, int in) { return cdiv(out, LOHA_P_ROWS); }
static inline int loha_tiles_a(int out, int in) { return cdiv(in, LOHA_P_COLS); }
int launch_loha_merge(const LohaP& p, hipStream_t st);
int launch_loha_project(const LohaP& p, hipStream_t st);     // two launches: dB1 | dB2, dA1 | dA2

// ---- LoKr by merge and project (lokr.hip; SDXL_DTYPE_LOKR): dW = s kron(C, W2), W2 full or B A, table-driven like LoRA's, always kind-aware ----
#define LOKR_MAX_RANK 128
#define LOKR_M_ROWS 32    // merge tile
#define LOKR_M_COLS 64
#define LOKR_M_KC 32      // ranks staged per step
#define LOKR_P_TILE 1024  // project, launch 1: elements of W2 per workgroup (SDXL_LOKR_TILE), 4 per thread
#define LOKR_P_NB 8       //   blocks (a, b) whose loads are in flight together and whose partial sums share one barrier
#define LOKR_Q_THREADS 256      // project, launch 2: one output element per thread
// source -> native, the inverses of lora_src_col / lora_src_row
__host__ __device__ static inline int lora_nat_col(int kind, int cg, int i) {
  return kind == LORA_KIND_CONV3 ? (i % 9) * cg + i / 9 : i;
}
__host__ __device__ static inline int lora_nat_row(int kind, int cg, int c4, int o) {
  if (kind != LORA_KIND_GEGLU) return o;
  const int half = o >= c4 ? 1 : 0, c = o - half * c4, grp = c / cg;
  return grp * 2 * cg + half * cg + c - grp * cg;
}
struct LokrTarget {       // LoraTarget (w_off, base_off, out, in, kind, cg; tile_m: merge, tile_b: project launch 1, tile_a: launch 2;
  LoraTarget t;           // a_off / ga_off: A, b_off / gb_off: W2 or B) and the factorisation.  Only the rows < out are read or written
  long c_off;             // adapter and adapter-gradient arena: C [out_l][in_m]
  long part_off, dw2_off; // scratch, in floats: partial sums [ptiles][out_l * in_m]; a factored target's s dW2 [out_k][n2]
  int out_l, out_k;       // out = out_l * out_k
  int in_m, in_n;         // cin = in_m * in_n
  int khw, n2;            // 1 or 9; n2 = in_n * khw: in = in_m * n2
  int full;               // W2 stored as it is (b_off), else W2 = B A; also picks the scale: LokrP::scale_full or LokrP::scale
  int ptiles;             // cdiv(out_k * n2, LOKR_P_TILE)
};
struct LokrP {
  const LokrTarget* table;      // device [n], or nullptr: a table of one, passed by value in `one`
  LokrTarget one;
  int n, rank;                  // rank 1 .. LOKR_MAX_RANK (read by the factored targets only)
  float scale, scale_full;      // s of a factored target and of a full one (per call, not in the table: a restoring merge passes 0 for both)
  int tiles_m, tiles_p, tiles_q;
  bf16* w;                      // merge: out
  const bf16* base;             // merge
  const bf16 *c, *b, *a;        // what c_off / b_off / a_off count from: the adapter arena three times, or the hook's factors (offsets 0)
  const float* dw;              // project
  float *gc, *gb, *ga;          // project: out, overwritten
  float* scratch;               // project
};
// LyCORIS' factorization(dimension, factor), the smaller number first (include/sdxlstep.h restates the rule)
static inline void lokr_fact(int dim, int factor, int* m_, int* n_) {
  int m = 1, n = dim;
  if (factor > 0 && dim % factor == 0) { m = factor; n = dim / factor; }
  else {
    if (factor < 0) factor = dim;
    while (m < n) {
      int nm = m + 1;
      while (dim % nm) ++nm;
      const int nn = dim / nm;
      if (nm + nn > m + n || nm > factor) break;
      m = nm; n = nn;
    }
  }
  *m_ = m < n ? m : n; *n_ = m < n ? n : m;
}
static inline bool lokr_rule_full(int out_k, int in_n, int rank) { return 2 * rank >= (out_k > in_n ? out_k : in_n); }
// the geometry of one target: cin = the channel count (in for a 2-D weight, in / 9 for a 3x3 convolution)
static inline void lokr_geometry(LokrTarget& x, int cin, int factor, int full) {
  lokr_fact(x.t.out, factor, &x.out_l, &x.out_k);
  lokr_fact(cin, factor, &x.in_m, &x.in_n);
  x.khw = x.t.in / cin; x.n2 = x.in_n * x.khw;
  x.full = full;
  x.ptiles = (int)cdiv((long)x.out_k * x.n2, (long)LOKR_P_TILE);
}
static inline size_t lokr_pad4(size_t n) { return (n + 3) / 4 * 4; }
static inline size_t lokr_part_floats(const LokrTarget& x) { return lokr_pad4((size_t)x.ptiles * x.out_l * x.in_m); }
static inline size_t lokr_dw2_floats(const LokrTarget& x) { return x.full ? 0 : lokr_pad4((size_t)x.out_k * x.n2); }
static inline int lokr_tiles_m(const LokrTarget& x) { return cdiv(x.t.out, LOKR_M_ROWS) * cdiv(x.t.in, LOKR_M_COLS); }
// (lokr_check_size, capi.h, keeps out_k * n2, out_k * rank and rank * n2 below 2^31: launch 2 indexes its outputs with 32-bit integers)
static inline int lokr_tiles_q(const LokrTarget& x, int rank) {
  return cdiv((long)x.out_l * x.in_m, LOKR_Q_THREADS) + (x.full ? 0 : cdiv((long)x.out_k * rank, LOKR_Q_THREADS) + cdiv((long)rank * x.n2, LOKR_Q_THREADS));
}
int launch_lokr_merge(const LokrP& p, hipStream_t st);
int launch_lokr_project(const LokrP& p, hipStream_t st);     // two launches: dW2 and the partial sums of dC; dC, dB, dA

// ---- DoRA by merge and project (dora.hip; SDXL_DTYPE_DORA): W = c_o (W0 + s B A), c_o = (1 + mu_o) n0_o / n_o, table-driven like LoRA's ----
#define DORA_R_ROWS 32    // row reductions (norm, norm0, dmu): rows per workgroup (= LORA_B_ROWS: they share LoraTarget::tile_b with dB)
#define DORA_R_COLS 64    //     columns per pass of the column loop, 8 per thread
#define DORA_R_KC 32      //     ranks staged per step
#define DORA_R_NORM 0     // what a row reduction writes: norm = sqrt(sum v^2), v = W0 + s B A
#define DORA_R_NORM0 1    //     norm0 = the same with s B A taken as 0 (A, B, scale are not read)
#define DORA_R_DMU 2      //     dmu = (n0 / n) sum G v
struct DoraTarget {       // LoraTarget (a_off / b_off and ga_off / gb_off: A, B; tile_m: merge and restore, tile_b: the row reductions and dB,
  LoraTarget t;           // tile_a: dA; t.nrows is not used: only the rows < out of a target are read or written)
  long mu_off;            // adapter and adapter-gradient arena: mu [out], indexed like the state-dict rows
  long n_off;             // norm0 / norm: [out] floats, indexed like the state-dict rows
};
struct DoraP {
  const DoraTarget* table;      // device [n], or nullptr: a table of one, passed by value in `one`
  DoraTarget one;
  int n, rank;                  // rank 1 .. 128
  float scale;
  int tiles_m, tiles_b, tiles_a;
  int mapped;                   // as LoraP::mapped
  bf16* w;                      // merge, restore: out
  const bf16* base;             // every launch but dB and dA
  const bf16 *a, *b, *mu;       // what a_off / b_off / mu_off count from: the adapter arena three times, or the hook's operands (offsets 0)
  const float* dw;              // project
  float *ga, *gb, *gmu;         // project: out, overwritten
  float* norm0;                 // init: out; merge, project: in
  float* norm;                  // merge: out (by its first launch), then in; project: in
};
static inline long dora_pad4(long n) { return (n + 3) / 4 * 4; }
int launch_dora_init(const DoraP& p, hipStream_t st);        // one launch: norm0
int launch_dora_merge(const DoraP& p, hipStream_t st);       // two launches: norm, W
int launch_dora_restore(const DoraP& p, hipStream_t st);     // one launch: W = W0
int launch_dora_project(const DoraP& p, hipStream_t st);     // three launches: dmu, dB, dA

// ---- direct LoRA adapter gradients (lora_grad.hip): dA, dB of every target of ONE linear op from its X and dY, no dW ----
#define LORA_G_CHUNK 512      // rows of M per partial block (a multiple of 32): the split of M is fixed by M alone
struct LoraGradTarget {
  long a_off, b_off;          // adapter arena: A [rank][in], B [out][rank]
  long ga_off, gb_off;        // adapter-gradient arena: dA, dB
  long part_off;              // this target's partial blocks [nchunk][rank][in + out] start at float part_off * nchunk of LoraGradP::part
                              // (= rank * the earlier targets' in + out: the table does not depend on M)
  int out, in;                // in % 8 == 0
  int dy_col;                 // first column of the target inside the op's dY (its first row inside the op's native weight)
  int tile0, red0;            // first 128-column tile of [in | out] / first workgroup of the reduce launch
  int pad;
};
struct LoraGradP {
  const LoraGradTarget* table;      // device [n], or nullptr: a table of one, passed by value in `one`
  LoraGradTarget one;
  int n, rank;                      // rank 1 .. 128
  float scale;
  int accumulate;                   // 0: dA, dB are overwritten; 1: added to
  const bf16* x; long ldx;          // [M][in], shared by the targets
  const bf16* dy; long ldy;         // [M][...]: a target's columns start at dy_col
  int M, Mp;                        // Mp = M rounded up to 64
  int xvec, yvec;                   // x / dy rows are addressable in 16-byte vectors (pointer and row stride multiples of 16 bytes)
  int nchunk, tiles, reds;          // cdiv(M, LORA_G_CHUNK); sum of the targets' tiles; of their reduce workgroups
  const bf16 *a, *b;                // what a_off / b_off count from
  float *ga, *gb;                   // what ga_off / gb_off count from
  bf16* tu;                         // scratch: lora_grad_tu_elems(n, rank, M) bf16, 16-byte aligned
  float* part;                      // scratch: the targets' partial blocks
};
static inline int lora_grad_rb(int rank) { return rank <= 16 ? 1 : rank <= 32 ? 2 : rank <= 64 ? 4 : 8; }      // 16-rank blocks the kernels are built for
static inline int lora_grad_mp(int M) { return cdiv(M, 64) * 64; }
static inline int lora_grad_chunks(int M) { return cdiv(M, LORA_G_CHUNK); }
static inline size_t lora_grad_tu_elems(int n, int rank, int M) { return (size_t)n * 2 * 16 * lora_grad_rb(rank) * lora_grad_mp(M); }
static inline size_t lora_grad_part_floats(int out, int in, int rank, int M) { return (size_t)lora_grad_chunks(M) * rank * ((size_t)in + out); }
static inline int lora_grad_tiles(int out, int in) { return cdiv(in, 128) + cdiv(out, 128); }
static inline int lora_grad_reds(int out, int in, int rank) { return cdiv((long)rank * ((long)in + out), 256); }
int launch_lora_grad(const LoraGradP& p, hipStream_t st);     // three launches: T | U, partial blocks, reduce
