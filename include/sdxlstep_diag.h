/* libsdxlstep -- test hooks and experiment ABI.  NOT part of the drop-in boundary (include/sdxlstep.h is): nothing a caller of the
 * training step needs is declared here.  Implemented in csrc/hooks.hip (with the sdxl_op_* entry points of sdxlstep.h): each builds its launch
 * with the builders the plan uses (csrc/kernels.h) and takes scratch from one grow-only buffer of the process (one stream at a time).
 *
 * Part 1, exported by the product library too: hooks the parity tests and the measurement tools use to force one kernel
 * configuration or to look inside a plan.
 * Part 2, exported ONLY by the diagnostics build (`python sdxl-training-improvements_amd/build.py --diag` -> libsdxlstep_diag.so,
 * compiled with -DSDXL_DIAG): measured, parity-tested experiments that the shipped plan never runs -- the knob table, the
 * persistent stream-K GEMM (csrc/gemm_sk.hip), the stride-2 convolution forward / weight gradient on phase planes
 * (GemmP::up2 == 3), the W = 32 form of the three-tap convolution weight gradient.  DESIGN.md sections 10-12 hold their numbers;
 * tests of them carry the `diag` marker and run with SDXL_DIAG=1. */
#ifndef SDXLSTEP_DIAG_H
#define SDXLSTEP_DIAG_H
#include "sdxlstep.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- part 1: test hooks (product library) ---- */
/* run ds_read_b64_tr_b16 / MFMA layout probes (tests/test_gpu_ops.py::test_hw_layout_probe) */
SDXL_API int sdxl_probe_layout(void* out_dev, void* stream);
/* tile-kernel selection of the GEMM family, for A/B measurements and parity tests: 0 = 128-row kernel only,
 * 1 = the plan's policy (default), 2 = 256 x 256 kernel wherever it is applicable;
 * + 4 * c forces configuration c of the 128-row kernel (1, 2, 3, 13, 23) or the co-resident 256-row kernel (31: 256 x 160 tiles,
 * 32: 256 x 128) wherever applicable.  Process-global: restore 1 after use. */
SDXL_API int sdxl_set_gemm_mode(int mode);
/* checksum of every activation (grads != 0: of every activation gradient) of the current plan, in creation
 * order; synchronises the device.  n_out receives the number of activations. */
SDXL_API int sdxl_debug_act_checksums(sdxl_handle* h, unsigned long long* out_host, int cap, int* n_out, int grads);

/* stand-in for a collective's device kernel on one GPU (bench.py --exchange-shadow): `workgroups` x 256 threads holding `lds_bytes` of
 * LDS each stream `buf` for `busy_us` microseconds; run beside the backward it prices the co-residency of the gradient exchange. */
SDXL_API int sdxl_op_exchange_shadow(void* buf, size_t bytes, int workgroups, int lds_bytes, float busy_us, void* stream);

/* sdxl_op_gemm's NT (form 0) / NN (form 1) with explicit leading dimensions (elements) and a configuration forced for this launch only
 * (cfg as in sdxl_set_gemm_mode's upper bits; 0 = the policy): C [M][N] = A [M][K] . B (+ bias [N]) (+ resid [M][ldr]) */
SDXL_API int sdxl_op_gemm_ld(int form, const void* A, const void* B, void* C, int M, int N, int K, long lda, long ldb, long ldc, const void* bias,
                    const void* resid, long ldr, int cfg, void* stream);
/* the out-projection dgrad whose epilogue also writes the self-attention backward's Delta (csrc/kernels.h, GemmP::delta_out; the plan
 * uses it at the 1280-channel level, csrc/engine.hip LinearOp::plan_bwd): dO [M][N] = dY [M][K] . W [K][N] (+ addend, or null), bf16, and
 * Delta[(b * heads + h) * Nq + q] = sum_d bf16(dO[m][64 h + d]) * O[m][64 h + d] with m = b * Nq + q, heads = N / 64.  M = B * Nq,
 * N % 128 == 0, K % 64 == 0. */
SDXL_API int sdxl_op_linear_dgrad_delta(const void* dy, const void* w, const void* o, const void* addend, void* d_o, float* delta, int B, int Nq,
                               int N, int K, void* stream);

/* the sampler step kernel behind sdxl_batch.sampler on caller buffers, without a UNet: x [B][4][H][W] fp32 in place (s->x is
 * not read), pred and x_in [(s->cfg ? 2B : B) * H * W][8] bf16 with the conditional rows first; B = samples.  Same argument checks. */
SDXL_API int sdxl_op_sampler_step(float* x, const void* pred, void* x_in, int B, int H, int W, const sdxl_sampler_step* s, void* stream);

/* the conditioning-gradient kernel the plan launches (csrc/cond_dgrad.hip) on caller buffers: C [M][N] fp32 (row stride ldc, overwritten) =
 * sum over n <= 2 groups of A[g] [M][K[g]] bf16 (row stride lda[g]; rows >= M are never read) . W[g] [K[g]][N] bf16 (row stride ldb[g] >= N),
 * fp32 sums in a fixed order (no atomics).  K[g] % 64 == 0, N % 8 == 0, M >= 1.  The split-K slab is library-owned. */
SDXL_API int sdxl_op_cond_dgrad(int n, const void* const* A, const long* lda, const void* const* W, const long* ldb, const int* K, float* C,
                       long ldc, int M, int N, void* stream);

/* where the current plan's conditioning-gradient launches find their operands, so that a test can hand the same buffers to
 * sdxl_op_cond_dgrad: which = 0 (d prompt_embeds; g = 0 .. *n_groups - 1, the K | V projections in forward order) or 1 (d pooled; g = 0).
 * A = workspace + *a_ws_byte_off (bf16 [M][*lda]), W = weight arena + *w_elem_off (bf16 [*K][*ldb]).  g out of range is a bad argument. */
SDXL_API int sdxl_debug_cond_operands(sdxl_handle* h, int which, int g, int* n_groups, size_t* a_ws_byte_off, long* lda, size_t* w_elem_off,
                             long* ldb, int* K);

/* the LoRA kernels of SDXL_DTYPE_LORA (csrc/lora.hip) on caller buffers, a table of one target, no handle: W0, w [out][in] bf16, A [rank][in],
 * B [out][rank] bf16, dw [out][in] fp32, dA [rank][in], dB [out][rank] fp32 (overwritten).  Same argument checks: rank 1 .. 128, in % 8 == 0,
 * out >= 1, every pointer 16-byte aligned. */
SDXL_API int sdxl_op_lora_merge(const void* base, const void* A, const void* B, void* w, int out, int in, int rank, float scale, void* stream);
SDXL_API int sdxl_op_lora_project(const float* dw, const void* A, const void* B, float* dA, float* dB, int out, int in, int rank, float scale,
                         void* stream);
/* ... and of SDXL_DTYPE_LORA_LAYOUTS: one target held in a packed layout (include/sdxlstep.h has the maps).  kind 0: plain rows; 1: a 3x3
 * convolution, cg = cin and in == 9 cin; 2: GEGLU rows, cg = the group G, (out / 2) % G == 0.  W0, w (bf16) and dw (fp32) are NATIVE:
 * [native_rows][in], native_rows >= out and == out unless kind is 1; A [rank][in], B [out][rank], dA, dB are indexed like the state-dict
 * tensor.  merge writes every native row (W0's bits into the rows past `out`); project never reads those rows of dw.  These hooks always
 * take the kind-aware kernels, kind 0 included. */
SDXL_API int sdxl_op_lora_merge_layout(const void* base, const void* A, const void* B, void* w, int out, int in, int rank, float scale, int kind,
                              int cg, int native_rows, void* stream);
SDXL_API int sdxl_op_lora_project_layout(const float* dw, const void* A, const void* B, float* dA, float* dB, int out, int in, int rank,
                                float scale, int kind, int cg, int native_rows, void* stream);
/* the LoHa kernels of SDXL_DTYPE_LOHA (csrc/loha.hip) on caller buffers, a table of one target, no handle: base, w (bf16) and dw (fp32) are
 * NATIVE [out][in]; A1, A2 [rank][in], B1, B2 [out][rank] bf16 and dA1, dA2, dB1, dB2 fp32 (overwritten) are indexed like the state-dict tensor.
 * kind / group as the _layout hooks' kind / cg (0: plain rows, group unused; 1: a 3x3 convolution, group = cin and in == 9 cin; 2: GEGLU rows,
 * group = G, (out / 2) % G == 0); there are no padded native rows.  Argument checks: rank 1 .. 64, in % 8 == 0, out >= 1, a finite scale,
 * every pointer 16-byte aligned. */
SDXL_API int sdxl_op_loha_merge(const void* base, const void* A1, const void* B1, const void* A2, const void* B2, void* w, int out, int in, int rank,
                       float scale, int kind, int group, void* stream);
SDXL_API int sdxl_op_loha_project(const float* dw, const void* A1, const void* B1, const void* A2, const void* B2, float* dA1, float* dB1, float* dA2,
                         float* dB2, int out, int in, int rank, float scale, int kind, int group, void* stream);
/* the LoKr kernels of SDXL_DTYPE_LOKR (csrc/lokr.hip) on caller buffers, a table of one target, no handle.  This hook is a dtype, not a
 * function: the library exports no symbol for it.  sdxl_load_weight with a NULL handle, a NULL name, a HOST pointer to the struct below and
 * dtype SDXL_DTYPE_LOKR_ONE runs the merge; sdxl_export_grad called the same way runs the projection (two launches).
 * base, w (bf16) and dw (fp32) are NATIVE [out][in]; C [out_l][in_m], W2 [out_k][n2] (full = 1) or W2 = B [out_k][rank] with A [rank][n2]
 * (full = 0; A and dA may be NULL when full) bf16 and dC, dW2 (dB when factored), dA fp32 (overwritten) are indexed like the state-dict
 * tensors.  kind / group as the LoHa hooks'; the factorisation is fact(out, factor) x fact(cin, factor), cin = group for a 3x3 convolution
 * and `in` otherwise.  `full` and `scale` are the caller's: the form rule of SDXL_DTYPE_LOKR is not applied.  scratch: SDXL_DTYPE_LOKR's
 * formula for this one target (the merge reads neither it nor dw, dC, dW2, dA; the projection reads neither base nor w).
 * Argument checks (1, before any launch): a non-NULL handle or name, rank 1 .. 128, factor -1 or >= 1, full 0 / 1, in % 8 == 0, out >= 1, a
 * finite scale, every pointer the call uses 16-byte aligned, and for the projection a scratch of the required size. */
#define SDXL_DTYPE_LOKR_ONE 7
typedef struct {
  const void* base; const void* C; const void* W2; const void* A; void* w;      /* merge: in, in, in, in, out */
  const float* dw; float* dC; float* dW2; float* dA;                            /* project: in, out, out, out */
  int out, in, group, kind, factor, rank, full;
  float scale;
  float* scratch; size_t scratch_floats;
} sdxl_lokr_one;
/* the DoRA kernels of SDXL_DTYPE_DORA (csrc/dora.hip) on caller buffers, a table of one target, no handle.  A dtype like SDXL_DTYPE_LOKR_ONE:
 * sdxl_load_weight with a NULL handle, a NULL name, a HOST pointer to the struct below and dtype SDXL_DTYPE_DORA_ONE runs `mode` 0 (merge: two
 * launches, norm then w), 1 (init: norm0) or 2 (restore: w = base); sdxl_export_grad called the same way runs the projection (three launches:
 * dmu, dB, dA; `mode` is not read).  base, w (bf16) and dw (fp32) are NATIVE [out][in]; A [rank][in], B [out][rank], mu [out] bf16, dA, dB, dmu
 * fp32 (overwritten) and norm0, norm [out] fp32 are indexed like the state-dict tensors.  kind / group as the LoHa hooks'.
 * What a call uses: merge base, A, B, mu, norm0 (read), norm (written), w; init base, norm0; restore base, w; project dw, base, A, B, mu, norm0,
 * norm (read), dA, dB, dmu.  Argument checks (1, before any launch): a non-NULL handle or name, rank 1 .. 128, mode 0 .. 2, in % 8 == 0,
 * out >= 1, a finite scale, every pointer the call uses 16-byte aligned and non-NULL. */
#define SDXL_DTYPE_DORA_ONE 9
typedef struct {
  const void* base; const void* A; const void* B; const void* mu; void* w;      /* merge: in, in, in, in, out */
  const float* dw; float* dA; float* dB; float* dmu;                            /* project: in, out, out, out */
  float* norm0; float* norm;
  int out, in, group, kind, rank, mode;
  float scale;
} sdxl_dora_one;
/* the direct adapter-gradient kernels of sdxl_grad_select.lora (csrc/lora_grad.hip) on caller buffers, a table of one target, no handle:
 * x [M][in] (row stride ldx), dy [M][out] (row stride ldy: a column slice of a wider tensor is dy + offset), A [rank][in], B [out][rank] bf16;
 * dA [rank][in], dB [out][rank] fp32 = (accumulate ? previous : 0) + scale * (dY B)^T X, scale * dY^T (X A^T).  Rows past M and columns outside
 * the operands are never read.  Stream-ordered; its scratch is one buffer of the process, kept between calls and grown when a call needs
 * more (one stream at a time). */
SDXL_API int sdxl_op_lora_grad(const void* x, long ldx, const void* dy, long ldy, const void* A, const void* B, float* dA, float* dB, int M, int out,
                               int in, int rank, float scale, int accumulate, void* stream);

/* the two kernels of the additional skip residuals (sdxl_residuals; csrc/residual.hip) on caller buffers, as ConcatOp launches them:
 * o [B * HW][Ca + Cb] bf16 = a [B * HW][Ca] | b [B * HW][Cb], with ra [B][Ca][HW] / rb [B][Cb][HW] (rdtype 0 = fp32, 1 = bf16; either may be NULL,
 * both NULL = the plain concat) added to its half as bf16_rn(float(x) + float(r)), the bits of x where r == 0;
 * dra [B][Ca][HW] / drb [B][Cb][HW] fp32 (either may be NULL) = float(g [B * HW][Ca + Cb]) of their column range, exact zeros when
 * gate_dev (may be NULL) reads 0.  Ca, Cb multiples of 8, B <= 65535, every non-NULL pointer 16-byte aligned. */
SDXL_API int sdxl_op_concat_residual(const void* a, int Ca, const void* b, int Cb, const void* ra, const void* rb, int rdtype, void* o, int B, int HW,
                            void* stream);
SDXL_API int sdxl_op_concat_residual_grad(const void* g, int Ca, int Cb, float* dra, float* drb, const float* gate_dev, int B, int HW, void* stream);

/* the input-gradient kernel (csrc/input_dgrad.hip; the request: sdxl_batch_din) on caller buffers, through the launcher conv_in's backward calls:
 * dx [B][in_channels][H][W] fp32 (overwritten) = sum over ky, kx, o of dy [B * H * W][Cout] bf16 at pixel (y + 1 - ky, x + 1 - kx) times
 * w [Cout][9][Cs] bf16 (the arena's layout: Cs = 8 for in_channels <= 8, else 16; pad channels zero), pixels outside the image contributing
 * nothing; fp32 sums in a fixed order (no atomics).  Exact zeros, dy not read, when gate_dev (may be NULL) reads 0.  Cout % 32 == 0,
 * in_channels 1 .. 16, any B, H, W >= 1; dy, w, dx 16-byte aligned. */
SDXL_API int sdxl_op_input_dgrad(const void* dy, const void* w, float* dx, const float* gate_dev, int B, int H, int W, int in_channels, int Cout,
                        void* stream);
/* where the current plan's input-gradient launch finds its operands, so that a test can hand the same buffers to sdxl_op_input_dgrad:
 * dy = workspace + *dy_ws_byte_off (bf16 [B * H * W][*Cout], conv_in's output gradient, intact once a backward has finished), w = weight
 * arena + *w_elem_off (bf16 [*Cout][9][Cs]). */
SDXL_API int sdxl_debug_input_dgrad_operands(sdxl_handle* h, size_t* dy_ws_byte_off, size_t* w_elem_off, int* Cout);

/* which kernel a GEMM launch takes (csrc/gemm.hip, gemm_route: the single implementation of DESIGN.md section 4's table), without launching it and
 * without a device.  The descriptor is what the problem's line in the launch log (SDXL_LAUNCH_LOG) carries, in the same order: emit_bf16 / delta /
 * bias_grad are presence flags (GemmP::Cb, delta_out, bias_grad); Hm .. sd the 3x3 gather's image sizes and strides (taps != 1).  The same checks and normalisation as
 * a launch are applied first (their errors are returned).  rowvec, the struct's last field, is NOT in the launch log: a presence flag for a row vector in the
 * epilogue (GemmP::rowvec; the pipelined kernel has none and refuses the problem).  kernel: 0 the 128-row kernel (cfg 1, 2, 3, 13, 23, 5, 6), 1 the 256 x 256 kernel, 2 the
 * co-resident 256-row kernel (cfg 31 .. 36), 3 the pipelined kernel (cfg 7, 8), 4 the long-reduction weight gradient, 5 the three-tap convolution
 * weight gradient, 6 stream-K (diagnostics build); fast: the 128-row kernel's FAST staging; post: 0 none, 1 fp32 split-K reduce, 2 split-K sum +
 * bf16 epilogue. */
typedef struct sdxl_gemm_desc {
  int form, taps, M, N, K, splitk, group, cfg, geglu, geglu_group, Hm, Wm, Hs, Ws, sm, sd, up2, emit_bf16, delta, bias_grad, rowvec;
} sdxl_gemm_desc;
typedef struct sdxl_gemm_route { int kernel, cfg, fast, post; } sdxl_gemm_route;
SDXL_API int sdxl_debug_gemm_route(const sdxl_gemm_desc* problem, sdxl_gemm_route* out);

/* the time-embedding path on caller buffers.  sdxl_op_gemm_rowvec: the NT form (form 0 only) with the row-vector epilogue of a resnet's first
 * convolution, C [M][N] = bf16(A [M][K] . B [N][K]^T + bias [N] + rowvec [m / rows_per_batch][n] + resid [M][N]) in one rounding; rowvec points at the
 * first used column of a [M / rows_per_batch][ldv] bf16 matrix (a column slice: ldv >= N).  cfg as sdxl_op_gemm_ld's, splitk > 1 as sdxl_op_gemm's.
 * sdxl_op_conv3x3_fwd_rowvec: the same epilogue through the 3x3 convolution (stride 1, pad 1) as the plan builds it: its own split factor,
 * rows_per_batch = H * W.  Both refuse, before any launch, a vector that is NULL or not 16-byte aligned, ldv % 8 != 0 or ldv < N,
 * rows_per_batch < 1, M % rows_per_batch != 0. */
SDXL_API int sdxl_op_gemm_rowvec(int form, const void* A, const void* B, void* C, int M, int N, int K, const void* bias, const void* resid,
                        const void* rowvec, long ldv, int rows_per_batch, int splitk, int cfg, void* stream);
SDXL_API int sdxl_op_conv3x3_fwd_rowvec(const void* x, const void* w, const void* bias, const void* rowvec, long ldv, void* y, int B, int H, int W,
                               int Cin, int Cout, void* stream);
/* the backward of that broadcast: out [b][n] (fp32, row stride ld_out) += sum over r < rows of x [b * rows + r][n] (bf16, row stride ldx), fp32 sums
 * in a fixed order (no atomics between blocks: bitwise reproducible).  batches 1 .. 64, N % 8 == 0, ldx % 8 == 0; one batch with ld_out = 0 is the
 * up-sampler's bias gradient. */
SDXL_API int sdxl_op_colsum(const void* x, long ldx, float* out, long ld_out, int batches, int rows, int N, void* stream);
/* the sinusoidal embedding: out [rows][ldo] bf16, columns [0, dim / 2) = cos, [dim / 2, dim) = sin of t [r] (fp32) * exp(-ln(10000) k / (dim / 2));
 * dim even, ldo >= dim; columns past dim are not written. */
SDXL_API int sdxl_op_sincos(const float* t, void* out, int rows, int dim, long ldo, void* stream);

/* The plan map: what every op of the current plan reads and writes, so that a test can recompute each op of a finished step from the
 * operands it actually had (tests/_insitu.py).  Pure host code: nothing is launched, nothing is reserved, no offset of the plan moves.
 * The descriptor is a flat POD; SDXL_PLAN_NONE = (size_t)-1 marks an absent offset.  Offsets of activations, gradients, statistics and scratch
 * are BYTE offsets into the workspace; w / b are ELEMENT offsets into the bf16 weight arena and the fp32 gradient arena alike.
 * Tensor roles (t[r]; rows == 0: the op has no such role), by kind:
 *   LINEAR     0 x, 1 y, 2 resid, 3 gact (the GEGLU first projection's activation output), 4 gu (the second projection: the pre-activation u)
 *   CONV       0 x, 1 y, 2 resid, 3 rowvec (the time-embedding row vector [B][Cout], a column slice), 4 x_low (the nearest-2x input of up2)
 *   GROUPNORM / LAYERNORM / SILU / UPSAMPLE   0 x, 1 y
 *   ATTN       0 q, 1 o, 3 kv (self attention: q == kv == the fused q | k | v tensor, k at column C, v at 2 C; cross: k at 0, v at C of kv)
 *   CONCAT     0 a, 1 o, 3 b
 *   EMBED_IN   0 te_sin, 1 aug_in, 3 tid_emb
 * Gradient destinations: dy_off the output gradient read; dx / dres / d3 the (out, addend) pairs of Plan::grad_dst for role 0 (LINEAR with gu:
 * for gu), role 2 and role 3; an absent pair is NONE / NONE.  resid_alias: the residual's gradient IS dy (no launch).
 * intact_after_step: bit r = the DATA of role r, bit 8 + r = its GRADIENT (for role 1: dy) holds after a finished step what the op read or wrote;
 * a clear bit = never produced in this plan or overwritten by a later launch of the same step: an audit must skip that role. */
#define SDXL_PLAN_NONE ((size_t)-1)
#define SDXL_PLAN_ROLES 5
enum { SDXL_OP_LINEAR = 0, SDXL_OP_CONV = 1, SDXL_OP_GROUPNORM = 2, SDXL_OP_LAYERNORM = 3, SDXL_OP_ATTN = 4, SDXL_OP_SILU = 5, SDXL_OP_CONCAT = 6,
       SDXL_OP_UPSAMPLE = 7, SDXL_OP_EMBED_IN = 8 };
typedef struct sdxl_plan_tensor {
  size_t off, goff;            /* data / gradient (goff: NONE without one) */
  long rows, cols, ld;         /* ld: row stride in elements (a column slice: the parent's width) */
  int pad_rows, col0;          /* rows allocated behind `rows`; first column inside the parent */
} sdxl_plan_tensor;
typedef struct sdxl_plan_op_desc {
  int kind, seg, hoist_fwd, resid_alias;
  unsigned intact_after_step;
  int K, N, splitk, wgroup, crcfg, crsplit, fsplit, dsplit, delta_on, ln_mode, ggroup;      /* LINEAR (splitk, fsplit, dsplit: CONV too) */
  int B, H, W, Cin, Cout, stride, up2, up_fs, up_ds, up_ws, up_wg, three_tap, rows_per_batch, s2_dgrad;      /* CONV; B, H, W, Cin (= C): UPSAMPLE; B, H (= HW), Cin (= C): GROUPNORM */
  int groups, silu;            /* GROUPNORM */
  int heads, Nq, Nk, self_attn, qsplit, delta_fused, bwd_route;      /* ATTN; bwd_route: 0 dq + dkv, 1 dq + split dkv + reduce, 2 fused, 3 pipelined, -1 unknown (no workspace bound) */
  int skip, first;             /* CONCAT */
  int dims[4];                 /* EMBED_IN: ch0, addition_time_embed_dim, pooled_dim, 0 */
  float eps;
  long ldq, ldk, ldv, ldvec;   /* ATTN row strides; CONV: the row vector's */
  size_t dy_off, dx_out, dx_addend, dres_out, dres_addend, d3_out, d3_addend, dy32_off;
  size_t w_off, w_numel, b_off, b_numel;      /* weight | gamma, bias | beta */
  size_t stats_off, lse_off, delta_off, rv32_off, planar_off, weff_off, dweff_off, s2_planar_off;
  sdxl_plan_tensor t[SDXL_PLAN_ROLES];
} sdxl_plan_op_desc;
/* buffers that belong to no op */
typedef struct sdxl_plan_tail {
  int B, H, W, ctx;
  sdxl_plan_tensor x_in, pred, ehs;
  size_t tp32_off, tp32_bytes, t_off, tid_off, loss_off, workspace_bytes;
} sdxl_plan_tail;
SDXL_API int sdxl_debug_plan_num_ops(sdxl_handle* h, int* n);
/* out_bytes: sizeof the caller's struct; a size that is not the library's is refused before anything else is looked at (a binding whose
 * layout has drifted can never be written past) */
SDXL_API int sdxl_debug_plan_op(sdxl_handle* h, int i, sdxl_plan_op_desc* out, size_t out_bytes);
SDXL_API int sdxl_debug_plan_tail(sdxl_handle* h, sdxl_plan_tail* out, size_t out_bytes);
/* The loss's buffers in the current plan (byte offsets into the workspace, named after the Plan fields of csrc/engine.h; NONE where the plan
 * reserves none): the partial rows of loss_fwd_kernel, the [B] per-sample losses, the [B] masked_mean normaliser and the staged copies graph
 * mode reads in place of the caller's arrays.  staged: 1 when the last sdxl_forward_loss handed the loss kernels the staged copies, 0 the
 * caller's arrays, -1 before the first one.  part_floats: loss_part_floats(B, HW); ps_slots: loss_ps_slots(B, HW).  Pure host code. */
typedef struct sdxl_plan_loss {
  size_t loss_part_off, ps_loss_off, mask_norm_off;
  size_t in_lat_off, in_noise_off, in_nin_off, in_sig_off, in_tag_off, in_sw_off, in_hc_off, in_mask_off, in_cond_off;
  size_t part_floats;
  int ps_slots, staged;
} sdxl_plan_loss;
SDXL_API int sdxl_debug_plan_loss(sdxl_handle* h, sdxl_plan_loss* out, size_t out_bytes);

/* ---- part 2: experiment ABI (diagnostics build only) ---- */
/* the linear dgrad whose epilogue runs the backward of the LayerNorm that produced its input (csrc/kernels.h, GemmP::ln_x): dY [M][K] bf16,
 * W [K][N] bf16 (N = the LayerNorm width), x [M][N] the LayerNorm's input, stats [M][2] its (mean, rstd), gamma [N]; dx [M][N] = the
 * LayerNorm's input gradient (+ addend, or null); dy_out (or null) [M][N] = dY W; pcol (or null) [cdiv(M, 128)][2][N] fp32 partial sums of
 * dgamma | dbeta per 128-row block.  N <= 1280, cdiv(M, 128) * cdiv(N, 128) <= 512.  Runs the launch three times (epochs 1, 2, 3) on one scratch
 * buffer, zeroed on `stream` first; stream-ordered (it does not synchronise). */
SDXL_API int sdxl_op_linear_dgrad_ln_bwd(const void* dy, const void* w, const void* x, const float* stats, const void* gamma, const void* addend,
                                void* dx, void* dy_out, float* pcol, int M, int N, int K, void* stream);

/* experiment knobs of the plan (A/B runs; 0 = the shipped policy): see csrc/kernels.h.  Process-global, read at plan-build, forward
 * and backward time: set them before sdxl_plan / the first step and do not change them while a handle is in use. */
SDXL_API int sdxl_set_knob(int id, int value);
/* Persistent stream-K GEMM (csrc/gemm_sk.hip; 256 x 256 tiles, one workgroup per CU, the K-steps of ALL problems of a launch
 * cut evenly over the CUs).  sdxl_set_sk_mode: mode 0 = never (default), 1 = the policy gemm_use_sk, 2 = wherever a problem is
 * applicable (M, N multiples of 256, K of 64); workers > 0 forces the worker count (microbenchmarks), 0 = policy.
 * sdxl_sk_error: *out != 0 iff an owner workgroup ever gave up waiting for a partial tile on that stream (results invalid:
 * callers of modes 1 / 2 must check it).
 * sdxl_op_gemm_sk: n (<= 4) problems in ONE launch, arguments per problem as the single-problem GEMM op takes them (form 2: bias[i] = fp32 bias
 * gradient accumulator or NULL, C fp32). */
SDXL_API int sdxl_set_sk_mode(int mode, int workers);
SDXL_API int sdxl_sk_error(void* stream, unsigned* out);
/* *out != 0 iff a LayerNorm-backward epilogue (sdxl_op_linear_dgrad_ln_bwd, knob 26) gave up its in-launch meeting since the last call (bit 0: the ready
 * flags of its row block's other column tiles, bit 1: a granule): the results of that launch are invalid.  Synchronises the device; clears the word. */
SDXL_API int sdxl_ln_error(unsigned* out);
/* L2 prefetch of the weight (B operand) of a coming one-round launch of the pipelined kernel (form 0 NT: B [N][ldb]; 1 NN: B [K][ldb]), on `stream`:
 * workgroup i (XCD i % 8) reads the columns that XCD's tiles will stage, `parts` workgroups per XCD (profiles/tools/l2_prefetch_bench.py). */
SDXL_API int sdxl_op_pl_prefetch_b(int form, const void* B, int M, int N, int K, long ldb, int parts, void* stream);
SDXL_API int sdxl_op_gemm_sk(int n, const int* form, const void* const* A, const void* const* B, void* const* C, const int* M,
                    const int* N, const int* K, const void* const* bias, const void* const* resid, const int* accumulate,
                    void* stream);
/* The stride-2 3x3 convolution (pad 1, H and W even) on the four phase planes of its input, and its weight / bias gradient from the
   same planes: xplanar [4 * roundup(B*(H/2)*(W/2), 128)][Cin] bf16 is written by _fwd and read by _wgrad; y / dy [B][H/2][W/2][Cout];
   dw [Cout][9][Cin] fp32 (accumulate 0: =, 1: +=), dbias += (may be NULL). */
SDXL_API int sdxl_op_conv3x3_s2_fwd(const void* x, const void* w, const void* bias, void* xplanar, void* y, int B, int H, int W, int Cin,
                           int Cout, void* stream);
SDXL_API int sdxl_op_conv3x3_s2_wgrad(const void* dy, const void* xplanar, float* dw, float* dbias, int accumulate, int B, int H, int W, int Cin,
                             int Cout, int splitk, void* stream);

#ifdef __cplusplus
}
#endif
#endif
