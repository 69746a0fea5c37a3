// LoRA by merge and project (include/sdxlstep.h, SDXL_DTYPE_LORA): the engine, the plan and every other kernel never see an adapter.
//   merge    W[o][i]  = bf16_rn(W0[o][i] + s * sum_k B[o][k] A[k][i])      into the weight arena, before the forward
//   project  dB[o][k] = s * sum_i dW[o][i] A[k][i],  dA[k][i] = s * sum_o B[o][k] dW[o][i]      from the fp32 gradient arena, behind the backward
// All three kernels are table-driven: one launch covers every target, a workgroup finds its (target, tile) by a binary search of the
// targets' first-tile indices.  The single-target test hooks pass their one descriptor by value (LoraP::one, table == nullptr).
// No atomics anywhere; every reduction order is fixed by (out, in, rank) and the target's kind alone, so a target's bits do not depend on the
// table around it.
// Packed layouts (SDXL_DTYPE_LORA_LAYOUTS; LoraTarget::kind, kernels.h): a native row is `in` elements long for every kind, so the tiles walk
// NATIVE rows and columns, W0 / W / dW stay on contiguous 16-byte vectors, and only the indices into the small operands are mapped while they
// are staged through LDS (lora_src_col into A / dA, lora_src_row into B / dB).  Every kernel is instantiated twice: MAPPED = false is the code
// a table of plain targets has always run (it never reads kind / cg / nrows), MAPPED = true is taken when LoraP::mapped says that some target
// needs a map, and runs the plain targets of such a table with the identity maps and the same arithmetic in the same order.
#include "kernels.h"

namespace {

// ---- merge: 32 x 64 tile, thread = (row tid / 8, the 8 columns of one 16-byte vector) ----
// acc <- acc + B[o][k] * A[k][i] for k = 0 .. rank - 1, every product and sum rounded on its own; t = s * acc; W = bf16_rn(W0 + t), and
// W = W0 where t == 0 (so s = 0 or B = 0 give back W0's bits, a -0 included).  tests/_lora_ref.py restates it in torch, bit for bit.
// (hipcc's default -ffp-contract would fuse them, also behind __fmul_rn / __fadd_rn, whose bodies are compiled under it: contraction is
// switched off for this kernel and the operators are written out)
template <bool MAPPED>
__global__ __launch_bounds__(256) void lora_merge_kernel(const LoraP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float As[LORA_M_KC][LORA_M_COLS];
  __shared__ float Bs[LORA_M_ROWS][LORA_M_KC + 1];
  const LoraTarget t = adapter_find<&LoraTarget::tile_m>(p, (int)blockIdx.x);
  const int tid = threadIdx.x, local = (int)blockIdx.x - t.tile_m, ncb = (t.in + LORA_M_COLS - 1) / LORA_M_COLS;
  const int rb = local / ncb, cb = local - rb * ncb;
  const int lr = tid >> 3, lc = (tid & 7) * 8;
  const int row = rb * LORA_M_ROWS + lr, col = cb * LORA_M_COLS + lc;
  const bf16* A = p.a + t.a_off;
  const bf16* B = p.b + t.b_off;
  const int kind = MAPPED ? t.kind : LORA_KIND_PLAIN, cg = MAPPED ? t.cg : 1, c4 = t.out >> 1, nrows = MAPPED ? t.nrows : t.out;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int k0 = 0; k0 < p.rank; k0 += LORA_M_KC) {
    const int kc = min(LORA_M_KC, p.rank - k0);
    __syncthreads();
    for (int idx = tid; idx < kc * LORA_M_COLS; idx += 256) {
      const int k = idx / LORA_M_COLS, c = idx - k * LORA_M_COLS, gc = cb * LORA_M_COLS + c;
      As[k][c] = gc < t.in ? (float)A[(long)(k0 + k) * t.in + (MAPPED ? lora_src_col(kind, cg, gc) : gc)] : 0.f;
    }
    for (int idx = tid; idx < LORA_M_ROWS * LORA_M_KC; idx += 256) {
      const int r = idx / LORA_M_KC, k = idx - r * LORA_M_KC, gr = rb * LORA_M_ROWS + r;
      if (k < kc) Bs[r][k] = gr < t.out ? (float)B[(long)(MAPPED ? lora_src_row(kind, cg, c4, gr) : gr) * p.rank + k0 + k] : 0.f;
    }
    __syncthreads();
    for (int k = 0; k < kc; ++k) {
      const float b = Bs[lr][k];
      const f32x4 a0 = *(const f32x4*)&As[k][lc], a1 = *(const f32x4*)&As[k][lc + 4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p0 = b * a0[j], p1 = b * a1[j];
        acc[j] = acc[j] + p0;
        acc[j + 4] = acc[j + 4] + p1;
      }
    }
  }
  if (row < nrows && col < t.in) {        // in % 8 == 0: a vector is whole or absent (a native row past `out`: acc == 0, W0's bits)
    const long e = (long)row * t.in + col;
    const bf16x8 w0 = *(const bf16x8*)(p.base + t.base_off + e);
    bf16x8 w;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = p.scale * acc[j];
      const float sum = (float)w0[j] + d;
      w[j] = d == 0.f ? w0[j] : (bf16)sum;
    }
    *(bf16x8*)(p.w + t.w_off + e) = w;
  }
}

// ---- dB: one workgroup per (target, 32 rows), looping over `in` in steps of 256 columns and over the rank in steps of 16 ----
// thread = (lane column group j = tid % 16, rows tid / 16 and tid / 16 + 16): partial sums over the columns 256 c + 64 q + 4 j + (0..3) in
// ascending order, then the 16 partials of a row are added in a butterfly (xor 1, 2, 4, 8): the order depends on (in, rank) only.
template <bool MAPPED>
__global__ __launch_bounds__(256) void lora_db_kernel(const LoraP p) {
  __shared__ __attribute__((aligned(16))) float As[LORA_B_KC][LORA_B_COLS];
  const LoraTarget t = adapter_find<&LoraTarget::tile_b>(p, (int)blockIdx.x);
  const int tid = threadIdx.x, j = tid & 15, rr = tid >> 4;
  const int r0 = ((int)blockIdx.x - t.tile_b) * LORA_B_ROWS + rr, r1 = r0 + 16;
  const bf16* A = p.a + t.a_off;
  const float* d0 = p.dw + t.w_off + (long)r0 * t.in;
  const float* d1 = p.dw + t.w_off + (long)r1 * t.in;
  float* dB = p.gb + t.gb_off;
  const int kind = MAPPED ? t.kind : LORA_KIND_PLAIN, cg = MAPPED ? t.cg : 1;
  const int s0 = MAPPED && r0 < t.out ? lora_src_row(kind, cg, t.out >> 1, r0) : r0;      // r0, r1: native rows; s0, s1: their rows of dB
  const int s1 = MAPPED && r1 < t.out ? lora_src_row(kind, cg, t.out >> 1, r1) : r1;
  for (int k0 = 0; k0 < p.rank; k0 += LORA_B_KC) {
    float acc0[LORA_B_KC], acc1[LORA_B_KC];
#pragma unroll
    for (int k = 0; k < LORA_B_KC; ++k) acc0[k] = acc1[k] = 0.f;
    for (int c0 = 0; c0 < t.in; c0 += LORA_B_COLS) {
      __syncthreads();
#pragma unroll
      for (int m = 0; m < LORA_B_KC * LORA_B_COLS / 8 / 256; ++m) {      // 16 x 256 bf16 as 16-byte vectors
        const int idx = tid + 256 * m, k = idx / (LORA_B_COLS / 8), v = idx - k * (LORA_B_COLS / 8), gc = c0 + v * 8;
        bf16x8 a;
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = (bf16)0.f;
        if (k0 + k < p.rank && gc < t.in) {
          if (MAPPED && kind == LORA_KIND_CONV3) {      // the 8 native columns gc .. gc + 7 are 8 scattered columns of A
            const bf16* ar = A + (long)(k0 + k) * t.in;
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = ar[lora_src_col(kind, cg, gc + e)];
          } else a = *(const bf16x8*)(A + (long)(k0 + k) * t.in + gc);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) As[k][v * 8 + e] = (float)a[e];
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < LORA_B_COLS / 64; ++q) {
        const int c = q * 64 + 4 * j, gc = c0 + c;
        if (gc < t.in) {                  // in % 4 == 0
          f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = {0.f, 0.f, 0.f, 0.f};
          if (r0 < t.out) x0 = *(const f32x4*)(d0 + gc);
          if (r1 < t.out) x1 = *(const f32x4*)(d1 + gc);
#pragma unroll
          for (int k = 0; k < LORA_B_KC; ++k) {
            const f32x4 a = *(const f32x4*)&As[k][c];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              acc0[k] = fmaf(x0[e], a[e], acc0[k]);
              acc1[k] = fmaf(x1[e], a[e], acc1[k]);
            }
          }
        }
      }
    }
    float mine0 = 0.f, mine1 = 0.f;
#pragma unroll
    for (int k = 0; k < LORA_B_KC; ++k) {
      float v0 = acc0[k], v1 = acc1[k];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        v0 += __shfl_xor(v0, o, 64);
        v1 += __shfl_xor(v1, o, 64);
      }
      if (k == j) { mine0 = v0; mine1 = v1; }
    }
    if (k0 + j < p.rank) {
      if (r0 < t.out) dB[(long)s0 * p.rank + k0 + j] = p.scale * mine0;
      if (r1 < t.out) dB[(long)s1 * p.rank + k0 + j] = p.scale * mine1;
    }
  }
}

// ---- dA: one workgroup per (target, 128 columns), looping over `out` sequentially, the accumulators in registers ----
// wave g holds the ranks [g KPT, (g + 1) KPT) of the columns (lane, lane + 64): its B reads are wave-uniform.  acc <- fma(B[o][k], dW[o][i], acc)
// for the native rows 0 .. out - 1 in ascending order (rows past `out` of the last step of 32 add +0): the order depends on `out` and the kind only.
template <int KPT, bool MAPPED>
__global__ __launch_bounds__(256) void lora_da_kernel(const LoraP p) {
  __shared__ __attribute__((aligned(16))) float Ds[LORA_A_ROWS][LORA_A_COLS];
  __shared__ __attribute__((aligned(16))) float Bs[LORA_A_ROWS][4 * KPT];
  const LoraTarget t = adapter_find<&LoraTarget::tile_a>(p, (int)blockIdx.x);
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const int col0 = ((int)blockIdx.x - t.tile_a) * LORA_A_COLS;
  const bf16* B = p.b + t.b_off;
  const float* dw = p.dw + t.w_off;
  const int kind = MAPPED ? t.kind : LORA_KIND_PLAIN, cg = MAPPED ? t.cg : 1, c4 = t.out >> 1;
  float acc0[KPT], acc1[KPT];
#pragma unroll
  for (int k = 0; k < KPT; ++k) acc0[k] = acc1[k] = 0.f;
  for (int o0 = 0; o0 < t.out; o0 += LORA_A_ROWS) {
    __syncthreads();
#pragma unroll
    for (int m = 0; m < LORA_A_ROWS * LORA_A_COLS / 4 / 256; ++m) {
      const int idx = tid + 256 * m, r = idx / (LORA_A_COLS / 4), v = idx - r * (LORA_A_COLS / 4), gc = col0 + 4 * v;
      f32x4 x = {0.f, 0.f, 0.f, 0.f};
      if (o0 + r < t.out && gc < t.in) x = *(const f32x4*)(dw + (long)(o0 + r) * t.in + gc);
      *(f32x4*)&Ds[r][4 * v] = x;
    }
    for (int idx = tid; idx < LORA_A_ROWS * 4 * KPT; idx += 256) {
      const int r = idx / (4 * KPT), k = idx - r * (4 * KPT);
      Bs[r][k] = (o0 + r < t.out && k < p.rank) ? (float)B[(long)(MAPPED ? lora_src_row(kind, cg, c4, o0 + r) : o0 + r) * p.rank + k] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < LORA_A_ROWS; ++r) {
      const float x0 = Ds[r][lane], x1 = Ds[r][lane + 64];
#pragma unroll
      for (int k = 0; k < KPT; k += 4) {
        const f32x4 b = *(const f32x4*)&Bs[r][g * KPT + k];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc0[k + e] = fmaf(b[e], x0, acc0[k + e]);
          acc1[k + e] = fmaf(b[e], x1, acc1[k + e]);
        }
      }
    }
  }
  float* dA = p.ga + t.ga_off;
  const int n0 = col0 + lane, n1 = n0 + 64;      // native columns; c0, c1: their columns of dA
  const int c0 = MAPPED && n0 < t.in ? lora_src_col(kind, cg, n0) : n0, c1 = MAPPED && n1 < t.in ? lora_src_col(kind, cg, n1) : n1;
#pragma unroll
  for (int k = 0; k < KPT; ++k) {
    const int gk = g * KPT + k;
    if (gk < p.rank) {
      if (n0 < t.in) dA[(long)gk * t.in + c0] = p.scale * acc0[k];
      if (n1 < t.in) dA[(long)gk * t.in + c1] = p.scale * acc1[k];
    }
  }
}

}  // namespace

int launch_lora_merge(const LoraP& p, hipStream_t st) {
  if (p.mapped) hipLaunchKernelGGL(lora_merge_kernel<true>, dim3(p.tiles_m), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(lora_merge_kernel<false>, dim3(p.tiles_m), dim3(256), 0, st, p);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

template <bool MAPPED>
static void launch_lora_da(const LoraP& p, hipStream_t st) {
  if (p.rank <= 16) hipLaunchKernelGGL((lora_da_kernel<4, MAPPED>), dim3(p.tiles_a), dim3(256), 0, st, p);
  else if (p.rank <= 32) hipLaunchKernelGGL((lora_da_kernel<8, MAPPED>), dim3(p.tiles_a), dim3(256), 0, st, p);
  else if (p.rank <= 64) hipLaunchKernelGGL((lora_da_kernel<16, MAPPED>), dim3(p.tiles_a), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((lora_da_kernel<32, MAPPED>), dim3(p.tiles_a), dim3(256), 0, st, p);
}

int launch_lora_project(const LoraP& p, hipStream_t st) {
  if (p.mapped) hipLaunchKernelGGL(lora_db_kernel<true>, dim3(p.tiles_b), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(lora_db_kernel<false>, dim3(p.tiles_b), dim3(256), 0, st, p);
  HIP_CHECK_RET(hipGetLastError());
  if (p.mapped) launch_lora_da<true>(p, st); else launch_lora_da<false>(p, st);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
