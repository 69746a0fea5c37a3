// DoRA by merge and project (include/sdxlstep.h, SDXL_DTYPE_DORA): LoRA's merged weight with every output row rescaled by a trained magnitude.
//   v[o][i] = W0[o][i] + s * sum_k B[o][k] A[k][i]        LoRA's chain (lora.hip), every product and sum rounded on its own
//   n_o = sqrt(sum_i v^2),  n0_o = n_o at s B A == 0,  q_o = n0_o / n_o (1 when n_o == 0),  c_o = (1 + mu_o) q_o
//   merge    W[o][i] = bf16_rn(c_o v[o][i]), and W0's bits where s * acc == 0 and c_o == 1
//   project  dmu_o = q_o sum_i G v,  dB[o][k] = c_o (s sum_i G A[k][i]),  dA[k][i] = s sum_o (c_o B[o][k]) G[o][i]      (n_o held constant)
// One row-reduction kernel serves norm (merge), norm0 (init) and dmu (project); the merge and the two projections are lora.hip's loop shapes
// with c_o applied.  Table-driven like lora.hip: the same LoraTarget kinds and maps, MAPPED on and off, native rows on 16-byte vectors.
// No atomics, no out x in scratch; every summation order is fixed by (out, in, rank, kind) alone.  mu, dmu, norm0 and norm are indexed like the
// state-dict rows (lora_src_row of the native row).
#include "kernels.h"

namespace {

// c_o of the state-dict row `srow`: one division, one sum, one product, each rounded on its own
__device__ __forceinline__ float dora_q(const DoraP& p, const DoraTarget& x, int srow) {
  const float n0 = p.norm0[x.n_off + srow], n = p.norm[x.n_off + srow];
  return n == 0.f ? 1.f : n0 / n;
}
__device__ __forceinline__ float dora_c(const DoraP& p, const DoraTarget& x, int srow) {
#pragma clang fp contract(off)
  const float q = dora_q(p, x, srow);
  const float m = 1.f + (float)p.mu[x.mu_off + srow];
  return m * q;
}

// ---- row reductions: one workgroup per (target, 32 rows), looping over `in` in passes of 64 columns ----
// thread = (row tid / 8, the 8 columns of one 16-byte vector of each pass).  v is formed exactly as the merge forms it; the thread adds its
// terms (v * v, or G * v) for the columns 64 c + 8 (tid % 8) + (0 .. 7), c ascending, each product and sum rounded on its own, and the 8
// partials of a row are added in a butterfly (xor 1, 2, 4): the order depends on `in` only.
template <int MODE, bool MAPPED>
__global__ __launch_bounds__(256) void dora_rows_kernel(const DoraP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float As[DORA_R_KC][DORA_R_COLS];
  __shared__ float Bs[DORA_R_ROWS][DORA_R_KC + 1];
  const DoraTarget x = adapter_find<&LoraTarget::tile_b>(p, (int)blockIdx.x);
  const LoraTarget& t = x.t;
  const int tid = threadIdx.x, rb = (int)blockIdx.x - t.tile_b;
  const int lr = tid >> 3, lc = (tid & 7) * 8;
  const int row = rb * DORA_R_ROWS + lr;
  const bf16* A = p.a + t.a_off;
  const bf16* B = p.b + t.b_off;
  const int kind = MAPPED ? t.kind : LORA_KIND_PLAIN, cg = MAPPED ? t.cg : 1, c4 = t.out >> 1;
  float part = 0.f;
  for (int c0 = 0; c0 < t.in; c0 += DORA_R_COLS) {
    const int col = c0 + lc;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    if (MODE != DORA_R_NORM0) {
      for (int k0 = 0; k0 < p.rank; k0 += DORA_R_KC) {
        const int kc = min(DORA_R_KC, p.rank - k0);
        __syncthreads();
        for (int idx = tid; idx < kc * DORA_R_COLS; idx += 256) {
          const int k = idx / DORA_R_COLS, c = idx - k * DORA_R_COLS, gc = c0 + c;
          As[k][c] = gc < t.in ? (float)A[(long)(k0 + k) * t.in + (MAPPED ? lora_src_col(kind, cg, gc) : gc)] : 0.f;
        }
        for (int idx = tid; idx < DORA_R_ROWS * DORA_R_KC; idx += 256) {
          const int r = idx / DORA_R_KC, k = idx - r * DORA_R_KC, gr = rb * DORA_R_ROWS + r;
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
    }
    if (row < t.out && col < t.in) {        // in % 8 == 0: a vector is whole or absent
      const long e = (long)row * t.in + col;
      const bf16x8 w0 = *(const bf16x8*)(p.base + t.base_off + e);
      f32x4 g0 = {0.f, 0.f, 0.f, 0.f}, g1 = {0.f, 0.f, 0.f, 0.f};
      if (MODE == DORA_R_DMU) {
        g0 = *(const f32x4*)(p.dw + t.w_off + e);
        g1 = *(const f32x4*)(p.dw + t.w_off + e + 4);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = MODE == DORA_R_NORM0 ? 0.f : p.scale * acc[j];
        const float v = (float)w0[j] + d;
        const float term = MODE == DORA_R_DMU ? (j < 4 ? g0[j] : g1[j - 4]) * v : v * v;
        part = part + term;
      }
    }
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) part = part + __shfl_xor(part, o, 64);
  if (row < t.out && (tid & 7) == 0) {
    const int srow = MAPPED ? lora_src_row(kind, cg, c4, row) : row;
    if (MODE == DORA_R_NORM) p.norm[x.n_off + srow] = sqrtf(part);
    else if (MODE == DORA_R_NORM0) p.norm0[x.n_off + srow] = sqrtf(part);
    else p.gmu[x.mu_off + srow] = dora_q(p, x, srow) * part;
  }
}

// ---- merge: lora_merge_kernel's 32 x 64 tile and chain, then W = bf16_rn(c_o (W0 + t)), and W0's bits where t == 0 and c_o == 1 ----
// RESTORE: W = W0 on the same tiles; no adapter, no norm is read
template <bool MAPPED, bool RESTORE>
__global__ __launch_bounds__(256) void dora_merge_kernel(const DoraP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float As[LORA_M_KC][LORA_M_COLS];
  __shared__ float Bs[LORA_M_ROWS][LORA_M_KC + 1];
  const DoraTarget x = adapter_find<&LoraTarget::tile_m>(p, (int)blockIdx.x);
  const LoraTarget& t = x.t;
  const int tid = threadIdx.x, local = (int)blockIdx.x - t.tile_m, ncb = (t.in + LORA_M_COLS - 1) / LORA_M_COLS;
  const int rb = local / ncb, cb = local - rb * ncb;
  const int lr = tid >> 3, lc = (tid & 7) * 8;
  const int row = rb * LORA_M_ROWS + lr, col = cb * LORA_M_COLS + lc;
  const bool mine = row < t.out && col < t.in;        // in % 8 == 0: a vector is whole or absent
  const long e = (long)row * t.in + col;
  if (RESTORE) {
    if (mine) *(bf16x8*)(p.w + t.w_off + e) = *(const bf16x8*)(p.base + t.base_off + e);
    return;
  }
  const bf16* A = p.a + t.a_off;
  const bf16* B = p.b + t.b_off;
  const int kind = MAPPED ? t.kind : LORA_KIND_PLAIN, cg = MAPPED ? t.cg : 1, c4 = t.out >> 1;
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
  if (mine) {
    const float c = dora_c(p, x, MAPPED ? lora_src_row(kind, cg, c4, row) : row);
    const bf16x8 w0 = *(const bf16x8*)(p.base + t.base_off + e);
    bf16x8 w;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = p.scale * acc[j];
      const float v = (float)w0[j] + d;
      const float cv = c * v;
      w[j] = d == 0.f && c == 1.f ? w0[j] : (bf16)cv;
    }
    *(bf16x8*)(p.w + t.w_off + e) = w;
  }
}

// ---- dB: lora_db_kernel, the row's result times c_o ----
// one workgroup per (target, 32 rows), looping over `in` in steps of 256 columns and over the rank in steps of 16; thread = (lane column group
// j = tid % 16, rows tid / 16 and tid / 16 + 16): partial sums over the columns 256 c + 64 q + 4 j + (0..3) in ascending order, then the 16
// partials of a row are added in a butterfly (xor 1, 2, 4, 8): the order depends on (in, rank) only.
template <bool MAPPED>
__global__ __launch_bounds__(256) void dora_db_kernel(const DoraP p) {
  __shared__ __attribute__((aligned(16))) float As[LORA_B_KC][LORA_B_COLS];
  const DoraTarget x = adapter_find<&LoraTarget::tile_b>(p, (int)blockIdx.x);
  const LoraTarget& t = x.t;
  const int tid = threadIdx.x, j = tid & 15, rr = tid >> 4;
  const int r0 = ((int)blockIdx.x - t.tile_b) * LORA_B_ROWS + rr, r1 = r0 + 16;
  const bf16* A = p.a + t.a_off;
  const float* d0 = p.dw + t.w_off + (long)r0 * t.in;
  const float* d1 = p.dw + t.w_off + (long)r1 * t.in;
  float* dB = p.gb + t.gb_off;
  const int kind = MAPPED ? t.kind : LORA_KIND_PLAIN, cg = MAPPED ? t.cg : 1;
  const int s0 = MAPPED && r0 < t.out ? lora_src_row(kind, cg, t.out >> 1, r0) : r0;      // r0, r1: native rows; s0, s1: their rows of dB
  const int s1 = MAPPED && r1 < t.out ? lora_src_row(kind, cg, t.out >> 1, r1) : r1;
  const float cr0 = r0 < t.out ? dora_c(p, x, s0) : 0.f, cr1 = r1 < t.out ? dora_c(p, x, s1) : 0.f;
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
      if (r0 < t.out) dB[(long)s0 * p.rank + k0 + j] = cr0 * (p.scale * mine0);
      if (r1 < t.out) dB[(long)s1 * p.rank + k0 + j] = cr1 * (p.scale * mine1);
    }
  }
}

// ---- dA: lora_da_kernel with c_o B[o][k] staged in place of B[o][k] ----
// one workgroup per (target, 128 columns), looping over `out` sequentially, the accumulators in registers; wave g holds the ranks
// [g KPT, (g + 1) KPT) of the columns (lane, lane + 64).  acc <- fma(c_o B[o][k], dW[o][i], acc) for the native rows 0 .. out - 1 in ascending
// order (rows past `out` of the last step of 32 add +0): the order depends on `out` and the kind only.
template <int KPT, bool MAPPED>
__global__ __launch_bounds__(256) void dora_da_kernel(const DoraP p) {
  __shared__ __attribute__((aligned(16))) float Ds[LORA_A_ROWS][LORA_A_COLS];
  __shared__ __attribute__((aligned(16))) float Bs[LORA_A_ROWS][4 * KPT];
  __shared__ float Cs[LORA_A_ROWS];      // c_o and the state-dict row of the step's rows
  __shared__ int Rs[LORA_A_ROWS];
  const DoraTarget x = adapter_find<&LoraTarget::tile_a>(p, (int)blockIdx.x);
  const LoraTarget& t = x.t;
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
      f32x4 xv = {0.f, 0.f, 0.f, 0.f};
      if (o0 + r < t.out && gc < t.in) xv = *(const f32x4*)(dw + (long)(o0 + r) * t.in + gc);
      *(f32x4*)&Ds[r][4 * v] = xv;
    }
    if (tid < LORA_A_ROWS) {                // c_o once per row of the step
      const bool live = o0 + tid < t.out;
      Rs[tid] = live ? (MAPPED ? lora_src_row(kind, cg, c4, o0 + tid) : o0 + tid) : 0;
      Cs[tid] = live ? dora_c(p, x, Rs[tid]) : 0.f;
    }
    __syncthreads();
    for (int idx = tid; idx < LORA_A_ROWS * 4 * KPT; idx += 256) {
      const int r = idx / (4 * KPT), k = idx - r * (4 * KPT);
      Bs[r][k] = (o0 + r < t.out && k < p.rank) ? Cs[r] * (float)B[(long)Rs[r] * p.rank + k] : 0.f;
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

template <int MODE>
int launch_rows(const DoraP& p, hipStream_t st) {
  if (p.mapped) hipLaunchKernelGGL((dora_rows_kernel<MODE, true>), dim3(p.tiles_b), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((dora_rows_kernel<MODE, false>), dim3(p.tiles_b), dim3(256), 0, st, p);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

template <bool MAPPED>
void launch_da(const DoraP& p, hipStream_t st) {
  if (p.rank <= 16) hipLaunchKernelGGL((dora_da_kernel<4, MAPPED>), dim3(p.tiles_a), dim3(256), 0, st, p);
  else if (p.rank <= 32) hipLaunchKernelGGL((dora_da_kernel<8, MAPPED>), dim3(p.tiles_a), dim3(256), 0, st, p);
  else if (p.rank <= 64) hipLaunchKernelGGL((dora_da_kernel<16, MAPPED>), dim3(p.tiles_a), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((dora_da_kernel<32, MAPPED>), dim3(p.tiles_a), dim3(256), 0, st, p);
}

}  // namespace

int launch_dora_init(const DoraP& p, hipStream_t st) { return launch_rows<DORA_R_NORM0>(p, st); }

int launch_dora_merge(const DoraP& p, hipStream_t st) {
  if (int r = launch_rows<DORA_R_NORM>(p, st)) return r;
  if (p.mapped) hipLaunchKernelGGL((dora_merge_kernel<true, false>), dim3(p.tiles_m), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((dora_merge_kernel<false, false>), dim3(p.tiles_m), dim3(256), 0, st, p);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_dora_restore(const DoraP& p, hipStream_t st) {
  hipLaunchKernelGGL((dora_merge_kernel<false, true>), dim3(p.tiles_m), dim3(256), 0, st, p);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_dora_project(const DoraP& p, hipStream_t st) {
  if (int r = launch_rows<DORA_R_DMU>(p, st)) return r;
  if (p.mapped) hipLaunchKernelGGL(dora_db_kernel<true>, dim3(p.tiles_b), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(dora_db_kernel<false>, dim3(p.tiles_b), dim3(256), 0, st, p);
  HIP_CHECK_RET(hipGetLastError());
  if (p.mapped) launch_da<true>(p, st); else launch_da<false>(p, st);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
