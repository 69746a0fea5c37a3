// Direct LoRA adapter gradients (include/sdxlstep.h, sdxl_grad_select.lora): for a target W [out][in] of a linear layer with input X [M][in] and
// output gradient dY [M][out] (a column slice of the op's dY, row stride ldy >= out),
//   T = X A^T [M][r],  U = dY B [M][r],      dB (+)= s dY^T T [out][r],      dA (+)= s U^T X [r][in]
// -- the LoRA gradients at the merged weight without ever forming dW [out][in].  Three table-driven launches cover every target of one op:
//   1. lora_tu_kernel    T and U of 64 rows per workgroup on the 16x16x32 bf16 MFMA (operands straight from global memory: both are
//                        k-contiguous), rounded ONCE to bf16 and stored TRANSPOSED, Tt | Ut [R][Mp], R = the rank padded to 16, Mp = M padded
//                        to 64; ranks past r and rows past M are zeros (computed from zero fragments: rows past M are never read)
//   2. lora_part_kernel  partial [r][in | out] blocks = Ut . X | Tt . dY over a fixed row chunk of LORA_G_CHUNK rows per workgroup and 128
//                        columns: the X / dY tile is loaded in whole 16-byte vectors and transposed through LDS ([column][row], the MFMA's
//                        B fragment is then one 16-byte read), the Ut / Tt fragment comes from global memory (L2: 2 r Mp bytes per target)
//   3. lora_red_kernel   adds the chunks' partials in ascending chunk order, scales, and overwrites or accumulates dA [r][in], dB [out][r]
// No atomics; fp32 accumulation; the chunking depends on M alone and every sum's order on (M, in, out, rank) alone, so bits are
// reproducible and a target's bits do not depend on the table around it.
#include "kernels.h"

namespace {

__device__ __forceinline__ LoraGradTarget lg_find_tile(const LoraGradP& p, int tile, int* idx) {
  if (!p.table) { *idx = 0; return p.one; }
  int lo = 0, hi = p.n - 1;
  while (lo < hi) {                        // the last target whose first tile is <= tile
    const int mid = (lo + hi + 1) >> 1;
    if (p.table[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  *idx = lo;
  return p.table[lo];
}
__device__ __forceinline__ LoraGradTarget lg_find_red(const LoraGradP& p, int blk) {
  if (!p.table) return p.one;
  int lo = 0, hi = p.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.table[mid].red0 <= blk) lo = mid; else hi = mid - 1;
  }
  return p.table[lo];
}

__device__ __forceinline__ bf16x8 zero8() {
  bf16x8 z;
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = (bf16)0.f;
  return z;
}
// elements [k, k + 8) of a row of n elements: one 16-byte load when the row is vector-addressable (vec) and the group is whole, else element
// by element; nothing at or past n is read
__device__ __forceinline__ bf16x8 load8(const bf16* row, int k, int n, bool vec) {
  bf16x8 v = zero8();
  if (k >= n) return v;
  if (vec && k + 8 <= n) return *(const bf16x8*)(row + k);
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (k + e < n) v[e] = row[k + e];
  return v;
}

// ---- 1. T^T | U^T: workgroup = (target, 64 rows), wave = 16 rows, RB blocks of 16 ranks ----
template <int RB>
__global__ __launch_bounds__(256) void lora_tu_kernel(const LoraGradP p) {
  const int nrb = p.Mp / 64;
  const int ti = (int)blockIdx.x / nrb, rb = (int)blockIdx.x - ti * nrb;
  const LoraGradTarget t = p.table ? p.table[ti] : p.one;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
  const int m0 = rb * 64 + wave * 16, row = m0 + r16;
  const bool live = row < p.M;
  const bf16* A = p.a + t.a_off;
  const bf16* B = p.b + t.b_off;
  const bf16* xr = p.x + (long)row * p.ldx;
  const bf16* yr = p.dy + (long)row * p.ldy + t.dy_col;
  const bool xvec = p.xvec != 0, yvec = p.yvec != 0 && (t.dy_col & 7) == 0;
  f32x4 accT[RB], accU[RB];
#pragma unroll
  for (int c = 0; c < RB; ++c) { accT[c] = f32x4{0.f, 0.f, 0.f, 0.f}; accU[c] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  // T[m][c] = sum_i X[m][i] A[c][i]: A operand = X rows, B operand (k = i, column c) = A[c][i .. i + 8): both 16-byte loads
  for (int k0 = 0; k0 < t.in; k0 += 32) {
    const int k = k0 + 8 * q;
    const bf16x8 xa = live ? load8(xr, k, t.in, xvec) : zero8();
#pragma unroll
    for (int c = 0; c < RB; ++c) {
      const int rk = c * 16 + r16;
      const bf16x8 af = rk < p.rank ? load8(A + (long)rk * t.in, k, t.in, true) : zero8();      // (in % 8 == 0, A 16-byte aligned)
      accT[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa, af, accT[c], 0, 0, 0);
    }
  }
  // U[m][c] = sum_o dY[m][o] B[o][c]: B operand (k = o, column c) = B[o .. o + 8)[c], stride rank: element loads (B is small, L1 / L2)
  for (int k0 = 0; k0 < t.out; k0 += 32) {
    const int k = k0 + 8 * q;
    const bf16x8 ya = live ? load8(yr, k, t.out, yvec) : zero8();
#pragma unroll
    for (int c = 0; c < RB; ++c) {
      const int rk = c * 16 + r16;
      bf16x8 bfr = zero8();
      if (rk < p.rank) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (k + e < t.out) bfr[e] = B[(long)(k + e) * p.rank + rk];
      }
      accU[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ya, bfr, accU[c], 0, 0, 0);
    }
  }
  // accumulator: column = rank rk = 16 c + r16, rows m0 + 4 q + (0..3) -> four consecutive m of Tt[rk][.]: one 8-byte store
  const int R = RB * 16;
  bf16* Tt = p.tu + (long)ti * 2 * R * p.Mp;
  bf16* Ut = Tt + (long)R * p.Mp;
#pragma unroll
  for (int c = 0; c < RB; ++c) {
    const long o = (long)(c * 16 + r16) * p.Mp + m0 + 4 * q;
    bf16x4 tv, uv;
#pragma unroll
    for (int e = 0; e < 4; ++e) { tv[e] = (bf16)accT[c][e]; uv[e] = (bf16)accU[c][e]; }
    *(bf16x4*)(Tt + o) = tv;
    *(bf16x4*)(Ut + o) = uv;
  }
}

// ---- 2. partial blocks: workgroup = (target, 128 columns of [in | out], row chunk), wave = 32 columns ----
// LDS image Zt[column][row], 32 rows of a step per column in four 16-byte groups; group g of column c sits at slot g ^ ((c >> 3) & 3), so the
// 16 column groups a wave writes at once spread over four bank groups instead of one
#define LG_ZROW 40      // bf16 per column of the image (32 + 8 padding: 80-byte rows)
template <int RB>
__global__ __launch_bounds__(256) void lora_part_kernel(const LoraGradP p) {
  __shared__ __attribute__((aligned(16))) bf16 Zt[128 * LG_ZROW];
  const int S = p.nchunk;
  const int tile = (int)blockIdx.x / S, s = (int)blockIdx.x - tile * S;
  int ti;
  const LoraGradTarget t = lg_find_tile(p, tile, &ti);
  const int tin = (t.in + 127) / 128;
  const int ct = tile - t.tile0;
  const bool xside = ct < tin;                      // X columns -> dA; else dY columns -> dB^T
  const int col0 = (xside ? ct : ct - tin) * 128, ncol = xside ? t.in : t.out;
  const bf16* Z = xside ? p.x : p.dy + t.dy_col;
  const long ldz = xside ? p.ldx : p.ldy;
  const bool zvec = xside ? p.xvec != 0 : (p.yvec != 0 && (t.dy_col & 7) == 0);
  const int R = RB * 16;
  const bf16* P = p.tu + (long)ti * 2 * R * p.Mp + (xside ? (long)R * p.Mp : 0);      // Ut for the X side, Tt for the dY side
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, q = lane >> 4;
  f32x4 acc[RB][2];
#pragma unroll
  for (int c = 0; c < RB; ++c) { acc[c][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[c][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const int mbeg = s * LORA_G_CHUNK, mend = min(mbeg + LORA_G_CHUNK, p.Mp);
  // staging: thread = (column group cv = tid % 16, row pair pr = tid / 16): two 16-byte loads, eight 4-byte LDS stores (rows 2 pr, 2 pr + 1)
  const int cv = tid & 15, pr = tid >> 4;
  for (int m = mbeg; m < mend; m += 32) {
    const int ra = m + 2 * pr, rbw = ra + 1, gc = col0 + 8 * cv;
    const bf16x8 z0 = ra < p.M ? load8(Z + (long)ra * ldz, gc, ncol, zvec) : zero8();
    const bf16x8 z1 = rbw < p.M ? load8(Z + (long)rbw * ldz, gc, ncol, zvec) : zero8();
    __syncthreads();                                 // the previous step's fragment reads are done
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = 8 * cv + e;
      const int slot = ((2 * pr) >> 3) ^ (cv & 3);
      bf16x2 v;
      v[0] = z0[e]; v[1] = z1[e];
      *(bf16x2*)&Zt[c * LG_ZROW + slot * 8 + ((2 * pr) & 7)] = v;
    }
    __syncthreads();
    bf16x8 zb[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int c = wave * 32 + nb * 16 + r16;
      zb[nb] = *(const bf16x8*)&Zt[c * LG_ZROW + ((q ^ ((c >> 3) & 3)) * 8)];
    }
#pragma unroll
    for (int c = 0; c < RB; ++c) {
      const bf16x8 pa = *(const bf16x8*)(P + (long)(c * 16 + r16) * p.Mp + m + 8 * q);      // A operand: row = rank, k = the step's rows
      acc[c][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, zb[0], acc[c][0], 0, 0, 0);
      acc[c][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, zb[1], acc[c][1], 0, 0, 0);
    }
  }
  // accumulator: column = tile column, rows = ranks 16 c + 4 q + (0..3); partial layout [chunk][rank][in | out]
  const int wid = t.in + t.out;
  float* part = p.part + t.part_off * p.nchunk + (long)s * p.rank * wid;
#pragma unroll
  for (int c = 0; c < RB; ++c)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int col = col0 + wave * 32 + nb * 16 + r16;
      if (col < ncol) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int rk = c * 16 + 4 * q + e;
          if (rk < p.rank) part[(long)rk * wid + (xside ? 0 : t.in) + col] = acc[c][nb][e];
        }
      }
    }
}

// ---- 3. chunks added in ascending order, scaled; thread = one element of [rank][in | out] ----
__global__ __launch_bounds__(256) void lora_red_kernel(const LoraGradP p) {
#pragma clang fp contract(off)      // accumulate adds the ROUNDED increment s * sum: what an overwrite would have stored
  const LoraGradTarget t = lg_find_red(p, (int)blockIdx.x);
  const int wid = t.in + t.out;
  const long n = (long)p.rank * wid, e = (long)((int)blockIdx.x - t.red0) * 256 + threadIdx.x;
  if (e >= n) return;
  const float* part = p.part + t.part_off * p.nchunk + e;
  float sum = 0.f;
  for (int s = 0; s < p.nchunk; ++s) sum += part[(long)s * n];
  const int rk = (int)(e / wid), g = (int)(e - (long)rk * wid);
  float* dst = g < t.in ? p.ga + t.ga_off + (long)rk * t.in + g : p.gb + t.gb_off + (long)(g - t.in) * p.rank + rk;
  const float v = p.scale * sum;
  *dst = p.accumulate ? *dst + v : v;
}

}  // namespace

int launch_lora_grad(const LoraGradP& p, hipStream_t st) {
  const int rbk = lora_grad_rb(p.rank);
  const dim3 g1((unsigned)(p.n * (p.Mp / 64))), g2((unsigned)(p.tiles * p.nchunk)), g3((unsigned)p.reds), blk(256);
  switch (rbk) {
    case 1: hipLaunchKernelGGL(lora_tu_kernel<1>, g1, blk, 0, st, p); hipLaunchKernelGGL(lora_part_kernel<1>, g2, blk, 0, st, p); break;
    case 2: hipLaunchKernelGGL(lora_tu_kernel<2>, g1, blk, 0, st, p); hipLaunchKernelGGL(lora_part_kernel<2>, g2, blk, 0, st, p); break;
    case 4: hipLaunchKernelGGL(lora_tu_kernel<4>, g1, blk, 0, st, p); hipLaunchKernelGGL(lora_part_kernel<4>, g2, blk, 0, st, p); break;
    default: hipLaunchKernelGGL(lora_tu_kernel<8>, g1, blk, 0, st, p); hipLaunchKernelGGL(lora_part_kernel<8>, g2, blk, 0, st, p); break;
  }
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(lora_red_kernel, g3, blk, 0, st, p);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
