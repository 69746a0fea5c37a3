// LoHa (LyCORIS Hadamard product) by merge and project (include/sdxlstep.h, SDXL_DTYPE_LOHA): like LoRA's (lora.hip), the engine, the plan and
// every other kernel never see an adapter.  With P1 = B1 A1, P2 = B2 A2 ([out][in], never stored):
//   merge    W[o][i]   = bf16_rn(W0[o][i] + s * (P1[o][i] * P2[o][i]))                          into the weight arena, before the forward
//   project  dB1[o][k] = s * sum_i (dW[o][i] P2[o][i]) A1[k][i],  dA1[k][i] = s * sum_o B1[o][k] (dW[o][i] P2[o][i])
//            dB2[o][k] = s * sum_i (dW[o][i] P1[o][i]) A2[k][i],  dA2[k][i] = s * sum_o B2[o][k] (dW[o][i] P1[o][i])       from the fp32 gradient arena
// Three table-driven kernels: one launch covers every target, a workgroup finds its (target, tile) by a binary search of the targets' first-tile
// indices; the single-target test hooks pass their one descriptor by value (LohaP::one, table == nullptr).  No out x in scratch: both
// projection launches read dW once and recompute P1, P2 of their tile from the staged factor tiles.  No atomics; every reduction order is
// fixed by (out, in, rank) and the target's kind alone, so a target's bits do not depend on the table around it.
// Packed layouts (LoraTarget::kind, kernels.h): as in lora.hip the tiles walk NATIVE rows and columns, W0 / W / dW stay on contiguous 16-byte
// vectors, and only the indices into the small operands are mapped while they are staged through LDS (lora_src_col into A1, A2 and their
// gradients, lora_src_row into B1, B2 and theirs).  There is one instantiation: a plain target runs with the identity maps.  Only the rows
// < out of a target are touched (conv_out's padded native rows are neither read nor written).
#include "kernels.h"

namespace {

// ---- merge: 32 x 64 tile, thread = (row tid / 8, the 8 columns of one 16-byte vector) ----
// p1 <- p1 + B1[o][k] * A1[k][i] and p2 <- p2 + B2[o][k] * A2[k][i] for k = 0 .. rank - 1, every product and sum rounded on its own;
// h = p1 * p2; t = s * h; W = bf16_rn(W0 + t), and W = W0 where t == 0 (so s = 0, B1 = 0 or B2 = 0 give back W0's bits, a -0 included).
// tests/_loha_ref.py restates it in torch, bit for bit.  (contraction off and the operators written out: see lora_merge_kernel)
__global__ __launch_bounds__(256) void loha_merge_kernel(const LohaP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float As[2][LOHA_M_KC][LOHA_M_COLS];
  __shared__ float Bs[2][LOHA_M_ROWS][LOHA_M_KC + 1];
  const LohaTarget h = adapter_find<&LoraTarget::tile_m>(p, (int)blockIdx.x);
  const LoraTarget& t = h.t;
  const int tid = threadIdx.x, local = (int)blockIdx.x - t.tile_m, ncb = (t.in + LOHA_M_COLS - 1) / LOHA_M_COLS;
  const int rb = local / ncb, cb = local - rb * ncb;
  const int lr = tid >> 3, lc = (tid & 7) * 8;
  const int row = rb * LOHA_M_ROWS + lr, col = cb * LOHA_M_COLS + lc;
  const bf16* A[2] = {p.a1 + t.a_off, p.a2 + h.a2_off};
  const bf16* B[2] = {p.b1 + t.b_off, p.b2 + h.b2_off};
  const int kind = t.kind, cg = t.cg, c4 = t.out >> 1;
  float acc[2][8];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[f][j] = 0.f;
  for (int k0 = 0; k0 < p.rank; k0 += LOHA_M_KC) {
    const int kc = min(LOHA_M_KC, p.rank - k0);
    __syncthreads();
    for (int idx = tid; idx < kc * LOHA_M_COLS; idx += 256) {
      const int k = idx / LOHA_M_COLS, c = idx - k * LOHA_M_COLS, gc = cb * LOHA_M_COLS + c;
      const long at = (long)(k0 + k) * t.in + (gc < t.in ? lora_src_col(kind, cg, gc) : 0);
#pragma unroll
      for (int f = 0; f < 2; ++f) As[f][k][c] = gc < t.in ? (float)A[f][at] : 0.f;
    }
    for (int idx = tid; idx < LOHA_M_ROWS * LOHA_M_KC; idx += 256) {
      const int r = idx / LOHA_M_KC, k = idx - r * LOHA_M_KC, gr = rb * LOHA_M_ROWS + r;
      if (k < kc) {
        const long at = (long)(gr < t.out ? lora_src_row(kind, cg, c4, gr) : 0) * p.rank + k0 + k;
#pragma unroll
        for (int f = 0; f < 2; ++f) Bs[f][r][k] = gr < t.out ? (float)B[f][at] : 0.f;
      }
    }
    __syncthreads();
    for (int k = 0; k < kc; ++k) {
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        const float b = Bs[f][lr][k];
        const f32x4 a0 = *(const f32x4*)&As[f][k][lc], a1 = *(const f32x4*)&As[f][k][lc + 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float q0 = b * a0[j], q1 = b * a1[j];
          acc[f][j] = acc[f][j] + q0;
          acc[f][j + 4] = acc[f][j + 4] + q1;
        }
      }
    }
  }
  if (row < t.out && col < t.in) {        // in % 8 == 0: a vector is whole or absent
    const long e = (long)row * t.in + col;
    const bf16x8 w0 = *(const bf16x8*)(p.base + t.base_off + e);
    bf16x8 w;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float hp = acc[0][j] * acc[1][j];
      const float d = p.scale * hp;
      const float sum = (float)w0[j] + d;
      w[j] = d == 0.f ? w0[j] : (bf16)sum;
    }
    *(bf16x8*)(p.w + t.w_off + e) = w;
  }
}

// ---- project: one kernel, two launches.  DA = false writes dB1 | dB2: one workgroup per (target, 32 native rows), walking `in` in steps of 32
// columns; DA = true writes dA1 | dA2: one workgroup per (target, 32 native columns), walking `out` in steps of 32 rows. ----
// Per step of a 32 x 32 tile of G = dW, with the factor tiles A1, A2 [rank][32] and B1, B2 [32][rank] in LDS (the pair that does not move with
// the walk is staged once):
//   1. thread (row tid / 8, columns 4 (tid % 8) .. + 3) loads its 16 bytes of G, recomputes p1 = sum_k B1[o][k] A1[k][i] and p2 likewise (fma,
//      k ascending) and leaves X1 = G * p2, X2 = G * p1 in LDS;
//   2. DA = false: thread (row tid % 32, ranks tid / 32 + 8 m, m < KPT)  acc1[m] <- fma(X1[row][c], A1[k][c], acc1[m]), acc2 with X2, A2,
//      for c = 0 .. 31 ascending;  DA = true: thread (column tid % 32, ranks tid / 32 + 8 m)  acc1[m] <- fma(B1[r][k], X1[r][c], acc1[m]),
//      acc2 with B2, X2, for r = 0 .. 31 ascending.
// Every accumulator is one sequential sum over the native columns (rows) 0 .. in - 1 (out - 1) in ascending order -- rows and columns past the
// target add +0 -- so the order depends on (out, in, rank) and the kind only.  KPT = ceil(rank / 8) rounded up to 1, 2, 4, 8 sizes the LDS
// tiles and the accumulators; nothing is indexed dynamically in registers.  A step is short (4 KiB of G), so its global loads -- G and the
// moving factor tiles -- are issued one step ahead into registers, behind part 2 of the step before.
template <int KPT, bool DA>
__global__ __launch_bounds__(256) void loha_project_kernel(const LohaP p) {
  constexpr int R = 8 * KPT, XS = LOHA_P_COLS + 4;      // row stride 36 floats: 16-byte rows, 16 consecutive rows fall on the 16 distinct 16-byte slots of a bank row
  __shared__ __attribute__((aligned(16))) float As[2][R][XS];
  __shared__ float Bs[2][LOHA_P_ROWS][R + 1];
  __shared__ __attribute__((aligned(16))) float Xs[2][LOHA_P_ROWS][XS];
  const LohaTarget h = DA ? adapter_find<&LoraTarget::tile_a>(p, (int)blockIdx.x) : adapter_find<&LoraTarget::tile_b>(p, (int)blockIdx.x);
  const LoraTarget& t = h.t;
  const int tid = threadIdx.x;
  const int fixed0 = ((int)blockIdx.x - (DA ? t.tile_a : t.tile_b)) * 32;      // first native column (DA) or row of this workgroup
  const bf16* A[2] = {p.a1 + t.a_off, p.a2 + h.a2_off};
  const bf16* B[2] = {p.b1 + t.b_off, p.b2 + h.b2_off};
  const float* dw = p.dw + t.w_off;
  const int kind = t.kind, cg = t.cg, c4 = t.out >> 1, rank = p.rank;

  // a factor tile is 256 KPT elements per pair: thread tid holds the elements tid + 256 m, m < KPT, of both pairs between global memory and LDS
  auto fetch_a = [&](int c0, float (&v)[2][KPT]) {      // A1, A2 [rank][c0 .. c0 + 31]; ranks and columns past the target: 0
#pragma unroll
    for (int m = 0; m < KPT; ++m) {
      const int idx = tid + 256 * m, k = idx / LOHA_P_COLS, c = idx - k * LOHA_P_COLS, gc = c0 + c;
      const bool in_range = k < rank && gc < t.in;
      const long at = in_range ? (long)k * t.in + lora_src_col(kind, cg, gc) : 0;
#pragma unroll
      for (int f = 0; f < 2; ++f) v[f][m] = in_range ? (float)A[f][at] : 0.f;
    }
  };
  auto store_a = [&](const float (&v)[2][KPT]) {
#pragma unroll
    for (int m = 0; m < KPT; ++m) {
      const int idx = tid + 256 * m, k = idx / LOHA_P_COLS, c = idx - k * LOHA_P_COLS;
#pragma unroll
      for (int f = 0; f < 2; ++f) As[f][k][c] = v[f][m];
    }
  };
  auto fetch_b = [&](int r0, float (&v)[2][KPT]) {      // B1, B2 [r0 .. r0 + 31][rank]
#pragma unroll
    for (int m = 0; m < KPT; ++m) {
      const int idx = tid + 256 * m, r = idx / R, k = idx - r * R, gr = r0 + r;
      const bool in_range = k < rank && gr < t.out;
      const long at = in_range ? (long)lora_src_row(kind, cg, c4, gr) * rank + k : 0;
#pragma unroll
      for (int f = 0; f < 2; ++f) v[f][m] = in_range ? (float)B[f][at] : 0.f;
    }
  };
  auto store_b = [&](const float (&v)[2][KPT]) {
#pragma unroll
    for (int m = 0; m < KPT; ++m) {
      const int idx = tid + 256 * m, r = idx / R, k = idx - r * R;
#pragma unroll
      for (int f = 0; f < 2; ++f) Bs[f][r][k] = v[f][m];
    }
  };
  const int lr = tid >> 3, lc = (tid & 7) * 4;                    // step 1's element
  auto load_g = [&](int r0, int c0) {
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    if (r0 + lr < t.out && c0 + lc < t.in) g = *(const f32x4*)(dw + (long)(r0 + lr) * t.in + c0 + lc);      // in % 4 == 0
    return g;
  };

  float acc[2][KPT], nxt[2][KPT];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int m = 0; m < KPT; ++m) acc[f][m] = 0.f;
  // the pair that stays, then step 0's moving pair and G; every later step's loads are issued one step ahead, behind the compute of the current one
  if (DA) { fetch_a(fixed0, nxt); store_a(nxt); fetch_b(0, nxt); } else { fetch_b(fixed0, nxt); store_b(nxt); fetch_a(0, nxt); }
  f32x4 g = DA ? load_g(0, fixed0) : load_g(fixed0, 0);
  const int steps = ((DA ? t.out : t.in) + 31) / 32;
  for (int s = 0; s < steps; ++s) {
    __syncthreads();                      // the previous step's readers of As / Bs / Xs are done
    if (DA) store_b(nxt); else store_a(nxt);
    __syncthreads();
    {
      f32x4 p1 = {0.f, 0.f, 0.f, 0.f}, p2 = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < rank; ++k) {
        const float b1 = Bs[0][lr][k], b2 = Bs[1][lr][k];
        const f32x4 a1 = *(const f32x4*)&As[0][k][lc], a2 = *(const f32x4*)&As[1][k][lc];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          p1[e] = fmaf(b1, a1[e], p1[e]);
          p2[e] = fmaf(b2, a2[e], p2[e]);
        }
      }
      f32x4 x1, x2;
#pragma unroll
      for (int e = 0; e < 4; ++e) { x1[e] = g[e] * p2[e]; x2[e] = g[e] * p1[e]; }
      *(f32x4*)&Xs[0][lr][lc] = x1;
      *(f32x4*)&Xs[1][lr][lc] = x2;
    }
    if (s + 1 < steps) {                  // the next step's loads, in flight during step 2
      const int n0 = (s + 1) * 32;
      if (DA) { fetch_b(n0, nxt); g = load_g(n0, fixed0); } else { fetch_a(n0, nxt); g = load_g(fixed0, n0); }
    }
    __syncthreads();
    const int kg = tid >> 5;              // uniform over half a wave: at a low rank whole waves have no rank to sum and skip part 2
    if (kg >= rank) continue;             // (no barrier is skipped: the loop's next one is its first statement)
    if (DA) {
      const int c = tid & 31;
#pragma unroll 4
      for (int r = 0; r < LOHA_P_ROWS; ++r) {
        const float x1 = Xs[0][r][c], x2 = Xs[1][r][c];
#pragma unroll
        for (int m = 0; m < KPT; ++m) {
          acc[0][m] = fmaf(Bs[0][r][kg + 8 * m], x1, acc[0][m]);
          acc[1][m] = fmaf(Bs[1][r][kg + 8 * m], x2, acc[1][m]);
        }
      }
    } else {
      const int r = tid & 31;
#pragma unroll 2
      for (int c = 0; c < LOHA_P_COLS; c += 4) {
        const f32x4 x1 = *(const f32x4*)&Xs[0][r][c], x2 = *(const f32x4*)&Xs[1][r][c];
#pragma unroll
        for (int m = 0; m < KPT; ++m) {
          const f32x4 a1 = *(const f32x4*)&As[0][kg + 8 * m][c], a2 = *(const f32x4*)&As[1][kg + 8 * m][c];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[0][m] = fmaf(x1[e], a1[e], acc[0][m]);
            acc[1][m] = fmaf(x2[e], a2[e], acc[1][m]);
          }
        }
      }
    }
  }
  if (DA) {
    const int n = fixed0 + (tid & 31), kg = tid >> 5;             // native column; its column of dA1 / dA2
    if (n < t.in) {
      const int c = lora_src_col(kind, cg, n);
      float* dA1 = p.ga1 + t.ga_off;
      float* dA2 = p.ga2 + h.ga2_off;
#pragma unroll
      for (int m = 0; m < KPT; ++m) {
        const int k = kg + 8 * m;
        if (k < rank) {
          dA1[(long)k * t.in + c] = p.scale * acc[0][m];
          dA2[(long)k * t.in + c] = p.scale * acc[1][m];
        }
      }
    }
  } else {
    const int n = fixed0 + (tid & 31), kg = tid >> 5;             // native row; its row of dB1 / dB2
    if (n < t.out) {
      const int r = lora_src_row(kind, cg, c4, n);
      float* dB1 = p.gb1 + t.gb_off;
      float* dB2 = p.gb2 + h.gb2_off;
#pragma unroll
      for (int m = 0; m < KPT; ++m) {
        const int k = kg + 8 * m;
        if (k < rank) {
          dB1[(long)r * rank + k] = p.scale * acc[0][m];
          dB2[(long)r * rank + k] = p.scale * acc[1][m];
        }
      }
    }
  }
}

template <bool DA>
void launch_loha_half(const LohaP& p, hipStream_t st) {
  const dim3 grid(DA ? p.tiles_a : p.tiles_b), block(256);
  if (p.rank <= 8) hipLaunchKernelGGL((loha_project_kernel<1, DA>), grid, block, 0, st, p);
  else if (p.rank <= 16) hipLaunchKernelGGL((loha_project_kernel<2, DA>), grid, block, 0, st, p);
  else if (p.rank <= 32) hipLaunchKernelGGL((loha_project_kernel<4, DA>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((loha_project_kernel<8, DA>), grid, block, 0, st, p);
}

}  // namespace

int launch_loha_merge(const LohaP& p, hipStream_t st) {
  hipLaunchKernelGGL(loha_merge_kernel, dim3(p.tiles_m), dim3(256), 0, st, p);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_loha_project(const LohaP& p, hipStream_t st) {
  launch_loha_half<false>(p, st);
  HIP_CHECK_RET(hipGetLastError());
  launch_loha_half<true>(p, st);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
