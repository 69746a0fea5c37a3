// LoKr (LyCORIS Kronecker product) by merge and project (include/sdxlstep.h, SDXL_DTYPE_LOKR): like LoRA's (lora.hip) and LoHa's (loha.hip), the
// engine, the plan and every other kernel never see an adapter.  With out = out_l out_k, in = in_m n2 and W2 [out_k][n2] either stored (a full
// target) or W2 = B A (a factored one):
//   merge    W[a out_k + c][b n2 + j] = bf16_rn(W0 + s * (C[a][b] * W2[c][j]))                       into the weight arena, before the forward
//   project  dC[a][b]  = s * sum_{c,j} dW[a out_k + c][b n2 + j] W2[c][j]
//            dW2[c][j] = s * sum_{a,b} C[a][b] dW[a out_k + c][b n2 + j],   factored: dB = dW2 A^T, dA = B^T dW2     from the fp32 gradient arena
// Three table-driven kernels: one launch covers every target, a workgroup finds its (target, tile) by a binary search of the targets' first-tile
// indices; the single-target test hooks pass their one descriptor by value (LokrP::one, table == nullptr).  The projection reads dW once, keeps no
// out x in scratch and uses no atomics; every reduction order is fixed by (out, in, factor, rank, form, kind) alone, so a target's bits do not
// depend on the table around it.
// Packed layouts (LoraTarget::kind, kernels.h): the (row, column) of the formulas above are SOURCE indices (the state-dict tensor flattened to
// [out][in]).  The merge walks NATIVE rows and columns -- W0 / W stay on contiguous 16-byte vectors -- and maps each native row to (a, c) and each
// native column to (b, j) once per tile (lora_src_row / lora_src_col).  The projection walks W2 in native order and maps back (lora_nat_row,
// lora_nat_col).  Only the rows < out of a target are touched (conv_out's padded native rows are neither read nor written).
#include "kernels.h"

namespace {

// ---- merge: 32 x 64 tile, thread = (row tid / 8, the 8 columns of one 16-byte vector) ----
// factored: q <- q + B[c][k] * A[k][j] for k = 0 .. rank - 1, every product and sum rounded on its own; full: q = (float)W2[c][j];
// h = C[a][b] * q; t = s * h; W = bf16_rn(W0 + t), and W = W0 where t == 0 (so s = 0, C = 0, W2 = 0, A = 0 or B = 0 give back W0's bits, a -0
// included).  tests/_lokr_ref.py restates it in torch, bit for bit.  (contraction off and the operators written out: see lora_merge_kernel)
// A vector of 8 native columns may straddle two blocks b (in_n need not be a multiple of 8): b and j are per column, not per vector.
__global__ __launch_bounds__(256) void lokr_merge_kernel(const LokrP p) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float As[LOKR_M_KC][LOKR_M_COLS];
  __shared__ float Bs[LOKR_M_ROWS][LOKR_M_KC + 1];
  __shared__ int Ra[LOKR_M_ROWS], Rc[LOKR_M_ROWS], Cb[LOKR_M_COLS], Cj[LOKR_M_COLS];
  const LokrTarget h = adapter_find<&LoraTarget::tile_m>(p, (int)blockIdx.x);
  const LoraTarget& t = h.t;
  const int tid = threadIdx.x, local = (int)blockIdx.x - t.tile_m, ncb = (t.in + LOKR_M_COLS - 1) / LOKR_M_COLS;
  const int rb = local / ncb, cb = local - rb * ncb;
  const int lr = tid >> 3, lc = (tid & 7) * 8;
  const int row = rb * LOKR_M_ROWS + lr, col = cb * LOKR_M_COLS + lc;
  const int kind = t.kind, cg = t.cg, c4 = t.out >> 1;
  if (tid < LOKR_M_ROWS) {                 // native row -> (a, c); rows past the target: (0, 0), never stored
    const int gr = rb * LOKR_M_ROWS + tid;
    const int o = gr < t.out ? lora_src_row(kind, cg, c4, gr) : 0, a = o / h.out_k;
    Ra[tid] = a; Rc[tid] = o - a * h.out_k;
  } else if (tid >= 64 && tid < 64 + LOKR_M_COLS) {      // native column -> (b, j)
    const int c = tid - 64, gc = cb * LOKR_M_COLS + c;
    const int i = gc < t.in ? lora_src_col(kind, cg, gc) : 0, b = i / h.n2;
    Cb[c] = b; Cj[c] = i - b * h.n2;
  }
  __syncthreads();
  const bool live = row < t.out && col < t.in;      // in % 8 == 0: a vector is whole or absent
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (h.full) {                            // (uniform over the workgroup)
    const bf16* W2 = p.b + t.b_off;
    if (live) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = (float)W2[(long)Rc[lr] * h.n2 + Cj[lc + j]];
    }
  } else {
    const bf16* A = p.a + t.a_off;
    const bf16* B = p.b + t.b_off;
    for (int k0 = 0; k0 < p.rank; k0 += LOKR_M_KC) {
      const int kc = min(LOKR_M_KC, p.rank - k0);
      if (k0) __syncthreads();
      for (int idx = tid; idx < kc * LOKR_M_COLS; idx += 256) {
        const int k = idx / LOKR_M_COLS, c = idx - k * LOKR_M_COLS;
        As[k][c] = cb * LOKR_M_COLS + c < t.in ? (float)A[(long)(k0 + k) * h.n2 + Cj[c]] : 0.f;
      }
      for (int idx = tid; idx < LOKR_M_ROWS * LOKR_M_KC; idx += 256) {
        const int r = idx / LOKR_M_KC, k = idx - r * LOKR_M_KC;
        if (k < kc) Bs[r][k] = rb * LOKR_M_ROWS + r < t.out ? (float)B[(long)Rc[r] * p.rank + k0 + k] : 0.f;
      }
      __syncthreads();
      for (int k = 0; k < kc; ++k) {
        const float b = Bs[lr][k];
        const f32x4 a0 = *(const f32x4*)&As[k][lc], a1 = *(const f32x4*)&As[k][lc + 4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float q0 = b * a0[j], q1 = b * a1[j];
          acc[j] = acc[j] + q0;
          acc[j + 4] = acc[j + 4] + q1;
        }
      }
    }
  }
  if (live) {
    const bf16* Cm = p.c + h.c_off;
    const float s = h.full ? p.scale_full : p.scale;
    const long e = (long)row * t.in + col;
    const bf16x8 w0 = *(const bf16x8*)(p.base + t.base_off + e);
    bf16x8 w;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float cv = (float)Cm[Ra[lr] * h.in_m + Cb[lc + j]];
      const float hp = cv * acc[j];
      const float d = s * hp;
      const float sum = (float)w0[j] + d;
      w[j] = d == 0.f ? w0[j] : (bf16)sum;
    }
    *(bf16x8*)(p.w + t.w_off + e) = w;
  }
}

// ---- project, launch 1: dW2 and the partial sums of dC.  One workgroup per (target, LOKR_P_TILE consecutive elements of W2 in NATIVE order) ----
// W2's native order is [c][jn], jn = tap in_n + d for a 3x3 convolution (j = d 9 + tap), jn = j otherwise: inside one block (a, b) the native
// columns tap cin + b in_n + d of consecutive jn are consecutive, so a wave's 64 loads of G are runs of in_n contiguous floats.  Thread tid owns the
// elements tile * 1024 + tid + 256 m, m < 4: their W2 (loaded, or B A by fma over k ascending) and their dW2 accumulators stay in registers.
// The blocks (a, b) are walked in ascending a in_m + b, LOKR_P_NB at a time (32 loads of G per thread in flight):
//   acc[m] <- fma(C[a][b], G, acc[m])                                   so dW2 is one sequential sum over the blocks in ascending order;
//   part   <- fma(G[m], W2[m], part) over m = 0 .. 3, then the xor tree over the wave's 64 lanes, then the 4 waves added in order
//                                                                       -> scratch partial [tile][a in_m + b].
// Elements past the end of W2 (the last tile) hold W2 = 0 and load nothing.  One barrier per LOKR_P_NB blocks (the wave sums are double-buffered).
__global__ __launch_bounds__(256) void lokr_project_w2_kernel(const LokrP p) {
  __shared__ float red[2][LOKR_P_NB][4];
  const LokrTarget h = adapter_find<&LoraTarget::tile_b>(p, (int)blockIdx.x);
  const LoraTarget& t = h.t;
  const int tid = threadIdx.x, tile = (int)blockIdx.x - t.tile_b;
  const int kind = t.kind, cg = t.cg, c4 = t.out >> 1, n2 = h.n2, in_n = h.in_n, rank = p.rank;
  const int nw2 = h.out_k * n2, nblk = h.out_l * h.in_m;
  const float* dw = p.dw + t.w_off;
  const bf16* Cm = p.c + h.c_off;
  int cc[4], colbase[4], widx[4];
  bool valid[4];
  float w2[4], acc[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int e = tile * LOKR_P_TILE + m * 256 + tid;
    valid[m] = e < nw2;
    const int c = valid[m] ? e / n2 : 0, jn = valid[m] ? e - c * n2 : 0;
    const int tap = jn / in_n, d = jn - tap * in_n;      // (khw == 1: tap = 0, d = jn)
    cc[m] = c;
    const int j = d * h.khw + tap;                       // the state-dict order
    colbase[m] = lora_nat_col(kind, cg, j);              // block b = 0: tap cg + d; block b lies b in_n native columns further
    widx[m] = c * n2 + j;                                // [c][j]
    acc[m] = 0.f;
    float v = 0.f;
    if (valid[m]) {
      if (h.full) v = (float)(p.b + t.b_off)[widx[m]];
      else {
        const bf16* B = p.b + t.b_off + (long)c * rank;
        const bf16* A = p.a + t.a_off + j;
        for (int k = 0; k < rank; ++k) v = fmaf((float)B[k], (float)A[(long)k * n2], v);
      }
    }
    w2[m] = v;
  }
  const int lane = tid & 63, wave = tid >> 6;
  int a = 0, b = 0, buf = 0;
  for (int blk0 = 0; blk0 < nblk; blk0 += LOKR_P_NB) {
    float g[LOKR_P_NB][4], cv[LOKR_P_NB];
    int aa = a, bb = b;
#pragma unroll
    for (int u = 0; u < LOKR_P_NB; ++u) {
      const bool on = blk0 + u < nblk;     // (uniform)
      cv[u] = on ? (float)Cm[aa * h.in_m + bb] : 0.f;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        float v = 0.f;
        if (on && valid[m]) {
          const int nr = lora_nat_row(kind, cg, c4, aa * h.out_k + cc[m]);
          v = dw[(long)nr * t.in + colbase[m] + bb * in_n];
        }
        g[u][m] = v;
      }
      if (++bb == h.in_m) { bb = 0; ++aa; }
    }
    a = aa; b = bb;
    float part[LOKR_P_NB];
#pragma unroll
    for (int u = 0; u < LOKR_P_NB; ++u) {
      float s = 0.f;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        acc[m] = fmaf(cv[u], g[u][m], acc[m]);
        s = fmaf(g[u][m], w2[m], s);
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
      part[u] = s;
    }
    if (lane == 0) {
#pragma unroll
      for (int u = 0; u < LOKR_P_NB; ++u) red[buf][u][wave] = part[u];
    }
    __syncthreads();
    if (tid < LOKR_P_NB && blk0 + tid < nblk)
      p.scratch[h.part_off + (long)tile * nblk + blk0 + tid] = ((red[buf][tid][0] + red[buf][tid][1]) + red[buf][tid][2]) + red[buf][tid][3];
    buf ^= 1;                              // (the next batch writes the other half; the one after comes behind the next barrier)
  }
  float* out = h.full ? p.gb + t.gb_off : p.scratch + h.dw2_off;
  const float sc = h.full ? p.scale_full : p.scale;
#pragma unroll
  for (int m = 0; m < 4; ++m)
    if (valid[m]) out[widx[m]] = sc * acc[m];
}

// ---- project, launch 2: one output element per thread, each one sequential sum in ascending order ----
//   dC[a][b]  = s * (partial[0][ab] + partial[1][ab] + ...)                      every target
//   dB[c][k]  = sum_j dW2s[c][j] A[k][j],   dA[k][j] = sum_c B[c][k] dW2s[c][j]     a factored target, dW2s = s dW2 from launch 1's scratch
__global__ __launch_bounds__(LOKR_Q_THREADS) void lokr_project_out_kernel(const LokrP p) {
  const LokrTarget h = adapter_find<&LoraTarget::tile_a>(p, (int)blockIdx.x);
  const LoraTarget& t = h.t;
  const int nblk = h.out_l * h.in_m, n2 = h.n2, rank = p.rank;
  int local = (int)blockIdx.x - t.tile_a;
  const int q1 = (nblk + LOKR_Q_THREADS - 1) / LOKR_Q_THREADS;
  if (local < q1) {
    const int idx = local * LOKR_Q_THREADS + (int)threadIdx.x;
    if (idx >= nblk) return;
    const float* part = p.scratch + h.part_off;
    float s = 0.f;
    for (int tl = 0; tl < h.ptiles; ++tl) s += part[(long)tl * nblk + idx];
    (p.gc + h.c_off)[idx] = (h.full ? p.scale_full : p.scale) * s;
    return;
  }
  local -= q1;                             // (a full target has no further workgroups)
  const float* dw2 = p.scratch + h.dw2_off;
  const int q2 = (h.out_k * rank + LOKR_Q_THREADS - 1) / LOKR_Q_THREADS;
  if (local < q2) {
    const int idx = local * LOKR_Q_THREADS + (int)threadIdx.x;
    if (idx >= h.out_k * rank) return;
    const int c = idx / rank, k = idx - c * rank;
    const bf16* A = p.a + t.a_off + (long)k * n2;
    const float* x = dw2 + (long)c * n2;
    float s = 0.f;
    for (int j = 0; j < n2; ++j) s = fmaf(x[j], (float)A[j], s);
    (p.gb + t.gb_off)[idx] = s;
    return;
  }
  local -= q2;
  const int idx = local * LOKR_Q_THREADS + (int)threadIdx.x;
  if (idx >= rank * n2) return;
  const int k = idx / n2, j = idx - k * n2;
  const bf16* B = p.b + t.b_off + k;
  float s = 0.f;
  for (int c = 0; c < h.out_k; ++c) s = fmaf((float)B[(long)c * rank], dw2[(long)c * n2 + j], s);
  (p.ga + t.ga_off)[idx] = s;
}

}  // namespace

int launch_lokr_merge(const LokrP& p, hipStream_t st) {
  hipLaunchKernelGGL(lokr_merge_kernel, dim3(p.tiles_m), dim3(256), 0, st, p);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_lokr_project(const LokrP& p, hipStream_t st) {
  hipLaunchKernelGGL(lokr_project_w2_kernel, dim3(p.tiles_p), dim3(256), 0, st, p);
  HIP_CHECK_RET(hipGetLastError());
  hipLaunchKernelGGL(lokr_project_out_kernel, dim3(p.tiles_q), dim3(LOKR_Q_THREADS), 0, st, p);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
