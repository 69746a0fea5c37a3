// Input gradient of conv_in (sdxl_batch_din, include/sdxlstep.h): the gradient with respect to the UNet input, in fp32 NCHW.
//
//   dx[b][c][y][x] = sum_{ky, kx in 0..2} sum_{o < Cout} dy[b][y + 1 - ky][x + 1 - kx][o] . w[o][3 ky + kx][c]      (pixels outside the image: nothing)
//
// dy [B * H * W][Cout] bf16 is conv_in's output gradient as the plan holds it, w [Cout][9][Cs] bf16 the arena's conv_in (Cs = 8 | 16, pad
// channels zero), dx [B][in_channels][H][W] fp32 the caller's buffer.  As a GEMM this is M = B * H * W pixels, N = Cs, K = 9 Cout: sixteen
// columns at most, so the tile kernels of the GEMM family would spend 15 / 16 of their MFMAs on padding, and the work is the one pass over
// dy (SDXL-base, B = 4, 128 x 128: 42 MB against 6 GFLOP).  Hence a kernel of its own:
//   * a workgroup (4 waves) owns ID_T x ID_T = 16 x 16 pixels of one sample, wave v the rows 4 v .. 4 v + 3; blockIdx = (x tile, y tile, b).
//     A tile never crosses a sample, and its one-pixel halo stops at the image border: what lies outside is zeros made in registers, never
//     read -- row -1 of sample b + 1 is not row H - 1 of sample b.
//   * v_mfma_f32_16x16x32_bf16 with the 16 pixels of a tile row on the rows and the channels c (Cs, zero fragments behind it) on the columns;
//     one K-step is 32 output channels of one tap.  A fragment of dy at halo row r and tap column kx serves the three (pixel row, ky) pairs
//     with row + 2 - ky == r, so a wave reads 6 x 3 fragments per K-step for its 36 MFMAs.
//   * Cout is walked in chunks of 64 (the last may be 32): the chunk's dy tile with halo (18 x 18 pixels x 128 B) and weight slice
//     ([9][16][64] bf16, 18 KiB) are staged global -> registers -> LDS, the loads of chunk t + 1 in flight under the MFMAs of chunk t.  Each dy
//     element is fetched once per workgroup, not once per tap.
//   * LDS images: a pixel (dy) or a (tap, c) pair (w) is one 128-byte row of eight 16-byte slots, slot s of row n stored at s ^ ((n' >> 1) & 7)
//     with n' = the halo column / c.  ds_read_b128 serves 16 lanes per cycle from the sixteen slots of a 256-byte bank row (two neighbouring
//     rows): sixteen consecutive n' with one s cover them all.  A 16-lane group of ds_read_b128 mixes two s that differ in bit 0 (eight
//     lanes each); with a first column that is a multiple of 4 (w always; dy at kx = 2) that is still conflict-free, at kx = 0 and 1 it is
//     2-way (derived from the bank rules, not measured with counters).
//   * fp32 accumulation in the order chunk, K-step, halo row, kx, ky: a function of the shape alone.  No atomics, bitwise reproducible.
//   * the store transposes through LDS ([c][row][x], 260 floats per c): a lane's four accumulator values are four consecutive x, and the
//     NCHW write goes out in runs of 16 consecutive x (float4 when W % 4 == 0, else scalar), masked by y < H, x < W, c < in_channels.
// A closed gradient gate (*gate == 0) stores exact zeros and reads neither dy nor w (residual_grad_kernel's rule).
#include "kernels.h"

#define ID_T 16                              // tile edge in pixels
#define ID_HALO (ID_T + 2)                   // ... with its halo
#define ID_CHUNK 64                          // output channels per LDS stage
#define ID_THREADS 256
#define ID_DY_BYTES (ID_HALO * ID_HALO * 128)
#define ID_W_BYTES (9 * 16 * 128)
#define ID_DY_VECS (ID_HALO * ID_HALO * 8)   // 16-byte vectors of a whole dy stage
#define ID_DY_ITERS ((ID_DY_VECS + ID_THREADS - 1) / ID_THREADS)
#define ID_W_ITERS ((ID_CHUNK * 9 * 2 + ID_THREADS - 1) / ID_THREADS)
#define ID_OUT_LD 260                        // floats per channel of the store image (16 x 16 + 4: consecutive c fall on consecutive slots)

namespace {
typedef __attribute__((ext_vector_type(4))) unsigned int idu32x4;

template <bool VEC>
__global__ __launch_bounds__(ID_THREADS) void input_dgrad_kernel(const bf16* __restrict__ dy, const bf16* __restrict__ w, float* __restrict__ dx,
                                                                 const float* __restrict__ gate, int H, int W, int Cin, int Cs, int Cout) {
  __shared__ __attribute__((aligned(16))) char smem[ID_DY_BYTES + ID_W_BYTES];
  char* Dt = smem;
  char* Wt = smem + ID_DY_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, g4 = lane >> 4;
  const int x0 = blockIdx.x * ID_T, y0 = blockIdx.y * ID_T;
  const long b = blockIdx.z;
  const bool closed = gate && *gate == 0.f;      // block-uniform

  f32x4 acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (!closed) {
    const int csv = Cs >> 3;                        // 16-byte vectors per (o, tap) of w: 1 | 2
    idu32x4 rd[ID_DY_ITERS], rw[ID_W_ITERS];
    // chunk o0 .. o0 + cc - 1 (cc = 64 | 32) into registers: dy vector i = (halo pixel i >> 3, channel group i & 7), w vector j = 8 elements of
    // the contiguous slice w[o0 .. o0 + cc - 1][9][Cs]
    auto load_regs = [&](int o0, int cc) {
      const int cv = cc >> 3;
#pragma unroll
      for (int i = 0; i < ID_DY_ITERS; ++i) {
        const int idx = tid + ID_THREADS * i;
        const int v = idx & 7, px = idx >> 3;
        const int hy = px / ID_HALO, hx = px - hy * ID_HALO;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        idu32x4 val = {0u, 0u, 0u, 0u};
        if (idx < ID_DY_VECS && v < cv && y >= 0 && y < H && x >= 0 && x < W)
          val = *(const idu32x4*)(dy + ((b * H + y) * W + x) * Cout + o0 + 8 * v);
        rd[i] = val;
      }
      const int nw = cc * 9 * csv;
      const bf16* wsrc = w + (long)o0 * 9 * Cs;
#pragma unroll
      for (int i = 0; i < ID_W_ITERS; ++i) {
        const int j = tid + ID_THREADS * i;
        idu32x4 val = {0u, 0u, 0u, 0u};
        if (j < nw) val = *(const idu32x4*)(wsrc + (long)j * 8);
        rw[i] = val;
      }
    };
    auto store_lds = [&](int cc) {
#pragma unroll
      for (int i = 0; i < ID_DY_ITERS; ++i) {
        const int idx = tid + ID_THREADS * i;
        const int v = idx & 7, px = idx >> 3;
        const int hx = px % ID_HALO;
        if (idx < ID_DY_VECS) *(idu32x4*)(Dt + px * 128 + ((v ^ ((hx >> 1) & 7)) << 4)) = rd[i];
      }
      const int nw = cc * 9 * csv;
#pragma unroll
      for (int i = 0; i < ID_W_ITERS; ++i) {
        const int j = tid + ID_THREADS * i;
        if (j >= nw) continue;
        const int cvi = j % csv, ot = j / csv;      // ot = o_local * 9 + tap
        const int ol = ot / 9, tap = ot - ol * 9;
#pragma unroll
        for (int k = 0; k < 8; ++k) {      // element k of the vector is channel c of (o_local, tap): transposed to [tap][c][o_local]
          const int c = cvi * 8 + k;
          const unsigned int word = rw[i][k >> 1];
          *(unsigned short*)(Wt + (tap * 16 + c) * 128 + (((ol >> 3) ^ ((c >> 1) & 7)) << 4) + (ol & 7) * 2) =
              (unsigned short)((k & 1) ? word >> 16 : word & 0xffffu);
        }
      }
    };

    const bool c_ok = l16 < Cs;                    // the columns behind Cs: zero fragments (their LDS rows are never written)
    const int c_rd = l16 & (Cs - 1);
    load_regs(0, min(ID_CHUNK, Cout));
    for (int o0 = 0; o0 < Cout; o0 += ID_CHUNK) {
      const int cc = min(ID_CHUNK, Cout - o0);
      store_lds(cc);
      __syncthreads();
      if (o0 + ID_CHUNK < Cout) load_regs(o0 + ID_CHUNK, min(ID_CHUNK, Cout - o0 - ID_CHUNK));
      for (int ks = 0; ks < (cc >> 5); ++ks) {
        const int cs = ks * 4 + g4;                // the 16-byte slot of this lane's 8 reduction channels
        bf16x8 fb[9];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const bf16x8 v = *(const bf16x8*)(Wt + (tap * 16 + c_rd) * 128 + ((cs ^ ((c_rd >> 1) & 7)) << 4));
          const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
          fb[tap] = c_ok ? v : z;
        }
#pragma unroll
        for (int hr = 0; hr < 6; ++hr) {           // halo rows 4 wave + hr of this wave's four pixel rows
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int hx = l16 + 2 - kx;
            const bf16x8 fa = *(const bf16x8*)(Dt + ((4 * wave + hr) * ID_HALO + hx) * 128 + ((cs ^ ((hx >> 1) & 7)) << 4));
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
              const int r = hr - 2 + ky;           // pixel row r reads halo row r + 2 - ky
              if (r >= 0 && r < 4) acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[3 * ky + kx], acc[r], 0, 0, 0);
            }
          }
        }
      }
      __syncthreads();
    }
  }

  // accumulators -> LDS [c][row][x]: lane (g4, l16) holds x = 4 g4 .. 4 g4 + 3 of channel l16 for each of its wave's rows
  float* Ot = (float*)smem;
#pragma unroll
  for (int r = 0; r < 4; ++r) *(f32x4*)(Ot + l16 * ID_OUT_LD + (4 * wave + r) * ID_T + 4 * g4) = acc[r];
  __syncthreads();
  const int xq = (tid & 3) * 4, row = (tid >> 2) & 15;
  const int y = y0 + row, x = x0 + xq;
  if (y >= H || x >= W) return;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int c = (tid >> 6) + 4 * it;
    if (c >= Cin) continue;
    const f32x4 v = *(const f32x4*)(Ot + c * ID_OUT_LD + row * ID_T + xq);
    float* dst = dx + ((b * Cin + c) * H + y) * W + x;
    if (VEC) {
      *(f32x4*)dst = v;                            // W % 4 == 0: x + 3 < W, and the address is 16-byte aligned
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x + k < W) dst[k] = v[k];
    }
  }
}
}  // namespace

int launch_input_dgrad(const bf16* dy, const bf16* w, float* dx, const float* gate, int B, int H, int W, int in_channels, int Cout, hipStream_t st) {
  ARG_CHECK(dy && w && dx && ((((uintptr_t)dy) | ((uintptr_t)w) | ((uintptr_t)dx)) & 15) == 0, "input_dgrad: dy, w, dx must be non-NULL and 16-byte aligned");
  ARG_CHECK(B >= 1 && H >= 1 && W >= 1 && B <= 65535 && cdiv(H, ID_T) <= 65535, "input_dgrad: B = %d, H = %d, W = %d", B, H, W);
  ARG_CHECK(in_channels >= 1 && in_channels <= 16, "input_dgrad: in_channels = %d (1 .. 16)", in_channels);
  ARG_CHECK(Cout >= 32 && Cout % 32 == 0, "input_dgrad: Cout = %d must be a positive multiple of 32", Cout);
  const dim3 grid(cdiv(W, ID_T), cdiv(H, ID_T), B), block(ID_THREADS);
  const int Cs = input_cs(in_channels);
  if (W % 4 == 0) hipLaunchKernelGGL(input_dgrad_kernel<true>, grid, block, 0, st, dy, w, dx, gate, H, W, in_channels, Cs, Cout);
  else hipLaunchKernelGGL(input_dgrad_kernel<false>, grid, block, 0, st, dy, w, dx, gate, H, W, in_channels, Cs, Cout);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
