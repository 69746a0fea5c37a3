// Additional skip residuals (sdxl_residuals, include/sdxlstep.h): the skip concat that also adds a caller's NCHW tensor to either half, and
// the gradient with respect to such a tensor, which is a column range of the concat's output gradient.  Both are layout transposes between
// the engine's token-major [B * HW][C] bf16 images and the caller's [B][C][HW] planes, HBM-bound: a workgroup moves one tile of
// RS_TP pixels x RS_TC channels of one sample through LDS, so that both sides are read and written along their contiguous index.
//   token-major side: 16 bytes (8 channels) per lane, 8 lanes cover 128 contiguous bytes of one pixel row;
//   NCHW side: VW pixels per lane along a plane (VW = 4, 2, 1: the widest the plane stride HW keeps aligned);
//   LDS: fp32 [channel][pixel] with a row stride of RS_LD = 65 dwords.  The channel-strided accesses of the token-major phase (lane =
//   (pixel l / 8, channel group l % 8), element k of the group: dword (8 cg + k) 65 + pixel) fall on bank (8 cg + k + pixel) mod 32: the 32
//   lanes that share an LDS cycle (8 groups x 4 consecutive pixels) take 32 different banks.  The pixel-contiguous accesses of the NCHW phase
//   are consecutive dwords (VW = 1) or VW dwords apart (2-way at VW = 4); the kernel's rate is set by HBM, a twentieth of the LDS's.
// Every global access is guarded by pixel < HW and channel < Ca + Cb; a tile never crosses a sample (blockIdx.z).
#include "kernels.h"

#define RS_TP 64
#define RS_TC 64
#define RS_LD 65
#define RS_THREADS 256

namespace {
template <class T, int N> struct RsVec { typedef T type __attribute__((ext_vector_type(N))); };

// VW consecutive pixels of one plane as floats (p % VW == 0 and HW % VW == 0: the access is aligned and whole)
template <class RT, int VW>
__device__ __forceinline__ void rs_load(const RT* __restrict__ src, float* v) {
  if constexpr (VW == 1) {
    v[0] = (float)src[0];
  } else {
    const typename RsVec<RT, VW>::type x = *(const typename RsVec<RT, VW>::type*)src;
#pragma unroll
    for (int k = 0; k < VW; ++k) v[k] = (float)x[k];
  }
}
template <int VW>
__device__ __forceinline__ void rs_store(float* __restrict__ dst, const float* v) {
  if constexpr (VW == 1) {
    dst[0] = v[0];
  } else {
    typename RsVec<float, VW>::type x;
#pragma unroll
    for (int k = 0; k < VW; ++k) x[k] = v[k];
    *(typename RsVec<float, VW>::type*)dst = x;
  }
}

// o [B * HW][Ca + Cb] = a [B * HW][Ca] | b [B * HW][Cb], with ra [B][Ca][HW] / rb [B][Cb][HW] (either may be null) added to its half:
// bf16_rn(float(x) + float(r)), one fp32 add and one round to nearest even; where r == 0 the bits of x pass unchanged.
template <class RT, int VW>
__global__ __launch_bounds__(RS_THREADS) void concat_residual_kernel(const bf16* __restrict__ a, int Ca, const bf16* __restrict__ b, int Cb,
                                                                     const RT* __restrict__ ra, const RT* __restrict__ rb, bf16* __restrict__ o, int HW) {
  __shared__ float tile[RS_TC * RS_LD];
  const int t = threadIdx.x, Ct = Ca + Cb;
  const int p0 = blockIdx.x * RS_TP, c0 = blockIdx.y * RS_TC;
  const long n = blockIdx.z;
  const int c1 = min(c0 + RS_TC, Ct);
  const bool has = (ra && c0 < Ca) || (rb && c1 > Ca);      // block-uniform: a tile none of whose channels has a residual is a plain copy
  if (has) {
    constexpr int PV = RS_TP / VW, ROWS = RS_THREADS / PV;
    const int pl = (t % PV) * VW;
    for (int j = t / PV; j < RS_TC && c0 + j < Ct; j += ROWS) {
      const int cc = c0 + j;
      const RT* r = cc < Ca ? ra : rb;
      float v[VW];
#pragma unroll
      for (int k = 0; k < VW; ++k) v[k] = 0.f;
      if (r && p0 + pl < HW) rs_load<RT, VW>(r + (n * (cc < Ca ? Ca : Cb) + (cc < Ca ? cc : cc - Ca)) * HW + p0 + pl, v);
#pragma unroll
      for (int k = 0; k < VW; ++k) tile[j * RS_LD + pl + k] = v[k];
    }
    __syncthreads();
  }
  for (int i = t; i < RS_TP * (RS_TC / 8); i += RS_THREADS) {
    const int cg = i % (RS_TC / 8), pl = i / (RS_TC / 8);
    const int p = p0 + pl, cc = c0 + 8 * cg;
    if (p >= HW || cc >= Ct) continue;
    const long row = n * HW + p;
    bf16x8 x = cc < Ca ? *(const bf16x8*)(a + row * Ca + cc) : *(const bf16x8*)(b + row * Cb + (cc - Ca));
    if (has) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float r = tile[(8 * cg + k) * RS_LD + pl];
        if (r != 0.f) x[k] = (bf16)((float)x[k] + r);
      }
    }
    *(bf16x8*)(o + row * Ct + cc) = x;
  }
}

// da [B][Ca][HW] / db [B][Cb][HW] fp32 (either may be null) = float(g [B * HW][Ca + Cb]) of their column range; exact zeros when the
// gate scalar reads 0 (g is then 0 x anything: it is not read at all)
template <int VW>
__global__ __launch_bounds__(RS_THREADS) void residual_grad_kernel(const bf16* __restrict__ g, int Ca, int Cb, float* __restrict__ da,
                                                                   float* __restrict__ db, const float* __restrict__ gate, int HW) {
  __shared__ float tile[RS_TC * RS_LD];
  const int t = threadIdx.x, Ct = Ca + Cb;
  const int p0 = blockIdx.x * RS_TP, c0 = blockIdx.y * RS_TC;
  const long n = blockIdx.z;
  const int c1 = min(c0 + RS_TC, Ct);
  if (!((da && c0 < Ca) || (db && c1 > Ca))) return;      // block-uniform: nothing of this tile is asked for
  const bool closed = gate && *gate == 0.f;
  if (!closed) {
    for (int i = t; i < RS_TP * (RS_TC / 8); i += RS_THREADS) {
      const int cg = i % (RS_TC / 8), pl = i / (RS_TC / 8);
      const int p = p0 + pl, cc = c0 + 8 * cg;
      if (p >= HW || cc >= Ct || !(cc < Ca ? da : db)) continue;
      const bf16x8 x = *(const bf16x8*)(g + (n * HW + p) * Ct + cc);
#pragma unroll
      for (int k = 0; k < 8; ++k) tile[(8 * cg + k) * RS_LD + pl] = (float)x[k];
    }
    __syncthreads();
  }
  constexpr int PV = RS_TP / VW, ROWS = RS_THREADS / PV;
  const int pl = (t % PV) * VW;
  if (p0 + pl >= HW) return;
  for (int j = t / PV; j < RS_TC && c0 + j < Ct; j += ROWS) {
    const int cc = c0 + j;
    float* dst = cc < Ca ? da : db;
    if (!dst) continue;
    float v[VW];
#pragma unroll
    for (int k = 0; k < VW; ++k) v[k] = closed ? 0.f : tile[j * RS_LD + pl + k];
    rs_store<VW>(dst + (n * (cc < Ca ? Ca : Cb) + (cc < Ca ? cc : cc - Ca)) * HW + p0 + pl, v);
  }
}

static bool rs_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static int rs_check(const char* who, int Ca, int Cb, int B, int HW) {
  ARG_CHECK(Ca >= 8 && Cb >= 8 && Ca % 8 == 0 && Cb % 8 == 0, "%s: Ca = %d, Cb = %d (positive multiples of 8)", who, Ca, Cb);
  ARG_CHECK(B >= 1 && B <= 65535 && HW >= 1 && cdiv(Ca + Cb, RS_TC) <= 65535, "%s: B = %d, HW = %d", who, B, HW);
  return 0;
}
// pixels per NCHW access: every plane starts a multiple of HW elements behind a 16-byte aligned base
static int rs_vw(int HW) { return HW % 4 == 0 ? 4 : HW % 2 == 0 ? 2 : 1; }

template <class RT>
static void rs_launch_fwd(int vw, dim3 grid, hipStream_t st, const bf16* a, int Ca, const bf16* b, int Cb, const void* ra, const void* rb, bf16* o, int HW) {
  const RT *pa = (const RT*)ra, *pb = (const RT*)rb;
  if (vw == 4) hipLaunchKernelGGL((concat_residual_kernel<RT, 4>), grid, dim3(RS_THREADS), 0, st, a, Ca, b, Cb, pa, pb, o, HW);
  else if (vw == 2) hipLaunchKernelGGL((concat_residual_kernel<RT, 2>), grid, dim3(RS_THREADS), 0, st, a, Ca, b, Cb, pa, pb, o, HW);
  else hipLaunchKernelGGL((concat_residual_kernel<RT, 1>), grid, dim3(RS_THREADS), 0, st, a, Ca, b, Cb, pa, pb, o, HW);
}
}  // namespace

int launch_concat_residual(const bf16* a, int Ca, const bf16* b, int Cb, const void* ra, const void* rb, int rdtype, bf16* o, int B, int HW,
                           hipStream_t st) {
  if (int rc = rs_check("concat_residual", Ca, Cb, B, HW)) return rc;
  ARG_CHECK(rdtype == 0 || rdtype == 1, "concat_residual: residual dtype %d (0 = fp32, 1 = bf16)", rdtype);
  ARG_CHECK(a && b && o && rs_aligned(a, 16) && rs_aligned(b, 16) && rs_aligned(o, 16) && rs_aligned(ra, 16) && rs_aligned(rb, 16),
            "concat_residual: a, b, o must be non-NULL, every pointer 16-byte aligned");
  if (!ra && !rb) return launch_concat(a, Ca, b, Cb, o, (long)B * HW, st);
  const dim3 grid(cdiv(HW, RS_TP), cdiv(Ca + Cb, RS_TC), B);
  if (rdtype == 0) rs_launch_fwd<float>(rs_vw(HW), grid, st, a, Ca, b, Cb, ra, rb, o, HW);
  else rs_launch_fwd<bf16>(rs_vw(HW), grid, st, a, Ca, b, Cb, ra, rb, o, HW);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_residual_grad(const bf16* g, int Ca, int Cb, float* da, float* db, const float* gate, int B, int HW, hipStream_t st) {
  if (int rc = rs_check("concat_residual_grad", Ca, Cb, B, HW)) return rc;
  ARG_CHECK(g && rs_aligned(g, 16) && rs_aligned(da, 16) && rs_aligned(db, 16), "concat_residual_grad: g must be non-NULL, every pointer 16-byte aligned");
  if (!da && !db) return 0;
  const dim3 grid(cdiv(HW, RS_TP), cdiv(Ca + Cb, RS_TC), B);
  const int vw = rs_vw(HW);
  if (vw == 4) hipLaunchKernelGGL(residual_grad_kernel<4>, grid, dim3(RS_THREADS), 0, st, g, Ca, Cb, da, db, gate, HW);
  else if (vw == 2) hipLaunchKernelGGL(residual_grad_kernel<2>, grid, dim3(RS_THREADS), 0, st, g, Ca, Cb, da, db, gate, HW);
  else hipLaunchKernelGGL(residual_grad_kernel<1>, grid, dim3(RS_THREADS), 0, st, g, Ca, Cb, da, db, gate, HW);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
