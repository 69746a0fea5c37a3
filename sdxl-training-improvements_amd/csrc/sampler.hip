// One sampler step on device (sdxl_sampler_step, include/sdxlstep.h): guidance, denoiser, solver step and the next UNet input in
// one pass over the latent, between two UNet forwards of a sampling loop.
//
//   F       = F_c                                  | F_u + g * (F_c - F_u)          (cfg: rows [0,B) conditional, [B,2B) unconditional)
//   F       = (phi * (F * r)) + ((1 - phi) * F)    r = std(F_c) / std(F) per sample (guidance rescale, phi != 0 only)
//   den     = a_skip * x + a_out * F
//   x_next  = p * x + q * den
//   in_next = bf16(clamp(a_in_next * x_next, +-clamp))                              (clamp <= 0: none)
//
// The extended step (SamplerP::ext, sdxl_sampler_step_ext) is its own instantiation of the step kernel and widens the solver line to
//   acc     = p * x + q * den  [+ r * hist] [+ u * xsave] [+ s * noise]                (a term is read iff its coefficient != 0)
//   hist   <- den (save & 1) ; xsave <- x before the step (save & 2)                   (after hist / xsave were read)
//   y       = k_a * known [+ k_b * knoise] ; x_next = m * acc + (1 - m) * y            (mask != NULL only; m one value per pixel)
// with the same rule: every product and sum rounded on its own, left to right.  All of it is elementwise per pixel, so a buffer may be
// read and overwritten by the same step; the new planes are NCHW fp32 like x (one 256-byte run per wave and channel, one for the mask).
//
// fp32 throughout, every product, sum and difference rounded on its own (no FMA contraction) and in exactly the order written above:
// tests/_sampler_ref.py restates it in separate fp32 torch ops and the kernel is held to it bit for bit.  x is the caller's fp32 NCHW
// state, updated in place; F_c / F_u are read from, and in_next is written to, token-major [rows][8] bf16 images (the plan's prediction and
// input buffers: one 16-byte vector per pixel, channels 4..7 written as zero).  With cfg both halves of the input image receive in_next.
// Extra input channels (SamplerCondP): in_next is [rows][Cs], Cs = 8 | 16, channels 4.. = bf16(cond) from row b (conditional half) and
// row B + b (unconditional half) of cond [rows][ncond][HW], the rest zero; the prediction images stay 8 wide.
//
// Access pattern: one thread per pixel, the sample in blockIdx.y.  A wave reads 64 consecutive pixels: four 256-byte runs of x (one per
// channel plane) and one 1-KiB run of 16-byte vectors per prediction half, and writes the same shapes back, so every access is a full
// run of lines without an LDS transpose; HW is indexed exactly (the last block of a sample is partly idle, nothing is padded).
//
// Guidance rescale needs two standard deviations per sample.  sampler_stats_kernel writes each block's four sums (sum F_c, sum F_c^2,
// sum F, sum F^2 over its pixels' four channels) as a partial row; every block of the step kernel then adds its sample's rows in one fixed
// order.  No atomics, the same bits on every run.  The deviation is the one-pass form sqrt((Q - S * S / n) / (n - 1)): exact enough for
// model outputs, whose mean is small against their spread (it cancels when |mean| >> std).  A sample whose variance is not positive keeps
// r = 1.
#include "kernels.h"
#include <type_traits>

#pragma clang fp contract(off)

__device__ __forceinline__ float sampler_guide(const SamplerP& p, float fc, float fu) {
  if (!p.cfg) return fc;
  float t = fc - fu;
  t = p.guidance * t;
  return fu + t;
}

// the four sums of 256 threads in a fixed order: butterfly inside each wave, then the four wave sums left to right (every thread gets them)
__device__ __forceinline__ void sampler_block_sum4(float v[4], float (*sm)[4]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float s = wave_sum(v[k]);
    if (lane == 0) sm[wv][k] = s;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = ((sm[0][k] + sm[1][k]) + sm[2][k]) + sm[3][k];
  __syncthreads();
}

__global__ __launch_bounds__(256) void sampler_stats_kernel(const SamplerP p) {
  __shared__ float sm[4][4];
  const int b = blockIdx.y;
  const long hw = (long)blockIdx.x * 256 + threadIdx.x;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (hw < p.HW) {
    const bf16x8 fc = *(const bf16x8*)(p.pred + ((long)b * p.HW + hw) * 8);
    bf16x8 fu = fc;
    if (p.cfg) fu = *(const bf16x8*)(p.pred + ((long)(p.B + b) * p.HW + hw) * 8);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float a = (float)fc[c], f = sampler_guide(p, a, (float)fu[c]);
      v[0] += a;
      v[1] += a * a;
      v[2] += f;
      v[3] += f * f;
    }
  }
  sampler_block_sum4(v, sm);
  if (threadIdx.x < 4) p.part[((long)b * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = v[threadIdx.x];
}

// CS / COND as in loss_prepare_kernel (loss.hip): <.., 8, false> are the kernels of the 4-channel UNet, instruction for instruction
template <int RESCALE, int EXT, int CS, bool COND>
__global__ __launch_bounds__(256) void sampler_step_kernel(const std::conditional_t<COND, SamplerCondP, SamplerP> p) {
  __shared__ float sm[4][4];
  const int b = blockIdx.y;
  const long hw = (long)blockIdx.x * 256 + threadIdx.x;
  float ratio = 1.f;
  if (RESCALE) {      // the sample's four sums: thread t adds rows t, t + 256, ... in order, then the block sum
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = threadIdx.x; r < (int)gridDim.x; r += 256) {
      const float* row = p.part + ((long)b * gridDim.x + r) * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] += row[k];
    }
    sampler_block_sum4(v, sm);
    const float n = 4.f * (float)p.HW;
    const float var_c = (v[1] - v[0] * v[0] / n) / (n - 1.f), var_f = (v[3] - v[2] * v[2] / n) / (n - 1.f);
    if (var_c > 0.f && var_f > 0.f) ratio = sqrtf(var_c) / sqrtf(var_f);
  }
  if (hw >= p.HW) return;
  const long ic = ((long)b * p.HW + hw) * 8, iu = ((long)(p.B + b) * p.HW + hw) * 8;
  bf16x8 fc = {}, fu = {}, o;
  float m = 1.f;
  if (EXT && p.mask && !p.init) m = p.mask[(long)b * p.HW + hw];
  if (!p.init) {
    fc = *(const bf16x8*)(p.pred + ic);
    fu = fc;
    if (p.cfg) fu = *(const bf16x8*)(p.pred + iu);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const long idx = ((long)b * 4 + c) * p.HW + hw;
    float x = p.x[idx];
    if (!p.init) {
      float f = sampler_guide(p, (float)fc[c], (float)fu[c]);
      if (RESCALE) {
        float t1 = f * ratio;
        t1 = p.rescale * t1;
        const float t2 = (1.f - p.rescale) * f;
        f = t1 + t2;
      }
      const float d1 = p.a_skip * x, d2 = p.a_out * f;
      const float den = d1 + d2;
      const float u1 = p.p * x, u2 = p.q * den;
      if (EXT) {
        float acc = u1 + u2;
        if (p.r != 0.f) { const float t = p.r * p.hist[idx]; acc = acc + t; }
        if (p.u != 0.f) { const float t = p.u * p.xsave[idx]; acc = acc + t; }
        if (p.s != 0.f) { const float t = p.s * p.noise[idx]; acc = acc + t; }
        if (p.save & 1) p.hist[idx] = den;
        if (p.save & 2) p.xsave[idx] = x;
        if (p.mask) {
          float y = p.k_a * p.known[idx];
          if (p.k_b != 0.f) { const float t = p.k_b * p.knoise[idx]; y = y + t; }
          const float t1 = m * acc, t2 = (1.f - m) * y;
          acc = t1 + t2;
        }
        x = acc;
      } else {
        x = u1 + u2;
      }
      p.x[idx] = x;
    }
    float v = p.a_in_next * x;
    if (p.clamp > 0.f) v = fminf(fmaxf(v, -p.clamp), p.clamp);
    o[c] = (bf16)v;
    o[c + 4] = (bf16)0.f;
  }
  if constexpr (!COND) {
    *(bf16x8*)(p.x_in + ic) = o;
    if (p.cfg) *(bf16x8*)(p.x_in + iu) = o;
  } else {
    // extra input channels: the halves share channels 0..3 and take 4.. from their own rows of cond (b: conditional, B + b: unconditional)
    for (int half = 0; half < (p.cfg ? 2 : 1); ++half) {
      const long row = half ? p.B + b : b;
      const float* cp = p.cond + row * p.ncond * p.HW + hw;
      bf16x8 oh = o;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < p.ncond) oh[c + 4] = (bf16)cp[(long)c * p.HW];
      bf16* dst = p.x_in + (row * p.HW + hw) * CS;
      *(bf16x8*)dst = oh;
      if (CS == 16) {
        bf16x8 o2;
#pragma unroll
        for (int c = 0; c < 8; ++c) o2[c] = (c + 4 < p.ncond) ? (bf16)cp[(long)(c + 4) * p.HW] : (bf16)0.f;
        *(bf16x8*)(dst + 8) = o2;
      }
    }
  }
}

template <int CS, bool COND>
static int launch_sampler_cs(const std::conditional_t<COND, SamplerCondP, SamplerP>& p, bool rescale, bool ext, dim3 grid, dim3 block, hipStream_t st) {
  if (ext) {
    if (rescale) hipLaunchKernelGGL((sampler_step_kernel<1, 1, CS, COND>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((sampler_step_kernel<0, 1, CS, COND>), grid, block, 0, st, p);
  } else {
    if (rescale) hipLaunchKernelGGL((sampler_step_kernel<1, 0, CS, COND>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((sampler_step_kernel<0, 0, CS, COND>), grid, block, 0, st, p);
  }
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_sampler_step(const SamplerP& p, hipStream_t st, const float* cond, int ncond) {
  ARG_CHECK(p.B > 0 && p.HW > 0, "sampler: empty batch");
  ARG_CHECK(p.x && p.x_in && (p.init || p.pred), "sampler: missing buffers");
  const bool rescale = !p.init && p.rescale != 0.f;
  ARG_CHECK(!rescale || p.part, "sampler: guidance rescale needs the partial-row scratch (sampler_part_floats)");
  ARG_CHECK(ncond >= 0 && ncond <= 12 && (ncond == 0 || cond), "sampler: input_cond is missing for %d extra input channels (0 .. 12)", ncond);
  const dim3 grid(cdiv(p.HW, 256), p.B), block(256);
  if (rescale) hipLaunchKernelGGL(sampler_stats_kernel, grid, block, 0, st, p);
  const bool ext = p.ext && !p.init;      // (init writes the input image only: the plain kernel)
  if (ncond == 0) return launch_sampler_cs<8, false>(p, rescale, ext, grid, block, st);
  SamplerCondP q;
  static_cast<SamplerP&>(q) = p;
  q.cond = cond; q.ncond = ncond;
  if (input_cs(4 + ncond) == 8) return launch_sampler_cs<8, true>(q, rescale, ext, grid, block, st);
  return launch_sampler_cs<16, true>(q, rescale, ext, grid, block, st);
}
