// Loss side of compute_loss() on device, fp32 arithmetic.
//
// DDPM (reference ddpm_trainer.py:303-384 + novelai_v3.py:111-137):
//   noisy  = clamp(x + sigma_b*noise, +-20000)                  (add_noise, ZTSNR clamp)
//   target = (noise - x)/sqrt(sigma_b^2)   | noise              (v_prediction | epsilon)
//   w_b    = min((1/sigma_b)^2, gamma)     | 1                  (MinSNR, per-sample: SURVEY D3)
//   loss   = mean(w_b * (pred-target)^2) [* mean(tag_w)]  -> guard
// Flow matching (flow_matching_trainer.py:298-335, :387-419):
//   xt = (1-t_b)*x0 + t_b*x1 ; target = x1 - x0 ; loss = mean_b(mean_chw((pred-target)^2)) [* mean(tag_w)] -> guard
// Guard: non-finite -> 1000 (no gradient) ; clamp(max=1000) (zero gradient above the cap).
//
// Beyond the reference, all off by default (LossP: loss_type, sample_w, huber_cb, ps_out), with d = pred - target:
//   element loss l(d): l2 d^2 | huber 2c(sqrt(d^2+c^2)-c) | smooth_l1 2(sqrt(d^2+c^2)-c), c = c_b or the scalar;
//   sqrt(d^2+c^2)-c is computed as d^2/(sqrt(d^2+c^2)+c) (the plain difference cancels for |d| << c)
//   every sample's terms carry (s_b w_b): raw sum = sum_b sum_chw (s_b w_b) l(d), dpred = gate grad_scale (s_b w_b) l'(d) / numel
//   L_b = s_b w_b mean_chw l(d) goes to ps_out, before the tag mean and the guard
// Masked loss (LossP: mask, mask_norm, mnorm), m >= 0 per latent pixel, M_b = sum_hw m; m joins the weight first, (s_b w_b) m:
//   mean        raw = sum (s_b w_b m) l(d), L_b = s_b w_b sum_chw m l(d) / (4 HW), dpred = gate grad_scale (s_b w_b m) l'(d) / numel
//   masked_mean L_b = s_b w_b sum_chw m l(d) / (4 M_b) (0 when M_b = 0), raw = 4 HW sum_b L_b, loss = guard(tm mean_b L_b),
//               dpred = gate grad_scale (s_b w_b m) l'(d) / (B 4 M_b) (0 when M_b = 0); M_b goes from the finalize kernel to the
//               backward through mnorm
//   m = 0 is an exact zero in dpred whatever d is.  The six other sums ignore the mask.
// Input perturbation (LossP: noise_in): only loss_prepare_kernel reads it, in place of noise.
//
// Inputs arrive as the reference hands them over: NCHW fp32 latents / noise.  The UNet consumes and
// produces token-major [B*HW][8] bf16 (4 real channels + 4 zero pad so every row is one 16-byte vector).
// Extra input channels (in_channels 5 .. 16, LossCondP): the input image is [B*HW][Cs], Cs = 8 up to 8 channels, else 16 (one or two
// 16-byte vectors per pixel); channels 4 .. hold bf16(cond), the rest zero.  Only loss_prepare_kernel knows: pred / dpred stay 8 wide.
#include "kernels.h"
#include <type_traits>

// a * b + c and friends with every operation rounded on its own, as separate torch ops do (hipcc contracts a * b + c into
// an FMA by default, and __fmul_rn / __fadd_rn are plain operators to it)
__device__ __forceinline__ float mul_add_rn(float a, float b, float c) {
#pragma clang fp contract(off)
  const float t = a * b;
  return t + c;
}
__device__ __forceinline__ float mul_mul_add_rn(float a, float b, float c, float d) {   // a * b + c * d
#pragma clang fp contract(off)
  const float t = a * b, u = c * d;
  return t + u;
}

__device__ __forceinline__ void loss_target(const LossP& p, int b, float x, float n, float sg, float* target,
                                            float* w) {
  if (p.method == 0) {
    *target = p.prediction_type == 1 ? (n - x) / sqrtf(sg * sg) : n;
    const float inv = 1.f / sg;
    float snr = inv * inv;
    *w = p.use_min_snr ? fminf(snr, p.min_snr_gamma) : 1.f;
  } else {
    *target = x - n;  // x1 - x0
    *w = 1.f;
  }
}

// CS = the stored width of an input pixel (8 | 16, input_cs); COND: channels 4 .. 4 + ncond - 1 hold bf16(cond), the rest zero.
// <8, false> is the kernel of the 4-channel UNet, instruction for instruction; channels 0..3 are the same operations in every instantiation.
template <int CS, bool COND>
__global__ void loss_prepare_kernel(const std::conditional_t<COND, LossCondP, LossP> p) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over B*HW
  if (i >= (long)p.B * p.HW) return;
  int b = (int)(i / p.HW), hw = (int)(i - (long)b * p.HW);
  float sg = p.sigma[b];
  bf16x8 o;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    long idx = ((long)b * 4 + c) * p.HW + hw;
    float x = p.latents[idx], n = p.noise_in[idx];
    float v;
    // every product and sum rounded on its own (no FMA contraction), exactly as the reference's separate torch ops do:
    // the bf16 UNet input is then the round-to-nearest-even image of the reference's fp32 tensor, bit for bit
    if (p.method == 0) {
      v = mul_add_rn(sg, n, x);
      if (p.use_ztsnr) v = fminf(fmaxf(v, -20000.f), 20000.f);
    } else {
      v = mul_mul_add_rn(1.f - sg, n, sg, x);
    }
    o[c] = (bf16)v;
    o[c + 4] = (bf16)0.f;
  }
  if constexpr (COND) {      // (a wave reads 64 consecutive pixels of each cond plane: one 256-byte run per channel, like latents / noise)
    const float* cp = p.cond + (long)b * p.ncond * p.HW + hw;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (c < p.ncond) o[c + 4] = (bf16)cp[(long)c * p.HW];
  }
  *(bf16x8*)(p.unet_in + i * CS) = o;
  if (CS == 16) {
    bf16x8 o2;
#pragma unroll
    for (int c = 0; c < 8; ++c) o2[c] = (bf16)0.f;
    if constexpr (COND) {
      const float* cp = p.cond + (long)b * p.ncond * p.HW + hw;
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c + 4 < p.ncond) o2[c] = (bf16)cp[(long)(c + 4) * p.HW];
    }
    *(bf16x8*)(p.unet_in + i * CS + 8) = o2;
  }
}

// sqrt(d^2 + c^2) - c without the cancellation
__device__ __forceinline__ float pseudo_huber(float d, float c) { return d * d / (sqrtf(d * d + c * c) + c); }

// LT = LossP::loss_type.  The per-sample weight, the per-sample c, the mask and the per-sample output are wave-uniform branches on
// their pointers: with all of them NULL and LT = 0 the arithmetic is the reference's, operation for operation.
template <int LT>
__global__ void loss_fwd_kernel(const LossP p) {
  __shared__ float sred[4][8];
  __shared__ float sps[4], spm[4];
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float mk = 0.f;   // this thread's mask value (0 past the end)
  const bool mm = p.mask && p.mask_norm == 1;
  int bs = -1;      // this thread's sample (-1: past the end)
  if (i < (long)p.B * p.HW) {
    int b = (int)(i / p.HW), hw = (int)(i - (long)b * p.HW);
    bs = b;
    float sg = p.sigma[b];
    const float sw = p.sample_w ? p.sample_w[b] : 1.f;
    const float hc = LT != 0 ? (p.huber_cb ? p.huber_cb[b] : p.huber_c) : 0.f;
    if (p.mask) mk = p.mask[i];
    bf16x8 pv = *(const bf16x8*)(p.pred + i * 8);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      long idx = ((long)b * 4 + c) * p.HW + hw;
      float x = p.latents[idx], n = p.noise[idx], pr = (float)pv[c];
      float tg, w;
      loss_target(p, b, x, n, sg, &tg, &w);
      float d = pr - tg;
      if (p.sample_w) w = sw * w;      // (s_b w_b) first: s_b = 1 leaves every bit as without weights
      if (p.mask) w = w * mk;          // ... then m: m = 1 leaves every bit as without a mask
      if (LT == 0) acc[0] += w * d * d;
      else if (LT == 1) acc[0] += w * (2.f * hc * pseudo_huber(d, hc));
      else acc[0] += w * (2.f * pseudo_huber(d, hc));
      acc[1] += fabsf(pr);
      acc[2] += pr * pr;
      acc[3] += fabsf(n);
      acc[4] += n * n;
      acc[5] += x * x;
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    float s = wave_sum(acc[k]);
    if (lane == 0) sred[wv][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 6)      // the block's six sums as a partial row: loss_finalize_kernel adds the rows in a fixed order (bitwise reproducible loss)
    p.part[(long)blockIdx.x * 6 + threadIdx.x] = sred[0][threadIdx.x] + sred[1][threadIdx.x] + sred[2][threadIdx.x] + sred[3][threadIdx.x];
  if (p.ps_out || mm) {      // the block's loss sum once more, split by sample: slot j = the j-th sample this block touches
    const int S = loss_ps_slots(p.B, p.HW);
    const long nb = ((long)p.B * p.HW + 255) / 256;
    const int b0 = (int)(((long)blockIdx.x * 256) / p.HW);
    for (int j = 0; j < S; ++j) {
      float s = wave_sum(bs == b0 + j ? acc[0] : 0.f);      // selected, not multiplied: a non-finite sample stays in its own slot
      float t = mm ? wave_sum(bs == b0 + j ? mk : 0.f) : 0.f;      // masked_mean: the slot's share of M_b, the column behind
      __syncthreads();
      if (lane == 0) { sps[wv] = s; spm[wv] = t; }
      __syncthreads();
      if (threadIdx.x == 0) {
        p.part[6 * nb + (long)blockIdx.x * S + j] = sps[0] + sps[1] + sps[2] + sps[3];
        if (mm) p.part[(6 + S) * nb + (long)blockIdx.x * S + j] = spm[0] + spm[1] + spm[2] + spm[3];
      }
    }
  }
}

// one wave: lane l adds the partial rows l, l + 64, ... in order, lane 0 then adds the 64 lane sums in order
__global__ void loss_finalize_kernel(const LossP p) {
  __shared__ float sl[6][64];
  __shared__ float sp[64], sq[64];
  const long nb = ((long)p.B * p.HW + 255) / 256;
  const bool mm = p.mask && p.mask_norm == 1;
  float sum_lb = 0.f;      // masked_mean, thread 0: sum_b L_b in sample order
  for (int k = 0; k < 6; ++k) {
    float s = 0.f;
    for (long r = threadIdx.x; r < nb; r += 64) s += p.part[r * 6 + k];
    sl[k][threadIdx.x] = s;
  }
  __syncthreads();
  if (p.ps_out || mm) {      // per sample: the slots of the blocks [b*HW/256, ((b+1)*HW-1)/256] that belong to it, in the same fixed order
    const int S = loss_ps_slots(p.B, p.HW);
    for (int b = 0; b < p.B; ++b) {
      const long lo = ((long)b * p.HW) / 256, hi = ((long)(b + 1) * p.HW - 1) / 256;
      float s = 0.f, q = 0.f;
      for (long r = lo + threadIdx.x; r <= hi; r += 64) {
        const long slot = r * S + (b - (int)((r * 256) / p.HW));
        s += p.part[6 * nb + slot];
        if (mm) q += p.part[(6 + S) * nb + slot];
      }
      sp[threadIdx.x] = s;
      sq[threadIdx.x] = q;
      __syncthreads();
      if (threadIdx.x == 0) {
        float t = 0.f;
        for (int l = 0; l < 64; ++l) t += sp[l];
        if (mm) {      // L_b over the sample's own mask sum; an empty mask is a zero loss (and, in the backward, a zero gradient)
          float M = 0.f;
          for (int l = 0; l < 64; ++l) M += sq[l];
          const float lb = M == 0.f ? 0.f : t / (4.f * M);
          p.mnorm[b] = M;
          sum_lb += lb;
          if (p.ps_out) p.ps_out[b] = lb;
        } else {
          p.ps_out[b] = t / (4.f * (float)p.HW);
        }
      }
      __syncthreads();
    }
  }
  if (threadIdx.x != 0) return;
  for (int k = 0; k < 6; ++k) {
    float s = 0.f;
    for (int l = 0; l < 64; ++l) s += sl[k][l];
    p.out[1 + k] = s;
  }
  float numel = (float)p.B * 4.f * (float)p.HW;
  if (mm) p.out[1] = 4.f * (float)p.HW * sum_lb;      // so that out[0] = out[1] / numel * tm still holds
  float l = mm ? sum_lb / (float)p.B : p.out[1] / numel;
  float tm = 1.f;
  if (p.tag_w) {
    float s = 0.f;
    for (int b = 0; b < p.B; ++b) s += p.tag_w[b];
    tm = s / (float)p.B;
    l *= tm;
  }
  if (!isfinite(l)) { p.out[0] = 1000.f; p.out[7] = 0.f; }
  else if (l > 1000.f) { p.out[0] = 1000.f; p.out[7] = 0.f; }
  else { p.out[0] = l; p.out[7] = tm; }
}

template <int LT>
__global__ void loss_bwd_kernel(const LossP p) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)p.B * p.HW) return;
  int b = (int)(i / p.HW), hw = (int)(i - (long)b * p.HW);
  float sg = p.sigma[b];
  const float sw = p.sample_w ? p.sample_w[b] : 1.f;
  const float hc = LT != 0 ? (p.huber_cb ? p.huber_cb[b] : p.huber_c) : 0.f;
  const float mk = p.mask ? p.mask[i] : 1.f;
  float k = p.out[7] * p.grad_scale * 2.f / ((float)p.B * 4.f * (float)p.HW);
  if (p.mask && p.mask_norm == 1) {      // masked_mean: the sample's own normaliser, left by loss_finalize_kernel
    const float M = p.mnorm[b];
    k = M == 0.f ? 0.f : p.out[7] * p.grad_scale * 2.f / ((float)p.B * 4.f * M);
  }
  bf16x8 pv = *(const bf16x8*)(p.pred + i * 8), o;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    long idx = ((long)b * 4 + c) * p.HW + hw;
    float tg, w;
    loss_target(p, b, p.latents[idx], p.noise[idx], sg, &tg, &w);
    if (p.sample_w) w = sw * w;
    if (p.mask) w = w * mk;
    float d = (float)pv[c] - tg;
    if (LT != 0) {      // l'(d) / 2: huber c d / sqrt(d^2 + c^2), smooth_l1 d / sqrt(d^2 + c^2)
      const float q = sqrtf(d * d + hc * hc);
      d = LT == 1 ? hc * d / q : d / q;
    }
    // guard taken (non-finite or clamped loss, out[7] == 0): an exact zero gradient, also where pred - target is inf / nan;
    // s_b = 0: an exact zero slab for that sample, m = 0: an exact zero pixel, whatever d is
    o[c] = (k == 0.f || (p.sample_w && sw == 0.f) || (p.mask && mk == 0.f)) ? (bf16)0.f : (bf16)(k * w * d);
    o[c + 4] = (bf16)0.f;
  }
  *(bf16x8*)(p.dpred + i * 8) = o;
}

static int check_loss(const LossP& p) {
  ARG_CHECK(p.C == 4, "loss: latent channels must be 4 (got %d)", p.C);
  ARG_CHECK(p.B > 0 && p.HW > 0, "loss: empty batch");
  ARG_CHECK(p.latents && p.noise && p.sigma, "loss: missing inputs");
  ARG_CHECK(p.loss_type >= 0 && p.loss_type <= 2, "loss: loss_type %d (0 = l2, 1 = huber, 2 = smooth_l1)", p.loss_type);
  ARG_CHECK(p.loss_type == 0 || p.huber_cb || p.huber_c > 0.f, "loss: loss_type %d needs huber_c > 0 (got %g)", p.loss_type,
            (double)p.huber_c);
  ARG_CHECK(!p.mask || (p.mask_norm >= 0 && p.mask_norm <= 1), "loss: mask_norm %d (0 = mean, 1 = masked_mean)", p.mask_norm);
  return 0;
}
int launch_loss_prepare(const LossP& p, hipStream_t st, const float* cond, int ncond) {
  if (int e = check_loss(p)) return e;
  long n = (long)p.B * p.HW;
  ARG_CHECK(p.noise_in != nullptr, "loss: missing noise_in (the callers set it to noise)");
  ARG_CHECK(ncond >= 0 && ncond <= 12 && (ncond == 0 || cond), "loss: input_cond is missing for %d extra input channels (0 .. 12)", ncond);
  const dim3 grid(cdiv(n, 256)), block(256);
  LossCondP q;
  static_cast<LossP&>(q) = p;
  q.cond = cond; q.ncond = ncond;
  if (ncond == 0) hipLaunchKernelGGL((loss_prepare_kernel<8, false>), grid, block, 0, st, p);
  else if (input_cs(4 + ncond) == 8) hipLaunchKernelGGL((loss_prepare_kernel<8, true>), grid, block, 0, st, q);
  else hipLaunchKernelGGL((loss_prepare_kernel<16, true>), grid, block, 0, st, q);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
int launch_loss_fwd(const LossP& p, hipStream_t st) {
  if (int e = check_loss(p)) return e;
  long n = (long)p.B * p.HW;
  ARG_CHECK(p.part != nullptr, "loss: missing partial-row scratch (loss_part_floats)");
  ARG_CHECK(!(p.mask && p.mask_norm == 1) || p.mnorm, "loss: masked_mean needs the [B] normaliser scratch");
  if (p.loss_type == 0) hipLaunchKernelGGL(loss_fwd_kernel<0>, dim3(cdiv(n, 256)), dim3(256), 0, st, p);
  else if (p.loss_type == 1) hipLaunchKernelGGL(loss_fwd_kernel<1>, dim3(cdiv(n, 256)), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(loss_fwd_kernel<2>, dim3(cdiv(n, 256)), dim3(256), 0, st, p);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, st, p);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
int launch_loss_bwd(const LossP& p, hipStream_t st) {
  if (int e = check_loss(p)) return e;
  long n = (long)p.B * p.HW;
  ARG_CHECK(!(p.mask && p.mask_norm == 1) || p.mnorm, "loss: masked_mean needs the [B] normaliser scratch");
  if (p.loss_type == 0) hipLaunchKernelGGL(loss_bwd_kernel<0>, dim3(cdiv(n, 256)), dim3(256), 0, st, p);
  else if (p.loss_type == 1) hipLaunchKernelGGL(loss_bwd_kernel<1>, dim3(cdiv(n, 256)), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(loss_bwd_kernel<2>, dim3(cdiv(n, 256)), dim3(256), 0, st, p);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
