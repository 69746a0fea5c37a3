// Fused AdamW_BF16 step for gfx950 (row f1): one pass over the parameter arena.
//
// Reference: src/training/optimizers/adamw_bfloat16/__init__.py:146-197 (`_make_step`) + stochastic/__init__.py:46-124:
// bf16 parameters, bf16 first / second moments, a bf16 error-feedback `shift` (true value = p + shift), three
// stochastically rounded accumulations + one more for the feedback, lazy weight decay.  The reference runs it as ~15
// separate torch kernels per parameter tensor (1 680 tensors); here it is one launch over the packed arena:
// per element 12 B read (p, m, v, shift bf16 + fp32 gradient) and 8 B written = 20 B -> 51.3 GB per step for the
// 2.567 B-parameter UNet -> HBM-bound, >= 6.4 ms at 8 TB/s.
//
// The arithmetic is the reference's float32 sequence with the rounding of each torch op reproduced exactly (see
// oracle/adamw_ref.py, pinned bit-for-bit to fixtures produced by the reference itself): fused multiply-add where
// torch's kernels fuse, bf16-rounded scalars where torch casts them, IEEE divide / sqrt.  `#pragma clang fp
// contract(off)` keeps the compiler from fusing anything else.  Stochastic rounding: r in [0, 2^16) is added to the
// fp32 bit pattern and the low half dropped; r comes from a counter-based generator (Philox-4x32-7 keyed by the
// seed, counter = (element-pair index, step)) or, for the parity tests, from a caller-supplied table.
//
// Two more updates share its entry point and its core, each with its own head comment below: the schedule-free Kahan AdamW
// (algorithm 1, one pass, 16 / 20 B per element) and Prodigy (algorithm 2, two passes around a chip-wide reduction, 50 B per element).
// Adafactor (algorithm 3) shares the entry point and the element-loop parts, but walks a table of tensors in tiles: five launches.
#include "kernels.h"
#include "../../include/sdxlstep.h"
#include <type_traits>

#pragma clang fp contract(off)

__device__ __forceinline__ unsigned mulhi32(unsigned a, unsigned b) { return __umulhi(a, b); }
// Philox-4x32-7 (Salmon et al. 2011; 7 rounds is the variant that passes BigCrush with margin): 128 random bits per
// (counter, key) = the 8 sixteen-bit integers of two elements
__device__ __forceinline__ void philox4x32_7(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                             unsigned out[4]) {
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    const unsigned h0 = mulhi32(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = mulhi32(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ float bf(bf16 x) { return (float)x; }
__device__ __forceinline__ bf16 rn(float x) { return (bf16)x; }                       // round-to-nearest-even
__device__ __forceinline__ bf16 sr(float x, unsigned r16) {                           // stochastic/__init__.py:55-68
  const unsigned u = __float_as_uint(x) + r16;
  return __builtin_bit_cast(bf16, (unsigned short)(u >> 16));
}

// fp32 EMA of the weights, fused into both updates (diffusers EMAModel.step, `s_param.sub_(one_minus_decay * (s_param - param))`)
// on 8 elements whose new bf16 p is final: t1 = e - p, t2 = omd * t1, e = e - t2, each rounded on its own -- the file-wide
// fp contract(off) keeps the compiler from fusing t2 into the last subtraction.  +8 B per element (fp32 read + write).
__device__ __forceinline__ void ema_update8(float* ema, const bf16x8& pv, float omd) {
  f32x4 a = __builtin_nontemporal_load((const f32x4*)ema), b = __builtin_nontemporal_load((const f32x4*)(ema + 4));
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a[e] = a[e] - omd * (a[e] - bf(pv[e]));
    b[e] = b[e] - omd * (b[e] - bf(pv[e + 4]));
  }
  __builtin_nontemporal_store(a, (f32x4*)ema);
  __builtin_nontemporal_store(b, (f32x4*)(ema + 4));
}

// ---- what both update kernels do the same way (OptimP: the fields they share) ----
// 8 gradients from e0 on as floats.  f32: the native fp32 arena (else bf16 gradients); NT_BF16: stream the bf16 gradients past the
// caches like the arenas (the fp32 ones always are)
template <bool NT_BF16>
__device__ __forceinline__ void load_grad8(const OptimP& q, bool f32, size_t e0, float g[8]) {
  if (f32) {
    const f32x4 a = __builtin_nontemporal_load((const f32x4*)(q.grad_f32 + e0)), b = __builtin_nontemporal_load((const f32x4*)(q.grad_f32 + e0 + 4));
    g[0] = a[0]; g[1] = a[1]; g[2] = a[2]; g[3] = a[3]; g[4] = b[0]; g[5] = b[1]; g[6] = b[2]; g[7] = b[3];
  } else {
    const bf16x8 gv = NT_BF16 ? __builtin_nontemporal_load((const bf16x8*)(q.grad_bf16 + e0)) : *(const bf16x8*)(q.grad_bf16 + e0);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = bf(gv[e]);
  }
}
// the gradient the update sees: fused unscale / clip coefficient, then bf16 as the reference's gradients are bf16 tensors
__device__ __forceinline__ float scaled_grad(const OptimP& q, float g, float gscale) {
  const float gr = g * gscale;
  return q.grad_round_bf16 ? bf(rn(gr)) : gr;
}
// exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2) -> v;  denom = exp_avg_sq.sqrt().add_(eps), returned
// (adamw_bfloat16/__init__.py:164, :176-181; the schedule-free reference has the same ops)
__device__ __forceinline__ float second_moment(const OptimP& q, bf16& v, float gr) {
  const float v1 = bf(rn(bf(v) * q.beta2));
  v = rn(__builtin_fmaf(q.one_minus_beta2 * gr, gr, v1));
  const float den = bf(rn(__builtin_sqrtf(bf(v))));
  return bf(rn(den + q.eps_bf16));
}

// EMA: also update q.ema from the new p (ema_update8); EMA = false is the update alone
template <bool INJECT, bool EMA>
__global__ __launch_bounds__(256) void adamw_bf16_kernel(const AdamWP q) {
  const size_t nvec = q.n / 8;
  const float gscale = q.grad_scale ? *q.grad_scale : 1.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e0 = i * 8;
    bf16x8 pv = __builtin_nontemporal_load((const bf16x8*)(q.p + e0)), mv = __builtin_nontemporal_load((const bf16x8*)(q.m + e0)),
           vv = __builtin_nontemporal_load((const bf16x8*)(q.v + e0)), sv = __builtin_nontemporal_load((const bf16x8*)(q.shift + e0));
    float g[8];
    load_grad8<false>(q, q.grad_f32 != nullptr, e0, g);
    unsigned rnd[4][4];     // [element pair][word]: counter = (pair index, step), key = seed
    if (!INJECT) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const size_t pair = q.elem_offset / 2 + i * 4 + k;
        philox4x32_7((unsigned)pair, (unsigned)(pair >> 32), q.step_counter, 0x5D71A3B1u, q.seed_lo, q.seed_hi, rnd[k]);
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      unsigned r0, r1, r2, r3;
      if (INJECT) {
        r0 = q.rand[e0 + e]; r1 = q.rand[q.n + e0 + e]; r2 = q.rand[2 * q.n + e0 + e]; r3 = q.rand[3 * q.n + e0 + e];
      } else {
        const unsigned a = rnd[e >> 1][(e & 1) * 2], b = rnd[e >> 1][(e & 1) * 2 + 1];
        r0 = a & 0xFFFFu; r1 = a >> 16; r2 = b & 0xFFFFu; r3 = b >> 16;
      }
      const float gr = scaled_grad(q, g[e], gscale);
      const float pf = bf(pv[e]), sf = bf(sv[e]);
      // exp_avg.mul_(beta1); add_stochastic_(exp_avg, grad, alpha=1-beta1)       (__init__.py:162-163)
      const float m1 = bf(rn(bf(mv[e]) * q.beta1));
      const float rm = q.reference_ema ? __builtin_fmaf(m1, q.one_minus_beta1, gr)      // grad + alpha * exp_avg (D17)
                                       : __builtin_fmaf(gr, q.one_minus_beta1, m1);     // exp_avg + alpha * grad
      const bf16 m2b = sr(rm, r0);
      const float m2 = bf(m2b);
      bf16 v2b = vv[e];
      const float den = second_moment(q, v2b, gr);
      // addcdiv_stochastic_(shift, exp_avg, denom, value=-lr*sqrt(1-beta2^t))       (stochastic:106-124)
      const bf16 s1b = sr(sf + (q.value * m2) / den, r1);
      const float s1 = bf(s1b);
      // buffer = p.clone(); add_stochastic_(p, shift); add_stochastic_(shift, buffer - p)   (:183-190)
      const bf16 p1b = sr(s1 + pf, r2);
      const float diff = bf(rn(pf - bf(p1b)));
      bf16 s2b = sr(diff + s1, r3);
      // lazy decay, when this tensor's accumulated decay is due: shift.add_(p, alpha=-decay)  (:192-193)
      if (q.decay_alpha_bf16 != 0.f) s2b = rn(__builtin_fmaf(bf(p1b), q.decay_alpha_bf16, bf(s2b)));
      pv[e] = p1b; mv[e] = m2b; vv[e] = v2b; sv[e] = s2b;
    }
    __builtin_nontemporal_store(pv, (bf16x8*)(q.p + e0));      // streamed once per update: keep them out of the caches
    __builtin_nontemporal_store(mv, (bf16x8*)(q.m + e0));
    __builtin_nontemporal_store(vv, (bf16x8*)(q.v + e0));
    __builtin_nontemporal_store(sv, (bf16x8*)(q.shift + e0));
    if constexpr (EMA) ema_update8(q.ema + e0, pv, q.ema_omd);   // tracks p itself, not p + shift
  }
}

// shift.add_(p, alpha) over one parameter tensor's range (alpha already rounded to bf16, as torch does)
__global__ void adamw_decay_kernel(bf16* shift, const bf16* p, size_t n, float alpha) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    shift[i] = rn(__builtin_fmaf(bf(p[i]), alpha, bf(shift[i])));
}

// ---- what both launches do the same way ----
// the argument checks, `who` in front of each message: the buffers are there (third: shift / kahan_comp, may be NULL unless
// need_third), n and the launch's arena offset are multiples of 8 (mult8: that message, which names what the algorithm has), and
// every buffer is 16-byte aligned
static int check_arenas(const OptimP& q, const bf16* third, bool need_third, size_t elem_offset, const char* who, const char* mult8) {
  ARG_CHECK(q.p && q.m && q.v && (third || !need_third) && (q.grad_f32 || q.grad_bf16), "%s: missing buffers", who);
  ARG_CHECK(q.n % 8 == 0 && elem_offset % 8 == 0, mult8, who, q.n, elem_offset);
  ARG_CHECK((((uintptr_t)q.p | (uintptr_t)q.m | (uintptr_t)q.v | (uintptr_t)third | (uintptr_t)q.grad_f32 | (uintptr_t)q.grad_bf16 |
              (uintptr_t)q.ema) & 15) == 0,
            "%s: buffers must be 16-byte aligned", who);
  return 0;
}
// 256 threads x 8 elements per workgroup, at most 16 workgroups per CU (256 CUs): the kernels grid-stride the rest
static_assert(SDXL_PRODIGY_MAX_GRID == 256 * 16, "SDXL_PRODIGY_STATE_FLOATS is sized by the largest grid arena_grid returns");
static dim3 arena_grid(size_t n) {
  size_t blocks = (n / 8 + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  return dim3((unsigned)blocks);
}
// runtime flags -> bool template arguments: with_flags(f, a, b, ...) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...)
template <class F>
static void with_flags(F f) { f(); }
template <class F, class... Flags>
static void with_flags(F f, bool flag, Flags... rest) {
  if (flag) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

int launch_adamw_bf16(const AdamWP& q, hipStream_t st) {
  if (int rc = check_arenas(q, q.shift, true, q.elem_offset, "adamw", "%s: n=%zu, elem_offset=%zu: each must be a multiple of 8")) return rc;
  if (q.n == 0) return 0;
  with_flags([&](auto inject, auto ema) {
    hipLaunchKernelGGL((adamw_bf16_kernel<decltype(inject)::value, decltype(ema)::value>), arena_grid(q.n), dim3(256), 0, st, q);
  }, q.rand != nullptr, q.ema != nullptr);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_adamw_decay(bf16* shift, const bf16* p, size_t n, float alpha_bf16, hipStream_t st) {
  if (n == 0) return 0;
  size_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(adamw_decay_kernel, dim3((unsigned)blocks), dim3(256), 0, st, shift, p, n, alpha_bf16);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// ---- schedule-free Kahan AdamW (reference: src/training/optimizers/adamw_schedulefree/__init__.py, `step`) ----------------
// One grid-stride pass, no random numbers.  Per element 16 B (p, m, v bf16 read and written + fp32 gradient read), 20 B with
// the Kahan arena c: 41.1 / 51.3 GB over the 2.567 B-parameter arena.  Moments and denominator are the reference's bf16 ops
// in both modes:  m = rn(rn(m*b1) + bf16(1-b1)*g)  v = rn(rn(v*b2) + ((1-b2)*g)*g)  d = rn(rn(sqrt(v)) + bf16(eps)).
//   REF  (optimizer.schedule_free_arithmetic "reference"): the reference's sequence bit for bit --
//        g = rn(g + c); p = rn(p + bf16(-wd)*p); u = rn(rn(m/d) * -step_size); p = rn(p + u);
//        c = rn(rn(p - rn(p + u)) + rn(rn(p + u) - p))   (+0 for every finite value, as in the reference).
//        The gradient is read only: the reference's in-place p.grad += kahan_comp is not reproduced.
//   !REF ("compensated"): x = p + c in fp32; x -= (step_size*wd)*x; x -= step_size*(m/d); p = rn(x); c = rn(x - p).
// KAHAN = kahan_sum (without it c is neither read nor written); F32G = fp32 (native arena) or bf16 gradients; EMA = also update
// q.ema from the new p (ema_update8: tracks p, not p + c).
template <bool REF, bool KAHAN, bool F32G, bool EMA>
__global__ __launch_bounds__(256) void sfk_kernel(const SfkP q) {
  const size_t nvec = q.n / 8;
  const float gscale = q.grad_scale ? *q.grad_scale : 1.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e0 = i * 8;
    bf16x8 pv = __builtin_nontemporal_load((const bf16x8*)(q.p + e0)), mv = __builtin_nontemporal_load((const bf16x8*)(q.m + e0)),
           vv = __builtin_nontemporal_load((const bf16x8*)(q.v + e0));
    bf16x8 cv;
    if constexpr (KAHAN) cv = __builtin_nontemporal_load((const bf16x8*)(q.c + e0));
    float g[8];
    load_grad8<true>(q, F32G, e0, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float gr = scaled_grad(q, g[e], gscale);
      if constexpr (REF && KAHAN) gr = bf(rn(gr + bf(cv[e])));  // grad.add_(kahan_comp)
      const float m1 = bf(rn(bf(mv[e]) * q.beta1));
      const bf16 m2b = rn(__builtin_fmaf(gr, q.one_minus_beta1_bf16, m1));
      const float m2 = bf(m2b);
      bf16 v2b = vv[e];
      const float den = second_moment(q, v2b, gr);
      float pf = bf(pv[e]);
      if constexpr (REF) {
        if (q.has_wd) pf = bf(rn(__builtin_fmaf(pf, q.wd_alpha_bf16, pf)));   // p.data.add_(p.data, alpha=-weight_decay)
        const float u = bf(rn(bf(rn(m2 / den)) * q.neg_step));                 // -step_size * (exp_avg / denom)
        const float p1 = bf(rn(pf + u));
        pv[e] = rn(p1);
        if constexpr (KAHAN) {
          const float b = bf(rn(p1 + u));
          cv[e] = rn(bf(rn(p1 - b)) + bf(rn(b - p1)));
        }
      } else {
        float x = pf;
        if constexpr (KAHAN) x = pf + bf(cv[e]);
        if (q.has_wd) x = x - q.decay * x;
        x = x - q.step * (m2 / den);
        const bf16 pb = rn(x);
        pv[e] = pb;
        if constexpr (KAHAN) cv[e] = rn(x - bf(pb));
      }
      mv[e] = m2b; vv[e] = v2b;
    }
    __builtin_nontemporal_store(pv, (bf16x8*)(q.p + e0));
    __builtin_nontemporal_store(mv, (bf16x8*)(q.m + e0));
    __builtin_nontemporal_store(vv, (bf16x8*)(q.v + e0));
    if constexpr (KAHAN) __builtin_nontemporal_store(cv, (bf16x8*)(q.c + e0));
    if constexpr (EMA) ema_update8(q.ema + e0, pv, q.ema_omd);
  }
}

int launch_sfk(const SfkP& q, int reference, hipStream_t st) {
  if (int rc = check_arenas(q, q.c, false, 0, "schedule-free", "%s: n=%zu must be a multiple of 8")) return rc;
  if (q.n == 0) return 0;
  with_flags([&](auto ref, auto kahan, auto f32g, auto ema) {
    hipLaunchKernelGGL((sfk_kernel<decltype(ref)::value, decltype(kahan)::value, decltype(f32g)::value, decltype(ema)::value>),
                       arena_grid(q.n), dim3(256), 0, st, q);
  }, reference != 0, q.c != nullptr, q.grad_f32 != nullptr, q.ema != nullptr);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// ---- Prodigy (Mishchenko & Defazio 2023; include/sdxlstep.h, algorithm 2, is the contract) -------------------------------------
// AdamW whose step size d is estimated from two sums over the arena, A = sum g.(p0 - x) and Bs = sum |s|, so one update is two
// grid-stride passes with a chip-wide reduction between them, in three launches; the kernel boundary is the only synchronisation
// (no atomics, no in-launch ticket), and d lives in q.state on the device: a step costs no host read-back.
//   accumulate: reads p, c, p0 (bf16), the fp32 gradient, m, v, s (fp32) = 22 B; writes m, v, s = 12 B; one partial pair per workgroup
//   finalize:   one workgroup: the partials in ascending workgroup index, in double; the scalar recurrence of d
//   apply:      reads p, c (bf16), m, v (fp32) = 12 B; writes p, c = 4 B (+8 B with the EMA)
// Per element 50 B (48 B with bf16 gradients) -> 128 GB over the 2.567 B-parameter arena, >= 16 ms at 8 TB/s; the adapter arenas
// it is mostly used on are a few MB.  fp32 throughout, each operation rounded on its own (fp contract(off) above).
struct ProdigyScalars { float dlr, cm, cv, cs, cn; };
__device__ __forceinline__ ProdigyScalars prodigy_scalars(const ProdigyP& q, float d) {
  ProdigyScalars k;
  k.dlr = (d * q.lr) * q.bc;
  k.cm = d * q.one_minus_beta1;
  k.cv = (d * d) * q.one_minus_beta2;
  const float r = d / q.d0;
  k.cs = r * (q.safeguard ? d : k.dlr);
  k.cn = r * k.dlr;
  return k;
}
__device__ __forceinline__ void load8(const float* x, float o[8]) {
  const f32x4 a = __builtin_nontemporal_load((const f32x4*)x), b = __builtin_nontemporal_load((const f32x4*)(x + 4));
  o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3]; o[4] = b[0]; o[5] = b[1]; o[6] = b[2]; o[7] = b[3];
}
__device__ __forceinline__ void store8(float* x, const float o[8]) {
  const f32x4 a = {o[0], o[1], o[2], o[3]}, b = {o[4], o[5], o[6], o[7]};
  __builtin_nontemporal_store(a, (f32x4*)x);
  __builtin_nontemporal_store(b, (f32x4*)(x + 4));
}

template <bool F32G>
__global__ __launch_bounds__(256) void prodigy_accumulate_kernel(const ProdigyP q) {
  __shared__ float red_t[256], red_a[256];
  const size_t nvec = q.n / 8;
  const float gscale = q.grad_scale ? *q.grad_scale : 1.f;
  const ProdigyScalars k = prodigy_scalars(q, q.state[0]);
  float sum_t = 0.f, sum_a = 0.f;       // this thread's vectors in grid-stride order, elements 0 .. 7 of each
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e0 = i * 8;
    const bf16x8 pv = __builtin_nontemporal_load((const bf16x8*)(q.p + e0)), cv = __builtin_nontemporal_load((const bf16x8*)(q.c + e0)),
                 p0v = __builtin_nontemporal_load((const bf16x8*)(q.p0 + e0));
    float g[8], m[8], v[8], s[8];
    load_grad8<true>(q, F32G, e0, g);
    load8(q.m32 + e0, m);
    load8(q.v32 + e0, v);
    load8(q.s + e0, s);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float gr = scaled_grad(q, g[e], gscale);
      const float x = bf(pv[e]) + bf(cv[e]);
      const float t = gr * (bf(p0v[e]) - x);
      m[e] = (q.beta1 * m[e]) + (k.cm * gr);
      v[e] = (q.beta2 * v[e]) + ((k.cv * gr) * gr);
      s[e] = (q.beta3 * s[e]) + (k.cs * gr);
      sum_t = sum_t + t;
      sum_a = sum_a + __builtin_fabsf(s[e]);
    }
    store8(q.m32 + e0, m);
    store8(q.v32 + e0, v);
    store8(q.s + e0, s);
  }
  // the workgroup's fixed tree: x[j] += x[j + h], h = 128 .. 1
  red_t[threadIdx.x] = sum_t;
  red_a[threadIdx.x] = sum_a;
  __syncthreads();
#pragma unroll
  for (int h = 128; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) {
      red_t[threadIdx.x] = red_t[threadIdx.x] + red_t[threadIdx.x + h];
      red_a[threadIdx.x] = red_a[threadIdx.x] + red_a[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    q.state[8 + 2 * (size_t)blockIdx.x] = red_t[0];
    q.state[8 + 2 * (size_t)blockIdx.x + 1] = red_a[0];
  }
}

// one workgroup of 256 threads; grid = the accumulate launch's grid (<= SDXL_PRODIGY_MAX_GRID partial pairs)
__global__ __launch_bounds__(256) void prodigy_finalize_kernel(const ProdigyP q, int grid) {
  __shared__ double red_t[256], red_a[256];
  const int per = (grid + 255) / 256;
  double st = 0.0, sa = 0.0;
  for (int b = (int)threadIdx.x * per; b < ((int)threadIdx.x + 1) * per && b < grid; ++b) {
    st = st + (double)q.state[8 + 2 * b];
    sa = sa + (double)q.state[8 + 2 * b + 1];
  }
  red_t[threadIdx.x] = st;
  red_a[threadIdx.x] = sa;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double At = 0.0, Ba = 0.0;
  for (int j = 0; j < 256; ++j) {
    At = At + red_t[j];
    Ba = Ba + red_a[j];
  }
  const float A = (float)At, Bs = (float)Ba;
  const float d = q.state[0], d_max = q.state[1], num = q.state[2];
  const ProdigyScalars k = prodigy_scalars(q, d);
  const float num1 = (q.beta3 * num) + (k.cn * A);
  float d_new = d, d_max_new = d_max, d_hat = d;
  if (Bs > 0.f) {
    d_hat = (q.d_coef * num1) / Bs;
    const float d1 = d == q.d0 ? __builtin_fmaxf(d, d_hat) : d;
    d_max_new = __builtin_fmaxf(d_max, d_hat);
    d_new = __builtin_fminf(d_max_new, d1 * q.growth);
  }
  q.state[0] = d_new; q.state[1] = d_max_new; q.state[2] = num1; q.state[3] = Bs;
  q.state[4] = d_hat; q.state[5] = k.dlr; q.state[6] = A; q.state[7] = 0.f;
}

template <bool EMA>
__global__ __launch_bounds__(256) void prodigy_apply_kernel(const ProdigyP q) {
  const size_t nvec = q.n / 8;
  const float de = q.state[0] * q.eps, dlr = q.state[5];
  const float decay = q.wd * dlr;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e0 = i * 8;
    bf16x8 pv = __builtin_nontemporal_load((const bf16x8*)(q.p + e0)), cv = __builtin_nontemporal_load((const bf16x8*)(q.c + e0));
    float m[8], v[8];
    load8(q.m32 + e0, m);
    load8(q.v32 + e0, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float x = bf(pv[e]) + bf(cv[e]);
      if (q.wd != 0.f) x = x - (decay * x);
      x = x - (dlr * (m[e] / (__builtin_sqrtf(v[e]) + de)));
      const bf16 pb = rn(x);
      pv[e] = pb;
      cv[e] = rn(x - bf(pb));
    }
    __builtin_nontemporal_store(pv, (bf16x8*)(q.p + e0));
    __builtin_nontemporal_store(cv, (bf16x8*)(q.c + e0));
    if constexpr (EMA) ema_update8(q.ema + e0, pv, q.ema_omd);
  }
}

int launch_prodigy(const ProdigyP& q, hipStream_t st) {
  const char* who = "prodigy (algorithm 2)";
  if (int rc = check_arenas(q, q.c, true, 0, who, "%s: n=%zu must be a multiple of 8")) return rc;
  ARG_CHECK(q.p0 && q.s && q.state, "%s: missing buffers (p0, s, prodigy_state)", who);
  ARG_CHECK((((uintptr_t)q.p0 | (uintptr_t)q.s | (uintptr_t)q.state) & 15) == 0, "%s: buffers must be 16-byte aligned", who);
  if (q.n == 0 || q.lr == 0.f) return 0;      // a schedule that starts at 0: nothing is written
  const dim3 grid = arena_grid(q.n);
  with_flags([&](auto f32g) {
    hipLaunchKernelGGL((prodigy_accumulate_kernel<decltype(f32g)::value>), grid, dim3(256), 0, st, q);
  }, q.grad_f32 != nullptr);
  hipLaunchKernelGGL(prodigy_finalize_kernel, dim3(1), dim3(256), 0, st, q, (int)grid.x);
  with_flags([&](auto ema) {
    hipLaunchKernelGGL((prodigy_apply_kernel<decltype(ema)::value>), grid, dim3(256), 0, st, q);
  }, q.ema != nullptr);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

// ---- Adafactor (Shazeer & Stern 2018; include/sdxlstep.h, algorithm 3, is the contract) ------------------------------------------
// The second moment of a matrix is a row and a column statistic, and the update is clipped by its own RMS per tensor, so the step
// is per-tensor reductions around element passes.  One grid covers every tensor: a workgroup takes tiles of AF_ROWS x AF_COLS
// elements from the prefix table (tensor, row block, column block); the kernel boundary is the only synchronisation.
//   stats:   reads g (4 B; + p, c = 4 B with scale_parameter); a tile's row sums, column sums and sum of x^2 from one pass
//   reduce:  the tile sums -> R', C' and the chunk partials of R' (a few bytes per row and column)
//   usq:     reads g (4 B; unfactored: v read and written); a tile's sum of u^2
//   scalars: one workgroup per tensor -> rho_t, eta_t
//   apply:   reads g, p, c (8 B), writes p, c (4 B); + 8 B with beta1, + 8 B with the EMA
// Per element 20 B (24 B with scale_parameter: g is read three times) against AdamW_BF16's 20 B; state rows + cols floats per matrix.
__device__ __forceinline__ int af_find(const AfTensor* tab, int n, int item, int AfTensor::*first) {
  int lo = 0, hi = n - 1;                  // the last entry whose first work item is <= item
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].*first <= item) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ float af_rsqrt(float y) { return 1.f / __builtin_sqrtf(y); }
// the workgroup's fixed tree over one value per thread: x[j] += x[j + h], h = 128 .. 1; the sum is returned to thread 0
__device__ __forceinline__ float af_block_sum(float* red, float x) {
  __syncthreads();                         // red may still be read from the previous use
  red[threadIdx.x] = x;
  __syncthreads();
#pragma unroll
  for (int h = 128; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + h];
    __syncthreads();
  }
  return red[0];
}
// where a thread stands in a tile
struct AfTile {
  const AfTensor* t;
  int rb, cb, lane, rl;                    // lane: its 8-column vector in the tile, rl: its first row in the tile
  int col0;                                // its first column in the tensor
  bool col_ok;
};
__device__ __forceinline__ AfTile af_tile(const AdafactorP& q, int tile) {
  AfTile a;
  a.t = q.table + af_find(q.table, q.n_tensors, tile, &AfTensor::tile0);
  const int local = tile - a.t->tile0;
  a.rb = local / a.t->ncb; a.cb = local - a.rb * a.t->ncb;
  a.lane = threadIdx.x & 31; a.rl = threadIdx.x >> 5;
  a.col0 = a.cb * AF_COLS + a.lane * 8;
  a.col_ok = a.col0 < a.t->cols;
  return a;
}
__device__ __forceinline__ float af_mean_row(const AfTensor& t) {
  float s = 0.f;
  for (int j = 0; j < t.nrc; ++j) s = s + t.rch[j];
  return s / (float)t.rows;
}
// rf = rsqrt(R'_r / mean) of a tile's rows into LDS, once per row (thread j takes row j of the tile); every thread of the workgroup calls it
__device__ __forceinline__ void af_row_factors(const AfTensor& t, int rb, float* rfs) {
  __syncthreads();                         // rfs may still be read from the previous tile
  if (t.factored && (int)threadIdx.x < AF_ROWS) {
    const int r = rb * AF_ROWS + (int)threadIdx.x;
    if (r < t.rows) rfs[threadIdx.x] = af_rsqrt(t.R[r] / af_mean_row(t));
  }
  __syncthreads();
}

template <bool F32G>
__global__ __launch_bounds__(256) void adafactor_stats_kernel(const AdafactorP q) {
  __shared__ float red[256];
  __shared__ float colred[8][AF_COLS];
  const float gscale = q.grad_scale ? *q.grad_scale : 1.f;
  for (int tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
    const AfTile a = af_tile(q, tile);
    const AfTensor& t = *a.t;
    if (!t.factored && !q.scale_parameter) continue;       // (uniform over the workgroup) nothing to sum
    float colacc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float sx = 0.f;
#pragma unroll 4
    for (int i = 0; i < AF_ROWS / 8; ++i) {
      const int r = a.rb * AF_ROWS + i * 8 + a.rl;
      const bool ok = a.col_ok && r < t.rows;
      float rs = 0.f;
      if (ok) {
        const size_t e0 = t.elem_off + (size_t)r * t.cols + a.col0;
        if (t.factored) {
          float g[8];
          load_grad8<true>(q, F32G, e0, g);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float gr = scaled_grad(q, g[e], gscale);
            const float qq = (gr * gr) + q.eps1;
            rs = rs + qq;
            colacc[e] = colacc[e] + qq;
          }
        }
        if (q.scale_parameter) {
          const bf16x8 pv = __builtin_nontemporal_load((const bf16x8*)(q.p + e0)), cv = __builtin_nontemporal_load((const bf16x8*)(q.c + e0));
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float x = bf(pv[e]) + bf(cv[e]);
            sx = sx + (x * x);
          }
        }
      }
      if (t.factored) {                                     // the row's 32 threads: every one of them ends with the same sum
#pragma unroll
        for (int h = 16; h >= 1; h >>= 1) rs = rs + __shfl_xor(rs, h);
        if (a.lane == 0 && r < t.rows) t.rowp[(size_t)r * t.ncb + a.cb] = rs;
      }
    }
    if (t.factored) {
      __syncthreads();                                      // colred may still be read from the previous tile
#pragma unroll
      for (int e = 0; e < 8; ++e) colred[a.rl][a.lane * 8 + e] = colacc[e];
      __syncthreads();
      const int col = a.cb * AF_COLS + (int)threadIdx.x;
      if (col < t.cols) {
        float s = colred[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < 8; ++k) s = s + colred[k][threadIdx.x];
        t.colp[(size_t)a.rb * t.cols + col] = s;
      }
    }
    if (q.scale_parameter) {
      const float s = af_block_sum(red, sx);
      if (threadIdx.x == 0) t.sx[tile - t.tile0] = s;
    }
  }
}

// work items: per factored tensor its chunks of 256 rows, then its chunks of 256 columns
__global__ __launch_bounds__(256) void adafactor_reduce_kernel(const AdafactorP q) {
  __shared__ float red[256];
  for (int item = blockIdx.x; item < q.chunks; item += gridDim.x) {
    const AfTensor& t = q.table[af_find(q.table, q.n_tensors, item, &AfTensor::chunk0)];
    const int local = item - t.chunk0;
    if (local < t.nrc) {
      const int o = local * 256 + (int)threadIdx.x;
      float r1 = 0.f;
      if (o < t.rows) {
        float s = 0.f;
        for (int cb = 0; cb < t.ncb; ++cb) s = s + t.rowp[(size_t)o * t.ncb + cb];
        r1 = (q.b2t * t.R[o]) + (q.omb2t * (s / (float)t.cols));
        t.R[o] = r1;
      }
      const float part = af_block_sum(red, r1);
      if (threadIdx.x == 0) t.rch[local] = part;
    } else {
      const int i = (local - t.nrc) * 256 + (int)threadIdx.x;
      if (i < t.cols) {
        float s = 0.f;
        for (int rb = 0; rb < t.nrb; ++rb) s = s + t.colp[(size_t)rb * t.cols + i];
        t.C[i] = (q.b2t * t.C[i]) + (q.omb2t * (s / (float)t.rows));
      }
    }
  }
}

// u of a thread's 8 elements in row r (factored: rf = rsqrt(R'_r / mean), cf = rsqrt(C') of its columns; unfactored: from v, which
// UPDATE_V also advances and writes back); the same expressions in usq and in apply, so both see the same bits
template <bool F32G, bool UPDATE_V>
__device__ __forceinline__ void af_update8(const AdafactorP& q, const AfTensor& t, size_t e0, size_t v0, float rf, const float cf[8], float gscale,
                                           float u[8]) {
  float g[8];
  load_grad8<true>(q, F32G, e0, g);
  if (t.factored) {
#pragma unroll
    for (int e = 0; e < 8; ++e) u[e] = (rf * cf[e]) * scaled_grad(q, g[e], gscale);
  } else {
    float v[8];
    load8(t.R + v0, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float gr = scaled_grad(q, g[e], gscale);
      if constexpr (UPDATE_V) v[e] = (q.b2t * v[e]) + (q.omb2t * ((gr * gr) + q.eps1));
      u[e] = af_rsqrt(v[e]) * gr;
    }
    if constexpr (UPDATE_V) store8(t.R + v0, v);
  }
}

template <bool F32G>
__global__ __launch_bounds__(256) void adafactor_usq_kernel(const AdafactorP q) {
  __shared__ float red[256], rfs[AF_ROWS];
  const float gscale = q.grad_scale ? *q.grad_scale : 1.f;
  for (int tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
    const AfTile a = af_tile(q, tile);
    const AfTensor& t = *a.t;
    float cf[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (t.factored && a.col_ok) {
#pragma unroll
      for (int e = 0; e < 8; ++e) cf[e] = af_rsqrt(t.C[a.col0 + e]);
    }
    af_row_factors(t, a.rb, rfs);
    float su = 0.f;
#pragma unroll 4
    for (int i = 0; i < AF_ROWS / 8; ++i) {
      const int r = a.rb * AF_ROWS + i * 8 + a.rl;
      if (a.col_ok && r < t.rows) {
        const size_t v0 = (size_t)r * t.cols + a.col0;
        const float rf = t.factored ? rfs[i * 8 + a.rl] : 0.f;
        float u[8];
        af_update8<F32G, true>(q, t, t.elem_off + v0, v0, rf, cf, gscale, u);
#pragma unroll
        for (int e = 0; e < 8; ++e) su = su + (u[e] * u[e]);
      }
    }
    const float s = af_block_sum(red, su);
    if (threadIdx.x == 0) t.su[tile - t.tile0] = s;
  }
}

// one workgroup per tensor
__global__ __launch_bounds__(256) void adafactor_scalars_kernel(const AdafactorP q) {
  __shared__ double red_u[256], red_x[256];
  for (int ti = blockIdx.x; ti < q.n_tensors; ti += gridDim.x) {
    const AfTensor& t = q.table[ti];
    const int T = t.nrb * t.ncb, per = (T + 255) / 256;
    double su = 0.0, sx = 0.0;
    for (int b = (int)threadIdx.x * per; b < ((int)threadIdx.x + 1) * per && b < T; ++b) {
      su = su + (double)t.su[b];
      if (q.scale_parameter) sx = sx + (double)t.sx[b];
    }
    __syncthreads();
    red_u[threadIdx.x] = su;
    red_x[threadIdx.x] = sx;
    __syncthreads();
    if (threadIdx.x == 0) {
      double U = 0.0, X = 0.0;
      for (int j = 0; j < 256; ++j) {
        U = U + red_u[j];
        X = X + red_x[j];
      }
      const float nf = (float)t.numel;
      const float rms_u = __builtin_sqrtf((float)U / nf), rms_p = __builtin_sqrtf((float)X / nf);
      const float rho_t = q.scale_parameter ? q.rho * __builtin_fmaxf(q.eps2, rms_p) : q.rho;
      const float eta_t = rho_t / __builtin_fmaxf(1.f, rms_u / q.clip);
      float* o = q.scal + 4 * (size_t)ti;
      o[0] = rho_t; o[1] = eta_t; o[2] = rms_u; o[3] = rms_p;
    }
  }
}

template <bool F32G, bool EMA, bool BETA1>
__global__ __launch_bounds__(256) void adafactor_apply_kernel(const AdafactorP q) {
  __shared__ float rfs[AF_ROWS];
  const float gscale = q.grad_scale ? *q.grad_scale : 1.f;
  for (int tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
    const AfTile a = af_tile(q, tile);
    const AfTensor& t = *a.t;
    af_row_factors(t, a.rb, rfs);
    if (!a.col_ok) continue;
    const float* sc = q.scal + 4 * (size_t)(a.t - q.table);
    const float rho_t = sc[0], eta_t = sc[1];
    const float decay = q.wd * rho_t;
    float cf[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (t.factored) {
#pragma unroll
      for (int e = 0; e < 8; ++e) cf[e] = af_rsqrt(t.C[a.col0 + e]);
    }
#pragma unroll 2
    for (int i = 0; i < AF_ROWS / 8; ++i) {
      const int r = a.rb * AF_ROWS + i * 8 + a.rl;
      if (r >= t.rows) break;
      const size_t v0 = (size_t)r * t.cols + a.col0, e0 = t.elem_off + v0;
      const float rf = t.factored ? rfs[i * 8 + a.rl] : 0.f;
      float u[8], m[8];
      af_update8<F32G, false>(q, t, e0, v0, rf, cf, gscale, u);
      bf16x8 pv = __builtin_nontemporal_load((const bf16x8*)(q.p + e0)), cv = __builtin_nontemporal_load((const bf16x8*)(q.c + e0));
      if constexpr (BETA1) load8(q.m32 + e0, m);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float d = eta_t * u[e];
        if constexpr (BETA1) {
          m[e] = (q.beta1 * m[e]) + (q.omb1 * d);
          d = m[e];
        }
        float x = bf(pv[e]) + bf(cv[e]);
        if (q.wd != 0.f) x = x - (decay * x);
        x = x - d;
        const bf16 pb = rn(x);
        pv[e] = pb;
        cv[e] = rn(x - bf(pb));
      }
      __builtin_nontemporal_store(pv, (bf16x8*)(q.p + e0));
      __builtin_nontemporal_store(cv, (bf16x8*)(q.c + e0));
      if constexpr (BETA1) store8(q.m32 + e0, m);
      if constexpr (EMA) ema_update8(q.ema + e0, pv, q.ema_omd);
    }
  }
}

int launch_adafactor(const AdafactorP& q, hipStream_t st) {
  const char* who = "adafactor (algorithm 3)";
  if (int rc = check_arenas(q, q.c, true, 0, who, "%s: n=%zu must be a multiple of 8")) return rc;
  ARG_CHECK((((uintptr_t)q.m32 | (uintptr_t)q.scal) & 15) == 0, "%s: buffers must be 16-byte aligned", who);
  if (q.n == 0 || q.n_tensors == 0) return 0;
  // one workgroup per tile (per chunk, per tensor) up to arena_grid's cap, the rest by grid stride
  const dim3 tiles = arena_grid((size_t)q.tiles * 2048), chunks = arena_grid((size_t)q.chunks * 2048), tensors = arena_grid((size_t)q.n_tensors * 2048);
  with_flags([&](auto f32g) {
    hipLaunchKernelGGL((adafactor_stats_kernel<decltype(f32g)::value>), tiles, dim3(256), 0, st, q);
    if (q.chunks > 0) hipLaunchKernelGGL(adafactor_reduce_kernel, chunks, dim3(256), 0, st, q);
    hipLaunchKernelGGL((adafactor_usq_kernel<decltype(f32g)::value>), tiles, dim3(256), 0, st, q);
  }, q.grad_f32 != nullptr);
  hipLaunchKernelGGL(adafactor_scalars_kernel, tensors, dim3(256), 0, st, q);
  with_flags([&](auto f32g, auto ema, auto beta1) {
    hipLaunchKernelGGL((adafactor_apply_kernel<decltype(f32g)::value, decltype(ema)::value, decltype(beta1)::value>), tiles, dim3(256), 0, st, q);
  }, q.grad_f32 != nullptr, q.ema != nullptr, q.m32 != nullptr);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}
