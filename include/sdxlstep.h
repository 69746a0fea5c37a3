/* libsdxlstep -- C ABI of the MI355X-native SDXL training step.
 *
 * Drop-in boundary for the hot path of DataCTE/SDXL-Training-Improvements (reference is 100 % Python and
 * has no native interface of its own; each entry point cites the reference call it replaces, paths under
 * /root/reference/src).  Plain pointers and sizes only -- no torch types.  All device pointers are raw HIP
 * device addresses (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as void*.
 *
 * Conventions: every function returns 0 on success, non-zero on failure (1 = bad argument, 2 = HIP error,
 * 3 = wrong state); sdxl_last_error() returns a thread-local message.  One handle per rank/GPU; a handle is not
 * thread-safe.  Calls are stream-ordered and do not synchronise unless stated.
 */
#ifndef SDXLSTEP_H
#define SDXLSTEP_H
#include <stddef.h>
#include <stdint.h>
/* Every entry point is marked SDXL_API: the library is built with -fvisibility=hidden, so these declarations (and the test hooks of
 * sdxlstep_diag.h) are the ONLY dynamic symbols libsdxlstep.so exports (tests/test_host_boundary.py checks `nm -D`). */
#ifndef SDXL_API
#define SDXL_API __attribute__((visibility("default")))
#endif
#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdxl_handle sdxl_handle;

/* UNet2DConditionModel config (the fields of diffusers' unet/config.json that determine the arithmetic;
 * loaded by the reference at models/sdxl.py:25-40). */
typedef struct {
  int in_channels, out_channels;       /* 4, 4; in_channels 4 .. 16 (extra input channels, below), out_channels 4 only */
  int block_out_channels[3];           /* 320, 640, 1280 */
  int layers_per_block;                /* 2 */
  int transformer_layers[3];           /* 0, 2, 10 */
  int head_dim;                        /* 64 (only value supported) */
  int cross_attention_dim;             /* 2048 */
  int norm_num_groups;                 /* 32 */
  int addition_time_embed_dim;         /* 256 */
  int pooled_dim;                      /* 1280 */
  float resnet_eps, tf_gn_eps, ln_eps; /* 1e-5, 1e-6, 1e-5 */
} sdxl_unet_config;

/* Loss configuration: config.yaml keys read by the path (training.method, training.prediction_type,
 * model.min_snr_gamma, model.use_ztsnr; ddpm_trainer.py:328,336, novelai_v3.py:106,117). */
typedef struct {
  int method;            /* 0 = ddpm (ddpm_trainer.py:280-405), 1 = flow_matching (flow_matching_trainer.py:267-356) */
  int prediction_type;   /* ddpm: 0 = epsilon, 1 = v_prediction */
  int use_min_snr;       /* model.min_snr_gamma is not None */
  float min_snr_gamma;
  int use_ztsnr;         /* clamp noisy latents to +-20000 */
  /* ---- appended: element loss (zero = squared error, as before).  With d = pred - target:
   *   0 l2        l(d) = d^2                          l'(d) = 2 d
   *   1 huber     l(d) = 2 c (sqrt(d^2 + c^2) - c)    l'(d) = 2 c d / sqrt(d^2 + c^2)   (-> d^2 for |d| << c, 2 c |d| for |d| >> c)
   *   2 smooth_l1 l(d) = 2 (sqrt(d^2 + c^2) - c)      l'(d) = 2 d / sqrt(d^2 + c^2)
   * The element loss is the low byte of loss_type; SDXL_LOSS_EXT may be or-ed in (below).  loss_type < 0, a low byte outside 0..2,
   * any other bit above the low byte, or 1 / 2 with neither huber_c > 0 here nor sdxl_batch.huber_c, is a bad argument (1). ---- */
  int   loss_type;
  float huber_c;         /* c of every sample; used when sdxl_batch.huber_c is NULL */
  /* ---- appended; read ONLY when loss_type & SDXL_LOSS_EXT (a caller without the flag may hold the 28-byte struct that ends above).
   * sdxl_forward_loss, sdxl_loss_fwd_bwd, sdxl_backward_* and sdxl_op_loss honour them.  With m the mask value of a latent pixel
   * (all 4 channels), M_b = sum_hw m, and s_b, w_b, l, the tag mean tm and the guard as without a mask, m joins the weight first,
   * (s_b w_b) m, so m = 1 leaves every bit as it is without a mask:
   *   mean        out[1] = sum_b sum_chw (s_b w_b m) l(d)     L_b = s_b w_b sum_chw m l(d) / (4 HW)
   *               loss = guard(out[1] / numel * tm)           dpred = gate grad_scale (s_b w_b m) l'(d) / numel
   *   masked_mean L_b = s_b w_b sum_chw m l(d) / (4 M_b), 0 when M_b = 0                out[1] = 4 HW sum_b L_b
   *               loss = guard(tm mean_b L_b)                 dpred = gate grad_scale (s_b w_b m) l'(d) / (B 4 M_b), 0 when M_b = 0
   * m = 0 gives an exact zero in dpred whatever d is; out[2..6] ignore the mask.  Fixed-order sums, no atomics: bitwise reproducible.
   * mask_norm outside 0..1 while a mask is set is a bad argument (1).
   * loss_mask is read AGAIN by the backward of the micro-step (like latents): outside graph mode the caller keeps it alive and
   * unchanged until that backward has been enqueued.  noise_in is read by the loss preparation only.  In graph mode both are staged
   * inside the plan. ---- */
  int          mask_norm;   /* 0 "mean", 1 "masked_mean" (above); read only with loss_mask */
  const float* loss_mask;   /* device, optional [B,H,W] fp32, m >= 0 per latent pixel, applied to all 4 channels; NULL = none */
  const float* noise_in;    /* device, optional [B,4,H,W] fp32: the noise (ddpm) / x0 (flow matching) the UNet INPUT is built from
                               (input perturbation), with the same separately rounded operations; the target, the MinSNR weight
                               and out[4], out[5] keep using sdxl_batch.noise; NULL = noise */
} sdxl_loss_config;
#define SDXL_LOSS_EXT 0x100   /* or-ed into loss_type: this sdxl_loss_config is the full current struct, the fields behind huber_c are read */

/* One sampler step, run by sdxl_unet_forward behind its forward (sdxl_batch.sampler): classifier-free guidance, the denoiser, the solver
 * step and the input of the next forward in one kernel that reads the plan's prediction buffer and writes the plan's input buffer, so a
 * sampling loop is one call per step and the latent never leaves the device.  With F_c / F_u the conditional / unconditional prediction:
 *   F       = F_c  (cfg 0)  |  F_u + guidance * (F_c - F_u)  (cfg 1)
 *   F       = guidance_rescale * (F * std(F_c) / std(F)) + (1 - guidance_rescale) * F      per sample over C.H.W; skipped when 0
 *   den     = a_skip * x + a_out * F
 *   x       = p * x + q * den                                                              the state, in place
 *   input   = bf16(clamp(a_in_next * x, +-clamp))                                          clamp <= 0: none; channels 4.. zero, or
 *                                                                                          bf16(input_cond) (sdxl_batch_cond)
 * fp32, every operation rounded on its own in this order (no FMA), the rescale sums in a fixed order: bitwise reproducible.  The scalars
 * are the caller's (sampler.py derives them for the trained ddpm denoiser, the reference's Karras scalings and flow matching).
 * The struct sdxl_sampler_step_ext below appends the terms of the second-order and stochastic solvers and of inpainting. */
typedef struct {
  float* x;                       /* [B,4,H,W] fp32 NCHW sampler state, in place */
  int    cfg;                     /* 1: the plan's batch is 2B = [cond; uncond] */
  int    init;                    /* 1: write the UNet input from x and return (no forward) */
  float  a_skip, a_out, p, q;     /* this step */
  float  a_in_next, clamp;        /* the input of the NEXT forward */
  float  guidance, guidance_rescale;
} sdxl_sampler_step;

/* The extended step: sdxl_sampler_step with the fields below appended behind guidance_rescale (`base` IS that struct, so the layout is
 * the appended one).  They are read ONLY when SDXL_SAMPLER_EXT is or-ed into base.init; the caller then passes a pointer to this struct
 * wherever a sdxl_sampler_step* is taken (sdxl_batch.sampler).  A caller without the flag may keep passing the struct that ends at
 * guidance_rescale: nothing behind it is read.  The solver line of the step widens to
 *   acc    = p * x + q * den
 *   acc    = acc + r * hist      (r != 0)        acc = acc + u * xsave   (u != 0)        acc = acc + s * noise   (s != 0)
 *   hist  <- den                 (save & 1, after hist was read)         xsave <- x before this step             (save & 2)
 *   y      = k_a * known  [+ k_b * knoise, k_b != 0] ;  acc = m * acc + (1 - m) * y                              (mask != NULL)
 *   x      = acc ;  input as above
 * fp32, every product and sum rounded on its own, left to right; guidance and guidance rescale combine with every term.  Every access
 * is elementwise per pixel, so one buffer may be read and overwritten by the same step (hist with r != 0 and save & 1).  A term whose
 * coefficient is 0 is not read at all.  With these one kernel is every solver of sampler.py: DPM++ 2M (hist = the previous denoised
 * estimate), Heun (hist / xsave = the first stage's estimate and state), ancestral Euler (noise), and the inpainting blend (the kept
 * region is carried as k_a * known + k_b * knoise on the noise level the new state lives at).  base.init with the flag writes the input
 * image only, as without it.  Bad arguments (1, before any launch): r, u or s != 0 or a save bit whose pointer is NULL, mask without
 * known, k_b != 0 without knoise, a non-finite r, u, s, k_a or k_b, save outside 0..3; and, with or without the flag, any bit of init
 * other than bit 0 and SDXL_SAMPLER_EXT. */
typedef struct {
  sdxl_sampler_step base;
  float*       hist;    /* [B,4,H,W] fp32: a denoised estimate of an earlier step */
  float*       xsave;   /* [B,4,H,W] fp32: a state of an earlier step */
  const float* noise;   /* [B,4,H,W] fp32: this step's standard normal draw */
  float        r, u, s; /* coefficients of hist, xsave, noise; a term is read iff its coefficient != 0 */
  int          save;    /* bit 0: hist <- den of this step; bit 1: xsave <- x before this step */
  const float* mask;    /* [B,H,W] fp32 in [0,1], 1 = generated, 0 = kept; NULL = no blend */
  const float* known;   /* [B,4,H,W] fp32: the latent to keep */
  const float* knoise;  /* [B,4,H,W] fp32: the noise the kept region is carried on */
  float        k_a, k_b;
} sdxl_sampler_step_ext;
#define SDXL_SAMPLER_EXT 0x100   /* or-ed into sdxl_sampler_step.init: the struct passed is a sdxl_sampler_step_ext */

/* One micro-batch, all device pointers.  RNG is the caller's: `noise` and `sigma_or_t` are inputs so that
 * fixtures are exact (reference draws them at ddpm_trainer.py:303-304 / flow_matching_trainer.py:298-306). */
typedef struct {
  int B, H, W;                 /* latent batch / height / width (pixels / 8) */
  int ctx_len;                 /* 77 */
  const float* latents;        /* [B,4,H,W] fp32 NCHW : batch["vae_latents"] (x for ddpm, x1 for flow matching) */
  const float* noise;          /* [B,4,H,W] fp32      : ddpm noise / flow-matching x0 */
  const float* sigma_or_t;     /* [B] fp32            : ddpm sigma = karras[timestep] ; flow matching t in (0,1) */
  const float* timestep;       /* [B] fp32            : value fed to the UNet time embedding (ddpm: index; fm: t) */
  const void* prompt_embeds;   /* [B,ctx_len,cross_attention_dim] bf16 : batch["prompt_embeds"] */
  const void* pooled;          /* [B,pooled_dim] bf16                 : batch["pooled_prompt_embeds"] */
  const float* time_ids;       /* [B,6] fp32                          : batch["time_ids"] */
  const float* tag_weights;    /* optional [B] fp32 (NULL = none)     : batch["tag_weights"] */
  /* ---- appended: per-sample weights in, per-sample losses out (NULL = none, as before).  sdxl_forward_loss, sdxl_loss_fwd_bwd,
   * sdxl_backward_* and sdxl_op_loss honour them; sdxl_unet_forward ignores them.
   * sample_weights and huber_c are read AGAIN by the backward of the micro-step (like latents / noise): outside graph mode the
   * caller keeps them alive and unchanged until that backward has been enqueued.  In graph mode they are staged inside the plan. ---- */
  const float* sample_weights; /* optional [B] fp32: s_b, multiplied into each sample's loss and gradient (with the MinSNR
                                  factor w_b: raw sum = sum_b sum_chw (s_b w_b) l(d)); s_b = 0 gives that sample an exact zero gradient */
  const float* huber_c;        /* optional [B] fp32: per-sample c_b > 0 (a schedule computed by the caller), loss_type 1 / 2 */
  float*       per_sample_loss;/* optional [B] fp32 OUT: L_b = s_b w_b mean_chw l(d), before the tag mean and the guard; written by
                                  sdxl_forward_loss / sdxl_op_loss phase 1, stream-ordered; fixed-order sums, bitwise reproducible */
  /* ---- appended: a sampler step (NULL = none, as before).  A HOST pointer, read during the call.  Only sdxl_unet_forward honours it;
   * every other entry point ignores it. ---- */
  const sdxl_sampler_step* sampler;
} sdxl_batch;

/* The batch with conditioning gradients: sdxl_batch with two output pointers appended behind `sampler` (`base` IS that struct, so the
 * layout is the one of a struct with the fields appended).  Passed as a sdxl_batch* with SDXL_BATCH_EXT or-ed into base.ctx_len; nothing
 * behind `sampler` is read without the flag, so a caller without it may keep passing the struct that ends at `sampler`
 * (sdxl_unet_forward) or at `per_sample_loss` (every other entry point).
 * sdxl_forward_loss, sdxl_loss_fwd_bwd and sdxl_unet_forward (without `sampler`) read the two pointers and remember the request for
 * that micro-step; the backward of that micro-step writes them, stream-ordered, by the time its last-executed segment returns
 * (sdxl_backward_segment(num_segments - 1), the segment that holds the K | V projection executed last; sdxl_backward_all;
 * sdxl_loss_fwd_bwd; sdxl_unet_backward).  The value is the gradient of grad_scale x loss with respect to prompt_embeds / pooled as the
 * UNet read them (bf16), in fp32: the same scale and gradient gate as that micro-step's parameter gradients (a closed gate gives exact
 * zeros; sdxl_unet_backward: of <dpred, pred>, no scale, no gate), summed in fp32 in a fixed order, bitwise reproducible.  Always
 * OVERWRITTEN, never accumulated: first_micro does not matter.  Either pointer alone is valid; either together with `sampler` is a bad
 * argument (1, before any launch).  The caller keeps the buffers alive until that backward has been enqueued.  In graph mode which of
 * the two is present is part of the capture key and the values leave through the plan's buffers by a copy behind the replay, so the
 * buffers may move between steps.  Exchanging the gradients of a text encoder across ranks is the caller's (DDP on its own modules). */
typedef struct {
  sdxl_batch base;
  float* d_prompt_embeds;      /* optional OUT [B,ctx_len,cross_attention_dim] fp32; NULL = none */
  float* d_pooled;             /* optional OUT [B,pooled_dim] fp32; NULL = none */
} sdxl_batch_ext;
#define SDXL_BATCH_EXT 0x10000   /* or-ed into sdxl_batch.ctx_len: the struct passed is a sdxl_batch_ext */

/* Extra input channels: a UNet whose conv_in reads more than the 4 latent channels (sdxl_unet_config.in_channels 5 .. 16: the inpainting
 * UNet has 9 = latents | mask | masked-image latents, the InstructPix2Pix one 8 = latents | source-image latents).  Channels 0..3 of the
 * UNet input stay what the loss preparation / the sampler step build from the latents; channels 4 .. in_channels - 1 are the caller's
 * `input_cond`, rounded to bf16 (nearest even) and concatenated behind them in the given order (diffusers' channel order is the caller's).
 * The batch that carries it is sdxl_batch_ext with the fields below appended (`base` IS that struct), passed as a sdxl_batch* with
 * SDXL_BATCH_COND or-ed into base.base.ctx_len: the flag says that the struct passed is this one, so its d_prompt_embeds / d_pooled are
 * read as well (they may be NULL) and SDXL_BATCH_EXT need not be set beside it.  Nothing behind `sampler` is read without a flag.
 * A pixel of the plan's input buffer is stored Cs = 8 channels wide for in_channels <= 8, else 16 ([B*H*W][Cs] bf16, the channels past
 * in_channels zero), and conv_in as [cout][9][Cs] with zero pad channels; callers only ever see [cout, in_channels, 3, 3]
 * (sdxl_load_weight, sdxl_export_weight, sdxl_export_grad, sdxl_param_info).  input_cond is read by the loss preparation / the sampler
 * step only: the backward never reads it (its gradient is channels 4 .. of the input gradient, on request: sdxl_batch_din).  In graph
 * mode it is staged inside the plan like the latents, and whether it is present is part of the capture key.
 * sdxl_forward_loss, sdxl_loss_fwd_bwd, sdxl_op_loss phase 0 and a sampler step (sdxl_unet_forward with `sampler`, init included) read
 * it; with cfg the plan's batch is 2B and row b of input_cond goes to the conditional half, row b + B to the unconditional one.
 * sdxl_unet_forward without `sampler` ignores it: the caller's sample already carries every channel ([B*H*W][Cs]).
 * cond_channels: 0 = in_channels - 4 of the handle; any other value must equal it.  sdxl_op_loss has no handle: there cond_channels IS
 * the number of extra channels (0 .. 12; unet_in is then [B*H*W][Cs] for in_channels = 4 + cond_channels).
 * Bad arguments (1, before any launch, the message names input_cond): in_channels > 4 (sdxl_op_loss: cond_channels > 0) without a
 * non-NULL input_cond on one of the readers above; in_channels == 4 with a non-NULL input_cond; a cond_channels that does not match. */
typedef struct {
  sdxl_batch_ext base;
  const float* input_cond;     /* device [Bplan, in_channels - 4, H, W] fp32 NCHW; NULL = none */
  int cond_channels;           /* 0, or in_channels - 4 (above) */
} sdxl_batch_cond;
#define SDXL_BATCH_COND 0x20000  /* or-ed into sdxl_batch.ctx_len: the struct passed is a sdxl_batch_cond */

/* Additional skip residuals (diffusers' down_block_additional_residuals / mid_block_additional_residual: how a ControlNet attaches to the
 * UNet), with gradients.  The batch that carries them is sdxl_batch_cond with one host pointer appended (`base` IS that struct), passed as
 * a sdxl_batch* with SDXL_BATCH_RES or-ed into base.base.base.ctx_len: the flag says that the struct passed is this one, so every field of
 * sdxl_batch_ext and sdxl_batch_cond is read as well and their flags need not be set beside it.  Nothing behind `sampler` is read without a flag.
 * Forward.  The UNet saves n = 1 + 3 * layers_per_block + 2 skips (SDXL-base: 9) in forward order: conv_in's output, then per down block
 * each layer's output and then its downsampler's; the up path joins them, last first, to its hidden state by a channel concat.  For
 * down[i] the skip half of its concat becomes bf16_rn(float(skip) + float(r)): one fp32 add, one round to nearest even; where r == 0 the
 * skip's bits pass unchanged.  `mid` is added the same way to the hidden half of the first concat (the mid block's output).  The saved skip
 * itself is NOT modified: the down path, its weight gradients and the backward read the plain skip, as diffusers adds the residuals
 * after the whole down path has run.  Scaling the residuals (conditioning_scale) is the caller's.  The residuals are read by the forward
 * only; the backward never reads them.  sdxl_forward_loss, sdxl_loss_fwd_bwd and sdxl_unet_forward (with and without `sampler`; init runs no
 * forward and reads none) honour the struct; with cfg the plan's batch is 2B and row b + B feeds the unconditional half, as for input_cond.
 * Gradients.  A given d_down[i] / d_mid is written by the backward of that micro-step: float(g) of the concat's bf16 output gradient for
 * that column range, transposed to NCHW.  The values follow that micro-step's parameter gradients' grad_scale and gradient gate (a
 * closed gate stores exact zeros; sdxl_unet_backward: of <dpred, pred>, no scale, no gate); always OVERWRITTEN, never accumulated.  A d_*
 * pointer may be given without the matching residual (the gradient at r = 0).  The writes go straight from the backward's kernels into the
 * caller's buffers (no plan copies), stream-ordered, complete once the last-executed backward segment has been enqueued; the caller keeps
 * the buffers alive until then.  d_* together with `sampler` is a bad argument.
 * Graph mode.  A call that carries a sdxl_residuals launches kernel by kernel even in graph mode (sdxl_set_graph_mode), as the sampler
 * path does -- its forward and the backward of that micro-step: the residuals (SDXL-base, B = 4, 128 x 128, fp32: about 430 MB) would
 * otherwise have to be staged at fixed addresses inside the plan.
 * Bad arguments (1, before any launch, the message names `residuals` and the index): n other than the handle's number of skips, a dtype
 * outside 0..1, a pointer that is not 16-byte aligned, d_* with `sampler`.  Without the flag or with residuals == NULL the launch
 * sequence, every workspace offset and every bit are those of a call without this struct. */
typedef struct {
  int n;                    /* number of skips of the handle: 1 + 3 * layers_per_block + 2 (SDXL-base: 9); any other value = bad argument */
  int dtype;                /* of down[] / mid: 0 = fp32, 1 = bf16 */
  const void* const* down;  /* HOST array [n] of device pointers, forward (diffusers) order; down[i] is [Bplan, C_i, h_i, w_i] NCHW contiguous;
                               an entry may be NULL (no residual at that skip); down == NULL = none */
  const void* mid;          /* device [Bplan, C_last, H/4, W/4] NCHW; NULL = none */
  float* const* d_down;     /* HOST array [n] of device fp32 OUT pointers, same shapes; entries may be NULL; NULL = none */
  float* d_mid;             /* device fp32 OUT; NULL = none */
} sdxl_residuals;
typedef struct {
  sdxl_batch_cond base;
  const sdxl_residuals* residuals;   /* HOST pointer, read during the call; NULL = none */
} sdxl_batch_res;
#define SDXL_BATCH_RES 0x40000   /* or-ed into sdxl_batch.ctx_len: the struct passed is a sdxl_batch_res */

/* Input gradient: the gradient with respect to the UNet input, the one tensor input that had none (prompt_embeds / pooled: sdxl_batch_ext;
 * the additional residuals: sdxl_residuals).  The batch that asks for it is sdxl_batch_res with one output pointer appended (`base` IS that
 * struct), passed as a sdxl_batch* with SDXL_BATCH_DIN or-ed into base.base.base.base.ctx_len: the flag says that the struct passed is this
 * one, so every field of sdxl_batch_ext, sdxl_batch_cond and sdxl_batch_res is read as well and their flags need not be set beside it.
 * Nothing behind `sampler` is read without a flag.
 * sdxl_forward_loss, sdxl_loss_fwd_bwd and sdxl_unet_forward (without `sampler`) read the pointer and remember the request for that
 * micro-step; the backward of that micro-step writes the buffer: sdxl_backward_segment of the segment that holds conv_in (executed last),
 * sdxl_backward_all, sdxl_loss_fwd_bwd, sdxl_unet_backward.  The write goes straight from conv_in's backward (csrc/input_dgrad.hip) into the
 * caller's buffer (nothing is allocated in the plan), stream-ordered, complete once the last-executed segment has been enqueued; the
 * caller keeps the buffer alive until then.
 * The value is the gradient of grad_scale x loss with respect to the UNet input as the UNet read it -- the bf16 [B*H*W][Cs] buffer the
 * loss preparation wrote, or the caller's sample (sdxl_unet_forward) -- for channels 0 .. in_channels - 1 (the four latent channels, then
 * the input_cond channels), in fp32, transposed to NCHW: dx[b][c][y][x] = sum over the nine taps and conv_in's output channels o of
 * dy[b][y + 1 - ky][x + 1 - kx][o] * w[o][3 ky + kx][c], pixels outside the image contributing nothing, fp32 sums in a fixed order that
 * depends on the shape alone (no atomics: bitwise reproducible).  The same scale and gradient gate as that micro-step's parameter
 * gradients (a closed gate stores exact zeros; sdxl_unet_backward: of <dpred, pred>, no scale, no gate).  Always OVERWRITTEN, never
 * accumulated: first_micro does not matter.  The chain rule through the loss preparation (x_t from latents and noise, a_in, the bf16
 * rounding) is the caller's: INTEGRATION.md section 1 "Input gradients" has the formulas per method.
 * The request changes no other bit (loss, parameter, conditioning and residual gradients) and combines with d_prompt_embeds, d_pooled,
 * input_cond, residuals, d_down / d_mid and any sdxl_grad_select, an all-frozen UNet included.
 * Graph mode.  The backward of a micro-step that asked for d_input launches kernel by kernel (the caller's buffer is written where it
 * lies), as one that carried residuals does; its forward is the unflagged call's.
 * Bad arguments (1, before any launch, the message names d_input): d_input together with `sampler`, a pointer that is not 16-byte
 * aligned, a conv_in whose output width is not a multiple of 32 (SDXL-base: 320).  Without the flag or with d_input == NULL the launch
 * sequence, every workspace offset and every bit are those of a call without this struct. */
typedef struct {
  sdxl_batch_res base;
  float* d_input;   /* optional OUT, device fp32 [B, in_channels, H, W] NCHW contiguous, 16-byte aligned; NULL = none */
} sdxl_batch_din;
#define SDXL_BATCH_DIN 0x80000   /* or-ed into sdxl_batch.ctx_len: the struct passed is a sdxl_batch_din */

SDXL_API const char* sdxl_last_error(void);
SDXL_API int sdxl_version(void);

/* ---- lifetime ---------------------------------------------------------------------------------------------- */
SDXL_API int sdxl_default_config(sdxl_unet_config* cfg);                 /* SDXL-base-1.0 */
SDXL_API int sdxl_create(const sdxl_unet_config* cfg, int device, sdxl_handle** out);
SDXL_API int sdxl_destroy(sdxl_handle* h);

/* ---- parameters (replaces model.unet.parameters()/state_dict(), models/sdxl.py:237-240) ---------------------- */
/* bytes of the packed bf16 weight arena and the fp32 gradient arena */
SDXL_API int sdxl_param_bytes(sdxl_handle* h, size_t* weight_bytes, size_t* grad_bytes);
/* bind caller-allocated arenas (NULL = library allocates with hipMalloc) */
SDXL_API int sdxl_bind_params(sdxl_handle* h, void* weights_dev, void* grads_dev);
SDXL_API int sdxl_num_params(sdxl_handle* h);                            /* diffusers state-dict tensors */
SDXL_API int sdxl_param_info(sdxl_handle* h, int i, char* name, int name_cap, int* ndim, long shape[4]);
/* the contiguous element range tensor i occupies in the packed weight / gradient arenas (per-tensor optimizer
 * bookkeeping such as AdamWBF16's lazy decay) */
SDXL_API int sdxl_param_range(sdxl_handle* h, int i, size_t* elem_off, size_t* elems);
/* copy one tensor in PyTorch layout ([out,in] / [cout,cin,kh,kw]) from device memory into the packed arena
 * (dtype: 0 = fp32, 1 = bf16).  Caller keeps ownership of src. */
SDXL_API int sdxl_load_weight(sdxl_handle* h, const char* name, const void* src_dev, int dtype, void* stream);
/* ---- LoRA by merge and project: dtype SDXL_DTYPE_LORA of sdxl_load_weight / sdxl_export_grad (no entry point of its own) ----
 * For a targeted weight W [out][in] with adapters A [rank][in], B [out][rank] and s = scale (alpha / rank):
 *   sdxl_load_weight(h, NULL, &op, SDXL_DTYPE_LORA, stream)   merge:   W = bf16_rn(W0 + s B A), written into the bound weight arena;
 *   sdxl_export_grad(h, NULL, &op, SDXL_DTYPE_LORA, stream)   project: dA = s B^T dW, dB = s dW A^T from the bound fp32 gradient arena.
 * With this dtype the pointer argument is a HOST pointer to the struct below, read during the call, and `name` must be NULL.  The
 * forward and the backward run unchanged between the two: dA and dB are exactly the LoRA gradients at the merged weight.
 * merge: acc <- acc + B[o][k] A[k][i] for k = 0 .. rank - 1, every product and every sum rounded on its own in fp32 (no FMA), then
 * t = s acc, W = bf16_rn(W0 + t) (round to nearest even), and W = W0 where t == 0: scale 0 or B = 0 give back W0 bit for bit.
 * project: fp32, no atomics, OVERWRITES its outputs; the summation order is fixed by (out, in, rank) alone, so results are bitwise
 * reproducible and a target's bits do not depend on the other targets of the call.  One launch merges, two launches project, whatever n.
 * A target is a 2-D tensor in plain row layout, listed once: attention projections, proj_in / proj_out, ff.net.2, time_emb_proj, the
 * embedding linears.  Bad arguments (1, before any launch, the message names the tensor): rank outside 1 .. 128, in % 8 != 0, a
 * convolution or ff.net.0.proj (interleaved rows), a tensor listed twice, a non-NULL name, a NULL or misaligned (16 bytes) pointer.
 * The handle keeps the device table of the last (target list, rank). */
#define SDXL_DTYPE_LORA 2
typedef struct {
  int n; const int* param;   /* host [n]: state-dict indices (sdxl_param_info order) */
  int rank; float scale;
  const void* adapters;      /* device bf16: per target A [rank][in] then B [out][rank], each padded to 8 elements */
  const void* base;          /* device bf16: the W0 copies, packed [out][in] in target order (load only) */
  float* adapter_grads;      /* device fp32, laid out like adapters (export only) */
} sdxl_lora_op;
/* ---- LoRA on the packed layouts: dtype SDXL_DTYPE_LORA_LAYOUTS of the same two calls, the same host struct ----
 * SDXL_DTYPE_LORA keeps refusing what it refuses.  With this dtype a target may be ANY 2-D or 4-D weight: out = shape[0], in = the product
 * of the other dimensions, A [rank][in] and B [out][rank] are indexed like the state-dict (PyTorch) tensor flattened to [out][in] -- so
 * exported adapters are views -- and the kernels find source element (o, i) where the arena keeps it:
 *   plain 2-D [out][in], 1x1 convolution [out][in][1][1]     o in + i
 *   ff.net.0.proj [2 C4][in] (GEGLU, groups of G)             row (c / G) 2G + half G + c % G, column i;  half = o / C4, c = o % C4
 *   3x3 convolution [cout][cin][3][3], i = c 9 + tap          (o 9 + tap) cin + c
 * merge and project are SDXL_DTYPE_LORA's, element for element: the merge arithmetic depends on (o, i) alone; the projection's summation
 * order is fixed by the target's shape and kind alone.  Still one launch to merge and two to project; a table without a packed target runs
 * SDXL_DTYPE_LORA's kernels.  `base` is the packed copy of each target's sdxl_param_range elements, in target order (out * in of them for
 * every accepted target).  conv_out: its 4 source rows are the first 4 of 8 native rows; the other 4 lie outside its sdxl_param_range and
 * are neither read nor written.  Nothing outside the targets' ranges is written.
 * Bad arguments (1, before any launch, the message names the tensor): everything SDXL_DTYPE_LORA refuses for other reasons (rank, a tensor
 * listed twice, a non-NULL name, a NULL or misaligned pointer, an index out of range), a bias or a norm parameter, in % 8 != 0, a 3x3
 * convolution whose input channels are padded in the arena -- together the last two refuse exactly conv_in.  sdxl_grad_select.lora keeps
 * SDXL_DTYPE_LORA's rule.  The cached device table is keyed by the dtype too. */
#define SDXL_DTYPE_LORA_LAYOUTS 4
/* ---- LoHa (LyCORIS Hadamard product) by merge and project: dtype SDXL_DTYPE_LOHA of the same two calls, the same host struct ----
 * For a targeted weight W [out][in] with the factors A1, A2 [rank][in], B1, B2 [out][rank] and s = scale:
 *   dW = s (B1 A1) .* (B2 A2)    (.* elementwise: effective rank up to rank^2 at the storage of rank 2 rank)
 * `adapters` holds per target A1 [rank][in], B1 [out][rank], A2 [rank][in], B2 [out][rank] in that order, bf16, each padded to 8 elements;
 * `adapter_grads` is fp32 and laid out the same way; `base` is SDXL_DTYPE_LORA_LAYOUTS' packed W0 copies.  The targets are everything
 * SDXL_DTYPE_LORA_LAYOUTS accepts, with its maps: the factors are indexed like the state-dict tensor flattened to [out][prod(rest)], and only
 * the rows < out of a target are read or written (conv_out's 4 other native rows are not touched).
 * merge (one launch): p1 <- p1 + B1[o][k] A1[k][i] for k = 0 .. rank - 1, every product and every sum rounded on its own in fp32 (no FMA);
 * p2 likewise from B2, A2; h = p1 p2, t = s h, W = bf16_rn(W0 + t) (round to nearest even), and W = W0 where t == 0: scale 0, B1 = 0 or
 * B2 = 0 give back W0 bit for bit.
 * project (two launches, from G = dW in the bound fp32 gradient arena, with P1 = B1 A1 and P2 = B2 A2 recomputed in fp32 on the fly):
 *   dB1[o][k] = s sum_i (G[o][i] P2[o][i]) A1[k][i]      dA1[k][i] = s sum_o B1[o][k] (G[o][i] P2[o][i])
 *   dB2[o][k] = s sum_i (G[o][i] P1[o][i]) A2[k][i]      dA2[k][i] = s sum_o B2[o][k] (G[o][i] P1[o][i])
 * one launch writes dB1 | dB2, the other dA1 | dA2; each reads G once.  No out x in scratch, no atomics, the outputs are OVERWRITTEN; the
 * summation order is fixed by (out, in, rank, kind) alone, so results are bitwise reproducible and a target's bits do not depend on the
 * other targets of the call.
 * Bad arguments (1, before any launch, the message names the tensor or `rank`): everything SDXL_DTYPE_LORA_LAYOUTS refuses, and a rank
 * outside 1 .. 64.  sdxl_grad_select.lora keeps SDXL_DTYPE_LORA's rule: adapter gradients written by the backward itself are LoRA's only.
 * The cached device table is keyed by the dtype too. */
#define SDXL_DTYPE_LOHA 5
/* ---- LoKr (LyCORIS Kronecker product) by merge and project: dtype SDXL_DTYPE_LOKR of the same two calls, the host struct sdxl_lokr_op ----
 * For a targeted weight with state-dict shape [out][cin] or [out][cin][kh][kw], flattened to [out][in], in = cin kh kw:
 *   (out_l, out_k) = fact(out, factor), (in_m, in_n) = fact(cin, factor), n2 = in_n kh kw    (fact: LyCORIS' factorization, smaller first:
 *   factor > 0 dividing the dimension gives (factor, dimension / factor) sorted; otherwise the divisor pair (m, n), m <= n, reached from
 *   (1, dimension) by stepping m to the next divisor while m + n does not grow and m stays <= factor, factor -1 meaning no cap)
 *   dW[a out_k + c][b n2 + j] = s C[a][b] W2[c][j]      = s kron(C, W2); for a 3x3 convolution j = d 9 + tap, channel = b in_n + d
 * C [out_l][in_m] (lokr_w1) is always a full matrix.  W2 [out_k][n2] is stored as it is (a FULL target, lokr_w2) or as W2 = B A with
 * B [out_k][rank] (lokr_w2_a) and A [rank][n2] (lokr_w2_b) (a FACTORED target).  A target is full when sdxl_lokr_op.full is 1 or when
 * 2 rank >= max(out_k, in_n); a full target uses s = 1 (and s = 0 when op.scale is 0: the restoring merge), a factored one s = op.scale.
 * `adapters` holds per target C, then W2 or B, A, in that order, bf16, each factor padded to 8 elements; `adapter_grads` is fp32 and laid
 * out the same way; `base` is SDXL_DTYPE_LORA_LAYOUTS' packed W0 copies.  The targets are everything SDXL_DTYPE_LORA_LAYOUTS accepts, with
 * its maps; only the rows < out of a target are read or written.
 * merge (one launch): factored q <- q + B[c][k] A[k][j] for k = 0 .. rank - 1, every product and every sum rounded on its own in fp32 (no
 * FMA), full q = (float)W2[c][j]; h = C[a][b] q, t = s h, W = bf16_rn(W0 + t), and W = W0 bit for bit where t == 0.
 * project (two launches, from G = dW in the bound fp32 gradient arena, read ONCE):
 *   dC[a][b] = s sum_{c,j} G[a out_k + c][b n2 + j] W2[c][j]       dW2[c][j] = s sum_{a,b} C[a][b] G[a out_k + c][b n2 + j]
 *   factored: dB = dW2 A^T, dA = B^T dW2
 * No out x in scratch, no atomics, the outputs are OVERWRITTEN; every summation order is fixed by (out, in, factor, rank, form, kind)
 * alone, so results are bitwise reproducible and a target's bits do not depend on the other targets of the call.
 * `scratch` is caller-owned device memory, 16-byte aligned, of at least the sum over the targets of
 *   SDXL_LOKR_PAD(tiles out_l in_m) + (full ? 0 : SDXL_LOKR_PAD(out_k n2)) floats,  tiles = ceil(out_k n2 / SDXL_LOKR_TILE)
 * (the projection's partial sums and a factored target's dW2); its previous contents do not matter.  The merge does not use it.
 * Bad arguments (1, before any launch, the message names the tensor or the field): everything SDXL_DTYPE_LORA_LAYOUTS refuses, a rank
 * outside 1 .. 128, factor == 0 or < -1, full outside 0 / 1, a second factor (or, factored, a B or an A) of 2^31 elements or more, and for the projection a NULL,
 * misaligned or too-small `scratch`.
 * sdxl_grad_select.lora keeps SDXL_DTYPE_LORA's rule.  The cached device table is keyed by (target list, rank, dtype, factor, full); the
 * scale is read per call, so a restoring merge (scale 0) between two merges rebuilds nothing. */
#define SDXL_DTYPE_LOKR 6
#define SDXL_LOKR_TILE 1024                          /* elements of W2 one workgroup of the projection owns */
#define SDXL_LOKR_PAD(n) (((size_t)(n) + 3) / 4 * 4) /* scratch regions start on 16 bytes */
typedef struct {
  sdxl_lora_op op;           /* n, param, rank, scale (alpha / rank, used by the factored targets), adapters, base, adapter_grads */
  int factor;                /* -1 or >= 1 */
  int full;                  /* 0: the rule above per target; 1: every target stores W2 in full */
  float* scratch;            /* device fp32, 16-byte aligned (export only) */
  size_t scratch_floats;
} sdxl_lokr_op;
/* ---- DoRA (a trained magnitude per output row on the merged LoRA weight) by merge and project: dtype SDXL_DTYPE_DORA of the same two calls,
 * the host struct sdxl_dora_op ----
 * For a targeted weight [out][in] (the targets and maps of SDXL_DTYPE_LORA_LAYOUTS) with A [rank][in], B [out][rank], s = op.scale and a
 * trained vector mu [out]:
 *   acc = sum_k B[o][k] A[k][i]      LoRA's chain: every product and sum rounded on its own in fp32, no FMA
 *   t = s acc;  v = (float)W0[o][i] + t
 *   n_o  = sqrt(sum_i v^2)           the fp32 row norm of V = W0 + s B A (a convolution: per out-channel over cin kh kw)
 *   n0_o = n_o at t == 0             the row norm of W0, by the same kernel (mode 1), frozen
 *   q_o = n0_o / n_o (1 when n_o == 0);  c_o = (1 + (float)mu_o) q_o
 *   W[o][i] = bf16_rn(c_o v), and W[o][i] = W0[o][i] bit for bit where t == 0 and c_o == 1
 * that is DoRA with the magnitude m_o = n0_o (1 + mu_o): mu = 0 and B = 0 give back W0's bits.  A row with n0_o == 0 stays 0.
 * `adapters` holds per target A, B, mu in that order, bf16, each padded to 8 elements; `adapter_grads` is fp32 and laid out the same way; pad
 * elements are neither read nor written.  `norm0` and `norm` are caller-owned device fp32 buffers, 16-byte aligned: one float per target row
 * (indexed like the state-dict rows) in target order, each target padded to 4 floats.
 * sdxl_load_weight, by `mode`: 0 merge (two launches: norm, then W; reads norm0), 1 init (one launch: writes norm0 only; A, B, mu, scale are
 * not read), 2 restore (one launch: W0's bits back; scale is ignored).
 * sdxl_export_grad (three launches; `mode` is not read), from G = dW in the bound fp32 gradient arena with n_o held constant (the value the
 * last merge wrote into `norm`), v recomputed as in the merge:
 *   dmu_o = q_o sum_i G[o][i] v[o][i]      dB[o][k] = c_o (s sum_i G[o][i] A[k][i])      dA[k][i] = s sum_o (c_o B[o][k]) G[o][i]
 * No out x in scratch, no atomics, the outputs are OVERWRITTEN; every summation order is fixed by (out, in, rank, kind) alone.
 * Bad arguments (1, before any launch, the message names the tensor or the field): everything SDXL_DTYPE_LORA_LAYOUTS refuses, a rank outside
 * 1 .. 128, a mode outside 0 .. 2, a NULL or misaligned norm0 or norm.  Both calls need `base`.
 * sdxl_grad_select.lora keeps SDXL_DTYPE_LORA's rule.  The cached device table is keyed by the dtype too. */
#define SDXL_DTYPE_DORA 8
typedef struct {
  sdxl_lora_op op;           /* n, param, rank, scale (alpha / rank), adapters, base, adapter_grads */
  int mode;                  /* sdxl_load_weight: 0 merge, 1 init, 2 restore */
  float* norm0;              /* device fp32, 16-byte aligned */
  float* norm;
} sdxl_dora_op;
/* ---- gradient selection: dtype SDXL_DTYPE_GRAD_SELECT of sdxl_export_grad (no entry point of its own) ----
 *   sdxl_export_grad(h, NULL, &sel, SDXL_DTYPE_GRAD_SELECT, stream)
 * tells the backward which state-dict tensors are trained.  `sel` is a HOST pointer, read during the call; `name` must be NULL; a NULL
 * struct pointer = every tensor trainable (the state after sdxl_create).  Nothing is launched; the selection holds for every plan of the
 * handle until it is changed, and a change drops the captured graphs.
 * What is skipped: an op's parameter-gradient work -- the weight-gradient GEMM / convolution launch with its bias column sums, the
 * zero-row memsets in front of it, the reduce of a norm's dgamma | dbeta -- if and only if EVERY tensor that maps into the op's native
 * parameters is frozen.  State-dict tensors do not map 1:1 to ops: attn1.to_q | to_k | to_v of a block are one fused weight, attn2.to_k |
 * to_v of ALL blocks of one width are one grouped weight, all time_emb_proj (weight and bias) are one op, a weight and its bias (a norm's
 * weight and bias) are one op.  An op with at least one trainable tensor runs exactly as without a selection, and the frozen tensors that
 * share it get their true gradient as a by-product.  A skipped op writes NOTHING into the fp32 gradient arena or the bf16 emit arena
 * (sdxl_set_grad_emit): not a zero, not a partial -- its ranges keep what they held (its bias / norm vectors the zeros of
 * sdxl_zero_grads).  The input-gradient side of the backward is untouched: every dgrad, the attention backward, the time-embedding
 * column sums and the conditioning gradients (sdxl_batch_ext) run and give the same bits under any selection.  Of the weight gradients
 * that still run, the linear ones that share a grouped launch may change their fp32 summation order with the group's composition.
 * sdxl_zero_grads, segment ranges and join modes keep their meaning; sdxl_grad_sumsq sums the whole arena, stale values of frozen
 * ranges included -- a caller with a selection takes its norm over its own tensors (sdxl_sumsq on their ranges).
 * `lora` (NULL = none): adapters whose gradients the backward writes itself (csrc/lora_grad.hip).  A linear op that holds targets launches,
 * in place of its weight-gradient launch (same stream, same place in the order), dA (+)= s (dY B)^T X and dB (+)= s dY^T (X A^T) for each of
 * its targets, from the op's input X and output gradient dY: the LoRA gradients at the merged weight, without dW.  The intermediates X A^T
 * and dY B are rounded once to bf16; fp32 accumulation, no atomics, the rows split across workgroups in chunks fixed by their number
 * alone and the partial sums added in ascending order: bits are reproducible and a target's bits do not depend on the other targets.
 * first_micro != 0 overwrites adapter_grads, otherwise the micro-step is added to them (the fp32 weight-gradient rule); `base` is not read.
 * Rows of the op's weight that belong to no target get nothing, so EVERY tensor of an op that holds a target must be flagged 0 (its bias
 * too).  The struct's rank, scale and the addresses of `adapters` / `adapter_grads` are taken at the call: they must stay valid until the
 * selection changes, and the call is repeated when one of them changes.  The plans reserve the kernels' scratch, so a change of `lora`
 * DROPS EVERY PLAN of the handle (it waits for the device first): call sdxl_plan and sdxl_bind_workspace again.
 * Bad arguments (1, before anything changes, the message names the cause): n != sdxl_num_params(h), a flag other than 0 / 1, a non-NULL
 * name; a selection that differs from the current one between sdxl_forward_loss and the end of its backward (a forward that is never
 * differentiated, an evaluation, keeps that wait open; it ends with the next backward, with a plain sdxl_unet_forward, or with a call of
 * sdxl_plan -- also for the shape that is current -- which is how a caller says that no backward will follow); with `lora`
 * everything SDXL_DTYPE_LORA refuses, with its messages, a trainable tensor in an op that holds a target, and `lora` together with a
 * bf16 emit arena (sdxl_set_grad_emit refuses the other order). */
#define SDXL_DTYPE_GRAD_SELECT 3
typedef struct {
  int n; const unsigned char* trainable;   /* host [n], n == sdxl_num_params(h): 1 = the backward produces this tensor's gradient, 0 = frozen */
  const sdxl_lora_op* lora;                /* NULL, or the adapters whose gradients the backward writes itself */
} sdxl_grad_select;
SDXL_API int sdxl_export_weight(sdxl_handle* h, const char* name, void* dst_dev, int dtype, void* stream);
SDXL_API int sdxl_export_grad(sdxl_handle* h, const char* name, void* dst_dev, int dtype, void* stream);

/* ---- plan: static execution plan for one bucket shape (B, H, W) ------------------------------------------------ */
SDXL_API int sdxl_plan(sdxl_handle* h, int B, int H, int W, int ctx_len, size_t* workspace_bytes);
SDXL_API int sdxl_bind_workspace(sdxl_handle* h, void* ws_dev, size_t bytes);   /* NULL = library allocates */

/* ---- the step (replaces compute_loss()/training_step() + loss.backward()) -------------------------------------- */
/* start of an accumulation cycle: zeroes the bias / norm gradient vectors (accumulated with atomics); the weight-matrix
 * gradients are NOT touched -- the first micro-step (first_micro != 0) overwrites them.  A cycle must therefore start
 * with first_micro = 1. */
SDXL_API int sdxl_zero_grads(sdxl_handle* h, void* stream);
/* loss preparation + UNet forward + loss.  Leaves loss/metrics on device. */
SDXL_API int sdxl_forward_loss(sdxl_handle* h, const sdxl_loss_config* lc, const sdxl_batch* b, void* stream);
/* backward, split into segments (reverse execution order) so the caller can overlap gradient all-reduce of a
 * finished segment with the remaining backward (replaces DDP hooks, core/distributed.py:153-157).
 * first_micro != 0: gradients are overwritten (first micro-step after sdxl_zero_grads); else accumulated. */
SDXL_API int sdxl_num_segments(sdxl_handle* h);
SDXL_API int sdxl_segment_range(sdxl_handle* h, int seg, size_t* grad_elem_offset, size_t* grad_elems);
SDXL_API int sdxl_backward_segment(sdxl_handle* h, int seg, float grad_scale, int first_micro, void* stream);
/* By default the stream waits, at the end of every segment, for that segment's weight gradients (they run on an internal
 * side stream), so a caller can hand the segment to the gradient exchange.  A caller that consumes gradients only after
 * the whole backward (single GPU, or accumulation micro-steps without exchange) may set last_only = 1: the wait then
 * happens once, in the last segment (sdxl_loss_fwd_bwd always ends with it).
 * mode 2: as 1, and at every segment end the SIDE stream (sdxl_side_stream) waits for the caller's stream instead: a
 * caller that enqueues the segment's cast (sdxl_grads_to_bf16) and collective on the side stream gets the exchange
 * started without the caller's stream -- the critical path of the backward -- ever waiting or running the casts. */
SDXL_API int sdxl_set_join_mode(sdxl_handle* h, int mode);
/* the engine's side stream (hipStream_t; NULL when the serialized measurement mode is on) */
SDXL_API int sdxl_side_stream(sdxl_handle* h, void** stream);
/* convenience: forward + all backward segments */
SDXL_API int sdxl_loss_fwd_bwd(sdxl_handle* h, const sdxl_loss_config* lc, const sdxl_batch* b, float grad_scale,
                      int first_micro, void* stream);
/* every backward segment in one call (what a caller without a per-segment gradient exchange uses: one captured graph) */
SDXL_API int sdxl_backward_all(sdxl_handle* h, float grad_scale, int first_micro, void* stream);
/* hipGraph replay of forward / backward (default OFF: measured slower than eager two-stream launches on ROCm 7.2, see
 * DESIGN.md): the second call with a given (plan, loss configuration including loss_type / huber_c and which per-sample arrays are
 * present, the loss mask / noise_in and mask_norm, whether input_cond is present, first_micro, grad_scale) captures the launch sequence of both streams, later calls replay it with one hipGraphLaunch.  0 = launch
 * kernel by kernel.  Inputs are staged at fixed addresses inside the plan, so the caller's tensors may move between steps.
 * A micro-step that carries a sdxl_residuals is never captured: its forward and backward launch kernel by kernel (above). */
SDXL_API int sdxl_set_graph_mode(sdxl_handle* h, int on);
/* synchronises `stream`; out[0]=loss out[1]=sum s*w*l(pred-target) (s = 1, l = square unless set otherwise) out[2]=sum|pred| out[3]=sum pred^2
 * out[4]=sum|noise| out[5]=sum noise^2 (x0) out[6]=sum latents^2 (x1) out[7]=gradient gate */
SDXL_API int sdxl_read_loss(sdxl_handle* h, float out[8], void* stream);

/* UNet only: sample_nhwc8 [B*H*W][Cs] bf16 in (Cs = 8, or 16 with in_channels > 8; channels past in_channels ignored) -> pred [B*H*W][8] bf16 out.
 * (replaces unet(sample, t, ehs, added_cond_kwargs).sample, ddpm_trainer.py:320-325) */
/* With cond->sampler set, sample_nhwc8 and pred_nhwc8 must be NULL: the call uploads the conditioning, runs the forward on what the
 * plan's input buffer holds (B, or 2B = [cond; uncond] with cfg: both halves hold the same latent), then the step kernel, which leaves
 * the next input there -- no copy in or out.  init = 1 runs only the kernel's input-writing part (no upload, no forward): the first call
 * of a loop.  cfg with an odd plan batch, x == NULL or a non-finite scalar is a bad argument (1), reported before any launch.  The sampler
 * path always launches kernel by kernel, also in graph mode. */
SDXL_API int sdxl_unet_forward(sdxl_handle* h, const void* sample_nhwc8, const sdxl_batch* cond, void* pred_nhwc8, void* stream);
/* d(pred) in -> runs every backward segment.  The conditioning gradients are produced when the preceding sdxl_unet_forward asked for them
 * (sdxl_batch_ext): of <dpred, pred>, no scale, no gate; so are the residual gradients (sdxl_residuals) and d(sample) (sdxl_batch_din) */
SDXL_API int sdxl_unet_backward(sdxl_handle* h, const void* dpred_nhwc8, int first_micro, void* stream);

/* fp32 grads -> bf16 (scaled) for the gradient exchange; global L2 norm of the fp32 grads */
SDXL_API int sdxl_grads_to_bf16(sdxl_handle* h, size_t elem_offset, size_t elems, void* dst_bf16, float scale, void* stream);
/* Exchange micro-step without the cast pass: with a bf16 arena set (element offsets = the gradient arena's; NULL turns it
 * off), every weight-gradient GEMM of the following backward calls writes its FINAL value (including what earlier
 * micro-steps accumulated in fp32) x scale as bf16 there and leaves the fp32 arena alone; sdxl_small_grads_to_bf16 then
 * casts what the GEMMs do not produce (biases, norm parameters) for a segment range.  The fp32 arena is NOT the step's
 * gradient afterwards: use this only when the bf16 arena is what the exchange / optimizer consume. */
SDXL_API int sdxl_set_grad_emit(sdxl_handle* h, void* bf16_arena, float scale);
SDXL_API int sdxl_small_grads_to_bf16(sdxl_handle* h, size_t elem_offset, size_t elems, void* dst_bf16, float scale, void* stream);
SDXL_API int sdxl_grad_sumsq(sdxl_handle* h, float* out_dev, void* stream);
/* row f3 pieces: squared L2 norm of any fp32 (dtype 0) / bf16 (1) device array -- e.g. the all-reduced bf16 gradient
 * arena -- and torch.nn.utils.clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)) computed on the device;
 * the coefficient is consumed by sdxl_adamw_bf16_step's grad_scale_dev, so clipping costs no pass over the gradients
 * (reference: clip_grad_norm_ then optimizer.step, flow_matching_trainer.py:181-189). */
SDXL_API int sdxl_sumsq(const void* x_dev, int dtype, size_t n, float* out_dev, void* stream);
SDXL_API int sdxl_clip_coef(const float* sumsq_dev, float max_norm, float* coef_dev, void* stream);

/* ---- single-kernel entry points (parity tests call these; same kernels the plan launches) --------------------- */
/* C[M,N] = A.B ; form 0: A[M,K],B[N,K] ; 1: A[M,K],B[K,N] ; 2: A[K,M],B[K,N] -> fp32 C (+= if accumulate).
 * form 2 (wgrad): `bias`, when given, is the fp32 bias-GRADIENT accumulator float[M]: += column sums of A.
 * splitk > 1: deterministic split-K (fp32 partial slabs, fixed-order sum): the wgrad form always; forms 0 / 1 when K is a
 * multiple of 64 (what the plan does for problems with fewer than 128 output tiles), otherwise ignored. */
SDXL_API int sdxl_op_gemm(int form, const void* A, const void* B, void* C, int M, int N, int K, const void* bias,
                 const void* resid, int accumulate, int splitk, void* stream);
/* n (<= 4) weight gradients of one shape in one launch, as the plan groups them: dw[i][Mo][No] (+)= dy[i]^T . x[i] with
 * dy[i] [rows][Mo], x[i] [rows][No] bf16; dbias (may be NULL, entries may be NULL): dbias[i][Mo] += column sums of dy[i]. */
SDXL_API int sdxl_op_wgrad_group(int n, const void* const* dy, const void* const* x, float* const* dw, float* const* dbias, int Mo,
                        int No, int rows, int accumulate, void* stream);
/* 3x3 conv, pad 1, token-major: x [B,H,W,Cin], w [Cout][9][Cin] ; y [B,Ho,Wo,Cout] */
SDXL_API int sdxl_op_conv3x3_fwd(const void* x, const void* w, const void* bias, void* y, int B, int H, int W, int Cin,
                        int Cout, int stride, void* stream);
/* conv3x3(nearest-2x upsample(x)) and its input gradient WITHOUT the upsampled image (the pair `Upsample2D` of diffusers =
   F.interpolate(scale 2, nearest) + Conv2d 3x3, which the reference's UNet runs at the two up-level transitions): per output phase a
   2 x 2 stencil on the low-resolution image with summed taps.  x [B][H][W][Cin], w [Cout][9][Cin], y / dy [B][2H][2W][Cout];
   weff [Cout][16][Cin] and planar [4 * roundup(B*H*W, 128)][Cout] are bf16 scratch of the caller (weff: written by _fwd, read by _dgrad);
   dx = addend (may be NULL) + gradient. */
SDXL_API int sdxl_op_upconv3x3_fwd(const void* x, const void* w, const void* bias, void* weff, void* planar, void* y, int B, int H, int W,
                          int Cin, int Cout, void* stream);
SDXL_API int sdxl_op_upconv3x3_dgrad(const void* dy, const void* weff, void* planar, void* dx, const void* addend, int B, int H, int W, int Cin,
                            int Cout, void* stream);
/* Input gradient of the stride-2 3x3 convolution (the two `Downsample2D` convs; pad 1, H and W even) by output phase: input pixel
   (2r + a, 2c + b) receives 1 / 2 / 2 / 4 of the nine taps.  dy [B][H/2][W/2][Cout], w [Cout][9][Cin], dx [B][H][W][Cin] = addend
   (may be NULL) + gradient; planar [4 * roundup(B*(H/2)*(W/2), 128)][Cin] bf16 scratch. */
SDXL_API int sdxl_op_conv3x3_s2_dgrad(const void* dy, const void* w, void* planar, void* dx, const void* addend, int B, int H, int W, int Cin,
                             int Cout, void* stream);
/* ... and its weight / bias gradient: `planar` as _dgrad left it (dy de-interleaved into its four phases), x the low-resolution input;
   dweff [Cout][16][Cin] fp32 scratch; dw [Cout][9][Cin] fp32 (accumulate 0: =, 1: +=), dbias[Cout] += (may be NULL); splitk >= 1.
   The reduction over the B*H*W low-resolution pixels runs in whole 64-pixel steps: B*H*W % 64 != 0 is rejected as an argument
   error, where _fwd and _dgrad take any B*H*W (the plan then takes the weight gradient from the up-sampled image instead). */
SDXL_API int sdxl_op_upconv3x3_wgrad(const void* planar, const void* x, float* dweff, float* dw, float* dbias, int accumulate, int B, int H,
                            int W, int Cin, int Cout, int splitk, void* stream);
SDXL_API int sdxl_op_conv3x3_dgrad(const void* dy, const void* w, void* dx, int B, int H, int W, int Cin, int Cout,
                          int stride, void* stream);
SDXL_API int sdxl_op_conv3x3_wgrad(const void* x, const void* dy, float* dw, int B, int H, int W, int Cin, int Cout,
                          int stride, int splitk, void* stream);
/* the same with the plan's options: dbias[Cout] += column sums of dy (may be NULL), accumulate 0 / 1, splitk <= 0 = the plan's choice.
 * Same-size stride-1 convolutions with W % 64 == 0 and >= 16 384 pixels run on the three-taps-per-workgroup kernel (conv_wgrad3.hip). */
SDXL_API int sdxl_op_conv3x3_wgrad2(const void* x, const void* dy, float* dw, float* dbias, int B, int H, int W, int Cin, int Cout,
                           int stride, int splitk, int accumulate, void* stream);
SDXL_API int sdxl_op_attention_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int heads,
                          int Nq, int Nk, long ldq, long ldk, long ldv, long ldo, void* stream);
SDXL_API int sdxl_op_attention_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o,
                          const float* lse, float* delta, void* dq, void* dk, void* dv, int B, int heads, int Nq,
                          int Nk, long ldq, long ldk, long ldv, long ldo, void* stream);
SDXL_API int sdxl_op_groupnorm_fwd(const void* x, void* y, const void* gamma, const void* beta, float* stats, float* ws,
                          int B, int HW, int C, int G, float eps, int silu, void* stream);
SDXL_API int sdxl_op_groupnorm_bwd(const void* x, const void* dy, const void* gamma, const void* beta, const float* stats,
                          void* dx, float* dgamma, float* dbeta, float* ws, int B, int HW, int C, int G, int silu,
                          int accumulate, void* stream);
SDXL_API int sdxl_op_layernorm_fwd(const void* x, void* y, const void* gamma, const void* beta, float* stats, int M, int C,
                          float eps, void* stream);
SDXL_API int sdxl_op_layernorm_bwd(const void* x, const void* dy, const void* gamma, const float* stats, void* dx,
                          float* dgamma, float* dbeta, int M, int C, int accumulate, void* stream);
/* GEGLU feed-forward pair, fused into the two projections' GEMM epilogues.  w1 [2*C4][K] / b1 [2*C4] and the
 * pre-activation u [M][2*C4] use the library's packed order with group G = 64 or 80 (C4 % G == 0): channel c's value
 * half at row/column (c/G)*2G + c%G, its gate half G further.  sdxl_load_weight applies this to "ff.net.0.proj" with
 * G = 80 where 4*C divides (SDXL-base: 5120, 2560), else 64; callers only ever see the diffusers layout.
 * fwd: u = x @ w1^T + b1,  g[M][C4] = value * gelu(gate).
 * bwd: du[M][2*C4] from dy[M][C] @ w2[C][C4] (the second projection's input gradient) and u. */
SDXL_API int sdxl_op_ff_geglu_fwd(const void* x, const void* w1, const void* b1, void* u, void* g, int M, int K, int C4,
                         int group, void* stream);
SDXL_API int sdxl_op_ff_geglu_bwd(const void* dy, const void* w2, const void* u, void* du, int M, int C, int C4, int group,
                         void* stream);
/* phase 2 follows phase 1 of the same batch on the same stream: it reads the gate phase 1 left in out8_dev[7] and, with
 * mask_norm 1 (masked_mean), the per-sample normalisers M_b phase 1 left in the library's scratch.  Phase 0 reads
 * noise_in only: the mask, mask_norm and that scratch are nothing to it. */
SDXL_API int sdxl_op_loss(const sdxl_loss_config* lc, const sdxl_batch* b, void* unet_in, const void* pred, void* dpred,
                 float grad_scale, float* out8_dev, int phase /*0 prepare,1 loss,2 dpred*/, void* stream);
/* (phase 0 with a sdxl_batch_cond: unet_in is [B*H*W][Cs] for 4 + cond_channels input channels; phases 1 and 2 ignore input_cond) */
/* ---- row f1: fused AdamW_BF16 step (replaces AdamWBF16.step / _make_step,
 * reference src/training/optimizers/adamw_bfloat16/__init__.py:87-197 and stochastic/__init__.py:46-124).
 * One launch over flat arrays (the packed weight / gradient arenas, or any 16-byte aligned slice of them):
 * p, m (exp_avg), v (exp_avg_sq), shift are bf16 and updated in place; grad is fp32 (grad_dtype 0, the native arena) or
 * bf16 (1).  n must be a multiple of 8.  grad_scale_dev: optional device float multiplied into the gradient
 * (1/accumulation, clip coefficient).  rand_inject: optional uint16 [4][n] table of the random integers of the four
 * stochastic roundings in the reference's draw order (exp_avg, shift, p, shift) -- parity tests; NULL = Philox keyed
 * by (seed, step, element).  Weight decay is lazy in the reference (per tensor, paid when wd*lr accumulates past
 * 5e-3): decay_this_iteration applies to the whole launch; sdxl_adamw_decay pays it for one tensor's range. */
/* one tensor of the Adafactor table (algorithm 3, below): a row-major matrix inside the arena */
typedef struct sdxl_adafactor_tensor {
  size_t elem_off;             /* arena element offset of its element (0, 0), a multiple of 8 */
  int rows, cols;              /* cols is the arena row stride and a multiple of 8; the entry owns elem_off .. elem_off + rows*cols */
  size_t numel;                /* the real elements, 1 .. rows*cols: the divisor of both RMS (pads hold g = 0, p = 0) */
  int factored;                /* 1: row and column statistics R[rows], C[cols]; 0: one second moment per element, v[rows*cols] */
  size_t state_off;            /* float offset into af_state, a multiple of 4: R then C (rows + cols floats), or v (rows*cols floats) */
} sdxl_adafactor_tensor;
typedef struct {
  double lr, beta1, beta2, eps; /* doubles: the reference derives 1-beta, -lr*sqrt(1-beta2^t) in python floats */
  double step;                 /* t >= 1 of this update (denominator correction sqrt(1 - beta2^t)) */
  double decay_this_iteration; /* 0 = none */
  int reference_ema;           /* 1: the reference's arithmetic exactly, m <- SR(g + (1-beta1)*(beta1*m))  [its
                                  add_stochastic_ applies alpha to the wrong operand, stochastic/__init__.py:96];
                                  0: the documented EMA m <- SR(beta1*m + (1-beta1)*g) */
  int grad_round_bf16;         /* 1: round the scaled gradient to bf16 first (the reference's gradients are bf16) */
  unsigned long long seed;
  unsigned long long elem_offset; /* arena index of element 0 of this call (multiple of 8).  The stochastic-rounding counters are
                                   * (seed, step, arena index), so updating a sub-range [elem_offset, elem_offset + n) of the arena
                                   * (one rank's ZeRO-1 shard) gives exactly the bits of the full-arena update. */
  /* ---- appended: algorithm selection (sdxl_adamw_default_config zeroes them: algorithm 0 as before) ---- */
  int algorithm;               /* 0 = AdamW_BF16 (above); 1 = schedule-free Kahan AdamW (reference
                                  src/training/optimizers/adamw_schedulefree/__init__.py): m, v and shift carry exp_avg,
                                  exp_avg_sq and kahan_comp (shift may be NULL only when kahan_sum is 0); rand_inject must
                                  be NULL; lr, step, decay_this_iteration, reference_ema, seed and elem_offset are not read */
  int kahan_sum;               /* algorithm 1: 1 = keep the kahan_comp arena */
  int sf_reference;            /* algorithm 1: 1 = the reference's bf16 arithmetic bit for bit (its compensation stays +0,
                                  weight decay not scaled by lr); 0 = compensated: true parameter p + kahan_comp in fp32,
                                  decoupled decay step_size * weight_decay */
  double weight_decay;         /* algorithm 1 */
  double sf_step_size;         /* algorithm 1: the reference's step_size = adjusted_lr / sqrt(1 - beta2^(k+1)), computed by
                                  the caller in double precision */
  /* ---- appended: fp32 EMA of the weights, both algorithms (sdxl_adamw_default_config zeroes them: no EMA) ---- */
  float* ema;                  /* NULL = no EMA; else an fp32 array aligned with p (its element 0 is p's element 0, 16-byte
                                  aligned).  Once an element's new bf16 p is final: e <- e - omd * (e - float(p)), three
                                  separately rounded fp32 ops (t1 = e - p, t2 = omd * t1, e = e - t2), i.e. diffusers'
                                  EMAModel.step on the parameter the module holds (not p + shift / kahan_comp) */
  float ema_one_minus_decay;   /* omd: 1 - decay of this update, in [0, 1] (the caller's python double rounded to float32) */
  /* ---- appended: algorithm 2, Prodigy (sdxl_adamw_default_config zeroes them; algorithms 0 and 1 do not read them) ---- */
  double beta3, d0, d_coef, growth_rate;   /* beta3 in [0, 1); d0 > 0; d_coef > 0; growth_rate >= 1 (infinity = unbounded) */
  double prodigy_bc;           /* this step's bias-correction factor sqrt(1 - beta2^(k+1)) / (1 - beta1^(k+1)), computed by the
                                  caller in double precision; 1 when bias correction is off.  Finite and > 0 */
  int safeguard_warmup;        /* 1: s accumulates d/d0 * d * g instead of d/d0 * dlr * g */
  const void* p0;              /* bf16 [n]: the parameters at construction, read only */
  float* s;                    /* fp32 [n]: Prodigy's s */
  float* prodigy_state;        /* device array of SDXL_PRODIGY_STATE_FLOATS floats (below) */
  /* ---- appended: algorithm 3, Adafactor (sdxl_adamw_default_config zeroes them; algorithms 0, 1 and 2 do not read them) ---- */
  double clip_threshold;       /* > 0: the update of a tensor is divided by max(1, rms_u / clip_threshold) */
  double eps1, eps2;           /* eps1 is added to the squared gradient, eps2 is the floor of rms_p under scale_parameter; both >= 0 */
  double beta2t;               /* this step's decay of the second-moment statistics, 1 - k^decay_rate for step k >= 1, computed by
                                  the caller in double precision; in [0, 1) (0 at k = 1) */
  double rho;                  /* this step's step-size base, computed by the caller in double precision: lr, or with relative_step
                                  min(warmup_init ? 1e-6 * k : 1e-2, 1 / sqrt(k)).  Finite */
  int scale_parameter;         /* 1: rho is multiplied by max(eps2, rms_p) of each tensor */
  int use_beta1;               /* 1: m carries the fp32 first moment and the update goes through it */
  const struct sdxl_adafactor_tensor* tensors;   /* HOST array of n_tensors entries (below), read during the call */
  int n_tensors;
  float* af_state;             /* device, fp32: the factored statistics, addressed by each entry's state_off */
  float* af_scratch;           /* device, fp32: adafactor_scratch_floats(table) floats (below), written before they are read */
} sdxl_adamw_config;
/* ---- algorithm 2: Prodigy (Mishchenko & Defazio, "Prodigy: An Expeditiously Adaptive Parameter-Free Learner"): AdamW whose
 * step size d is estimated from two sums over the whole arena and lives on the device, so a step costs no host read-back.
 * Arguments of sdxl_adamw_bf16_step under algorithm 2: p bf16; shift = the bf16 compensation c (the true parameter is x = p + c);
 * m, v = FP32 exp_avg, exp_avg_sq; grad, grad_dtype, grad_scale_dev as above; rand_inject NULL; n a multiple of 8 and the whole
 * arena of the call (d is one number per call: there is no sub-range form).  Every pointer 16-byte aligned.  Read from the
 * config: lr (the multiplier on d), beta1, beta2, eps, weight_decay, grad_round_bf16, ema, ema_one_minus_decay and the fields
 * appended for algorithm 2; not read: elem_offset, step, seed, reference_ema, decay_this_iteration.  lr == 0 returns 0 without a
 * launch and writes nothing.  Argument errors (a NULL or misaligned buffer, n % 8, rand_inject, beta3 outside [0, 1), d0 <= 0,
 * d_coef <= 0, growth_rate < 1, prodigy_bc not finite and positive, lr < 0, weight_decay < 0) return 1 before anything touches
 * the device.
 *
 * prodigy_state: [0] d  [1] d_max  [2] num  [3] Bs  [4] d_hat  [5] dlr  [6] A  [7] 0; a fresh state is d = d_max = d0, the rest 0.
 * Floats 8 .. are the reduction scratch, written before they are read: workgroup b's partial sums at [8 + 2b], [8 + 2b + 1].
 *
 * The arithmetic, all fp32 with every operation rounded on its own (host doubles are rounded to float once: omb1 = float(1 - beta1)
 * and so on), three launches:
 *   scalars from d = state[0]:  dlr = (d*lr)*bc   cm = d*omb1   cv = (d*d)*omb2   r = d/d0   cs = r*(safeguard ? d : dlr)   cn = r*dlr
 *   accumulate, per element:    gr = grad * scale (rounded to bf16 with grad_round_bf16)     x = float(p) + float(c)
 *                               t = gr*(float(p0) - x)   m' = (b1*m) + (cm*gr)   v' = (b2*v) + ((cv*gr)*gr)   s' = (b3*s) + (cs*gr)
 *                               a = |s'|;   writes m', v', s' and each workgroup's partial sums of t and a
 *   finalize, one workgroup:    A = sum t   Bs = sum a   num' = (b3*num) + (cn*A)
 *                               Bs > 0:  d_hat = (d_coef*num')/Bs   d1 = (d == d0) ? max(d, d_hat) : d   d_max' = max(d_max, d_hat)
 *                                        d' = min(d_max', d1*growth)
 *                               else:    d, d_max unchanged, d_hat = d
 *   apply, per element:         de = d'*eps   x = float(p) + float(c)   weight_decay != 0: x = x - ((wd*dlr)*x)
 *                               x = x - (dlr*(m'/(sqrt(v') + de)))   p' = bf16_rn(x)   c' = bf16_rn(x - float(p'))
 *                               then the EMA of p' when one is attached
 * One deliberate departure from the prodigyopt package: when Bs == 0 (every s' is zero, e.g. all-zero gradients) the package
 * returns before the parameter update and does not count the step; here the apply pass runs (with m' = 0 it moves nothing but the
 * decay) and the caller counts the step, so that no step needs a read-back.
 *
 * The sums are bitwise reproducible: no atomics, the kernel boundary is the only synchronisation.  Geometry: workgroups of 256
 * threads, grid G(n) = min(ceil(n / 2048), SDXL_PRODIGY_MAX_GRID); thread j of workgroup b owns the 8-element vectors
 * i = b*256 + j, i + 256*G, ... below n/8 and adds their t (and a) in that order, element 0 .. 7 of each, into one fp32 sum, so a
 * thread adds at most T(n) = 8 * ceil(n / (2048 * G(n))) terms; the workgroup's 256 sums go through a fixed pairwise tree
 * (x[j] += x[j + h], h = 128, 64, .. 1); the finalize adds the G partials in double precision in ascending workgroup index
 * (thread j of its one workgroup takes the partials j*ceil(G/256) .., then the 256 sums are added in ascending j) and rounds
 * A and Bs to float once.  The bits depend on n and this geometry alone. */
#define SDXL_PRODIGY_MAX_GRID 4096                                   /* the largest grid of the optimizer launches: 256 CUs x 16 */
#define SDXL_PRODIGY_STATE_FLOATS (8 + 2 * SDXL_PRODIGY_MAX_GRID)
/* ---- algorithm 3: Adafactor (Shazeer & Stern, "Adafactor: Adaptive Learning Rates with Sublinear Memory Cost"; the arithmetic
 * follows transformers.optimization.Adafactor.step): the second moment of a weight matrix is kept as one row and one column
 * statistic, so the state is rows + cols floats per matrix instead of two arenas.  The update needs per-tensor sums (row and
 * column sums of g^2, the RMS of the update for clipping, the RMS of the parameter), so the call takes a table of the tensors
 * inside the arena and runs five launches whatever n_tensors is.
 * Arguments of sdxl_adamw_bf16_step under algorithm 3: p bf16; shift = the bf16 compensation c (the true parameter is
 * x = float(p) + float(c), as under algorithm 2); m = the FP32 first moment, or NULL when use_beta1 is 0; v must be NULL;
 * rand_inject must be NULL; n a multiple of 8 and the whole arena.  Every pointer 16-byte aligned.  Read from the config: beta1
 * (with use_beta1), weight_decay, grad_round_bf16, ema, ema_one_minus_decay and the fields appended for algorithm 3; not read: lr,
 * beta2, eps, step, seed, elem_offset, reference_ema, decay_this_iteration.  Elements that belong to no table entry are neither
 * read nor written: a frozen tensor is a tensor left out of the table.  n_tensors == 0 returns 0 without a launch.  The device
 * copy of the table is cached inside the library, keyed by its contents.
 * Argument errors return 1 before anything touches the device, and the message names the entry: entries that overlap or are not
 * sorted by elem_off, a range past n, elem_off % 8, cols % 8, rows < 1, numel of 0 or above rows*cols, state_off % 4, factored
 * other than 0 or 1; and a NULL or misaligned
 * buffer (af_state, af_scratch, tensors included), clip_threshold <= 0, beta2t outside [0, 1), a non-finite rho, negative eps1,
 * eps2 or weight_decay, a non-NULL v or rand_inject.
 *
 * Which tensors are factored is the caller's choice (optimizer.py::adafactor_layout): a 2-D weight as [out][in]; a 4-D
 * convolution weight as [shape[0]][prod(rest)], in the arena the plain row-major matrix [cout][9*cin].  That is deliberately
 * not the HF class's choice, which factors a 4-D tensor over its last two dimensions (kh, kw): factoring over a 3 x 3 pair
 * saves nothing (6 floats for 9), while [cout][cin*kh*kw] is the convention of this project's LoRA targets and a permutation of
 * the columns (tap-major in the arena) changes no statistic.  Row-permuted matrices (ff.net.0.proj) only permute R.
 *
 * The arithmetic, all fp32 with every operation rounded on its own (host doubles are rounded to float once: b2t = float(beta2t),
 * omb2t = float(1 - beta2t), omb1 = float(1 - beta1) and so on); rsqrt(y) = 1 / sqrt(y), both correctly rounded; rows and cols
 * enter the means as floats:
 *   per element:      gr = grad * scale (rounded to bf16 with grad_round_bf16)   q = (gr*gr) + eps1   x = float(p) + float(c)
 *   stats, factored:  R'_o = (b2t*R_o) + (omb2t*((sum_i q)/cols))      C'_i = (b2t*C_i) + (omb2t*((sum_o q)/rows))
 *                     mean = (sum_o R'_o)/rows      u = (rsqrt(R'_o/mean) * rsqrt(C'_i)) * gr
 *   unfactored:       v' = (b2t*v) + (omb2t*q)      u = rsqrt(v') * gr
 *   per tensor:       rms_u = sqrt((sum u*u)/numel)   rms_p = sqrt((sum x*x)/numel)  (read only with scale_parameter, else 0)
 *                     rho_t = scale_parameter ? rho*max(eps2, rms_p) : rho        eta_t = rho_t / max(1, rms_u/clip_threshold)
 *   apply:            D = eta_t*u    use_beta1: m' = (b1*m) + (omb1*D), D = m'    weight_decay != 0: x = x - ((wd*rho_t)*x)
 *                     x = x - D      p' = bf16_rn(x)      c' = bf16_rn(x - float(p'))      then the EMA of p' when one is attached
 * A pad (g = 0, p = 0, c = 0) stays +0 bit for bit: u = 0 there, and it adds eps1 to its row's and column's sums as any element.
 *
 * Geometry.  A tensor is cut into tiles of SDXL_AF_ROWS x SDXL_AF_COLS elements, row blocks outer, column blocks inner:
 * ncb = ceil(cols / SDXL_AF_COLS), nrb = ceil(rows / SDXL_AF_ROWS), tile (rb, cb) has the index rb*ncb + cb.  One workgroup of
 * 256 threads takes one tile: thread j owns the 8-column vector j % 32 of the tile in the rows (j / 32) + 8*i, i = 0 .. 15.
 * No atomics, no ticket or fence inside a launch: the kernel boundary is the only synchronisation, every sum has a fixed order that
 * depends on the tensor's (rows, cols, factored) alone, so a tensor's bits do not depend on the other entries or on its place
 * in the table, and repeated runs are bit-equal.
 *   launch 1, stats:   a tile's row sums: each thread adds q of its 8 columns in ascending column order, then the 32 threads of
 *                      the row combine by the butterfly s += s[lane ^ h], h = 16, 8, 4, 2, 1; its column sums: each thread adds
 *                      its rows in ascending i per column, then the 8 threads of a column are added in ascending j / 32; its
 *                      sum of x*x: per thread in (i, column) order, then the workgroup's tree x[j] += x[j + h], h = 128 .. 1.
 *   launch 2, reduce:  one thread per row adds the row's ncb tile sums in ascending cb, one thread per column adds the column's
 *                      nrb tile sums in ascending rb; R', C' are written; the R' of each chunk of 256 rows go through the
 *                      workgroup's tree into one partial.
 *   launch 3, usq:     mean = the chunk partials in ascending order / rows; u; v' is written; a tile's sum of u*u as for x*x.
 *   launch 4, scalars: one workgroup per tensor adds the tensor's tile sums in double precision (thread j takes the tiles
 *                      j*ceil(T/256) .. in ascending order, then the 256 sums are added in ascending j), rounds to float once,
 *                      and writes rho_t, eta_t, rms_u, rms_p.
 *   launch 5, apply:   u exactly as in launch 3, then the update.
 * A thread adds at most 128 terms into one fp32 sum in launch 1 or 3, and max(ncb, nrb, ceil(rows/256)) in launch 2 or 3.
 *
 * af_scratch, adafactor_scratch_floats(table) floats in all: first 4 floats per entry in table order (rho_t, eta_t, rms_u,
 * rms_p: what launch 4 writes and a caller may read back), then per entry in table order, with T = nrb*ncb:
 *   T floats (the tiles' sums of x*x), T floats (of u*u), and for a factored entry ceil(rows/256) floats (the chunk partials of
 *   R'), rows*ncb floats (row sums, [row][cb]) and nrb*cols floats (column sums, [rb][col]). */
#define SDXL_AF_ROWS 128
#define SDXL_AF_COLS 256
SDXL_API int sdxl_adamw_default_config(sdxl_adamw_config* c);   /* lr 1e-4, betas (0.9, 0.999), eps 1e-8, reference_ema 1, algorithm 0, no EMA */
SDXL_API int sdxl_adamw_bf16_step(void* p, const void* grad, int grad_dtype, void* m, void* v, void* shift, size_t n,
                         const sdxl_adamw_config* c, const float* grad_scale_dev, const unsigned short* rand_inject,
                         void* stream);
SDXL_API int sdxl_adamw_decay(void* shift, const void* p, size_t n, float decay, void* stream);

/* measurement: between begin and end every launch of the bf16 MFMA GEMM family (Linear / conv fwd, dgrad, wgrad) is
 * bracketed by HIP events on its launch stream; end synchronises and returns the summed algorithmic FLOPs
 * (2*M*N*K*taps), the summed event time and the number of launches (bench.py's roofline block). */
SDXL_API int sdxl_profile_gemm_begin(void);
SDXL_API int sdxl_profile_gemm_end(double* flops, double* ms, int* launches);

/* Test hooks (layout probe, forced kernel configurations, activation checksums) and the experiment ABI of the diagnostics build
 * (knobs, stream-K, phase-plane stride-2 convolution) are NOT part of this boundary: include/sdxlstep_diag.h. */

#ifdef __cplusplus
}
#endif
#endif
