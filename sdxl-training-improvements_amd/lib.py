"""ctypes binding of libsdxlstep.so (include/sdxlstep.h).  No fallback: if the HIP library is missing or a
call fails this raises -- the product path never silently degrades to PyTorch ops or to the CPU oracle.

SDXL_DIAG=1 in the environment (or use_diag() before the first load()) selects libsdxlstep_diag.so, the -DSDXL_DIAG build with the
experiment ABI of include/sdxlstep_diag.h part 2 (knobs, stream-K, ...): A/B tooling and the tests marked `diag` only."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import os

HERE = Path(__file__).resolve().parent
DIAG = os.environ.get("SDXL_DIAG", "") == "1"
LIB_PATH = HERE / ("libsdxlstep_diag.so" if DIAG else "libsdxlstep.so")


def use_diag() -> None:
    """select the diagnostics build (before the first load())"""
    global DIAG, LIB_PATH
    if _lib is not None and not DIAG:
        raise SdxlError("use_diag() after the product library has been loaded")
    DIAG, LIB_PATH = True, HERE / "libsdxlstep_diag.so"



class SdxlError(RuntimeError):
    pass


class UNetConfig(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("block_out_channels", C.c_int * 3),
                ("layers_per_block", C.c_int), ("transformer_layers", C.c_int * 3), ("head_dim", C.c_int),
                ("cross_attention_dim", C.c_int), ("norm_num_groups", C.c_int),
                ("addition_time_embed_dim", C.c_int), ("pooled_dim", C.c_int),
                ("resnet_eps", C.c_float), ("tf_gn_eps", C.c_float), ("ln_eps", C.c_float)]


class LossConfig(C.Structure):
    _fields_ = [("method", C.c_int), ("prediction_type", C.c_int), ("use_min_snr", C.c_int),
                ("min_snr_gamma", C.c_float), ("use_ztsnr", C.c_int),
                # appended: element loss 0 = l2, 1 = huber, 2 = smooth_l1 (LOSS_TYPES); the scalar c
                ("loss_type", C.c_int), ("huber_c", C.c_float)]


LOSS_EXT = 0x100      # SDXL_LOSS_EXT, or-ed into loss_type: the struct passed is a LossConfigExt


class LossConfigExt(LossConfig):
    """sdxl_loss_config in full: LossConfig (what every caller without a mask or a separate input noise passes) + the fields the
    library reads only when loss_type carries LOSS_EXT.  mask_norm: MASK_NORMS."""
    _fields_ = [("mask_norm", C.c_int), ("loss_mask", C.c_void_p), ("noise_in", C.c_void_p)]


class SamplerStep(C.Structure):
    """sdxl_sampler_step: one sampler step behind sdxl_unet_forward's forward (Batch.sampler)"""
    _fields_ = [("x", C.c_void_p), ("cfg", C.c_int), ("init", C.c_int),
                ("a_skip", C.c_float), ("a_out", C.c_float), ("p", C.c_float), ("q", C.c_float),
                ("a_in_next", C.c_float), ("clamp", C.c_float), ("guidance", C.c_float), ("guidance_rescale", C.c_float)]


SAMPLER_EXT = 0x100   # SDXL_SAMPLER_EXT, or-ed into SamplerStep.init: the struct passed is a SamplerStepExt


class SamplerStepExt(SamplerStep):
    """sdxl_sampler_step_ext: SamplerStep (what every caller of the plain step passes) + the fields the library reads only when init
    carries SAMPLER_EXT: the terms of the second-order and ancestral solvers and the inpainting blend (include/sdxlstep.h)"""
    _fields_ = [("hist", C.c_void_p), ("xsave", C.c_void_p), ("noise", C.c_void_p),
                ("r", C.c_float), ("u", C.c_float), ("s", C.c_float), ("save", C.c_int),
                ("mask", C.c_void_p), ("known", C.c_void_p), ("knoise", C.c_void_p), ("k_a", C.c_float), ("k_b", C.c_float)]


class Batch(C.Structure):
    _fields_ = [("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("ctx_len", C.c_int),
                ("latents", C.c_void_p), ("noise", C.c_void_p), ("sigma_or_t", C.c_void_p),
                ("timestep", C.c_void_p), ("prompt_embeds", C.c_void_p), ("pooled", C.c_void_p),
                ("time_ids", C.c_void_p), ("tag_weights", C.c_void_p),
                # appended: optional [B] fp32 per-sample weights s_b / Huber c_b in, per-sample losses L_b out
                ("sample_weights", C.c_void_p), ("huber_c", C.c_void_p), ("per_sample_loss", C.c_void_p)]


class SamplerBatch(Batch):
    """sdxl_batch in full: Batch (what the training entry points read; they never look past it) + the appended host pointer to the
    sampler step that sdxl_unet_forward -- the one entry point that takes this class -- runs behind its forward (NULL = none)"""
    _fields_ = [("sampler", C.POINTER(SamplerStep))]


BATCH_EXT = 0x10000    # SDXL_BATCH_EXT, or-ed into Batch.ctx_len: the struct passed is a CondGradBatch


class CondGradBatch(SamplerBatch):
    """sdxl_batch_ext: SamplerBatch + the two optional fp32 outputs of the conditioning gradients, which the library reads only when
    ctx_len carries BATCH_EXT (include/sdxlstep.h)"""
    _fields_ = [("d_prompt_embeds", C.c_void_p), ("d_pooled", C.c_void_p)]


BATCH_COND = 0x20000   # SDXL_BATCH_COND, or-ed into Batch.ctx_len: the struct passed is an InputCondBatch


class InputCondBatch(CondGradBatch):
    """sdxl_batch_cond: CondGradBatch + the extra UNet input channels (in_channels > 4) [B, in_channels - 4, H, W] fp32, read only
    when ctx_len carries BATCH_COND; cond_channels 0 = the handle's in_channels - 4 (sdxl_op_loss, which has no handle: their number)"""
    _fields_ = [("input_cond", C.c_void_p), ("cond_channels", C.c_int)]


BATCH_RES = 0x40000    # SDXL_BATCH_RES, or-ed into Batch.ctx_len: the struct passed is a ResidualBatch


class Residuals(C.Structure):
    """sdxl_residuals: the additional skip residuals of one call (diffusers' down_block_additional_residuals / mid_block_additional_residual)
    and the fp32 outputs of their gradients.  down / d_down are HOST arrays [n] of device pointers, entries may be NULL"""
    _fields_ = [("n", C.c_int), ("dtype", C.c_int), ("down", C.POINTER(C.c_void_p)), ("mid", C.c_void_p),
                ("d_down", C.POINTER(C.c_void_p)), ("d_mid", C.c_void_p)]


class ResidualBatch(InputCondBatch):
    """sdxl_batch_res: InputCondBatch + the host pointer to a Residuals, read only when ctx_len carries BATCH_RES (which also says that
    every field of CondGradBatch and InputCondBatch is there)"""
    _fields_ = [("residuals", C.POINTER(Residuals))]


BATCH_DIN = 0x80000    # SDXL_BATCH_DIN, or-ed into Batch.ctx_len: the struct passed is an InputGradBatch


class InputGradBatch(ResidualBatch):
    """sdxl_batch_din: ResidualBatch + the optional fp32 output [B, in_channels, H, W] of the gradient with respect to the UNet input, read
    only when ctx_len carries BATCH_DIN (which also says that every field of CondGradBatch, InputCondBatch and ResidualBatch is there)"""
    _fields_ = [("d_input", C.c_void_p)]


DTYPE_LORA = 2        # SDXL_DTYPE_LORA of sdxl_load_weight (merge) / sdxl_export_grad (project): the pointer is a host LoraOp*, name NULL
DTYPE_LORA_LAYOUTS = 4  # SDXL_DTYPE_LORA_LAYOUTS: the same two calls and struct, targets in the arena's packed layouts accepted (lora.py, kinds="all")
DTYPE_LOHA = 5        # SDXL_DTYPE_LOHA: the same two calls and struct, four factors per target: dW = s (B1 A1) .* (B2 A2) (lora.py, algo="loha")


class LoraOp(C.Structure):
    """sdxl_lora_op: the targets (state-dict indices), rank, scale and the adapter / base / adapter-gradient arenas of lora.LoRAAdapters"""
    _fields_ = [("n", C.c_int), ("param", C.POINTER(C.c_int)), ("rank", C.c_int), ("scale", C.c_float),
                ("adapters", C.c_void_p), ("base", C.c_void_p), ("adapter_grads", C.c_void_p)]


DTYPE_LOKR = 6        # SDXL_DTYPE_LOKR: the same two calls with a host LokrOp*: dW = s kron(C, W2), W2 full or B A (lora.py, algo="kronecker")
LOKR_TILE = 1024      # SDXL_LOKR_TILE: elements of W2 per workgroup of the projection (the scratch formula, lora.lokr_scratch_floats)


class LokrOp(C.Structure):
    """sdxl_lokr_op: LoraOp, the factor (-1 or >= 1), full (0: the form rule per target, 1: every W2 in full) and the projection's scratch"""
    _fields_ = [("op", LoraOp), ("factor", C.c_int), ("full", C.c_int), ("scratch", C.c_void_p), ("scratch_floats", C.c_size_t)]


DTYPE_LOKR_ONE = 7    # SDXL_DTYPE_LOKR_ONE (sdxlstep_diag.h part 1): the LoKr kernels on caller buffers, one target, NULL handle and name, a host LokrOne*


class LokrOne(C.Structure):
    """sdxl_lokr_one: the test hook of csrc/lokr.hip (a dtype of sdxl_load_weight: merge / sdxl_export_grad: project, not a function)"""
    _fields_ = ([(k, C.c_void_p) for k in ("base", "C", "W2", "A", "w", "dw", "dC", "dW2", "dA")] +
                [(k, C.c_int) for k in ("out", "in_", "group", "kind", "factor", "rank", "full")] +
                [("scale", C.c_float), ("scratch", C.c_void_p), ("scratch_floats", C.c_size_t)])


DTYPE_DORA = 8        # SDXL_DTYPE_DORA: the same two calls with a host DoraOp*: W = c_o (W0 + s B A), c_o = (1 + mu_o) n0_o / n_o (lora.py, algo="dora")
DORA_MERGE, DORA_INIT, DORA_RESTORE = 0, 1, 2      # sdxl_dora_op.mode of sdxl_load_weight


class DoraOp(C.Structure):
    """sdxl_dora_op: LoraOp, the mode of sdxl_load_weight and the two fp32 row-norm buffers (one float per target row, each target padded to 4)"""
    _fields_ = [("op", LoraOp), ("mode", C.c_int), ("norm0", C.c_void_p), ("norm", C.c_void_p)]


DTYPE_DORA_ONE = 9    # SDXL_DTYPE_DORA_ONE (sdxlstep_diag.h part 1): the DoRA kernels on caller buffers, one target, NULL handle and name, a host DoraOne*


class DoraOne(C.Structure):
    """sdxl_dora_one: the test hook of csrc/dora.hip (a dtype of sdxl_load_weight: merge / init / restore by `mode`, sdxl_export_grad: project)"""
    _fields_ = ([(k, C.c_void_p) for k in ("base", "A", "B", "mu", "w", "dw", "dA", "dB", "dmu", "norm0", "norm")] +
                [(k, C.c_int) for k in ("out", "in_", "group", "kind", "rank", "mode")] + [("scale", C.c_float)])


DTYPE_GRAD_SELECT = 3  # SDXL_DTYPE_GRAD_SELECT of sdxl_export_grad: the pointer is a host GradSelect* (NULL = every tensor trainable), name NULL


class GradSelect(C.Structure):
    """sdxl_grad_select: one flag per state-dict tensor (sdxl_param_info order), 1 = the backward produces its gradient"""
    _fields_ = [("n", C.c_int), ("trainable", C.POINTER(C.c_ubyte)), ("lora", C.POINTER(LoraOp))]


LOSS_TYPES = {"l2": 0, "huber": 1, "smooth_l1": 2}
MASK_NORMS = {"mean": 0, "masked_mean": 1}


class AdafactorTensor(C.Structure):
    """sdxl_adafactor_tensor: one tensor of the Adafactor table, a row-major matrix inside the arena"""
    _fields_ = [("elem_off", C.c_size_t), ("rows", C.c_int), ("cols", C.c_int), ("numel", C.c_size_t), ("factored", C.c_int),
                ("state_off", C.c_size_t)]


AF_ROWS, AF_COLS = 128, 256                          # SDXL_AF_ROWS, SDXL_AF_COLS: the tile of the Adafactor launches


class AdamWConfig(C.Structure):
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("step", C.c_double), ("decay_this_iteration", C.c_double), ("reference_ema", C.c_int),
                ("grad_round_bf16", C.c_int), ("seed", C.c_ulonglong), ("elem_offset", C.c_ulonglong),
                # appended: algorithm 0 = AdamW_BF16, 1 = schedule-free Kahan (optimizer.AdamWScheduleFreeKahanBF16)
                ("algorithm", C.c_int), ("kahan_sum", C.c_int), ("sf_reference", C.c_int),
                ("weight_decay", C.c_double), ("sf_step_size", C.c_double),
                # appended: fp32 EMA of the weights (ema.WeightEMA), NULL = none
                ("ema", C.c_void_p), ("ema_one_minus_decay", C.c_float),
                # appended: algorithm 2 = Prodigy (optimizer.ProdigyBF16)
                ("beta3", C.c_double), ("d0", C.c_double), ("d_coef", C.c_double), ("growth_rate", C.c_double),
                ("prodigy_bc", C.c_double), ("safeguard_warmup", C.c_int), ("p0", C.c_void_p), ("s", C.c_void_p),
                ("prodigy_state", C.c_void_p),
                # appended: algorithm 3 = Adafactor (optimizer.AdafactorBF16)
                ("clip_threshold", C.c_double), ("eps1", C.c_double), ("eps2", C.c_double), ("beta2t", C.c_double), ("rho", C.c_double),
                ("scale_parameter", C.c_int), ("use_beta1", C.c_int), ("tensors", C.c_void_p), ("n_tensors", C.c_int),
                ("af_state", C.c_void_p), ("af_scratch", C.c_void_p)]


PRODIGY_MAX_GRID = 4096                              # SDXL_PRODIGY_MAX_GRID: the largest grid of the optimizer launches
PRODIGY_STATE_FLOATS = 8 + 2 * PRODIGY_MAX_GRID      # SDXL_PRODIGY_STATE_FLOATS


_vp, _i, _f, _l, _sz = C.c_void_p, C.c_int, C.c_float, C.c_long, C.c_size_t
_P = C.POINTER

# name -> argtypes   (every function returns int except sdxl_last_error)
SIGNATURES = {
    "sdxl_version": [],
    "sdxl_default_config": [_P(UNetConfig)],
    "sdxl_create": [_P(UNetConfig), _i, _P(_vp)],
    "sdxl_destroy": [_vp],
    "sdxl_param_bytes": [_vp, _P(_sz), _P(_sz)],
    "sdxl_bind_params": [_vp, _vp, _vp],
    "sdxl_num_params": [_vp],
    "sdxl_param_info": [_vp, _i, C.c_char_p, _i, _P(_i), _P(_l)],
    "sdxl_load_weight": [_vp, C.c_char_p, _vp, _i, _vp],
    "sdxl_export_weight": [_vp, C.c_char_p, _vp, _i, _vp],
    "sdxl_export_grad": [_vp, C.c_char_p, _vp, _i, _vp],
    "sdxl_plan": [_vp, _i, _i, _i, _i, _P(_sz)],
    "sdxl_bind_workspace": [_vp, _vp, _sz],
    "sdxl_zero_grads": [_vp, _vp],
    "sdxl_forward_loss": [_vp, _P(LossConfig), _P(Batch), _vp],
    "sdxl_num_segments": [_vp],
    "sdxl_segment_range": [_vp, _i, _P(_sz), _P(_sz)],
    "sdxl_backward_segment": [_vp, _i, _f, _i, _vp],
    "sdxl_loss_fwd_bwd": [_vp, _P(LossConfig), _P(Batch), _f, _i, _vp],
    "sdxl_backward_all": [_vp, _f, _i, _vp],
    "sdxl_set_graph_mode": [_vp, _i],
    "sdxl_read_loss": [_vp, _P(_f), _vp],
    "sdxl_unet_forward": [_vp, _vp, _P(SamplerBatch), _vp, _vp],
    "sdxl_unet_backward": [_vp, _vp, _i, _vp],
    "sdxl_grads_to_bf16": [_vp, _sz, _sz, _vp, _f, _vp],
    "sdxl_set_grad_emit": [_vp, _vp, _f],
    "sdxl_small_grads_to_bf16": [_vp, _sz, _sz, _vp, _f, _vp],
    "sdxl_grad_sumsq": [_vp, _vp, _vp],
    "sdxl_op_gemm": [_i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _vp],
    "sdxl_op_wgrad_group": [_i, _P(_vp), _P(_vp), _P(_vp), _P(_vp), _i, _i, _i, _i, _vp],
    "sdxl_op_conv3x3_fwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "sdxl_op_upconv3x3_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "sdxl_op_upconv3x3_dgrad": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "sdxl_op_conv3x3_s2_dgrad": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "sdxl_op_upconv3x3_wgrad": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "sdxl_op_conv3x3_dgrad": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "sdxl_op_conv3x3_wgrad": [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
    "sdxl_op_conv3x3_wgrad2": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp],
    "sdxl_op_attention_fwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _l, _l, _l, _l, _vp],
    "sdxl_op_attention_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _l, _l, _l, _l, _vp],
    "sdxl_op_groupnorm_fwd": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp],
    "sdxl_op_groupnorm_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp],
    "sdxl_op_layernorm_fwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp],
    "sdxl_op_layernorm_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp],
    "sdxl_set_join_mode": [_vp, _i],
    "sdxl_side_stream": [_vp, _P(_vp)],
    "sdxl_sumsq": [_vp, _i, _sz, _vp, _vp],
    "sdxl_clip_coef": [_vp, _f, _vp, _vp],
    "sdxl_param_range": [_vp, _i, _P(_sz), _P(_sz)],
    "sdxl_adamw_default_config": [C.POINTER(AdamWConfig)],
    "sdxl_adamw_bf16_step": [_vp, _vp, _i, _vp, _vp, _vp, _sz, C.POINTER(AdamWConfig), _vp, _vp, _vp],
    "sdxl_adamw_decay": [_vp, _vp, _sz, _f, _vp],
    "sdxl_op_ff_geglu_fwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "sdxl_op_ff_geglu_bwd": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "sdxl_op_loss": [_P(LossConfig), _P(Batch), _vp, _vp, _vp, _f, _vp, _i, _vp],
    "sdxl_profile_gemm_begin": [],
    "sdxl_profile_gemm_end": [_P(C.c_double), _P(C.c_double), _P(_i)],
}
# include/sdxlstep_diag.h part 1: test hooks, exported by the product library too
TEST_HOOK_SIGNATURES = {
    "sdxl_probe_layout": [_vp, _vp],
    "sdxl_set_gemm_mode": [_i],
    "sdxl_debug_act_checksums": [_vp, _P(C.c_ulonglong), _i, _P(_i), _i],
    "sdxl_op_exchange_shadow": [_vp, _sz, _i, _i, _f, _vp],
    "sdxl_op_gemm_ld": [_i, _vp, _vp, _vp, _i, _i, _i, C.c_long, C.c_long, C.c_long, _vp, _vp, C.c_long, _i, _vp],
    "sdxl_op_linear_dgrad_delta": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp],
    "sdxl_op_sampler_step": [_vp, _vp, _vp, _i, _i, _i, _P(SamplerStep), _vp],
    "sdxl_debug_cond_operands": [_vp, _i, _i, _P(_i), _P(_sz), _P(_l), _P(_sz), _P(_l), _P(_i)],
    "sdxl_op_cond_dgrad": [_i, _P(_vp), _P(_l), _P(_vp), _P(_l), _P(_i), _vp, _l, _i, _i, _vp],
    "sdxl_op_concat_residual": [_vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp],
    "sdxl_op_concat_residual_grad": [_vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp],
    "sdxl_op_input_dgrad": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "sdxl_debug_input_dgrad_operands": [_vp, _P(_sz), _P(_sz), _P(_i)],
    "sdxl_op_lora_merge": [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp],
    "sdxl_op_lora_project": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp],
    "sdxl_op_lora_merge_layout": [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _i, _i, _vp],
    "sdxl_op_lora_project_layout": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _i, _i, _vp],
    "sdxl_op_loha_merge": [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _i, _vp],
    "sdxl_op_loha_project": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _i, _vp],
    "sdxl_op_lora_grad": [_vp, _l, _vp, _l, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp],
    "sdxl_debug_gemm_route": [_P(_i), _P(_i)],      # sdxl_gemm_desc (GEMM_DESC_FIELDS + GEMM_DESC_HOOK_FIELDS ints) -> sdxl_gemm_route (GEMM_ROUTE_FIELDS ints)
    "sdxl_op_gemm_rowvec": [_i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _l, _i, _i, _i, _vp],
    "sdxl_op_conv3x3_fwd_rowvec": [_vp, _vp, _vp, _vp, _l, _vp, _i, _i, _i, _i, _i, _vp],
    "sdxl_op_colsum": [_vp, _l, _vp, _l, _i, _i, _i, _vp],
    "sdxl_op_sincos": [_vp, _vp, _i, _i, _l, _vp],
    "sdxl_debug_plan_num_ops": [_vp, _P(_i)],
    "sdxl_debug_plan_op": [_vp, _i, _vp, _sz],       # sdxl_plan_op_desc* (PlanOpDesc), its size
    "sdxl_debug_plan_tail": [_vp, _vp, _sz],         # sdxl_plan_tail* (PlanTail), its size
    "sdxl_debug_plan_loss": [_vp, _vp, _sz],         # sdxl_plan_loss* (PlanLoss), its size
}
PLAN_NONE = (1 << 64) - 1      # SDXL_PLAN_NONE: an absent offset of the plan map
PLAN_KINDS = ("linear", "conv", "groupnorm", "layernorm", "attn", "silu", "concat", "upsample", "embed_in")
PLAN_ROLES = 5
PLAN_ATTN_ROUTES = {0: "dq + dkv", 1: "dq + split dkv + reduce", 2: "fused", 3: "pipelined", -1: "unknown"}


class PlanTensor(C.Structure):
    """sdxl_plan_tensor: byte offsets of the data and the gradient in the workspace, rows, cols, row stride (elements), pad rows, first column"""
    _fields_ = [("off", _sz), ("goff", _sz), ("rows", _l), ("cols", _l), ("ld", _l), ("pad_rows", _i), ("col0", _i)]


class PlanOpDesc(C.Structure):
    """sdxl_plan_op_desc (include/sdxlstep_diag.h has the roles per kind)"""
    _fields_ = ([(k, _i) for k in ("kind", "seg", "hoist_fwd", "resid_alias")] + [("intact_after_step", C.c_uint)] +
                [(k, _i) for k in ("K", "N", "splitk", "wgroup", "crcfg", "crsplit", "fsplit", "dsplit", "delta_on", "ln_mode", "ggroup",
                                   "B", "H", "W", "Cin", "Cout", "stride", "up2", "up_fs", "up_ds", "up_ws", "up_wg", "three_tap", "rows_per_batch",
                                   "s2_dgrad", "groups", "silu", "heads", "Nq", "Nk", "self_attn", "qsplit", "delta_fused", "bwd_route", "skip",
                                   "first")] + [("dims", _i * 4), ("eps", _f)] + [(k, _l) for k in ("ldq", "ldk", "ldv", "ldvec")] +
                [(k, _sz) for k in ("dy_off", "dx_out", "dx_addend", "dres_out", "dres_addend", "d3_out", "d3_addend", "dy32_off", "w_off", "w_numel",
                                    "b_off", "b_numel", "stats_off", "lse_off", "delta_off", "rv32_off", "planar_off", "weff_off", "dweff_off",
                                    "s2_planar_off")] + [("t", PlanTensor * PLAN_ROLES)])


class PlanTail(C.Structure):
    """sdxl_plan_tail: the buffers of the plan that belong to no op"""
    _fields_ = ([(k, _i) for k in ("B", "H", "W", "ctx")] + [(k, PlanTensor) for k in ("x_in", "pred", "ehs")] +
                [(k, _sz) for k in ("tp32_off", "tp32_bytes", "t_off", "tid_off", "loss_off", "workspace_bytes")])


class PlanLoss(C.Structure):
    """sdxl_plan_loss: the loss's buffers in the plan (named after the Plan fields) and whether the last forward_loss read the staged copies"""
    _fields_ = ([(k, _sz) for k in ("loss_part_off", "ps_loss_off", "mask_norm_off", "in_lat_off", "in_noise_off", "in_nin_off", "in_sig_off",
                                    "in_tag_off", "in_sw_off", "in_hc_off", "in_mask_off", "in_cond_off", "part_floats")] +
                [(k, _i) for k in ("ps_slots", "staged")])


def _plain(st):
    """a ctypes struct as a plain dict: absent offsets None, nested structs dicts, arrays lists"""
    out = {}
    for name, tp in st._fields_:
        v = getattr(st, name)
        if isinstance(v, C.Structure):
            v = _plain(v)
        elif isinstance(v, C.Array):
            v = [_plain(e) if isinstance(e, C.Structure) else e for e in v]
        elif tp is _sz and v == PLAN_NONE:
            v = None
        out[name] = v
    return out


def plan_map(handle):
    """(ops, tail) of the handle's current plan: one plain dict per op in forward order (kind by name, "index" added; a tensor role the op
    does not have is None) and the tail's dict.  Pure host code in the library: nothing is launched, the plan does not change."""
    L = load()
    n = _i()
    check(L.sdxl_debug_plan_num_ops(handle, C.byref(n)), "sdxl_debug_plan_num_ops")
    ops = []
    for i in range(n.value):
        d = PlanOpDesc()
        check(L.sdxl_debug_plan_op(handle, i, C.byref(d), C.sizeof(d)), "sdxl_debug_plan_op")
        o = _plain(d)
        o["index"], o["kind"] = i, PLAN_KINDS[o["kind"]]
        o["t"] = [None if t["rows"] == 0 else t for t in o["t"]]
        ops.append(o)
    t = PlanTail()
    check(L.sdxl_debug_plan_tail(handle, C.byref(t), C.sizeof(t)), "sdxl_debug_plan_tail")
    return ops, _plain(t)


def plan_loss(handle) -> dict:
    """the loss's buffers in the handle's current plan (sdxl_debug_plan_loss): byte offsets into the workspace, None where the plan has none;
    staged: 1 / 0 / -1 as the header says.  Pure host code in the library."""
    t = PlanLoss()
    check(load().sdxl_debug_plan_loss(handle, C.byref(t), C.sizeof(t)), "sdxl_debug_plan_loss")
    return _plain(t)


GEMM_DESC_FIELDS = ("form", "taps", "M", "N", "K", "splitk", "group", "cfg", "geglu", "geglu_group", "Hm", "Wm", "Hs", "Ws", "sm", "sd", "up2", "emit_bf16", "delta", "bias_grad")
GEMM_DESC_HOOK_FIELDS = ("rowvec",)      # the struct's tail that the launch log does not carry: a row vector in the epilogue (default 0)
GEMM_ROUTE_FIELDS = ("kernel", "cfg", "fast", "post")
GEMM_KERNELS = ("128-row", "256x256", "cr256", "pipelined", "wgrad256", "conv_wgrad3", "stream-K")
GEMM_POSTS = ("none", "splitk_reduce", "splitk_epilogue")


def gemm_route(**problem) -> dict:
    """what launch_gemm would run for a problem (sdxl_debug_gemm_route; no device needed): kernel and post by name, cfg, fast.  Unnamed fields: a plain
    unsplit linear problem."""
    fields = GEMM_DESC_FIELDS + GEMM_DESC_HOOK_FIELDS
    d = dict(dict.fromkeys(fields, 0), taps=1, splitk=1, group=1, sm=1, sd=1)
    assert set(problem) <= set(d), set(problem) - set(d)
    d.update(problem)
    out = (_i * len(GEMM_ROUTE_FIELDS))()
    check(load().sdxl_debug_gemm_route((_i * len(fields))(*[int(d[k]) for k in fields]), out), "sdxl_debug_gemm_route")
    r = dict(zip(GEMM_ROUTE_FIELDS, out))
    return dict(r, kernel=GEMM_KERNELS[r["kernel"]], post=GEMM_POSTS[r["post"]], fast=bool(r["fast"]))


# include/sdxlstep_diag.h part 2: experiment ABI, exported by libsdxlstep_diag.so only
DIAG_SIGNATURES = {
    "sdxl_op_linear_dgrad_ln_bwd": [_vp, _vp, _vp, _P(_f), _vp, _vp, _vp, _vp, _P(_f), _i, _i, _i, _vp],
    "sdxl_set_knob": [_i, _i],
    "sdxl_set_sk_mode": [_i, _i],
    "sdxl_sk_error": [_vp, _P(C.c_uint)],
    "sdxl_ln_error": [_P(C.c_uint)],
    "sdxl_op_pl_prefetch_b": [_i, _vp, _i, _i, _i, C.c_long, _i, _vp],
    "sdxl_op_gemm_sk": [_i, _P(_i), _P(_vp), _P(_vp), _P(_vp), _P(_i), _P(_i), _P(_i), _P(_vp), _P(_vp), _P(_i), _vp],
    "sdxl_op_conv3x3_s2_fwd": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp],
    "sdxl_op_conv3x3_s2_wgrad": [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp],
}

_lib = None


def load() -> C.CDLL:
    """Load libsdxlstep.so and declare every prototype.  Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise SdxlError(f"{LIB_PATH} is missing -- build it with `python {HERE / 'build.py'}{' --diag' if DIAG else ''}` "
                        "(there is no PyTorch/CPU fallback for the training step)")
    lib = C.CDLL(str(LIB_PATH))
    lib.sdxl_last_error.restype = C.c_char_p
    lib.sdxl_last_error.argtypes = []
    sigs = dict(SIGNATURES)
    sigs.update(TEST_HOOK_SIGNATURES)
    if DIAG:
        sigs.update(DIAG_SIGNATURES)
    for name, args in sigs.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.argtypes = args
        fn.restype = C.c_int
    _lib = lib
    if DIAG:      # diagnostics build: SDXL_KNOBS=id=value,id=value preset the experiment knobs for the whole process (A/B runs of tools AND tests)
        for kv in os.environ.get("SDXL_KNOBS", "").split(","):
            if kv:
                rc = lib.sdxl_set_knob(int(kv.split("=")[0]), int(kv.split("=")[1]))
                if rc != 0:
                    raise SdxlError(f"SDXL_KNOBS: sdxl_set_knob({kv}) failed")
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().sdxl_last_error()
        raise SdxlError(f"{what or 'libsdxlstep'} failed (rc={rc}): {msg.decode() if msg else '?'}")


def call(name: str, *args) -> None:
    check(getattr(load(), name)(*args), name)
