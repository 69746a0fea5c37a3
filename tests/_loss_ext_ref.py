"""CPU restatement of the device loss with per-sample weights, per-sample losses and the selectable element loss
(csrc/loss.hip, include/sdxlstep.h) -- the contract the GPU tests check the kernels against.  Not a test module.

Written in torch and differentiable in `pred`, in whatever dtype `pred` has (the tests use float64 for the limit checks and
for the reference of the fp32 device sums), so d(loss)/d(pred) comes out of autograd and can be compared with the closed form.

With d = pred - target, s_b the per-sample weight (1 when absent), w_b the MinSNR factor (1 when off / flow matching) and c_b
the per-sample Huber parameter:

    l2         l(d) = d^2                          l'(d) = 2 d
    huber      l(d) = 2 c (sqrt(d^2 + c^2) - c)    l'(d) = 2 c d / sqrt(d^2 + c^2)
    smooth_l1  l(d) = 2 (sqrt(d^2 + c^2) - c)      l'(d) = 2 d / sqrt(d^2 + c^2)

    L_b  = s_b w_b mean_chw l(d)                               (per-sample loss, before the tag mean and the guard)
    raw  = sum_b sum_chw (s_b w_b) l(d)
    loss = guard(raw / numel * mean(tag_w))                    (guard: non-finite -> 1000, no gradient; clamp(max = 1000))
    dpred = gate * grad_scale * (s_b w_b) l'(d) / numel        (gate = mean(tag_w) when the guard passes the loss through, else 0)
"""
from typing import Optional, Union

import torch

LOSS_TYPES = ("l2", "huber", "smooth_l1")
LOSS_CAP = 1000.0
Scalar = Union[float, torch.Tensor]


def _col(v: Scalar, like: torch.Tensor) -> torch.Tensor:
    """a scalar or a [B] tensor as a [B,1,1,1] (or 0-d) tensor of `like`'s dtype"""
    t = torch.as_tensor(v, dtype=like.dtype)
    return t.view(-1, 1, 1, 1) if t.dim() else t


def element_loss(d: torch.Tensor, loss_type: str = "l2", c: Scalar = 0.0) -> torch.Tensor:
    if loss_type == "l2":
        return d * d
    cc = _col(c, d)
    q = d * d / (torch.sqrt(d * d + cc * cc) + cc)          # sqrt(d^2 + c^2) - c without the cancellation for |d| << c
    if loss_type == "huber":
        return 2.0 * cc * q
    if loss_type == "smooth_l1":
        return 2.0 * q
    raise ValueError(loss_type)


def element_loss_grad(d: torch.Tensor, loss_type: str = "l2", c: Scalar = 0.0) -> torch.Tensor:
    """closed-form l'(d)"""
    if loss_type == "l2":
        return 2.0 * d
    cc = _col(c, d)
    r = torch.sqrt(d * d + cc * cc)
    if loss_type == "huber":
        return 2.0 * cc * d / r
    if loss_type == "smooth_l1":
        return 2.0 * d / r
    raise ValueError(loss_type)


def target_and_weight(method: str, latents: torch.Tensor, noise: torch.Tensor, sigma_or_t: torch.Tensor,
                      prediction_type: str = "v_prediction", min_snr_gamma: Optional[float] = 5.0):
    """target [B,4,H,W] and w_b [B] exactly as the device computes them today (ddpm: the trainer's velocity / epsilon target and
    min(sigma^-2, gamma); flow matching: x1 - x0 and 1), in the dtype of `latents`"""
    B = latents.shape[0]
    if method == "flow_matching":
        return latents - noise, torch.ones(B, dtype=latents.dtype)
    sig = sigma_or_t.to(latents.dtype)
    target = (noise - latents) / torch.sqrt(sig * sig).view(-1, 1, 1, 1) if prediction_type == "v_prediction" else noise
    if min_snr_gamma is None:
        return target, torch.ones(B, dtype=latents.dtype)
    snr = (1.0 / sig) ** 2
    return target, torch.minimum(snr, torch.full_like(snr, float(min_snr_gamma)))


def per_sample_loss(pred, target, w, sample_weights=None, loss_type="l2", c: Scalar = 0.0) -> torch.Tensor:
    """L_b [B]"""
    sw = w if sample_weights is None else sample_weights.to(pred.dtype) * w
    return sw * element_loss(pred - target, loss_type, c).mean(dim=(1, 2, 3))


def loss(pred, target, w, sample_weights=None, loss_type="l2", c: Scalar = 0.0, tag_weights=None) -> torch.Tensor:
    """the guarded scalar (out[0]); differentiable in `pred` where the guard passes it through"""
    l = per_sample_loss(pred, target, w, sample_weights, loss_type, c).mean()
    if tag_weights is not None:
        l = l * tag_weights.to(pred.dtype).mean()
    if not torch.isfinite(l):
        return torch.tensor(LOSS_CAP, dtype=pred.dtype)
    return torch.clamp(l, max=LOSS_CAP)


def dpred(pred, target, w, sample_weights=None, loss_type="l2", c: Scalar = 0.0, tag_weights=None, grad_scale: float = 1.0):
    """closed-form d(grad_scale * loss)/d(pred); zero where the guard takes over"""
    raw = per_sample_loss(pred.detach(), target, w, sample_weights, loss_type, c).mean()
    tm = 1.0 if tag_weights is None else float(tag_weights.to(pred.dtype).mean())
    if not torch.isfinite(raw * tm) or float(raw * tm) > LOSS_CAP:
        return torch.zeros_like(pred)
    sw = w if sample_weights is None else sample_weights.to(pred.dtype) * w
    return tm * grad_scale * sw.view(-1, 1, 1, 1) * element_loss_grad(pred - target, loss_type, c) / pred.numel()
