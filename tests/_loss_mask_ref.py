"""CPU restatement of the masked device loss and of the loss preparation with a separate input noise (csrc/loss.hip,
include/sdxlstep.h), on top of _loss_ext_ref.py -- the contract the GPU tests check the kernels against.  Not a test module.

With m >= 0 the mask value of a latent pixel (all four channels), M_b = sum_hw m, and d, s_b, w_b, l, l' and the guard as in
_loss_ext_ref.py, m joins the weight first, (s_b w_b) m:

    mean         L_b  = s_b w_b sum_chw m l(d) / (4 HW)
                 loss = guard(mean_b L_b * mean(tag_w))                  (= raw / numel * mean(tag_w), raw = sum (s_b w_b m) l(d))
                 dpred = gate * grad_scale * (s_b w_b m) l'(d) / numel
    masked_mean  L_b  = s_b w_b sum_chw m l(d) / (4 M_b)                 (0 when M_b = 0)
                 loss = guard(mean_b L_b * mean(tag_w))
                 dpred = gate * grad_scale * (s_b w_b m) l'(d) / (B 4 M_b)   (0 when M_b = 0)

Differentiable in `pred`, in whatever dtype `pred` has, like _loss_ext_ref.py."""
import torch

import _loss_ext_ref as X

MASK_NORMS = ("mean", "masked_mean")
LOSS_CAP = X.LOSS_CAP


def _weights(pred, w, sample_weights):
    return w if sample_weights is None else sample_weights.to(pred.dtype) * w


def _denominator(pred, mask, mask_norm):
    """[B]: what each sample's masked sum is divided by, and which samples have one at all"""
    B, C, H, W = pred.shape
    if mask_norm == "mean":
        return torch.full((B,), float(C * H * W), dtype=pred.dtype), torch.ones(B, dtype=torch.bool)
    if mask_norm != "masked_mean":
        raise ValueError(mask_norm)
    M = mask.to(pred.dtype).sum(dim=(1, 2))
    live = M > 0
    return torch.where(live, C * M, torch.ones_like(M)), live


def per_sample_loss(pred, target, w, mask, mask_norm="mean", sample_weights=None, loss_type="l2", c=0.0) -> torch.Tensor:
    """L_b [B]; mask [B,H,W]"""
    m = mask.to(pred.dtype).unsqueeze(1)
    s = (m * X.element_loss(pred - target, loss_type, c)).sum(dim=(1, 2, 3))
    den, live = _denominator(pred, mask, mask_norm)
    return torch.where(live, _weights(pred, w, sample_weights) * s / den, torch.zeros_like(s))


def loss(pred, target, w, mask, mask_norm="mean", sample_weights=None, loss_type="l2", c=0.0, tag_weights=None) -> torch.Tensor:
    """the guarded scalar (out[0]); differentiable in `pred` where the guard passes it through"""
    l = per_sample_loss(pred, target, w, mask, mask_norm, sample_weights, loss_type, c).mean()
    if tag_weights is not None:
        l = l * tag_weights.to(pred.dtype).mean()
    if not torch.isfinite(l):
        return torch.tensor(LOSS_CAP, dtype=pred.dtype)
    return torch.clamp(l, max=LOSS_CAP)


def dpred(pred, target, w, mask, mask_norm="mean", sample_weights=None, loss_type="l2", c=0.0, tag_weights=None,
          grad_scale: float = 1.0) -> torch.Tensor:
    """closed-form d(grad_scale * loss)/d(pred); zero where the guard takes over, where m = 0 and for a sample with M_b = 0"""
    raw = per_sample_loss(pred.detach(), target, w, mask, mask_norm, sample_weights, loss_type, c).mean()
    tm = 1.0 if tag_weights is None else float(tag_weights.to(pred.dtype).mean())
    if not torch.isfinite(raw * tm) or float(raw * tm) > LOSS_CAP:
        return torch.zeros_like(pred)
    B = pred.shape[0]
    den, live = _denominator(pred, mask, mask_norm)
    k = torch.where(live, tm * grad_scale * _weights(pred, w, sample_weights) / (B * den), torch.zeros_like(den))
    m = mask.to(pred.dtype).unsqueeze(1)
    g = k.view(-1, 1, 1, 1) * m * X.element_loss_grad(pred - target, loss_type, c)
    return torch.where(m > 0, g, torch.zeros_like(g))


def prepare(method: str, latents, noise_in, sigma_or_t, use_ztsnr: bool = True) -> torch.Tensor:
    """the UNet input [B,4,H,W] bf16 the loss preparation writes, built from `noise_in`: fp32, every product and sum rounded on
    its own (separate torch ops), then round-to-nearest-even to bf16"""
    x, n = latents.float(), noise_in.float()
    s = sigma_or_t.float().view(-1, 1, 1, 1)
    if method == "flow_matching":
        v = (1.0 - s) * n + s * x
    else:
        v = s * n + x
        if use_ztsnr:
            v = v.clamp(-20000.0, 20000.0)
    return v.to(torch.bfloat16)
