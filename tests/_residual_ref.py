"""The oracle's UNet forward (oracle/unet_ref.py::unet_forward) restated with diffusers' additional residuals: after the whole down
path has run, down[i] is added to saved skip i (forward order) and mid to the mid block's output -- what UNet2DConditionModel does with
down_block_additional_residuals / mid_block_additional_residual.  Built from the oracle's own _resnet, _transformer, sincos and _Rounder;
differentiable in the residuals.  Without residuals it computes unet_forward bit for bit (tests/test_host_residuals.py asserts that).
With emulate_bf16 a sum with a residual is rounded once, as the library's concat does."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import unet_ref as U


def residual_shapes(cfg, B: int, H: int, W: int):
    """([(B, C_i, h_i, w_i)] of the skips in forward order, the mid block's shape)"""
    ch = cfg.block_out_channels
    out, h, w = [(B, ch[0], H, W)], H, W
    for i in range(len(ch)):
        out += [(B, ch[i], h, w)] * cfg.layers_per_block
        if i < len(ch) - 1:
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            out.append((B, ch[i], h, w))
    return out, (B, ch[-1], h, w)


def make_residuals(cfg, B: int, H: int, W: int, scale: float = 1.0, seed: int = 11, dtype=torch.float32):
    """bf16-representable scale * randn residuals for every skip and mid (the same values whatever dtype carries them)"""
    g = torch.Generator().manual_seed(seed)
    shapes, mid = residual_shapes(cfg, B, H, W)
    mk = lambda s: (scale * torch.randn(*s, generator=g)).to(torch.bfloat16).to(dtype)
    return [mk(s) for s in shapes], mk(mid)


def unet_forward(w, sample, timestep, encoder_hidden_states, text_embeds, time_ids, cfg, down=None, mid=None, emulate_bf16: bool = False):
    r = U._Rounder(emulate_bf16)
    ch = cfg.block_out_channels
    nlev = len(ch)
    B = sample.shape[0]
    x = sample.float()
    ehs = encoder_hidden_states.float()
    t = timestep.reshape(-1)
    if t.numel() == 1:
        t = t.expand(B)
    te = r(U.sincos(t, ch[0]))
    te = r(F.silu(F.linear(te, w["time_embedding.linear_1.weight"], w["time_embedding.linear_1.bias"])))
    te = F.linear(te, w["time_embedding.linear_2.weight"], w["time_embedding.linear_2.bias"])
    tid = r(U.sincos(time_ids.reshape(-1).float(), cfg.addition_time_embed_dim)).reshape(B, -1)
    aug = r(torch.cat([text_embeds.reshape(B, -1).float(), tid], dim=-1))
    aug = r(F.silu(F.linear(aug, w["add_embedding.linear_1.weight"], w["add_embedding.linear_1.bias"])))
    aug = F.linear(aug, w["add_embedding.linear_2.weight"], w["add_embedding.linear_2.bias"])
    emb_act = r(F.silu(r(te + aug)))

    x = r(F.conv2d(x, w["conv_in.weight"], w["conv_in.bias"], padding=1))
    skips = [x]
    for i in range(nlev):
        for j in range(cfg.layers_per_block):
            x = U._resnet(f"down_blocks.{i}.resnets.{j}", w, x, emb_act, cfg, cfg.resnet_eps, r)
            if cfg.transformer_layers_per_block[i] > 0:
                x = U._transformer(f"down_blocks.{i}.attentions.{j}", w, x, ehs, cfg.transformer_layers_per_block[i], cfg, r)
            skips.append(x)
        if i < nlev - 1:
            x = r(F.conv2d(x, w[f"down_blocks.{i}.downsamplers.0.conv.weight"], w[f"down_blocks.{i}.downsamplers.0.conv.bias"], stride=2, padding=1))
            skips.append(x)
    x = U._resnet("mid_block.resnets.0", w, x, emb_act, cfg, cfg.resnet_eps, r)
    x = U._transformer("mid_block.attentions.0", w, x, ehs, cfg.transformer_layers_per_block[-1], cfg, r)
    x = U._resnet("mid_block.resnets.1", w, x, emb_act, cfg, cfg.resnet_eps, r)
    # diffusers' two places: the saved skips after the whole down path, the mid block's output
    if down is not None:
        assert len(down) == len(skips)
        skips = [s if d is None else r(s + d.float()) for s, d in zip(skips, down)]
    if mid is not None:
        x = r(x + mid.float())
    for ui in range(nlev):
        lvl = nlev - 1 - ui
        for j in range(cfg.layers_per_block + 1):
            x = torch.cat([x, skips.pop()], dim=1)
            x = U._resnet(f"up_blocks.{ui}.resnets.{j}", w, x, emb_act, cfg, cfg.resnet_eps, r)
            if cfg.transformer_layers_per_block[lvl] > 0:
                x = U._transformer(f"up_blocks.{ui}.attentions.{j}", w, x, ehs, cfg.transformer_layers_per_block[lvl], cfg, r)
        if ui < nlev - 1:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = r(F.conv2d(x, w[f"up_blocks.{ui}.upsamplers.0.conv.weight"], w[f"up_blocks.{ui}.upsamplers.0.conv.bias"], padding=1))
    x = r(F.silu(F.group_norm(x, cfg.norm_num_groups, w["conv_norm_out.weight"], w["conv_norm_out.bias"], cfg.resnet_eps)))
    return F.conv2d(x, w["conv_out.weight"], w["conv_out.bias"], padding=1)
