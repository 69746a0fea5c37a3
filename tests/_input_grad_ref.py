"""The input gradient of conv_in (csrc/input_dgrad.hip) in float64, written from the formula of include/sdxlstep.h on the arena's layouts:

    dx[b][c][y][x] = sum_{ky, kx in 0..2} sum_{o < Cout} dy[b][y + 1 - ky][x + 1 - kx][o] * w[o][3 ky + kx][c]     (pixels outside the image: nothing)

    dy [B * H * W][Cout]   conv_in's output gradient, token-major
    w  [Cout][9][Cs]       the arena's conv_in: Cs = 8 for in_channels <= 8, else 16, pad channels zero
    dx [B][in_channels][H][W]

tests/test_host_input_grad.py checks it against torch.autograd.grad of F.conv2d(x, w, padding=1); tests/test_gpu_input_grad.py holds the
kernel to it.  No GPU needed."""
from __future__ import annotations

import torch
import torch.nn.functional as F

import _exact as E


def input_cs(in_channels: int) -> int:
    return 8 if in_channels <= 8 else 16


def arena_weight(w_nchw: torch.Tensor) -> torch.Tensor:
    """[Cout][in_channels][3][3] -> the arena's [Cout][9][Cs] with zero pad channels"""
    cout, cin = w_nchw.shape[:2]
    out = torch.zeros(cout, 9, input_cs(cin), dtype=w_nchw.dtype)
    out[:, :, :cin] = w_nchw.permute(0, 2, 3, 1).reshape(cout, 9, cin)
    return out


def input_dgrad_ref64(dy, w, B: int, H: int, W: int, in_channels: int, absolute: bool = False) -> torch.Tensor:
    """dx [B][in_channels][H][W] in float64; absolute: the same sum on absolute values (the parenthesis of _exact.bound)"""
    cout = dy.shape[1]
    assert tuple(dy.shape) == (B * H * W, cout) and tuple(w.shape) == (cout, 9, input_cs(in_channels))
    d, k = dy.double().reshape(B, H, W, cout), w.double()
    if absolute:
        d, k = d.abs(), k.abs()
    dp = F.pad(d, (0, 0, 1, 1, 1, 1))      # one pixel of zeros around every sample: what lies outside the image contributes nothing
    dx = torch.zeros(B, H, W, k.shape[2], dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            src = dp[:, 2 - ky: 2 - ky + H, 2 - kx: 2 - kx + W, :]      # pixel (y + 1 - ky, x + 1 - kx), in padded coordinates
            dx += src @ k[:, 3 * ky + kx, :]
    return dx[..., :in_channels].permute(0, 3, 1, 2).contiguous()


def operands(B: int, H: int, W: int, in_channels: int, cout: int, integer: bool, seed: int = 0):
    """CPU float32 (dy [B * H * W][cout], w [cout][9][Cs] with zero pad channels): integers of {-2 .. 2} | bf16-rounded randn (w scaled by
    (9 cout)^-1/2, as tests/test_gpu_ops.py scales a weight by its reduction length)"""
    s = 1000 * seed
    if integer:
        dy, wn = E.ints(B * H * W, cout, seed=s + 1), E.ints(cout, in_channels, 3, 3, seed=s + 2)
    else:
        dy, wn = E.rnd(B * H * W, cout, seed=s + 1), E.rnd(cout, in_channels, 3, 3, seed=s + 2, scale=(9 * cout) ** -0.5)
    return dy, arena_weight(wn)
