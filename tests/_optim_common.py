"""What the optimizer and EMA tests share (a plain helper module, imported by name): the stand-ins for the native UNet that the
fused optimizers, the EMA and the trainer accept, and the bit-pattern / pointer helpers of the tests that call the C ABI."""
import ctypes as C

import numpy as np
import torch

from sdxl_amd import lib


def dev():
    return torch.device("cuda:0")


def to_dev_bits(a):          # uint16 bit patterns -> bf16 device tensor
    return torch.from_numpy(a.astype(np.int16)).to(dev()).view(torch.bfloat16)


def bits(t):
    """the bit patterns of a bf16 tensor (uint16) or an fp32 one (int32) as a numpy array"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().astype(np.uint16) if t.dtype == torch.bfloat16 else t.view(torch.int32).numpy()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Arena:
    """the arena surface the optimizers and the EMA read, on the device of `w`: weights (bf16, a copy of w) + fp32 gradients + the
    library; param_ranges {name: (offset, count)}: the "tensors" of AdamWBF16's lazy-decay bookkeeping (none by default)"""

    def __init__(self, w, param_ranges=None):
        self.L = lib.load()
        self.weights = w.clone()
        self.grads = torch.zeros(w.numel(), dtype=torch.float32, device=w.device)
        self._ranges = dict(param_ranges or {})

    def param_ranges(self):
        return dict(self._ranges)

    def zero_grads(self):
        self.grads.zero_()


class StandInNet:
    """the surface the optimizers, the EMA and the trainer read, on the CPU (no library unless one is handed in)"""

    def __init__(self, n=64, L=None):
        self.param_elems = n
        self.weights = (torch.arange(n, dtype=torch.float32) * 0.01).to(torch.bfloat16)
        self.grads = torch.zeros(n)
        self.L = L

    def zero_grads(self):
        pass

    def forward_loss(self, *a, **k):
        pass

    def backward(self, *a, **k):
        pass

    def read_loss(self):
        return [0.0] * 8
