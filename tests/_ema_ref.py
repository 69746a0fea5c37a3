"""CPU restatement of diffusers' EMAModel (training_utils.py: `get_decay`, `step`) -- the contract of the fused EMA of the weights
(sdxl-training-improvements_amd/ema.py, csrc/optimizer.hip `ema_update8`).  diffusers is not a dependency, so the two functions are
restated here in torch, in the same arithmetic: the decay in python doubles, the update on fp32 tensors with a python scalar."""
import torch


def get_decay(t, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3):
    """EMAModel.get_decay(optimization_step): t = optimizer steps so far, counting this one (1-based)"""
    step = max(0, t - update_after_step - 1)
    if step <= 0:
        return 0.0
    if use_ema_warmup:
        cur = 1 - (1 + step / inv_gamma) ** -power
    else:
        cur = (1 + step) / (10 + step)
    cur = min(cur, decay)
    cur = max(cur, min_decay)
    return cur


@torch.no_grad()
def step(ema: torch.Tensor, param: torch.Tensor, decay: float) -> torch.Tensor:
    """EMAModel.step for one tensor: `s_param.sub_(one_minus_decay * (s_param - param))`, in place on the fp32 `ema` (param is
    the bf16 weight; torch rounds the python scalar to float32 and rounds each of the three ops on its own)"""
    one_minus_decay = 1 - decay
    ema.sub_(one_minus_decay * (ema - param.float()))
    return ema
