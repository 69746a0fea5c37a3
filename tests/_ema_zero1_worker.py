"""Worker of tests/test_gpu_ema.py::test_zero1_ema_bit_equal_to_unsharded (one process per rank, all on cuda:0, gloo).

Path A is the trainer itself with training.use_ema on the tiny UNet (its real arena, segments and layout; the gradients come from a
seeded generator instead of a backward): bucketed reduce-scatter -> `optimizer_step()` (AdamW_BF16 and the fused EMA on this rank's
slices, all-gather of the parameters) -> `prepare_checkpoint()`.  Path B is bucketed all-reduce -> the same update with its own EMA
over the whole arena.  After three updates and prepare_checkpoint() the weights, the optimizer state and the EMA must be
bit-identical on every rank.  Before prepare_checkpoint() the EMA must not be (only the owned slices are current), and every reader
of it -- ema_state_dict(), sync_to_model(ema=True), a save -- must refuse; after it they must work."""
import importlib
import os
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace

import torch
import torch.distributed as dist

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import sdxl_amd  # noqa: E402,F401
from oracle import unet_ref as U  # noqa: E402
from sdxl_amd import unet as NU  # noqa: E402

from _optim_common import Arena  # noqa: E402

D = importlib.import_module("sdxl-training-improvements_amd.distributed")
O = importlib.import_module("sdxl-training-improvements_amd.optimizer")
E = importlib.import_module("sdxl-training-improvements_amd.ema")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
CFG = importlib.import_module("sdxl-training-improvements_amd.config")


class TorchUNetStandIn:
    """what sync_to_model writes into: a diffusers-keyed state_dict() / load_state_dict() in bf16"""

    def __init__(self, sd):
        self.sd = {k: v.to(torch.bfloat16).clone() for k, v in sd.items()}

    def state_dict(self):
        return self.sd

    def load_state_dict(self, sd, strict=True):
        assert set(sd) == set(self.sd)
        self.sd = {k: v.clone() for k, v in sd.items()}


def refuses(fn):
    try:
        fn()
    except RuntimeError as e:
        return "prepare_checkpoint" in str(e)
    return False


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    D.init_process_group("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ucfg = U.tiny_config()
    net = NU.NativeUNet(NU.make_config(block_out_channels=ucfg.block_out_channels, transformer_layers=ucfg.transformer_layers_per_block,
                                       cross_attention_dim=ucfg.cross_attention_dim,
                                       addition_time_embed_dim=ucfg.addition_time_embed_dim, pooled_dim=ucfg.pooled_dim), 0)
    torch_unet = TorchUNetStandIn(U.synth_weights(ucfg, seed=0))
    c = CFG.Config()
    c.training.clip_grad_norm = 0.0                     # the unclipped update on both paths
    c.training.use_ema, c.training.ema_update_after_step = True, 1
    c.optimizer.learning_rate = 1e-2
    tr = T.NativeSDXLTrainer(SimpleNamespace(unet=torch_unet), config=c, device=dev, native_factory=lambda _c: net,
                             native_config=net.cfg)
    total = net.param_elems
    segs = net.segment_ranges()                          # exchange order
    # path B: the weight arena, gradients and tensor ranges (the lazy per-tensor decay) of the same UNet, without its handle
    net_f = Arena(net.weights, net.param_ranges())
    opt_f = O.AdamWBF16(net_f, lr=1e-2, weight_decay=c.optimizer.weight_decay)
    ema_f = E.WeightEMA(net_f, update_after_step=1)
    opt_f.attach_ema(ema_f)
    ok = tr.sharded and tr.ema is not None and tr.optimizer.ema is tr.ema
    if not ok:
        print(f"rank {rank}: trainer not sharded or without EMA", flush=True)
    fs = None
    for step in range(3):
        g = torch.randn(total, generator=torch.Generator().manual_seed(100 * step + rank)).to(dev) * 3.0

        def cast(off, n, dst, g=g):
            dst.copy_((g[off:off + n] * (1.0 / world)).to(torch.bfloat16))

        if fs is None:
            fs = D.GradSync(total, cast, torch.bfloat16, dev)
        tr.sync.cast = fs.cast = cast
        for k, (off, n) in enumerate(segs):
            tr.sync.on_segment(k, off, n)
        tr.optimizer_step()                              # finish, update of the owned slices (+ EMA), all-gather of the weights
        for k, (off, n) in enumerate(segs):
            fs.on_segment(k, off, n)
        fs.finish()
        opt_f.step(fs.reduced())
        torch.cuda.synchronize()
        ok = ok and torch.equal(net.weights, net_f.weights)
        for off, n, _ in tr.sync.pieces:                 # the owned slices are current at every step
            ok = ok and torch.equal(tr.ema.arena[off:off + n], ema_f.arena[off:off + n])
        if not ok:
            print(f"rank {rank} step {step}: mismatch", flush=True)
    # ---- before the gather: the other ranks' slices are stale, and every reader of the EMA refuses
    ok_pre = not torch.equal(tr.ema.arena, ema_f.arena)
    synced_before = {k: v.clone() for k, v in torch_unet.sd.items()}
    ok_pre = ok_pre and refuses(tr.ema_state_dict) and refuses(lambda: tr.sync_to_model(ema=True))
    ok_pre = ok_pre and all(torch.equal(torch_unet.sd[k], v) for k, v in synced_before.items())
    if rank == 0:
        with tempfile.TemporaryDirectory() as d:
            ok_pre = ok_pre and refuses(lambda: tr.save_ema_state(d)) and not (Path(d) / "ema.json").exists()
    if not ok_pre:
        print(f"rank {rank}: the EMA was read before prepare_checkpoint()", flush=True)
    ok = ok and ok_pre
    # ---- the gather, then the same bits as path B and readers that work
    tr.prepare_checkpoint()                              # collective: every rank
    torch.cuda.synchronize()
    ok = ok and torch.equal(tr.ema.arena, ema_f.arena) and tr.ema.optimization_step == ema_f.optimization_step == 3
    ok = ok and not torch.equal(ema_f.arena, net_f.weights.float())
    for a, b in zip(tr.optimizer.state_arenas(), opt_f.state_arenas()):
        ok = ok and torch.equal(a, b)
    sd = tr.ema_state_dict()
    tr.sync_to_model(ema=True)
    ok = ok and set(sd) == set(torch_unet.sd) and all(torch.equal(torch_unet.sd[k], v.to(torch.bfloat16).cpu()) for k, v in sd.items())
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        print("EMA_ZERO1_OK" if float(flag) == 1.0 else "EMA_ZERO1_MISMATCH", flush=True)
    dist.barrier()
    tr.ema.close()
    net.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
