"""Worker of tests/test_gpu_sampler.py::test_zero1_ema_sampling_needs_prepare_checkpoint (one process per rank, all on cuda:0, gloo).

The trainer with training.use_ema on the tiny UNet under ZeRO-1 (the gradients come from a seeded generator instead of a backward, as in
tests/_ema_zero1_worker.py): after an optimizer step each rank's EMA is current on its own slices only, so sample(weights="ema") and
evaluate(weights="ema") must raise RuntimeError naming prepare_checkpoint(), and the trained weights must still be sampled; after
prepare_checkpoint() on every rank both work and every rank gets the same bits."""
import importlib
import os
import sys
from pathlib import Path
from types import SimpleNamespace

import torch
import torch.distributed as dist

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import sdxl_amd  # noqa: E402,F401
from oracle import unet_ref as U  # noqa: E402
from sdxl_amd import unet as NU  # noqa: E402

D = importlib.import_module("sdxl-training-improvements_amd.distributed")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
CFG = importlib.import_module("sdxl-training-improvements_amd.config")


class TorchUNetStandIn:
    def __init__(self, sd):
        self.sd = {k: v.to(torch.bfloat16).clone() for k, v in sd.items()}

    def state_dict(self):
        return self.sd

    def load_state_dict(self, sd, strict=True):
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
    c = CFG.Config()
    c.training.clip_grad_norm = 0.0
    c.training.use_ema, c.training.ema_update_after_step = True, 0
    c.training.validation_num_steps = 2
    c.optimizer.learning_rate = 1e-2
    tr = T.NativeSDXLTrainer(SimpleNamespace(unet=TorchUNetStandIn(U.synth_weights(ucfg, seed=0))), config=c, device=dev,
                             native_factory=lambda _c: net, native_config=net.cfg)
    ok = tr.sharded and tr.ema is not None
    total, segs = net.param_elems, net.segment_ranges()
    for step in range(2):
        g = torch.randn(total, generator=torch.Generator().manual_seed(100 * step + rank)).to(dev) * 1e-2
        tr.sync.cast = lambda off, n, dst, g=g: dst.copy_((g[off:off + n] * (1.0 / world)).to(torch.bfloat16))
        for k, (off, n) in enumerate(segs):
            tr.sync.on_segment(k, off, n)
        tr.optimizer_step()
    torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=gen)
    pe, po = r(2, 77, ucfg.cross_attention_dim), r(2, ucfg.pooled_dim)
    ti = torch.tensor([[128.0, 128, 0, 0, 128, 128]] * 2)
    noise = r(2, 4, 16, 16)
    batch = {"vae_latents": r(2, 4, 16, 16), "prompt_embeds": pe, "pooled_prompt_embeds": po, "time_ids": ti, "metadata": {}}
    sample = lambda w: tr.sample(pe, po, ti, height=16, width=16, noise=noise, weights=w)
    evaluate = lambda w: tr.evaluate([batch], [500], torch.Generator().manual_seed(2), weights=w)
    w_before = net.weights.clone()
    ok = ok and refuses(lambda: sample("ema")) and refuses(lambda: evaluate("ema")) and refuses(lambda: sample(None))
    ok = ok and bool(torch.isfinite(sample("trained")).all()) and torch.equal(net.weights, w_before)
    if not ok:
        print(f"rank {rank}: the EMA was sampled before prepare_checkpoint(), or the trained weights were not", flush=True)
    tr.prepare_checkpoint()                              # collective: every rank
    lat = sample("ema")
    per_t, mean = evaluate("ema")
    ok = ok and bool(torch.isfinite(lat).all()) and mean == mean and torch.equal(net.weights, w_before)
    ok = ok and not torch.equal(lat, sample("trained"))
    both = [torch.zeros_like(lat.cpu()) for _ in range(world)]
    dist.all_gather(both, lat.cpu())
    ok = ok and all(torch.equal(both[0], b) for b in both)
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        print("SAMPLER_ZERO1_OK" if float(flag) == 1.0 else "SAMPLER_ZERO1_MISMATCH", flush=True)
    dist.barrier()
    tr.ema.close()
    net.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
