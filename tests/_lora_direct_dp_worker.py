"""Worker of test_gpu_grad_select.py::test_two_ranks_exchange_direct_adapter_gradients_bit_equal_to_the_sum: one process per rank, both on
cuda:0, gloo.

Each rank runs one micro-step of a NativeLoRATrainer with lora_backward = "direct" on its own batch.  The backward scales by 1 / world and
writes the adapter gradients itself, so the trainer's _project() is its one all-reduce of the adapter-gradient arena: afterwards both ranks
must hold the same bits, and those must be the fp32 sum of the two ranks' own gradients."""
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
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
T = importlib.import_module("sdxl-training-improvements_amd.trainer")
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    D.init_process_group("gloo")
    torch.cuda.set_device(0)
    c = U.tiny_config()
    net = NU.NativeUNet(NU.make_config(block_out_channels=c.block_out_channels, transformer_layers=c.transformer_layers_per_block,
                                       cross_attention_dim=c.cross_attention_dim, addition_time_embed_dim=c.addition_time_embed_dim,
                                       pooled_dim=c.pooled_dim))
    net.load_state_dict(U.synth_weights(c, seed=0))
    cfg = CFG.Config()
    cfg.training.lora_rank = 4
    cfg.training.lora_backward = "direct"
    tr = T.create_trainer(SimpleNamespace(unet=net), config=cfg)
    ok = isinstance(tr, LORA.NativeLoRATrainer) and tr.sync.world == world == 2 and net.trainable() == set()
    g = torch.Generator().manual_seed(5)                       # the same adapters on both ranks
    for k in tr.lora.targets:
        tr.lora.B(k).copy_((torch.randn(tr.lora.B(k).shape, generator=g) * 0.02).to(torch.bfloat16))
    tr.lora.merge()
    tr.lora.grads.fill_(float("nan"))                          # the backward overwrites every gradient
    gb = torch.Generator().manual_seed(50 + rank)              # a different batch per rank
    r = lambda *s: torch.randn(*s, generator=gb)
    B, H, W = 2, 16, 16
    batch = {"vae_latents": r(B, 4, H, W), "prompt_embeds": r(B, 77, c.cross_attention_dim), "pooled_prompt_embeds": r(B, c.pooled_dim),
             "time_ids": torch.tensor([[128.0, 128, 0, 0, 128, 128]] * B), "metadata": {}}
    tr._execute_training_step(batch, timesteps=torch.tensor([650, 300]), noise=r(B, 4, H, W))
    torch.cuda.synchronize()
    own = tr.lora.grads.cpu().clone()                          # written by the backward: no projection
    written = torch.zeros(tr.lora.param_elems, dtype=torch.bool)
    for k in tr.lora.targets:
        a, b, o, i = tr.lora.layout[k]
        written[a: a + 4 * i] = True
        written[b: b + o * 4] = True
    ok = ok and bool(torch.isfinite(own[written]).all()) and bool(torch.isnan(own[~written]).all())
    tr.lora.grads[~written.to(tr.lora.grads.device)] = 0.0     # (the padding: NaN + NaN has no defined payload)
    own = tr.lora.grads.cpu().clone()
    tr._project()                                              # the one all-reduce
    torch.cuda.synchronize()
    got = tr.lora.grads.cpu().clone()
    owns = [torch.empty_like(own) for _ in range(world)]
    gots = [torch.empty_like(got) for _ in range(world)]
    dist.all_gather(owns, own)
    dist.all_gather(gots, got)
    bits = lambda t: t.view(torch.int32)
    ok = ok and not torch.equal(owns[0], owns[1]) and float(own.abs().max()) > 0
    ok = ok and torch.equal(bits(gots[0]), bits(gots[1])) and torch.equal(bits(got), bits(owns[0] + owns[1]))
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if rank == 0:
        print("LORA_DIRECT_DP_OK" if float(flag) == 1.0 else "LORA_DIRECT_DP_MISMATCH", flush=True)
    dist.barrier()
    net.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
