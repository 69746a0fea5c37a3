"""Real widths at the default buckets' two new row-count families (latent 104 x 152: 15 808 / 3952 / 988 pixels per sample; latent
80 x 192: 15 360 / 3840 / 960), on a real-width SHALLOW UNet.

The engine's choices that depend on a layer's widths -- the co-resident 256-row and the long-reduction weight gradients, the Delta
epilogue of the out-projection dgrad (C % 128 == 0), grouped weight gradients, the split-K of small-M problems, the zero-pad rows of
the linear weight gradients -- cannot be reached at the tiny model's widths, and do not depend on depth.  So: every field of
oracle.unet_ref.SDXL_BASE except transformer_layers_per_block = (0, 1, 1), 641 M parameters, synthetic weights.

  * B = 1 against the fp32 CPU oracle, loss and every gradient tensor (bars of tests/test_gpu_fullsize.py, imported);
  * B = 4 (what training and bench.py run: rows 3952 / 15 808 / 63 232) tied to B = 1 through the decomposition property, every tensor;
  * two plans, (4, 104, 152) and (4, 128, 128), alternating over accumulated micro-steps: a workspace or slab sized for the wrong plan,
    or pad rows left over from the other plan, would show here.

The oracle cases are the one place where a test is not a few seconds: fp32 autograd through 641 M parameters on the host CPU; their
wall time is printed."""
import math
import os
import time

import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import loss_ref as R
from oracle import unet_ref as U
from sdxl_amd import unet as NU

import _bucket_cases as BK
from _gradparity import GradParity, compare_autograd
from _isolation import assert_step_isolated
from test_gpu_fullsize import _grad_bar, _inputs      # the full-size tests' bars (TIGHT_GRAD_BAR / FULL_GRAD_BAR by role group) and inputs

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-3                                           # north_star: the loss against the fp32 CPU reference arithmetic
SHALLOW = U.UNetConfig(transformer_layers_per_block=(0, 1, 1))


@pytest.fixture(scope="module")
def shallow():
    n = len(os.sched_getaffinity(0))                       # the CPUs this process may run on, not the machine's count
    if os.environ.get("OMP_NUM_THREADS", "").isdigit():
        n = min(n, max(1, int(os.environ["OMP_NUM_THREADS"])))
    torch.set_num_threads(n)
    w = U.synth_weights(SHALLOW, seed=0)
    net = NU.NativeUNet(NU.make_config(transformer_layers=SHALLOW.transformer_layers_per_block))
    assert net.param_shapes() == {k: tuple(v) for k, v in U.param_shapes(SHALLOW).items()}
    assert 640e6 < net.param_elems < 643e6
    net.load_state_dict(w)
    yield w, net
    net.close()


@pytest.mark.parametrize("B,H,W", BK.SHALLOW_ORACLE, ids=lambda v: str(v))
def test_shallow_b1_loss_and_every_gradient_match_cpu_oracle(shallow, B, H, W):
    """Flow matching, one sample: loss <= 1e-3 and every gradient tensor against autograd of the fp32 oracle (biases, convs and the
    time-embedding path at TIGHT_GRAD_BAR, linears and norms at FULL_GRAD_BAR)."""
    w, net = shallow
    x = _inputs(B, H, W, seed=2000 + H)
    t = torch.tensor([0.3671875])                          # exactly representable in bf16 (t reaches the UNet in model dtype)
    for p in w.values():
        p.grad = None
        p.requires_grad_(True)
    t0 = time.perf_counter()
    try:
        unet_fn = lambda s, tt, e, p, ti: U.unet_forward(w, s, tt, e, p, ti, SHALLOW)
        batch = {"vae_latents": x["lat"], "prompt_embeds": x["ehs"], "pooled_prompt_embeds": x["pooled"], "time_ids": x["tid"]}
        net.zero_grads()
        net.forward_loss("flow_matching", x["lat"], x["noise"], t, t, x["ehs"], x["pooled"], x["tid"])
        net.backward(1.0, True)
        got = net.read_loss()[0]
        ref = R.compute_loss_flow(unet_fn, batch, x["noise"], t)
        ref_loss = float(ref["loss"].detach())
        rel = abs(got - ref_loss) / abs(ref_loss)
        print(f"[parity] shallow real-width {B}x{H}x{W} flow_matching loss: hip {got:.6e} oracle {ref_loss:.6e} rel {rel:.3e} (tol {LOSS_RTOL})")
        par = GradParity(f"shallow real-width flow_matching {B}x{H}x{W}")
        compare_autograd(par, ref["loss"], {k: w[k] for k in net.param_shapes()}, lambda k: net.export(k, grad=True))
    finally:
        for p in w.values():
            p.grad = None
            p.requires_grad_(False)
    print(f"[parity] shallow real-width {B}x{H}x{W}: step + fp32 CPU oracle forward and backward took {time.perf_counter() - t0:.1f} s")
    assert rel <= LOSS_RTOL
    par.check(_grad_bar(net.param_shapes()), expect=net.param_shapes())


@pytest.mark.parametrize("B,H,W", BK.SHALLOW_DECOMPOSE, ids=lambda v: str(v))
def test_shallow_batch4_every_gradient_decomposes(shallow, B, H, W):
    """The form and the bar of test_batch4_every_gradient_decomposes, no oracle involved: every tensor of the B = 4 gradient arena equals
    the 1/B-weighted sum of the four per-sample steps' arenas, and the batch loss the mean of the per-sample losses."""
    _, net = shallow
    x = _inputs(B, H, W, seed=303 + H)
    t = torch.sigmoid(torch.randn(B, generator=torch.Generator().manual_seed(9)))

    def run(idx, scale, first):
        s = slice(idx, idx + 1) if idx is not None else slice(None)
        net.forward_loss("flow_matching", x["lat"][s], x["noise"][s], t[s], t[s], x["ehs"][s], x["pooled"][s], x["tid"][s])
        net.backward(scale, first)
        return net.read_loss()[0]

    net.zero_grads()
    lb = run(None, 1.0, True)
    gb = net.grads.clone()
    net.zero_grads()
    ls = [run(i, 1.0 / B, i == 0) for i in range(B)]
    torch.cuda.synchronize()
    mean = sum(ls) / B
    print(f"[parity] shallow flow matching {B}x{H}x{W}: batch loss {lb:.6f} mean of per-sample {mean:.6f} rel {abs(lb - mean) / abs(lb):.3e}")
    par = GradParity(f"shallow B=4 decomposition flow_matching {B}x{H}x{W}")
    par.add_arena(net.grads, gb, net.param_ranges(), net.param_shapes())
    del gb
    assert math.isfinite(lb) and 0 < lb < 1000
    assert abs(lb - mean) <= 1e-3 * abs(lb)
    par.check(_grad_bar(net.param_shapes()), expect=net.param_shapes())


def test_shallow_mixed_buckets_accumulate_across_plans(shallow):
    """The form of test_configs4_mixed_buckets_accumulate_across_plans on the whole arena: two plans share the weights, the gradient arena
    and the workspace; four micro-steps alternating between them (A B A B and B A B A, four different inputs) accumulate the sum of the
    four steps' own gradients.  Same kernels in the same order on both sides: only the association of four fp32 additions differs."""
    _, net = shallow
    shapes = [BK.SHALLOW_MIXED[i % 2] for i in range(4)]
    xs = [_inputs(*s, seed=1410 + i) for i, s in enumerate(shapes)]
    ts = [torch.tensor([0.15, 0.4, 0.65, 0.9]), torch.tensor([0.1, 0.35, 0.6, 0.85]), torch.tensor([0.2, 0.45, 0.7, 0.95]),
          torch.tensor([0.05, 0.3, 0.55, 0.8])]

    def micro(i, first):
        x, t = xs[i], ts[i]
        net.forward_loss("flow_matching", x["lat"], x["noise"], t, t, x["ehs"], x["pooled"], x["tid"])
        net.backward(0.25, first)
        return net.read_loss()[0]

    want = torch.zeros_like(net.grads)
    own = []
    for i in range(4):
        net.zero_grads()
        own.append(micro(i, True))
        torch.cuda.synchronize()
        want += net.grads
    ranges, pshapes = net.param_ranges(), net.param_shapes()
    for order in ((0, 1, 2, 3), (1, 0, 3, 2)):
        net.zero_grads()
        losses = [micro(i, j == 0) for j, i in enumerate(order)]
        torch.cuda.synchronize()
        assert losses == [own[i] for i in order], (order, losses, own)      # the forward does not depend on the plan that ran before
        par = GradParity(f"shallow mixed buckets order {order}")
        par.add_arena(net.grads, want, ranges, pshapes)
        par.check((1e-5, 1.0 - 1e-9), expect=pshapes)


def test_shallow_step_does_not_depend_on_workspace_or_stale_gradients(shallow):
    """The form of tests/test_gpu_model.py::test_step_does_not_depend_on_workspace_or_stale_gradients at real widths, clean against 0xFF:
    the routes no tiny width reaches (co-resident 256-row tiles, the long-reduction and grouped weight gradients, the Delta epilogue, the
    split-K of small-M problems) on a workspace and a gradient arena of NaN.  No oracle: two steps."""
    _, net = shallow
    B, H, W = 1, 104, 152
    x = _inputs(B, H, W, seed=4100)
    t = torch.tensor([0.3671875])
    step = lambda: net.forward_loss("flow_matching", x["lat"], x["noise"], t, t, x["ehs"], x["pooled"], x["tid"])
    assert_step_isolated(net, (B, H, W), [step], fills=(0x00, 0xFF), what=f"shallow flow_matching {B}x{H}x{W}")
