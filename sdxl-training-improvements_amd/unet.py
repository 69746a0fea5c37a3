"""Host-side owner of one libsdxlstep handle: packed parameters, plans per bucket shape, the training step.

Replaces what the reference reaches through `model.unet` (models/sdxl.py:40-62): parameters()/state_dict(),
the forward call at ddpm_trainer.py:320-325 / flow_matching_trainer.py:400-405, and loss.backward().
PyTorch is used for device memory and streams only; every FLOP of the step runs in libsdxlstep.so.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Iterable, Optional, Tuple

import torch

from . import lib

SDXL_BASE_CFG = dict(in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280), layers_per_block=2,
                     transformer_layers=(0, 2, 10), head_dim=64, cross_attention_dim=2048, norm_num_groups=32,
                     addition_time_embed_dim=256, pooled_dim=1280, resnet_eps=1e-5, tf_gn_eps=1e-6, ln_eps=1e-5)

METHODS = {"ddpm": 0, "flow_matching": 1}
PRED_TYPES = {"epsilon": 0, "v_prediction": 1}


def make_config(**over) -> lib.UNetConfig:
    d = dict(SDXL_BASE_CFG)
    d.update(over)
    c = lib.UNetConfig()
    for k, v in d.items():
        if isinstance(v, (tuple, list)):
            arr = getattr(c, k)
            for i, x in enumerate(v):
                arr[i] = int(x)
        else:
            setattr(c, k, v)
    return c


def config_from_unet(unet, sd=None) -> lib.UNetConfig:
    """sdxl_unet_config of a PyTorch / diffusers UNet2DConditionModel: from its `.config` where present (diffusers), else
    from the shapes of its diffusers-keyed state dict (what models/sdxl.py:25-40 loads)."""
    sd = sd if sd is not None else unet.state_dict()
    c = getattr(unet, "config", None)
    get = (lambda k, d=None: (c.get(k, d) if isinstance(c, dict) else getattr(c, k, d))) if c is not None else (lambda k, d=None: d)
    ch = get("block_out_channels")
    if ch is None:
        ch = [sd["conv_in.weight"].shape[0]]
        for i in (1, 2):
            k = f"down_blocks.{i}.resnets.0.conv1.weight"
            if k in sd:
                ch.append(sd[k].shape[0])
    tl = get("transformer_layers_per_block")
    if tl is None or isinstance(tl, int):
        tl = []
        for i in range(len(ch)):
            n = 0
            while f"down_blocks.{i}.attentions.0.transformer_blocks.{n}.norm1.weight" in sd:
                n += 1
            tl.append(n)
    cross = get("cross_attention_dim")
    if cross is None or isinstance(cross, (list, tuple)):
        k = next(k for k in sd if k.endswith("attn2.to_k.weight"))
        cross = sd[k].shape[1]
    ad = get("addition_time_embed_dim", 256)
    add_in = get("projection_class_embeddings_input_dim", None) or sd["add_embedding.linear_1.weight"].shape[1]
    head = get("attention_head_dim", 64)
    head = 64 if isinstance(head, (list, tuple)) else head           # SDXL: heads = C / 64 at every level
    cin = get("in_channels")          # 4; 9 inpainting, 8 image-conditioned (InstructPix2Pix)
    if cin is None:
        cin = sd["conv_in.weight"].shape[1]
    return make_config(in_channels=int(cin), block_out_channels=tuple(int(x) for x in ch), transformer_layers=tuple(int(x) for x in tl),
                       layers_per_block=int(get("layers_per_block", 2)), cross_attention_dim=int(cross),
                       addition_time_embed_dim=int(ad), pooled_dim=int(add_in) - 6 * int(ad),
                       norm_num_groups=int(get("norm_num_groups", 32)), head_dim=64 if head in (5, 10, 20) else int(head))


def input_cs(in_channels: int) -> int:
    """stored width of a pixel of the library's UNet input ([B*H*W][Cs] bf16): 8 up to 8 input channels, 16 above"""
    return 8 if int(in_channels) <= 8 else 16


def widen_conv_in(state_dict, in_channels: int) -> dict:
    """A copy of a diffusers-keyed UNet state dict whose conv_in.weight [cout, c, 3, 3] is zero-extended along dim 1 to in_channels:
    the usual start of inpainting (9) or InstructPix2Pix (8) training from SDXL-base -- the widened UNet computes what the original
    does whatever the extra channels hold.  Every other tensor is the same object; the original slice is kept bit for bit."""
    w = state_dict["conv_in.weight"]
    c = int(w.shape[1])
    if not c <= int(in_channels) <= 16:
        raise ValueError(f"widen_conv_in: in_channels {in_channels} must lie in {c} .. 16 (conv_in.weight has {c})")
    out = dict(state_dict)
    wide = torch.zeros(w.shape[0], int(in_channels), *w.shape[2:], dtype=w.dtype, device=w.device)
    wide[:, :c] = w
    out["conv_in.weight"] = wide
    return out


class _UNetFunction(torch.autograd.Function):
    """NativeUNet.differentiable: unet_forward / unet_backward as one autograd node.  `net` needs unet_forward, unet_backward,
    read_input_grad, read_cond_grads, read_residual_grads, device and the forward-generation counter _fwd_gen."""

    @staticmethod
    def forward(ctx, net, timestep, time_ids, sample, prompt_embeds, pooled, *res):
        rg = lambda t: torch.is_tensor(t) and t.requires_grad
        dev = net.device
        kw = {}
        cond = [k for k, t in (("prompt", prompt_embeds), ("pooled", pooled)) if rg(t)]
        if cond:
            kw["cond_grads"] = tuple(cond)
        if res:
            given = [t for t in res if t is not None]
            dt = torch.bfloat16 if given and all(t.dtype == torch.bfloat16 for t in given) else torch.float32
            conv = lambda t: None if t is None else t.detach().to(dev, dt).contiguous()
            kw["residuals"] = ([conv(t) for t in res[:-1]], conv(res[-1]))
            want = [("mid" if i == len(res) - 1 else i) for i, t in enumerate(res) if rg(t)]
            if want:
                kw["residual_grads"] = want
        if rg(sample):
            kw["input_grad"] = True
        pred = net.unet_forward(sample.detach(), timestep, prompt_embeds.detach(), pooled.detach(), time_ids, **kw)
        ctx.net, ctx.gen = net, getattr(net, "_fwd_gen", 0)
        ctx.meta = [None if not torch.is_tensor(t) else (t.shape, t.dtype, t.device) for t in (sample, prompt_embeds, pooled) + tuple(res)]
        return pred

    @staticmethod
    def backward(ctx, dpred):
        net = ctx.net
        if getattr(net, "_fwd_gen", 0) != ctx.gen:
            raise lib.SdxlError("differentiable: backward of a stale forward -- the engine keeps the activations of one forward, and another "
                                "forward of this net (forward_loss, unet_forward, differentiable or a sampler step) has run since this one")
        net.unet_backward(dpred, first_micro=bool(getattr(net, "first_micro", True)))
        d_prompt, d_pooled = net.read_cond_grads()
        d_down, d_mid = net.read_residual_grads()
        n_res = len(ctx.meta) - 3
        dev = [net.read_input_grad(), d_prompt, d_pooled] + (list(d_down or [None] * (n_res - 1)) + [d_mid] if n_res else [])
        out = [None] * len(ctx.meta)
        for i, meta in enumerate(ctx.meta):
            if meta is not None and ctx.needs_input_grad[3 + i] and dev[i] is not None:
                shape, dtype, device = meta
                out[i] = dev[i].reshape(shape).to(device=device, dtype=dtype)
        return (None, None, None, *out)


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def loss_mask_bhw(m, latent_shape) -> torch.Tensor:
    """a loss mask given as [B,H,W] or [B,1,H,W] at latent resolution as [B,H,W] fp32; ValueError for any other shape and for a
    value that is negative or not finite (downsampling a pixel mask is the caller's job)"""
    B, _, H, W = latent_shape
    m = torch.as_tensor(m)
    if tuple(m.shape) not in ((B, H, W), (B, 1, H, W)):
        raise ValueError(f"loss_mask: expected shape {(B, H, W)} or {(B, 1, H, W)} (latent resolution), got {tuple(m.shape)}")
    m = m.to(torch.float32).reshape(B, H, W)
    if not bool(torch.isfinite(m).all()) or bool((m < 0).any()):
        raise ValueError("loss_mask: every value must be finite and >= 0")
    return m


def trainable_flags(all_names, names) -> list:
    """[0 | 1] per entry of all_names for set_trainable's argument: an iterable of names (each must exist: KeyError) or a predicate"""
    if callable(names):
        return [1 if names(k) else 0 for k in all_names]
    want = set(names)
    unknown = sorted(want - set(all_names))
    if unknown:
        raise KeyError(f"set_trainable: unknown parameter names {unknown[:5]}{'...' if len(unknown) > 5 else ''}")
    return [1 if k in want else 0 for k in all_names]


class NativeUNet:
    """SDXL UNet + loss, forward and backward, on one MI355X.

    Memory (all torch-allocated so torch.distributed can reduce the gradient arena in place):
      weights  bf16 packed arena (5.1 GB for SDXL-base), grads fp32 arena (10.3 GB),
      workspace = activations + activation gradients + statistics of the largest planned bucket.
    """

    def __init__(self, cfg: Optional[lib.UNetConfig] = None, device: int = 0):
        if not torch.cuda.is_available():
            raise lib.SdxlError("NativeUNet needs a GPU (no CPU fallback)")
        self.L = lib.load()
        self.cfg = cfg if cfg is not None else make_config()
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        lib.check(self.L.sdxl_create(C.byref(self.cfg), device, C.byref(h)), "sdxl_create")
        self.h = h
        wb, gb = C.c_size_t(), C.c_size_t()
        lib.check(self.L.sdxl_param_bytes(self.h, C.byref(wb), C.byref(gb)))
        self.param_elems = wb.value // 2
        self.weights = torch.zeros(self.param_elems, dtype=torch.bfloat16, device=self.device)
        self.grads = torch.zeros(self.param_elems, dtype=torch.float32, device=self.device)
        lib.check(self.L.sdxl_bind_params(self.h, _ptr(self.weights), _ptr(self.grads)), "sdxl_bind_params")
        self.workspace: Optional[torch.Tensor] = None
        self._plans: Dict[Tuple[int, int, int, int], int] = {}
        self._cur: Optional[Tuple[int, int, int, int]] = None
        self._keep = []          # tensors whose device pointers the library still references
        self._trainable = None   # set_trainable's flag per state-dict tensor (None: no selection, every tensor trainable)
        self._lora_sel = False   # ... and whether it handed adapters to the library
        self.first_micro = True  # differentiable(): its backward overwrites the gradient arena (True) or accumulates into it (False)
        self._fwd_gen = 0        # counts the forwards: the engine keeps the activations of the last one only (differentiable())
        self.param_table = self._read_param_table()

    # ------------------------------------------------------------------ parameters
    def _read_param_table(self):
        n = self.L.sdxl_num_params(self.h)
        out = {}
        buf = C.create_string_buffer(256)
        nd = C.c_int()
        shp = (C.c_long * 4)()
        for i in range(n):
            lib.check(self.L.sdxl_param_info(self.h, i, buf, 256, C.byref(nd), shp))
            out[buf.value.decode()] = tuple(int(shp[k]) for k in range(nd.value))
        return out

    def param_ranges(self) -> Dict[str, Tuple[int, int]]:
        """{diffusers key: (element offset, element count)} of every tensor inside the packed weight / gradient arenas."""
        out = {}
        off, cnt = C.c_size_t(), C.c_size_t()
        for i, name in enumerate(self.param_table):
            lib.check(self.L.sdxl_param_range(self.h, i, C.byref(off), C.byref(cnt)))
            out[name] = (int(off.value), int(cnt.value))
        return out

    def param_shapes(self) -> Dict[str, Tuple[int, ...]]:
        """{diffusers state-dict key: shape} -- same keys/shapes as unet.state_dict() in the reference."""
        return dict(self.param_table)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True) -> None:
        missing = [k for k in self.param_table if k not in sd]
        extra = [k for k in sd if k not in self.param_table]
        if strict and (missing or extra):
            raise KeyError(f"state_dict mismatch: missing {missing[:5]}... extra {extra[:5]}...")
        for k, t in sd.items():
            if k in self.param_table:
                self.load_weight(k, t)
        torch.cuda.current_stream().synchronize()

    def load_weight(self, name: str, t: torch.Tensor) -> None:
        if tuple(t.shape) != self.param_table[name]:
            raise ValueError(f"{name}: shape {tuple(t.shape)} != {self.param_table[name]}")
        if t.dtype not in (torch.float32, torch.bfloat16):
            t = t.float()
        t = t.to(self.device).contiguous()
        lib.check(self.L.sdxl_load_weight(self.h, name.encode(), _ptr(t), 0 if t.dtype == torch.float32 else 1,
                                          _stream()), f"load {name}")
        torch.cuda.current_stream().synchronize()   # t may be a temporary

    def export(self, name: str, grad: bool = False, dtype=torch.float32) -> torch.Tensor:
        out = torch.empty(self.param_table[name], dtype=dtype, device=self.device)
        fn = self.L.sdxl_export_grad if grad else self.L.sdxl_export_weight
        lib.check(fn(self.h, name.encode(), _ptr(out), 0 if dtype == torch.float32 else 1, _stream()))
        return out

    def state_dict(self, dtype=torch.bfloat16) -> Dict[str, torch.Tensor]:
        return {k: self.export(k, False, dtype) for k in self.param_table}

    def grad_dict(self, dtype=torch.float32) -> Dict[str, torch.Tensor]:
        return {k: self.export(k, True, dtype) for k in self.param_table}

    # ------------------------------------------------------------------ gradient selection
    def set_trainable(self, names=None, lora=None) -> None:
        """Tell the backward which tensors are trained: an iterable of state-dict keys, a predicate name -> bool, or None (every
        tensor, the default).  An op whose tensors are ALL frozen skips its weight / bias / norm-parameter gradient work and writes
        nothing into the gradient arena; an op with one trainable tensor runs as always, so the frozen tensors sharing it (to_q | to_k |
        to_v of a block, attn2.to_k | to_v of every block of a width, all time_emb_proj, a weight and its bias) still get their
        gradient.  Input gradients, the loss and the conditioning gradients do not change.  grad_norm() keeps summing the whole arena,
        stale frozen ranges included: with a selection take the norm over grad_dict() / param_ranges() of trainable().
        lora: a lib.LoraOp (lora.LoRAAdapters.select) whose targets' ops write the adapter gradients themselves in place of their
        weight gradient; every tensor of such an op must be frozen.  Changing it drops the plans (the next step plans again).
        Not allowed between forward_loss and its backward; after a forward that nothing differentiates, discard_forward() first."""
        if names is None and lora is None:
            lib.check(self.L.sdxl_export_grad(self.h, None, None, lib.DTYPE_GRAD_SELECT, _stream()), "set_trainable")
            flags = None
        else:
            flags = trainable_flags(list(self.param_table), (lambda _k: True) if names is None else names)
            sel = lib.GradSelect(len(flags), (C.c_ubyte * len(flags))(*flags), C.pointer(lora) if lora is not None else None)
            lib.check(self.L.sdxl_export_grad(self.h, None, C.byref(sel), lib.DTYPE_GRAD_SELECT, _stream()), "set_trainable")
            if all(flags):       # (the library's normal form of "every tensor": no selection)
                flags = None
        if lora is not None or self._lora_sel:      # the library dropped its plans
            self._plans, self._cur = {}, None
        self._lora_sel = lora is not None
        self._trainable = flags

    def trainable(self):
        """the state-dict keys flagged trainable by the last set_trainable; every key when there is no selection"""
        flags = self._trainable
        return {k for i, k in enumerate(self.param_table) if flags is None or flags[i]}

    def discard_forward(self) -> None:
        """say that the last forward_loss gets no backward (an evaluation): the selection may change again (set_trainable)"""
        if self._cur is not None:
            lib.check(self.L.sdxl_plan(self.h, *self._cur, None), "sdxl_plan")

    # ------------------------------------------------------------------ plans
    def plan(self, B: int, H: int, W: int, ctx: int = 77) -> None:
        key = (B, H, W, ctx)
        if self._cur == key:
            return
        need = C.c_size_t()
        lib.check(self.L.sdxl_plan(self.h, B, H, W, ctx, C.byref(need)), "sdxl_plan")
        self._plans[key] = need.value
        if self.workspace is None or self.workspace.numel() < need.value:
            torch.cuda.current_stream().synchronize()
            self.workspace = None
            self.workspace = torch.empty(need.value, dtype=torch.uint8, device=self.device)
        lib.check(self.L.sdxl_bind_workspace(self.h, _ptr(self.workspace), self.workspace.numel()))
        self._cur = key

    @property
    def num_segments(self) -> int:
        return self.L.sdxl_num_segments(self.h)

    def segment_range(self, k: int) -> Tuple[int, int]:
        off, n = C.c_size_t(), C.c_size_t()
        lib.check(self.L.sdxl_segment_range(self.h, k, C.byref(off), C.byref(n)))
        return off.value, n.value

    def segment_ranges(self):
        """[(offset, count)] of every backward segment, in exchange order."""
        return [self.segment_range(k) for k in range(self.num_segments)]

    # ------------------------------------------------------------------ the step
    def zero_grads(self) -> None:
        lib.check(self.L.sdxl_zero_grads(self.h, _stream()))

    def _batch(self, latents, noise, sigma_or_t, timestep, prompt_embeds, pooled, time_ids, tag_weights):
        d = self.device
        B, _, H, W = latents.shape
        f32 = lambda t: None if t is None else t.to(d, torch.float32).contiguous()
        b16 = lambda t: None if t is None else t.to(d, torch.bfloat16).contiguous()
        ts = [f32(latents), f32(noise), f32(sigma_or_t).reshape(-1), f32(timestep).reshape(-1), b16(prompt_embeds),
              b16(pooled).reshape(B, -1), f32(time_ids).reshape(B, 6), f32(tag_weights)]
        ctx = ts[4].shape[1]
        self.plan(B, H, W, ctx)
        self._keep = ts
        return lib.Batch(B, H, W, ctx, *[None if t is None else t.data_ptr() for t in ts])

    def _per_sample(self, t, B: int, what: str):
        """an optional [B] fp32 device array of the batch (kept alive until the next forward_loss: the backward reads it again)"""
        if t is None:
            return None
        t = torch.as_tensor(t, dtype=torch.float32).to(self.device).reshape(-1).contiguous()
        if t.numel() != B:
            raise ValueError(f"{what}: expected {B} values (one per sample), got {t.numel()}")
        return t

    def _loss_mask(self, m, latents):
        """an optional loss mask as a contiguous [B,H,W] fp32 device array (kept alive like the per-sample arrays: the backward reads
        it again); ValueError for a shape that is not the latents' [B,H,W] / [B,1,H,W] or a value that is negative or not finite"""
        return None if m is None else loss_mask_bhw(m, latents.shape).to(self.device).contiguous()

    def _cond_request(self, cond_grads, B: int, ctx: int):
        """the buffers a micro-step's conditioning gradients are written to: cond_grads is None / False (none), True (both) or a
        collection of "prompt" / "pooled".  Owned here and kept until the next request; read_cond_grads() hands them out."""
        want = {"prompt", "pooled"} if cond_grads is True else set(cond_grads or ())
        if want - {"prompt", "pooled"}:
            raise ValueError(f"cond_grads {cond_grads!r}: expected True, None or a collection of 'prompt' / 'pooled'")
        z = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        self._d_prompt = z(B, ctx, int(self.cfg.cross_attention_dim)) if "prompt" in want else None
        self._d_pooled = z(B, int(self.cfg.pooled_dim)) if "pooled" in want else None
        return bool(want)

    def _cond_batch(self, b):
        """b as a lib.CondGradBatch carrying the current request (flagged), or b itself when nothing is requested"""
        if getattr(self, "_d_prompt", None) is None and getattr(self, "_d_pooled", None) is None:
            return b
        x = lib.CondGradBatch(*[getattr(b, f[0]) for f in lib.Batch._fields_])
        x.ctx_len |= lib.BATCH_EXT
        x.d_prompt_embeds = None if self._d_prompt is None else self._d_prompt.data_ptr()
        x.d_pooled = None if self._d_pooled is None else self._d_pooled.data_ptr()
        return x

    def _input_cond_batch(self, b, input_cond, latent_shape, what: str, rows: Optional[int] = None, convert: bool = True):
        """b as a lib.InputCondBatch carrying input_cond (flagged), or b itself when input_cond is None: without it every call is
        the one a 4-channel UNet makes.  input_cond is [rows, in_channels - 4, H, W] (rows = the plan's batch) fp32 on the device,
        kept alive with the batch's other tensors; convert=False (the sampler path) checks instead of converting."""
        if input_cond is None:
            return b
        B, _c, H, W = latent_shape
        rows = B if rows is None else rows
        n = int(self.cfg.in_channels) - 4
        if input_cond.dim() != 4 or tuple(input_cond.shape) != (rows, int(input_cond.shape[1]), H, W) or (n > 0 and input_cond.shape[1] != n):
            raise ValueError(f"{what}: input_cond must be [{rows}, {n}, {H}, {W}] (in_channels - 4 = {n} extra channels), got {tuple(input_cond.shape)}")
        if convert:
            input_cond = input_cond.to(self.device, torch.float32).contiguous()
        elif input_cond.dtype != torch.float32 or not input_cond.is_cuda or not input_cond.is_contiguous():
            raise ValueError(f"{what}: input_cond must be a contiguous torch.float32 device tensor")
        self._keep = list(self._keep) + [input_cond]
        x = lib.InputCondBatch(*[getattr(b, f[0]) for f in lib.Batch._fields_])
        for f in ("sampler", "d_prompt_embeds", "d_pooled"):
            if hasattr(b, f):
                setattr(x, f, getattr(b, f))
        x.ctx_len |= lib.BATCH_COND
        x.input_cond = input_cond.data_ptr()
        x.cond_channels = int(input_cond.shape[1])
        return x

    def residual_shapes(self, B: int, H: int, W: int):
        """([(B, C_i, h_i, w_i)] of the saved skips in forward (diffusers) order, the mid block's (B, C, h, w)): the shapes of
        down_block_additional_residuals / mid_block_additional_residual for a plan of batch B and latent size H x W"""
        ch, lpb = [int(c) for c in self.cfg.block_out_channels], int(self.cfg.layers_per_block)
        out, h, w = [(B, ch[0], H, W)], H, W
        for i in range(3):
            out += [(B, ch[i], h, w)] * lpb
            if i < 2:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
                out.append((B, ch[i], h, w))
        return out, (B, ch[2], h, w)

    def _residual_batch(self, b, residuals, residual_grads, shape, what: str):
        """b as a lib.ResidualBatch carrying the additional skip residuals and / or the request for their gradients (flagged), or b
        itself when neither is given: without them every call is the one made before they existed.  residuals = (down, mid): down a
        list of one tensor (or None) per skip or None, mid a tensor or None; each a contiguous fp32 or bf16 (one dtype for all) device
        tensor of residual_shapes()'s shape -- checked, not converted (430 MB at SDXL-base B = 4 128 x 128: no silent copy).
        residual_grads: True (every skip and mid), None, or a collection of skip indices and / or "mid"."""
        self._d_down, self._d_mid = None, None
        if residuals is None and not residual_grads:
            return b
        shapes, mid_shape = self.residual_shapes(*shape)
        n = len(shapes)
        down, mid = (None, None) if residuals is None else residuals
        if down is not None and len(down) != n:
            raise ValueError(f"{what}: residuals: expected {n} down residuals (one per skip, None allowed), got {len(down)}")
        given = [(f"down[{i}]", t, shapes[i]) for i, t in enumerate(down or ()) if t is not None]
        if mid is not None:
            given.append(("mid", mid, mid_shape))
        dt = given[0][1].dtype if given else torch.float32
        for name, t, shp in given:
            if tuple(t.shape) != shp:
                raise ValueError(f"{what}: residuals: {name} must be {shp}, got {tuple(t.shape)}")
            if t.dtype not in (torch.float32, torch.bfloat16) or t.dtype != dt:
                raise ValueError(f"{what}: residuals: {name} is {t.dtype}; every residual must be torch.float32 or every one torch.bfloat16")
            if t.device.type != torch.device(self.device).type or not t.is_contiguous():
                raise ValueError(f"{what}: residuals: {name} must be a contiguous device tensor")
        want = set(range(n)) | {"mid"} if residual_grads is True else set(residual_grads or ())
        if want - (set(range(n)) | {"mid"}):
            raise ValueError(f"{what}: residual_grads {residual_grads!r}: expected True, None or a collection of skip indices 0..{n - 1} and 'mid'")
        z = lambda shp: torch.empty(shp, dtype=torch.float32, device=self.device)
        if want:
            self._d_down = [z(shapes[i]) if i in want else None for i in range(n)]
            self._d_mid = z(mid_shape) if "mid" in want else None
        ptrs = lambda ts: None if ts is None else (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
        arr_down, arr_d = ptrs(None if down is None else list(down)), ptrs(self._d_down)
        r = lib.Residuals(n, 0 if dt == torch.float32 else 1, arr_down, None if mid is None else mid.data_ptr(), arr_d,
                          None if self._d_mid is None else self._d_mid.data_ptr())
        self._keep = list(self._keep) + [t for _n, t, _s in given] + [arr_down, arr_d, r]
        x = lib.ResidualBatch(*[getattr(b, f[0]) for f in lib.Batch._fields_])
        for f in ("sampler", "d_prompt_embeds", "d_pooled", "input_cond", "cond_channels"):
            if hasattr(b, f):
                setattr(x, f, getattr(b, f))
        x.ctx_len |= lib.BATCH_RES
        x.residuals = C.pointer(r)
        return x

    def _input_grad_batch(self, b, input_grad, shape):
        """b as a lib.InputGradBatch carrying the output buffer of the gradient with respect to the UNet input (flagged), or b itself
        when input_grad is false: without the request every call is the one made before it existed.  The buffer [B, in_channels, H, W]
        fp32 is owned here and kept until the next forward; read_input_grad() hands it out."""
        self._d_input = None
        self._fwd_gen = getattr(self, "_fwd_gen", 0) + 1      # (every forward replaces the activations the engine keeps: _UNetFunction)
        if not input_grad:
            return b
        B, H, W = shape
        self._d_input = torch.empty(B, int(self.cfg.in_channels), H, W, dtype=torch.float32, device=self.device)
        x = lib.InputGradBatch(*[getattr(b, f[0]) for f in lib.Batch._fields_])
        for f in ("sampler", "d_prompt_embeds", "d_pooled", "input_cond", "cond_channels", "residuals"):
            if hasattr(b, f):
                setattr(x, f, getattr(b, f))
        x.ctx_len |= lib.BATCH_DIN
        x.d_input = self._d_input.data_ptr()
        return x

    def read_input_grad(self):
        """the gradient with respect to the UNet input, [B, in_channels, H, W] fp32 on the device, of the last forward_loss / unet_forward
        that asked for it (input_grad=True) and whose backward has been enqueued; stream-ordered (no synchronisation); None when nothing
        was asked.  Channels 0..3 belong to the latent input x_t as the UNet read it, channels 4.. to input_cond.  The gradient of
        grad_scale x loss, as the parameter gradients of that micro-step (unet_backward: of <dpred, pred>); the chain rule through the
        loss preparation (x_t from latents and noise) is the caller's ("Input gradients")."""
        return getattr(self, "_d_input", None)

    def read_residual_grads(self):
        """([d_down[i] | None per skip], d_mid | None) of the last call that asked for them (residual_grads) and whose backward has
        been enqueued: fp32 NCHW, on the device, stream-ordered (no synchronisation); (None, None) when nothing was asked.  The
        gradient of grad_scale x loss, as the parameter gradients of that micro-step (unet_backward: of <dpred, pred>)."""
        return getattr(self, "_d_down", None), getattr(self, "_d_mid", None)

    def read_cond_grads(self):
        """(d_prompt_embeds [B,ctx,cross_attention_dim] | None, d_pooled [B,pooled_dim] | None) of the last micro-step that asked for
        them (forward_loss / unet_forward with cond_grads) and whose backward has been enqueued: fp32, on the device, stream-ordered
        (no synchronisation).  The gradient of grad_scale x loss, as the parameter gradients of that micro-step."""
        return getattr(self, "_d_prompt", None), getattr(self, "_d_pooled", None)

    def forward_loss(self, method: str, latents, noise, sigma_or_t, timestep, prompt_embeds, pooled, time_ids,
                     tag_weights=None, prediction_type="v_prediction", min_snr_gamma: Optional[float] = 5.0,
                     use_ztsnr=True, sample_weights=None, huber_c=None, loss_type: str = "l2",
                     per_sample_loss: bool = False, loss_mask=None, noise_in=None, mask_norm: str = "mean",
                     cond_grads=None, input_cond=None, residuals=None, residual_grads=None, input_grad: bool = False) -> None:
        """loss preparation + UNet forward + loss; results stay on the device until read_loss().
        input_grad: the backward of this micro-step also produces the gradient with respect to the UNet input (every channel: x_t and
        input_cond), read with read_input_grad().
        residuals: (down, mid), diffusers' down_block_additional_residuals / mid_block_additional_residual (a ControlNet's outputs,
        already scaled): added to the skips where the up path reads them and to the mid block's output (_residual_batch has the
        shapes and dtypes).  residual_grads: True, None or a collection of skip indices / "mid": the backward of this micro-step also
        produces the gradient with respect to those residuals, read with read_residual_grads().
        input_cond: [B, in_channels - 4, H, W], channels 4.. of the UNet input (rounded to bf16) of a UNet with in_channels > 4:
        required there, refused (by the library) with in_channels = 4.  Read by this call only; the backward does not need it.
        sample_weights: optional [B] s_b multiplied into each sample's loss and gradient.  loss_type "l2" | "huber" |
        "smooth_l1" (include/sdxlstep.h), with huber_c a float (every sample) or [B] values (per sample).
        per_sample_loss: also produce the [B] per-sample losses, read with read_per_sample_loss() after read_loss().
        loss_mask: optional [B,H,W] or [B,1,H,W] at latent resolution, finite and >= 0, multiplied into every channel's loss and
        gradient; mask_norm "mean" divides by the element count as without a mask, "masked_mean" each sample by its own mask sum.
        noise_in: optional [B,4,H,W], the noise (ddpm) / x0 (flow matching) the UNet input is built from while the target keeps
        `noise` (input perturbation).
        cond_grads: ("prompt", "pooled"), a subset, True (both) or None: the backward of this micro-step also produces the gradient
        with respect to prompt_embeds / pooled, read with read_cond_grads()."""
        if loss_type not in lib.LOSS_TYPES:
            raise ValueError(f"loss_type {loss_type!r}: expected one of {sorted(lib.LOSS_TYPES)}")
        if mask_norm not in lib.MASK_NORMS:
            raise ValueError(f"mask_norm {mask_norm!r}: expected one of {sorted(lib.MASK_NORMS)}")
        B = latents.shape[0]
        mask = self._loss_mask(loss_mask, latents)
        if noise_in is not None and tuple(noise_in.shape) != tuple(latents.shape):
            raise ValueError(f"noise_in: expected the latents' shape {tuple(latents.shape)}, got {tuple(noise_in.shape)}")
        scalar_c = isinstance(huber_c, (int, float))
        lc = lib.LossConfig(METHODS[method], PRED_TYPES.get(prediction_type, 0), int(min_snr_gamma is not None),
                            float(min_snr_gamma or 0.0), int(bool(use_ztsnr)), lib.LOSS_TYPES[loss_type],
                            float(huber_c) if scalar_c else 0.0)
        ext = []
        if mask is not None or noise_in is not None:      # the full struct, flagged; without either the call is the short struct's
            nin = None if noise_in is None else noise_in.to(self.device, torch.float32).contiguous()
            ext = [mask, nin]
            lc = lib.LossConfigExt(*[getattr(lc, f[0]) for f in lib.LossConfig._fields_])
            lc.loss_type |= lib.LOSS_EXT
            lc.mask_norm = lib.MASK_NORMS[mask_norm]
            lc.loss_mask = None if mask is None else mask.data_ptr()
            lc.noise_in = None if nin is None else nin.data_ptr()
        b = self._batch(latents, noise, sigma_or_t, timestep, prompt_embeds, pooled, time_ids, tag_weights)
        sw = self._per_sample(sample_weights, B, "sample_weights")
        hc = None if scalar_c else self._per_sample(huber_c, B, "huber_c")
        self._ps_loss = torch.empty(B, dtype=torch.float32, device=self.device) if per_sample_loss else None
        self._keep = list(self._keep) + [sw, hc] + ext
        b.sample_weights = None if sw is None else sw.data_ptr()
        b.huber_c = None if hc is None else hc.data_ptr()
        b.per_sample_loss = None if self._ps_loss is None else self._ps_loss.data_ptr()
        self._cond_request(cond_grads, B, b.ctx_len)
        b = self._input_cond_batch(self._cond_batch(b), input_cond, latents.shape, "forward_loss")
        b = self._residual_batch(b, residuals, residual_grads, (B, latents.shape[2], latents.shape[3]), "forward_loss")
        b = self._input_grad_batch(b, input_grad, (B, latents.shape[2], latents.shape[3]))
        lib.check(self.L.sdxl_forward_loss(self.h, C.byref(lc), C.byref(b), _stream()), "sdxl_forward_loss")

    def backward(self, grad_scale: float = 1.0, first_micro: bool = True, on_segment=None, segment_stream: bool = False) -> None:
        """All backward segments in reverse execution order; `on_segment(k, offset, count)` is called after segment
        k's kernels are enqueued (used to start that bucket's gradient exchange under the rest of backward).
        segment_stream: the callbacks run with the engine's SIDE stream as torch's current stream (join mode 2): the
        bucket's cast and collective are ordered behind the segment's weight gradients there, and the caller's stream --
        the backward's critical path -- neither waits for the side stream nor runs the casts (3.5 ms of them per step)."""
        side = self._side_stream() if (segment_stream and on_segment is not None) else None
        lib.check(self.L.sdxl_set_join_mode(self.h, 0 if on_segment is not None else 1) if side is None
                  else self.L.sdxl_set_join_mode(self.h, 2))
        if on_segment is None and hasattr(self.L, "sdxl_backward_all"):     # no per-segment exchange: one call for the whole backward
            lib.check(self.L.sdxl_backward_all(self.h, float(grad_scale), int(first_micro), _stream()), "backward")
            return
        for k in range(self.num_segments):
            lib.check(self.L.sdxl_backward_segment(self.h, k, float(grad_scale), int(first_micro), _stream()),
                      f"backward segment {k}")
            if on_segment is not None:
                if side is None:
                    on_segment(k, *self.segment_range(k))
                else:
                    with torch.cuda.stream(side):
                        on_segment(k, *self.segment_range(k))
        if side is not None:      # whatever the callbacks left on the side stream (the last cast; host-staged copies of the
            torch.cuda.current_stream().wait_stream(side)      # gloo test transport) is ordered before the caller's next work

    def set_grad_emit(self, arena: Optional[torch.Tensor], scale: float = 1.0) -> None:
        """Exchange micro-step without the cast pass: the weight-gradient GEMMs of the next backward write their final
        value x scale as bf16 into `arena` (param_elems bf16, the exchange arena) and leave the fp32 arena alone; None = off.
        `cast_small` then covers the biases / norm parameters of a segment."""
        if arena is not None:
            assert arena.dtype == torch.bfloat16 and arena.numel() >= self.param_elems and arena.is_contiguous()
        lib.check(self.L.sdxl_set_grad_emit(self.h, None if arena is None else _ptr(arena), float(scale)))

    def cast_small(self, off: int, n: int, dst: torch.Tensor, scale: float = 1.0) -> None:
        lib.check(self.L.sdxl_small_grads_to_bf16(self.h, off, n, _ptr(dst), float(scale), _stream()))

    def _side_stream(self):
        if getattr(self, "_side_ext", None) is None:
            p = C.c_void_p()
            lib.check(self.L.sdxl_side_stream(self.h, C.byref(p)))
            self._side_ext = torch.cuda.ExternalStream(p.value, device=self.device) if p.value else False
        return self._side_ext or None

    def set_graph_mode(self, on: bool) -> None:
        """hipGraph replay of forward / backward (default off: eager two-stream launches measured faster on ROCm 7.2)."""
        lib.check(self.L.sdxl_set_graph_mode(self.h, int(bool(on))))

    def read_loss(self):
        out = (C.c_float * 8)()
        lib.check(self.L.sdxl_read_loss(self.h, out, _stream()))
        return [float(x) for x in out]

    def read_per_sample_loss(self) -> torch.Tensor:
        """the [B] per-sample losses of the last forward_loss(per_sample_loss=True), on the CPU.  Call it after read_loss(), which
        has synchronised the stream: this adds the copy only."""
        if getattr(self, "_ps_loss", None) is None:
            raise lib.SdxlError("read_per_sample_loss: the last forward_loss was not called with per_sample_loss=True")
        return self._ps_loss.cpu()

    # UNet only (sample NCHW fp32/bf16 in, NCHW fp32 out) -- for parity tests and validation sampling
    def unet_forward(self, sample, timestep, prompt_embeds, pooled, time_ids, cond_grads=None, residuals=None, residual_grads=None,
                     input_grad: bool = False) -> torch.Tensor:
        """cond_grads as in forward_loss: the following unet_backward also produces d prompt_embeds / d pooled of <dpred, pred>;
        residuals / residual_grads as in forward_loss (the gradients: of <dpred, pred>); input_grad: also d sample (read_input_grad())"""
        B, Cc, H, W = sample.shape
        d = self.device
        dummy = torch.zeros(B, 4, H, W, device=d)
        tb = self._batch(dummy, dummy, torch.zeros(B), timestep, prompt_embeds, pooled, time_ids, None)
        b = lib.SamplerBatch(*[getattr(tb, f[0]) for f in lib.Batch._fields_])      # sdxl_batch in full, sampler = NULL
        self._cond_request(cond_grads, B, tb.ctx_len)
        b = self._residual_batch(self._cond_batch(b), residuals, residual_grads, (B, H, W), "unet_forward")
        b = self._input_grad_batch(b, input_grad, (B, H, W))
        cin = int(self.cfg.in_channels)      # the sample carries every input channel, packed into Cs columns
        if Cc != cin:
            raise ValueError(f"unet_forward: sample has {Cc} channels, the UNet has in_channels = {cin}")
        x8 = torch.zeros(B * H * W, input_cs(cin), dtype=torch.bfloat16, device=d)
        x8[:, :cin] = sample.to(d).permute(0, 2, 3, 1).reshape(B * H * W, cin).to(torch.bfloat16)
        out8 = torch.empty(B * H * W, 8, dtype=torch.bfloat16, device=d)
        lib.check(self.L.sdxl_unet_forward(self.h, _ptr(x8), C.byref(b), _ptr(out8), _stream()), "sdxl_unet_forward")
        return out8[:, :4].float().reshape(B, H, W, 4).permute(0, 3, 1, 2).contiguous()

    # ------------------------------------------------------------------ sampling (sampler.py drives these)
    def _sampler_call(self, x, prompt_embeds, pooled, time_ids, timestep, step: "lib.SamplerStep", what: str, planes=(), input_cond=None, residuals=None) -> None:
        """sdxl_unet_forward with sdxl_batch.sampler set.  Every tensor is already on the device in the library's dtype and
        contiguous (checked, not converted: no torch arithmetic or copy runs here); the plan's batch is prompt_embeds' (B, or
        2B = [cond; uncond] with cfg), x is [B,4,H,W] fp32.  `planes`: (name, tensor, elements) of an extended step's buffers."""
        PB, ctx = int(prompt_embeds.shape[0]), int(prompt_embeds.shape[1])
        B, _c, H, W = x.shape
        for t, dt, n, name in ((x, torch.float32, B * 4 * H * W, "x"), (prompt_embeds, torch.bfloat16, None, "prompt_embeds"),
                               (pooled, torch.bfloat16, None, "pooled"), (time_ids, torch.float32, PB * 6, "time_ids"),
                               (timestep, torch.float32, PB, "timestep")) + tuple((t, torch.float32, n, name) for name, t, n in planes):
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous() or (n is not None and t.numel() != n):
                raise ValueError(f"{what}: {name} must be a contiguous {dt} device tensor" + (f" of {n} elements" if n is not None else ""))
        if _c != 4 or PB != (2 * B if step.cfg else B) or pooled.shape[0] != PB:
            raise ValueError(f"{what}: x {tuple(x.shape)} does not fit a conditioning batch of {PB} with cfg = {step.cfg}")
        self.plan(PB, H, W, ctx)
        self._keep = [x, prompt_embeds, pooled, time_ids, timestep] + [t for _n, t, _e in planes]
        step.x = x.data_ptr()
        for name, t, _e in planes:
            setattr(step, name, t.data_ptr())
        b = lib.SamplerBatch(PB, H, W, ctx, None, None, None, timestep.data_ptr(), prompt_embeds.data_ptr(), pooled.data_ptr(),
                             time_ids.data_ptr(), None)
        b.sampler = C.cast(C.pointer(step), C.POINTER(lib.SamplerStep))      # (a SamplerStepExt goes through the same pointer)
        b = self._input_cond_batch(b, input_cond, x.shape, what, rows=PB, convert=False)      # [PB, in_channels - 4, H, W]: the uncond half has rows of its own
        b = self._residual_batch(b, residuals, None, (PB, H, W), what)      # [PB, C_i, h_i, w_i]: rows b + B feed the unconditional half
        self._d_input, self._fwd_gen = None, getattr(self, "_fwd_gen", 0) + 1      # (a sampler step replaces the kept activations too)
        lib.check(self.L.sdxl_unet_forward(self.h, None, C.byref(b), None, _stream()), what)

    def sample_init(self, x, prompt_embeds, pooled, time_ids, timestep, *, cfg: bool, a_in: float = 1.0, clamp: float = 0.0,
                    input_cond=None, residuals=None) -> None:
        """write the first UNet input of a sampling loop, bf16(clamp(a_in * x, +-clamp)), into the plan's input buffer (no forward).
        input_cond (in_channels > 4): [PB, in_channels - 4, H, W] fp32 on the device, PB = prompt_embeds' batch -- channels 4.. of
        the input, row b for the conditional half and row b + B for the unconditional one; the same for sample_step."""
        s = lib.SamplerStep(None, int(cfg), 1, 0.0, 0.0, 0.0, 0.0, float(a_in), float(clamp), 1.0, 0.0)
        self._sampler_call(x, prompt_embeds, pooled, time_ids, timestep, s, "sample_init", input_cond=input_cond, residuals=residuals)

    def sample_step(self, x, prompt_embeds, pooled, time_ids, timestep, *, cfg, a_skip, a_out, p, q, a_in_next=1.0, clamp=0.0,
                    guidance=1.0, guidance_rescale=0.0, init=0, hist=None, xsave=None, noise=None, r=0.0, u=0.0, s=0.0, save=0,
                    mask=None, known=None, knoise=None, k_a=0.0, k_b=0.0, input_cond=None, residuals=None) -> None:
        """one forward on the plan's input buffer + the fused sampler step (include/sdxlstep.h sdxl_sampler_step): x is updated in
        place and the next input is left in the plan; stream-ordered, no synchronisation.  hist ... k_b are the fields of
        sdxl_sampler_step_ext ([B,4,H,W] fp32 device tensors, mask [B,H,W]); the extended struct and its flag are passed only when
        one of them is given, otherwise the call is the plain step's.  residuals: (down, mid) as in forward_loss, for the plan's batch
        (2B rows with cfg); read by this step's forward only."""
        base = (None, int(cfg), int(init), float(a_skip), float(a_out), float(p), float(q), float(a_in_next), float(clamp),
                float(guidance), float(guidance_rescale))
        tensors = (("hist", hist), ("xsave", xsave), ("noise", noise), ("mask", mask), ("known", known), ("knoise", knoise))
        if all(t is None for _n, t in tensors) and not any((r, u, s, save, k_a, k_b)):
            self._sampler_call(x, prompt_embeds, pooled, time_ids, timestep, lib.SamplerStep(*base), "sample_step", input_cond=input_cond, residuals=residuals)
            return
        st = lib.SamplerStepExt(*base)
        st.init |= lib.SAMPLER_EXT
        st.r, st.u, st.s, st.save, st.k_a, st.k_b = float(r), float(u), float(s), int(save), float(k_a), float(k_b)
        n = x.numel()
        planes = tuple((name, t, n // 4 if name == "mask" else n) for name, t in tensors if t is not None)
        self._sampler_call(x, prompt_embeds, pooled, time_ids, timestep, st, "sample_step", planes, input_cond=input_cond, residuals=residuals)

    def unet_backward(self, dpred_nchw: torch.Tensor, first_micro: bool = True) -> None:
        B, Cc, H, W = dpred_nchw.shape
        d8 = torch.zeros(B * H * W, 8, dtype=torch.bfloat16, device=self.device)
        d8[:, :4] = dpred_nchw.to(self.device).permute(0, 2, 3, 1).reshape(B * H * W, 4).to(torch.bfloat16)
        lib.check(self.L.sdxl_unet_backward(self.h, _ptr(d8), int(first_micro), _stream()), "sdxl_unet_backward")
        torch.cuda.current_stream().synchronize()

    # ------------------------------------------------------------------ the UNet as a differentiable torch function
    def differentiable(self, sample, timestep, prompt_embeds, pooled, time_ids, residuals=None) -> torch.Tensor:
        """pred [B,4,H,W] fp32 = the UNet, as a torch.autograd.Function differentiable in all of its tensor inputs: sample
        [B,in_channels,H,W], prompt_embeds, pooled and every residual of residuals = (down, mid) (as in forward_loss).  The backward
        runs unet_backward(dpred) and hands back the gradient of each of those that requires grad, in the input's own device and
        dtype; the parameter gradients go to the gradient arena, overwriting it when self.first_micro (an attribute, default True) else
        accumulating.  The engine keeps the activations of ONE forward: a backward after any other forward of this net raises
        SdxlError (retain_graph replays are refused the same way once another forward has run)."""
        down, mid = (None, None) if residuals is None else residuals
        res = () if residuals is None else tuple(down if down is not None else [None] * (3 * int(self.cfg.layers_per_block) + 3)) + (mid,)
        return _UNetFunction.apply(self, timestep, time_ids, sample, prompt_embeds, pooled, *res)

    def grad_norm(self) -> float:
        out = torch.zeros(1, dtype=torch.float32, device=self.device)
        lib.check(self.L.sdxl_grad_sumsq(self.h, _ptr(out), _stream()))
        return float(out.sqrt())

    def close(self):
        if getattr(self, "h", None):
            torch.cuda.synchronize()
            self.L.sdxl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
