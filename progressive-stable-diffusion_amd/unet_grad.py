"""The differentiable UNet of a training step: SD-1.x ``UNet2DConditionModel`` with the 16 ``attn2`` sites of the
reference (triple-pathway routing-gate mode, or the baseline two-segment mode), restated from the operators of
``grad_ops`` and ``conditioning_grad.time_embedding`` alone, in the manner of ``conditioning_grad``.

``unet_forward`` takes the backend and ``params``, a mapping from the reference's state-dict key names to the **fp32
master** tensors (leaves, or views / attached leaves of an ``optim.ParamArena``), with every matrix weight in the library
layout ``[N][taps*C]`` (``masters_from_state_dict``; ``state_dict_from_masters`` is the bit-exact inverse).  Activations are
16-bit NHWC, the tokens of a transformer are the same memory seen as ``[B][H*W][C]``.  Nothing is folded or fused: every
norm is an operator on its own masters, ``to_q`` / ``to_k`` / ``to_v`` (and the ``to_k_dis`` / ``to_v_dis`` of the routing
processor) are products of their own whose outputs ``torch.cat`` joins into the qkv / kv operand of the attention kernels.
Residual additions, the ``torch.cat`` of a skip connection and the token reshapes are torch.  The time path is one call of
``conditioning_grad.time_embedding``; a resnet's slice of its fp32 rows is the ``rowvec`` of the first conv.

``prepared``: an ``optim.DgradRelayout`` (anything with ``prepared(name) -> (w16, wt)`` and a ``kinds`` mapping).  Every
product whose weight it lists reads the optimizer's 16-bit copy and the re-laid data-gradient weight instead of casting
and re-laying per call (``grad_ops.linear``); ``relayout_entries`` lists every weight of the UNet that can take part.
Without it the same function runs on the masters alone.

The gates of the routing processor and ``delta_scale`` get no gradient, as ``grad_ops.tri_cross_attention`` documents.
The latent side must be a multiple of 32: the mid block runs on side / 8 squared queries, and ``attn_grad`` takes a
multiple of 16, at least 16.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Mapping, Optional, Tuple

import torch

from . import conditioning_grad as CG
from . import grad_ops as G
from . import lib as L
from . import weights as W

HEADS = 8
GROUPS = 32
BLOCK_OUT = W.UNET_BLOCK_OUT


# ---- master packing ----------------------------------------------------------------------------------------------------
def masters_from_state_dict(sd: Mapping[str, torch.Tensor], prefix: str = "unet.unet") -> "OrderedDict[str, torch.Tensor]":
    """fp32 masters of every key of ``sd`` under ``prefix``: a conv weight OIHW becomes the library layout
    ``[O][kh*kw*I]`` (``[O][ky][kx][I]`` flattened; a 1x1 conv ``[O][I]``), every other tensor is copied as it is."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for k, v in sd.items():
        if not k.startswith(prefix + "."):
            continue
        v = v.detach().float()
        out[k] = v.permute(0, 2, 3, 1).reshape(v.shape[0], -1).contiguous() if v.dim() == 4 else v.clone()
    return out


def state_dict_from_masters(masters: Mapping[str, torch.Tensor], prefix: str = "unet.unet") -> "OrderedDict[str, torch.Tensor]":
    """The inverse of ``masters_from_state_dict``: the conv weights under ``prefix`` back in OIHW (kernel size from
    ``weights.unet_shapes``), every other tensor (keys outside ``prefix`` included) copied as it is."""
    shapes = W.unet_shapes(prefix, routing_gates=True)
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for k, v in masters.items():
        v = v.detach()
        ref = shapes.get(k)
        if ref is not None and len(ref) == 4:
            o, i, kh, kw = ref
            if tuple(v.shape) != (o, kh * kw * i):
                raise ValueError(f"{k}: expected the library layout {(o, kh * kw * i)}, got {tuple(v.shape)}")
            out[k] = v.reshape(o, kh, kw, i).permute(0, 3, 1, 2).contiguous()
        else:
            out[k] = v.clone()
    return out


def _resnet_keys(u: str) -> List[str]:
    keys = [f"{u}down_blocks.{i}.resnets.{j}" for i in range(4) for j in range(2)]
    keys += [u + "mid_block.resnets.0", u + "mid_block.resnets.1"]
    return keys + [f"{u}up_blocks.{i}.resnets.{j}" for i in range(4) for j in range(3)]


def relayout_entries(params: Mapping[str, torch.Tensor], prefix: str = "unet.unet") -> List[Tuple[str, str, int]]:
    """``(name, kind, taps)`` of every UNet weight under ``prefix`` whose product takes ``prepared=``: the 3x3 convs of
    the resnets (T, 9 taps), the down- and upsamplers (S2, UPS), ``conv_out`` (COUT4) and every Linear / 1x1 conv (T, 1
    tap).  ``conv_in`` (its 4 channels are packed to 8 per call) and the fp32 row path (``time_embedding``,
    ``time_emb_proj``) cast their own weights."""
    u = prefix + "."
    out = []
    for k, v in params.items():
        if not k.startswith(u) or not k.endswith(".weight") or v.dim() != 2:
            continue
        if k.startswith(u + "conv_in.") or k.startswith(u + "time_embedding.") or ".time_emb_proj." in k:
            continue
        if k.startswith(u + "conv_out."):
            out.append((k, "COUT4", 9))
        elif ".downsamplers." in k:
            out.append((k, "S2", 9))
        elif ".upsamplers." in k:
            out.append((k, "UPS", 9))
        elif k.endswith((".conv1.weight", ".conv2.weight")):
            out.append((k, "T", 9))
        else:
            out.append((k, "T", 1))
    return out


def check_latent_side(h: int, w: int) -> None:
    if h % 32 or w % 32 or h < 32 or w < 32:
        raise ValueError(f"unet_grad: the latent sides must be multiples of 32, got {h} x {w}: the mid block attends over "
                         f"(side / 8)^2 queries and the attention backward takes a multiple of 16, at least 16")


# ---- blocks ------------------------------------------------------------------------------------------------------------
class _Net:
    def __init__(self, be, params, prepared):
        self.be, self.params = be, params
        self.listed = prepared.kinds if prepared is not None else {}
        self.owner = prepared

    def prep(self, key):
        return self.owner.prepared(key) if key in self.listed else None

    def lin(self, key, x, bias=True):
        p = self.params
        return G.linear(self.be, x, p[key + ".weight"], p[key + ".bias"] if bias else None, prepared=self.prep(key + ".weight"))

    def conv(self, key, x, rowvec=None):
        p = self.params
        return G.conv3x3(self.be, x, p[key + ".weight"], p[key + ".bias"], rowvec=rowvec, prepared=self.prep(key + ".weight"))

    def gn(self, key, x, eps=1e-5, silu=False):
        return G.group_norm(self.be, x, self.params[key + ".weight"], self.params[key + ".bias"], GROUPS, eps, silu)

    def ln(self, key, x):
        return G.layer_norm(self.be, x, self.params[key + ".weight"], self.params[key + ".bias"], 1e-5)

    def resnet(self, p, x, row):
        """GN-SiLU-conv3x3 (+ time row in the epilogue) GN-SiLU-conv3x3, 1x1 shortcut iff Cin != Cout."""
        h = self.conv(p + ".conv1", self.gn(p + ".norm1", x, silu=True), rowvec=row)
        h = self.conv(p + ".conv2", self.gn(p + ".norm2", h, silu=True))
        if (p + ".conv_shortcut.weight") in self.params:
            x = self.lin(p + ".conv_shortcut", x)
        return x + h

    def transformer(self, p, x, cond16, split, lam):
        """GroupNorm(1e-6) - proj_in - {LN, attn1} - {LN, attn2 against kv = Linear(cond)} - {LN, GEGLU FF} - proj_out +
        residual."""
        be, P = self.be, self.params
        b, hh, ww, c = x.shape
        h = self.lin(p + ".proj_in", self.gn(p + ".norm", x, eps=1e-6)).reshape(b, hh * ww, c)
        tb = p + ".transformer_blocks.0"
        a1, a2 = tb + ".attn1", tb + ".attn2"
        n = self.ln(tb + ".norm1", h)
        qkv = torch.cat([self.lin(a1 + k, n, bias=False) for k in (".to_q", ".to_k", ".to_v")], -1)
        h = h + self.lin(a1 + ".to_out.0", G.self_attention(be, qkv, HEADS))
        q = self.lin(a2 + ".to_q", self.ln(tb + ".norm2", h), bias=False)
        if split:
            kv = torch.cat([self.lin(k, cond16, bias=False) for k in (a2 + ".to_k", a2 + ".to_v", a2 + ".processor.to_k_dis",
                                                                     a2 + ".processor.to_v_dis")], -1)
            gates = torch.stack([P[a2 + ".processor.anat_gate"].detach().reshape(()),
                                 P[a2 + ".processor.dis_gate"].detach().reshape(())]).float()
            a = G.tri_cross_attention(be, q, kv, gates, lam, HEADS, L.XATTN_SPLIT)
        else:
            kv = torch.cat([self.lin(a2 + k, cond16, bias=False) for k in (".to_k", ".to_v")], -1)
            a = G.tri_cross_attention(be, q, kv, None, 0.0, HEADS, L.XATTN_BASELINE)
        h = h + self.lin(a2 + ".to_out.0", a)
        y = G.geglu(be, self.lin(tb + ".ff.net.0.proj", self.ln(tb + ".norm3", h)))
        h = h + self.lin(tb + ".ff.net.2", y)
        return self.lin(p + ".proj_out", h.reshape(b, hh, ww, c)) + x


def unet_forward(be, params: Mapping[str, torch.Tensor], x: torch.Tensor, t: torch.Tensor, cond: torch.Tensor, *,
                 prefix: str = "unet.unet", use_routing_gates: bool = True, delta_scale: float = 0.0,
                 dtype: torch.dtype = torch.float16, prepared=None) -> torch.Tensor:
    """epsilon prediction with autograd history: ``x`` fp32 NCHW latents [B,4,S,S] (data; a leaf that requires grad gets its gradient all the same), ``t`` [B] integer
    timesteps, ``cond`` [B,48,768] (routing-gate mode: 16 AOE, 16 image and 16 delta tokens) or [B,32,768] (baseline), any
    float type: it is rounded to ``dtype`` once, and its gradient arrives in its own type -> fp32 NCHW [B,4,S,S].
    ``oracle.sd_unet.unet_forward`` is the reference; the baseline's per-block frequency modes scale the probabilities by
    one and are the plain joint softmax."""
    if x.dim() != 4 or x.shape[1] != 4:
        raise ValueError(f"unet_grad: x must be the latents [B,4,S,S], got {tuple(x.shape)}")
    check_latent_side(x.shape[2], x.shape[3])
    want = 48 if use_routing_gates else 32
    if cond.dim() != 3 or cond.shape[0] != x.shape[0] or cond.shape[1] != want:
        raise ValueError(f"unet_grad: cond must be [B,{want},D] in {'routing-gate' if use_routing_gates else 'baseline'} mode, "
                         f"got {tuple(cond.shape)}")
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"unet_grad: the operand type is fp16 or bf16, got {dtype}")
    u = prefix + "."
    net = _Net(be, params, prepared)
    lam = float(delta_scale)
    cond16 = cond.to(dtype)
    t = t.reshape(-1)
    if t.shape[0] == 1:
        t = t.expand(x.shape[0])

    res_keys = _resnet_keys(u)
    rows = CG.time_embedding(be, params, t, [k + ".time_emb_proj" for k in res_keys], prefix=u + "time_embedding")
    row_of, off = {}, 0
    for k in res_keys:
        n = params[k + ".time_emb_proj.weight"].shape[0]
        row_of[k] = rows[:, off:off + n]
        off += n

    def resnet(k, h):
        return net.resnet(k, h, row_of[k])

    def transformer(k, h):
        return net.transformer(k, h, cond16, use_routing_gates, lam)

    want_dx = x.requires_grad and torch.is_grad_enabled()      # a training step's latents are data; a gradient check asks
    h = G.conv_in(be, x.float() if want_dx else x.detach().float(), params[u + "conv_in.weight"], params[u + "conv_in.bias"],
                  dtype, **({"data_grad": True} if want_dx else {}))
    skips = [h]
    for i in range(4):
        bp = u + f"down_blocks.{i}"
        for j in range(2):
            h = resnet(f"{bp}.resnets.{j}", h)
            if i < 3:
                h = transformer(f"{bp}.attentions.{j}", h)
            skips.append(h)
        if i < 3:
            k = f"{bp}.downsamplers.0.conv"
            h = G.downsample2d(be, h, params[k + ".weight"], params[k + ".bias"], prepared=net.prep(k + ".weight"))
            skips.append(h)

    h = resnet(u + "mid_block.resnets.0", h)
    h = transformer(u + "mid_block.attentions.0", h)
    h = resnet(u + "mid_block.resnets.1", h)

    for i in range(4):
        bp = u + f"up_blocks.{i}"
        for j in range(3):
            h = resnet(f"{bp}.resnets.{j}", torch.cat([h, skips.pop()], -1))
            if i > 0:
                h = transformer(f"{bp}.attentions.{j}", h)
        if i < 3:
            k = f"{bp}.upsamplers.0.conv"
            h = G.upsample2d(be, h, params[k + ".weight"], params[k + ".bias"], prepared=net.prep(k + ".weight"))

    h = net.gn(u + "conv_norm_out", h, silu=True)
    k = u + "conv_out"
    return G.conv_out(be, h, params[k + ".weight"], params[k + ".bias"], prepared=net.prep(k + ".weight"))
