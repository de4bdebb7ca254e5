"""Differentiable restatements of the trainable conditioning front-end (``FeaturePurifier``, ``ImageProjectionPlus``,
``ImageProjection``), built from the operators of ``grad_ops`` alone: the two parameter groups the reference trains at
twice the base learning rate (``image_projection.`` and ``feature_purifier.``, ``optim.reference_param_groups``).

Each function takes the backend and ``params``, a mapping from the reference's state-dict key names to the **fp32
master** tensors (leaves, or views of an ``optim.ParamArena``), and 16-bit inputs on the backend's device.  Unlike the
inference classes of ``conditioning.py`` nothing is folded or fused: every LayerNorm is a ``grad_ops.layer_norm`` on its
own masters, so that they receive their own gradients; the packed ``in_proj_weight`` / ``in_proj_bias`` of an
``nn.MultiheadAttention`` are sliced as torch views of the one master, into which autograd accumulates; ``cat``, the
residual additions (in the 16-bit type) and ``latents.expand`` are torch plumbing.  The attention is d = E / heads = 96
for the reference's 768 channels and 8 heads, against 16 AOE tokens (purifier) or the 257 CLIP tokens (resampler):
``grad_ops.attention`` takes any key count.  The forward of attention at d = 96 exists in fp16 only, so these run in fp16.

Not here: the ``ordinal_embedder.`` path (``aoe_interp`` and the fp32 ``linear_rows`` projector have no backward yet), the
frozen CLIP tower and the wiring into ``training_step``.  ``feature_purifier`` returns the gradient of
its ``source_aoe`` input, where the embedder attaches.
"""
from __future__ import annotations

import torch

from . import grad_ops as G


def _lin(be, params, key, x):
    return G.linear(be, x, params[key + ".weight"], params.get(key + ".bias"))


def _ln(be, params, key, x, eps=1e-5):
    return G.layer_norm(be, x, params[key + ".weight"], params[key + ".bias"], eps)


def mha(be, params, key, q_in, kv_in, heads):
    """``nn.MultiheadAttention(batch_first=True)`` with packed in_proj, no mask, no dropout: q_in [B,Nq,E] against
    kv_in [B,Nk,E].  Rows [0, E) of the packed master project the queries, rows [E, 3E) the keys and values in one
    product; the slices are views, so the master gets one gradient."""
    e = q_in.shape[-1]
    w, b = params[key + ".in_proj_weight"], params[key + ".in_proj_bias"]
    q = G.linear(be, q_in, w[:e], b[:e])
    kv = G.linear(be, kv_in, w[e:], b[e:])
    o = G.attention(be, q, kv[..., :e], kv[..., e:], heads)
    return _lin(be, params, key + ".out_proj", o)


def feature_purifier(be, params, image_embeds16, source_aoe16, heads=8, prefix="feature_purifier"):
    """LN -> MHA(q = img, kv = aoe) -> gate MLP (Linear, GELU, Linear) -> LN(img - sigmoid(z) * dis): image_embeds16
    [B,N,E] and source_aoe16 [B,Na,E] in fp16 -> fp32 [B,N,E].  Differentiable in every parameter under ``prefix`` and in
    both inputs."""
    p = prefix
    img_n = _ln(be, params, p + ".norm_img", image_embeds16)
    aoe_n = _ln(be, params, p + ".norm_aoe", source_aoe16)
    dis = mha(be, params, p + ".cross_attn", img_n, aoe_n, heads)
    h = G.gelu(be, _lin(be, params, p + ".gate.0", torch.cat([dis, img_n], -1)))
    z = _lin(be, params, p + ".gate.2", h)
    return G.purifier_gate_tail(be, image_embeds16, dis, z, params[p + ".norm_out.weight"], params[p + ".norm_out.bias"])


def image_projection_plus(be, params, hidden16, heads=8, prefix="image_projection"):
    """The Perceiver resampler: proj_in (when present), depth x {pre-LN MHA of the latents against the context + residual,
    pre-LN MLP (Linear, GELU, Linear) + residual}, LN: hidden16 [B,T,Cin] in fp16 -> fp16 [B,tokens,E].  Differentiable in
    every parameter under ``prefix`` (the latents and the packed in_proj masters included) and in ``hidden16``."""
    p = prefix
    x = _lin(be, params, p + ".proj_in", hidden16) if (p + ".proj_in.weight") in params else hidden16
    lat = params[p + ".latents"].expand(hidden16.shape[0], -1, -1).to(hidden16.dtype)
    i = 0
    while (p + f".layers.{i}.norm1.weight") in params:
        lp = p + f".layers.{i}"
        lat = lat + mha(be, params, lp + ".cross_attn", _ln(be, params, lp + ".norm1", lat), x, heads)
        h = G.gelu(be, _lin(be, params, lp + ".ff.0", _ln(be, params, lp + ".norm2", lat)))
        lat = lat + _lin(be, params, lp + ".ff.2", h)
        i += 1
    return _ln(be, params, p + ".norm_out", lat)


def image_projection(be, params, image_embeds16, num_tokens=16, prefix="image_projection"):
    """Linear -> [B,tokens,D] -> LN: image_embeds16 [B,Cin] in fp16 -> fp16 [B,tokens,D].  Differentiable in the
    parameters under ``prefix`` and in the input."""
    p = prefix
    d = params[p + ".norm.weight"].shape[0]
    x = _lin(be, params, p + ".projection", image_embeds16).reshape(-1, num_tokens, d)
    return _ln(be, params, p + ".norm", x)
