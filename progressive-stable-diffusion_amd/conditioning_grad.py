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

The fp32 row path (csrc/rows_grad.hip): ``ordinal_embedder`` restates ``AdditiveOrdinalEmbedder.__call__`` over the
``ordinal_embedder.`` masters (``grad_ops.aoe_interp`` and two ``grad_ops.linear_rows`` on fp32 weights, fp32 throughout);
its output, rounded to fp16, is the ``source_aoe`` of ``feature_purifier``, whose gradient of that input flows on into
``base``, ``deltas`` and the projector.  ``time_embedding`` is the UNet's time path: sinusoid -> ``linear_1`` -> SiLU ->
``linear_2`` -> SiLU -> every ``time_emb_proj`` in one product, fp16 weights as in ``engine.time_rows``; the column slices
of its fp32 rows are the ``rowvec`` of the resnets' first convs (``grad_ops.conv3x3(rowvec=)``).

Not here: the frozen CLIP tower; ``training.Trainer`` wires these into a training step.
"""
from __future__ import annotations

import torch

from . import grad_ops as G
from .backend import on_backend


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


def ordinal_embedder(be, params, labels, is_training=False, unconditional=False, noise_std=0.005, num_tokens=16,
                     prefix="ordinal_embedder"):
    """``AdditiveOrdinalEmbedder.__call__`` over the fp32 masters ``base`` [D], ``deltas`` [classes - 1][D] and
    ``projector.{0,2}.{weight,bias}`` under ``prefix``: class interpolation of ``labels`` [B] (or a scalar), the training
    noise (torch, ``is_training`` and ``noise_std > 0``), Linear(D, 2D) -> exact GELU -> Linear(2D, tokens * D) on the fp32
    row kernels -> fp32 [B][tokens][D] ([tokens][D] for a scalar label).  The GELU is the second product's ``act_in``.
    ``unconditional``: ``null_embedding`` expanded to [B][D], torch alone.  Differentiable in every master it reads; the
    module's unused ``norm.*`` gets no gradient, as in the reference, and neither do the labels."""
    p = prefix
    if unconditional:
        return params[p + ".null_embedding"].expand(labels.shape[0] if labels.dim() > 0 else 1, -1)
    scalar = labels.dim() == 0
    emb = G.aoe_interp(be, labels.reshape(1) if scalar else labels, params[p + ".base"], params[p + ".deltas"])
    if is_training and noise_std > 0:
        emb = emb + torch.randn_like(emb) * noise_std
    h = G.linear_rows(be, emb, params[p + ".projector.0.weight"], params[p + ".projector.0.bias"])
    out = G.linear_rows(be, h, params[p + ".projector.2.weight"], params[p + ".projector.2.bias"], act_in=2)
    out = out.view(-1, num_tokens, emb.shape[-1])
    return out[0] if scalar else out


def time_embedding(be, params, t, proj_keys, dim=320, prefix="unet.unet.time_embedding"):
    """The UNet's time path for the int64 timesteps ``t`` [B]: ``timestep_features`` (``dim`` sinusoids) -> ``linear_1``
    -> SiLU -> ``linear_2`` -> SiLU -> ONE product over ``torch.cat`` of the ``time_emb_proj`` masters named by
    ``proj_keys`` (key prefixes, e.g. ``unet.unet.down_blocks.0.resnets.0.time_emb_proj``) -> fp32 rows [B][sum of their
    widths] in the order of ``proj_keys``.  The slice of a resnet's columns is the ``rowvec`` of its first conv.  The
    matrices multiply in fp16 (``weight_dtype``), as in ``engine.time_rows``; each SiLU is the next product's ``act_in``.
    Differentiable in ``linear_1``, ``linear_2`` and every ``time_emb_proj`` weight and bias (autograd splits the
    gradient of the concatenation)."""
    f16 = torch.float16
    t = t.reshape(-1).to(torch.int64).contiguous()
    with on_backend(be):
        feat = be.empty((t.shape[0], dim), torch.float32)
        be.timestep_features(t, feat)
    h = G.linear_rows(be, feat, params[prefix + ".linear_1.weight"], params[prefix + ".linear_1.bias"], weight_dtype=f16)
    h = G.linear_rows(be, h, params[prefix + ".linear_2.weight"], params[prefix + ".linear_2.bias"], act_in=1, weight_dtype=f16)
    w = torch.cat([params[k + ".weight"] for k in proj_keys])
    b = torch.cat([params[k + ".bias"] for k in proj_keys])
    return G.linear_rows(be, h, w, b, act_in=1, weight_dtype=f16)
