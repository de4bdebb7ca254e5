"""TEST-ONLY helper (no tests here): cases, float64 references and a CPU stand-in backend for the attention backward
(csrc/attn_grad.hip, include/dadd_hip_attn_grad.h).

Two references, both float64 from the 16-bit-rounded operands:
  exact : float64 autograd of softmax(q k^T / sqrt(d)) v against dout * scale.
  model : the algebra of the three kernels in plain torch, tiled by 64 like them, with the rounding points the header
          documents: Qs = q * (log2e / sqrt(d)) in fp32 rounded to the storage type; LSE and D kept in fp32; P rounded
          to the storage type as the operand of P^T dO; dS (from the unrounded P) rounded as the operand of dS^T Q and
          dS K; every output rounded once.  Products and sums run in float64: the model does not restate the fp32
          accumulation order or the hardware exp2, which is what the factor 2 of the GPU bound is for.
          ``rounded=False`` switches every rounding off (the model then IS the exact gradient), ``drop_key_tile`` /
          ``drop_query_tile`` leave one tile out of the dq / dkv loops and ``ignore_scale`` forgets do_scale: the broken
          models that show that the bound has teeth.

GPU bound per tensor: rel_l2(kernel, exact) <= max(2 * E_model, ULP[dtype]) with E_model = rel_l2(model, exact).
"""
from __future__ import annotations

import contextlib
import functools
import math
from collections import namedtuple

import torch

from tests import attention_cases as A

F16, BF16, F32, F64 = A.F16, A.BF16, A.F32, A.F64
TILE = 64

# name -> (b, heads, d, nq, nk, do_scale, do_scale_dev, layout)
Case = namedtuple("Case", "name b heads d nq nk do_scale do_scale_dev layout")
CASES = [
    Case("one tile", 1, 2, 40, 64, 64, 1.0, None, "plain"),
    Case("tails both sides", 2, 2, 40, 144, 80, 1.5, None, "plain"),
    Case("pathway shape", 2, 8, 40, 128, 16, 0.3, 0.7, "plain"),
    Case("d = 80", 1, 2, 80, 80, 192, 1.0, None, "plain"),
    Case("d = 160", 1, 2, 160, 80, 144, 1.0, 0.6, "plain"),
    Case("self layout", 2, 2, 40, 192, 192, 1.0, None, "self"),
    Case("peaked", 1, 2, 40, 128, 192, 1.0, None, "peaked"),
]
BY_NAME = {c.name: c for c in CASES}
BF16_CASES = ("tails both sides", "pathway shape", "d = 160")
PEAK_LOGIT = 12.0          # natural units
PEAK_KEY = TILE + 5        # in the second key tile


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm())


def total_scale(case):
    return case.do_scale * (1.0 if case.do_scale_dev is None else case.do_scale_dev)


@functools.lru_cache(maxsize=None)
def inputs(name, dtype):
    """-> (q, k, v, dout): q, dout [b, nq, C], k, v [b, nk, C] in ``dtype``; 0.5 randn operands (moderate logits)."""
    c = BY_NAME[name]
    gen = torch.Generator().manual_seed(4000 + CASES.index(c))
    cc = c.heads * c.d
    q, k, v, do = (0.5 * torch.randn(c.b, n, cc, generator=gen) for n in (c.nq, c.nk, c.nk, c.nq))
    if c.layout == "peaked":     # one key with a logit of about +12 for every row, in the second key tile
        a = A.amplitude(PEAK_LOGIT, c.d)
        q += a
        k[:, PEAK_KEY] += a
    return tuple(t.to(dtype) for t in (q, k, v, do))


def _split(t, heads):
    b, n, c = t.shape
    return t.reshape(b, n, heads, c // heads).transpose(1, 2)


def _merge(t):
    b, h, n, d = t.shape
    return t.transpose(1, 2).reshape(b, n, h * d)


def exact(q, k, v, dout, heads, scale=1.0):
    """float64 autograd -> (dq, dk, dv) [b, n, C]."""
    d = q.shape[-1] // heads
    q64, k64, v64 = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    with torch.enable_grad():          # (also called from inside an autograd backward, by CpuAttnBackend)
        s = _split(q64, heads) @ _split(k64, heads).transpose(-1, -2) / math.sqrt(d)
        out = _merge(torch.softmax(s, dim=-1) @ _split(v64, heads))
    out.backward(dout.detach().double() * scale)
    return q64.grad, k64.grad, v64.grad


def model(q, k, v, dout, heads, scale=1.0, rounded=True, drop_key_tile=None, drop_query_tile=None, ignore_scale=False):
    """The three kernels' algebra -> (dq, dk, dv) float64 [b, n, C]."""
    dt, d = q.dtype, q.shape[-1] // heads
    r16 = (lambda x: x.float().to(dt).double()) if rounded else (lambda x: x)
    r32 = (lambda x: x.float().double()) if rounded else (lambda x: x)
    sc = 1.0 if ignore_scale else float(r32(torch.tensor(scale, dtype=F64)))
    qh, kh, vh, oh = (_split(t, heads).double() for t in (q, k, v, dout))
    qs = _split(A.scaled_q(q, d), heads).double() if rounded else qh * (A.LOG2E / math.sqrt(d))
    nq, nk = qh.shape[2], kh.shape[2]
    qtiles, ktiles = list(range(0, nq, TILE)), list(range(0, nk, TILE))
    # launch 1: LSE (log2 units) and D by the online recurrence over the key tiles
    m = torch.full(qh.shape[:3], -1e30, dtype=F64)
    l, dacc = torch.zeros_like(m), torch.zeros_like(m)
    for k0 in ktiles:
        s = qs @ kh[:, :, k0:k0 + TILE].transpose(-1, -2)
        dp = oh @ vh[:, :, k0:k0 + TILE].transpose(-1, -2)
        mn = torch.maximum(m, s.max(dim=-1).values)
        alpha = torch.exp2(m - mn)
        p = torch.exp2(s - mn[..., None])
        l, dacc, m = l * alpha + p.sum(-1), dacc * alpha + (p * dp).sum(-1), mn
    lse, dd = r32(m + torch.log2(l)), r32(sc * dacc / l)

    def tile(q0, k0):
        qsl, ksl = slice(q0, q0 + TILE), slice(k0, k0 + TILE)
        p = torch.exp2(qs[:, :, qsl] @ kh[:, :, ksl].transpose(-1, -2) - lse[:, :, qsl, None])
        dp = oh[:, :, qsl] @ vh[:, :, ksl].transpose(-1, -2)
        return p, p * (sc * dp - dd[:, :, qsl, None])

    # launch 2: dK, dV per key tile over the query tiles
    dk, dv = torch.zeros_like(kh), torch.zeros_like(vh)
    for k0 in ktiles:
        for q0 in qtiles:
            if drop_query_tile is not None and q0 == drop_query_tile * TILE:
                continue
            p, ds = tile(q0, k0)
            dv[:, :, k0:k0 + TILE] += r16(p).transpose(-1, -2) @ oh[:, :, q0:q0 + TILE]
            dk[:, :, k0:k0 + TILE] += r16(ds).transpose(-1, -2) @ qh[:, :, q0:q0 + TILE]
    # launch 3: dQ per query tile over the key tiles
    dq = torch.zeros_like(qh)
    for q0 in qtiles:
        for k0 in ktiles:
            if drop_key_tile is not None and k0 == drop_key_tile * TILE:
                continue
            _, ds = tile(q0, k0)
            dq[:, :, q0:q0 + TILE] += r16(ds) @ kh[:, :, k0:k0 + TILE]
    inv = float(r32(torch.tensor(1.0 / math.sqrt(d), dtype=F64)))
    return tuple(_merge(r16(t)) for t in (dq * inv, dk * inv, dv * sc))


Reference = namedtuple("Reference", "exact e_model bound")


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """-> Reference(exact (dq, dk, dv), E_model per tensor, bound per tensor) of a case; computed once per process."""
    c = BY_NAME[name]
    q, k, v, do = inputs(name, dtype)
    ex = exact(q, k, v, do, c.heads, total_scale(c))
    mo = model(q, k, v, do, c.heads, total_scale(c))
    e = tuple(rel_l2(a, b) for a, b in zip(mo, ex))
    return Reference(ex, e, tuple(max(2.0 * x, A.ULP[dtype]) for x in e))


# ---- the triple-pathway composition -----------------------------------------------------------------------------------
def tri_paths(c, gates, lam, mode):
    """(first token, tokens, first K column (V follows), scale of dy) per pathway, as grad_ops composes them."""
    if mode == 0:
        paths = [(16, 16, 0, float(gates[0])), (0, 16, 2 * c, float(gates[1]))]
        if lam != 0.0:
            paths.append((32, 16, 2 * c, float(lam)))
        return paths
    return [(0, 32, 0, 1.0)]


def tri_compose(q, kv, dy, gates, lam, mode, heads, grad=exact):
    """One attention gradient per pathway on its slice of kv -> (dq, dkv) float64; slices nobody reads stay zero."""
    c = q.shape[-1]
    dq, dkv = torch.zeros(q.shape, dtype=F64), torch.zeros(kv.shape, dtype=F64)
    for t0, nt, kc, scale in tri_paths(c, gates, lam, mode):
        g = grad(q, kv[:, t0:t0 + nt, kc:kc + c], kv[:, t0:t0 + nt, kc + c:kc + 2 * c], dy, heads, scale)
        dq += g[0]
        dkv[:, t0:t0 + nt, kc:kc + c] += g[1]
        dkv[:, t0:t0 + nt, kc + c:kc + 2 * c] += g[2]
    return dq, dkv


def tri_exact(q, kv, dy, gates, lam, mode, heads):
    """float64 autograd of the formula of dadd_tri_xattn (tests/attention_cases.xattn_reference) -> (dq, dkv)."""
    q64, kv64 = q.detach().double().clone().requires_grad_(True), kv.detach().double().clone().requires_grad_(True)
    A.xattn_reference(q64, kv64, gates, lam, mode, heads).backward(dy.double())
    return q64.grad, (kv64.grad if kv64.grad is not None else torch.zeros_like(kv64))


class CpuAttnBackend:
    """Stand-in for ``HipBackend`` under the attention operators of ``grad_ops``: the same method names on CPU tensors,
    float64 inside, outputs rounded to the tensors' type.  It lets the CPU suite run the operators' own code: the slices,
    scales and strides they hand to ``attn_grad``."""

    def __init__(self):
        self.calls = []

    def wait_current(self):
        pass

    def release_to_current(self):
        pass

    def ctx(self):
        return contextlib.nullcontext()

    def empty(self, shape, dtype):
        return torch.full(tuple(shape), float("nan"), dtype=dtype)

    def zeros(self, shape, dtype):
        return torch.zeros(tuple(shape), dtype=dtype)

    @staticmethod
    def attn_grad_ws_numel(b, heads, nq):
        return b * heads * nq * 2

    def self_attn(self, qkv, out, heads):
        c = out.shape[-1]
        self.attention(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], out, heads)

    def attention(self, q, k, v, out, heads):
        d = q.shape[-1] // heads
        s = _split(q.double(), heads) @ _split(k.double(), heads).transpose(-1, -2) / math.sqrt(d)
        out.copy_(_merge(torch.softmax(s, dim=-1) @ _split(v.double(), heads)))

    def tri_xattn(self, q, kv, out, gates, lam, mode, heads, lam_dev=None):
        out.copy_(A.xattn_reference(q, kv, gates, lam, mode, heads))

    def attn_grad(self, q, k, v, dout, *, dq=None, dk=None, dv=None, ws, heads, do_scale=1.0, do_scale_dev=None):
        assert ws.numel() >= self.attn_grad_ws_numel(q.shape[0], heads, q.shape[1]) and ws.dtype == F32
        scale = do_scale * (1.0 if do_scale_dev is None else float(do_scale_dev[0]))
        self.calls.append(dict(nq=q.shape[1], nk=k.shape[1], scale=scale, outputs=tuple(t is not None for t in (dq, dk, dv))))
        for dst, g in zip((dq, dk, dv), exact(q, k, v, dout, heads, scale)):
            if dst is not None:
                dst.copy_(g)
