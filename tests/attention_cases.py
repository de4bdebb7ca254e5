"""TEST-ONLY helper (no tests here): inputs with PLACED logits, float64 references and the variant table of the
attention kernels (csrc/attention.hip, compiled for fp16 and bf16).

The flash kernel's result depends on where the large logits sit: tile 0 sets the reference maximum, later 64-key tiles
move it only when an exponent exceeds 8 (log2 units), the last tile may be ragged.  The builders below put the row
maximum into a chosen tile, on either side of the re-centring threshold, or far below zero, so that the tests can say
which branch of the recurrence a case runs.

Common direction u = ones(d):  q = 0.5 randn + a u,  chosen keys k_j = 0.5 randn -/+ a u  with a = sqrt(L / sqrt(d)),
so that q . k_j / sqrt(d) ~ -/+ L (natural units; 1 natural unit = 1.4427 log2 units).

References, both float64 from the rounded operands:
  exact : softmax(q k^T / sqrt(d)) v
  model : the same with the kernel's two documented rounding points: q * (log2e / sqrt(d)) computed in fp32 and rounded
          to the storage type (the scale rides on Q), and P = exp2(s - rowmax) rounded to the storage type before P v
          and before the row sum.
"""
from __future__ import annotations

import math
import os
import re
from collections import namedtuple

import torch

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
LOG2E = 1.4426950408889634
TILE = 64                       # keys per tile of flash_kernel
RECENTRE = 8.0                  # the reference maximum moves when an exponent exceeds this (log2 units)
# the project's existing numbers: test_self_attention (fp16), test_self_attention_bf16
TOL = {F16: (3e-3, 3e-3), BF16: (2e-2, 2e-2)}
# one rounding of the storage type, relative (half an ulp is 2^-11 / 2^-8; a whole one is allowed)
ULP = {F16: 2.0 ** -10, BF16: 2.0 ** -7}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTENTION_HIP = os.path.join(ROOT, "progressive-stable-diffusion_amd", "csrc", "attention.hip")


# ------------------------------------------------------------------------------------------------ variant table
class Variant(namedtuple("Variant", "d qf prefetch nw b heads nq")):
    """One instantiation flash_kernel<d, qf, prefetch, nw> and a (b, heads, nq) that dadd_attn_* maps to it."""

    @property
    def key(self):
        return (self.d, self.qf, self.prefetch, self.nw)

    def kernel_name(self, dtype):
        base = "flash_kernel" + ("_bf16" if dtype == BF16 else "")
        return f"{base}<{self.d}, {self.qf}, {'true' if self.prefetch else 'false'}" + \
            ("" if self.nw == 4 else f", {self.nw}") + ">"

    def label(self, dtype):
        return f"{'bf16' if dtype == BF16 else 'f16'}-d{self.d}q{self.qf}w{self.nw}"


# d = 40: eight waves once b * heads * ceil(nq / 256) >= 512;  d = 160: 32 queries per wave once
# b * heads * ceil(nq / 128) >= 256.  nq != nk in the tests, so the variant is picked by nq while nk stays small.
_BIG40 = dict(b=1, heads=64, nq=2011)        # 64 * 8 = 512
_BIG160 = dict(b=2, heads=8, nq=2011)        # 16 * 16 = 256
_SMALL = dict(b=2, heads=8, nq=200)
VARIANTS = {
    F16: [Variant(40, 2, True, 8, **_BIG40), Variant(40, 2, True, 4, **_SMALL), Variant(64, 2, True, 4, **_SMALL),
          Variant(80, 2, True, 4, **_SMALL), Variant(96, 1, True, 4, **_SMALL), Variant(160, 2, True, 4, **_BIG160),
          Variant(160, 1, True, 4, **_SMALL), Variant(512, 1, False, 4, b=2, heads=2, nq=200)],
    BF16: [Variant(40, 2, True, 8, **_BIG40), Variant(40, 2, True, 4, **_SMALL), Variant(80, 2, True, 4, **_SMALL),
           Variant(160, 2, True, 4, **_BIG160), Variant(160, 1, True, 4, **_SMALL)],
}
# registered, but not reachable from a test process: reason
NOT_REACHED_IN_PROCESS = {
    (40, 4, True, 4): "chosen only with DADD_FLASH40=0 in the environment, which the library reads once per process",
}


def registered_variants(dtype, path=ATTENTION_HIP):
    """The (d, qf, prefetch, nw) that dadd_init_attention() registers, read from the source with the `#ifndef DADD_BF16`
    blocks taken (fp16) or left out (bf16)."""
    text = open(path).read()
    body = text[text.index("int dadd_init_attention()"):]
    body = body[:body.index("\n}")]
    out, skip = set(), False
    for line in body.splitlines():
        s = line.strip()
        if s.startswith("#ifndef DADD_BF16"):
            skip = dtype == BF16
        elif s.startswith("#ifdef DADD_BF16"):
            skip = dtype != BF16
        elif s.startswith("#else"):
            skip = not skip
        elif s.startswith("#endif"):
            skip = False
        elif not skip:
            for m in re.finditer(r"flash_attr<\s*(\d+)\s*,\s*(\d+)\s*,\s*(true|false)\s*(?:,\s*(\d+)\s*)?>", s):
                out.add((int(m.group(1)), int(m.group(2)), m.group(3) == "true", int(m.group(4) or 4)))
    return out


# ------------------------------------------------------------------------------------------------ references
def scale_log2(d):
    """log2(e) / sqrt(d) as the library computes it: in fp32."""
    return torch.tensor(LOG2E, dtype=F32) / torch.sqrt(torch.tensor(float(d), dtype=F32))


def scaled_q(q, d):
    """What the kernel multiplies K with: q * scale in fp32, rounded to the storage type."""
    return (q.float() * scale_log2(d).to(q.device)).to(q.dtype)


def _split(t, heads):
    b, n, c = t.shape
    return t.reshape(b, n, heads, c // heads).transpose(1, 2)        # [b, heads, n, d]


def model_logits(q, k, heads):
    """float64 exponents (log2 units) of the model reference: [b, heads, nq, nk]."""
    d = q.shape[-1] // heads
    return _split(scaled_q(q, d), heads).double() @ _split(k, heads).double().transpose(-1, -2)


def exact_logits(q, k, heads):
    """float64 logits (natural units) of the exact reference."""
    d = q.shape[-1] // heads
    return _split(q, heads).double() @ _split(k, heads).double().transpose(-1, -2) / math.sqrt(d)


def references(q, k, v, heads, max_elems=1 << 26):
    """-> (exact, model), float64 [b, nq, c], computed where q lives; (batch, head) slices are taken in chunks of at
    most ``max_elems`` scores so that the product shapes fit."""
    b, nq, c = q.shape
    nk, d, dt = k.shape[1], c // heads, q.dtype
    exact = torch.empty(b, heads, nq, d, dtype=F64, device=q.device)
    model = torch.empty_like(exact)
    qh, kh, vh = _split(q, heads), _split(k, heads), _split(v, heads)
    qs = _split(scaled_q(q, d), heads)
    hstep = max(1, min(heads, max_elems // (nq * nk)))
    for bi in range(b):
        for h0 in range(0, heads, hstep):
            sl = (bi, slice(h0, h0 + hstep))
            kt, vv = kh[sl].double().transpose(-1, -2), vh[sl].double()
            exact[sl] = torch.softmax(qh[sl].double() @ kt / math.sqrt(d), dim=-1) @ vv
            s = qs[sl].double() @ kt
            p = torch.exp2(s - s.max(dim=-1, keepdim=True).values).float().to(dt).double()
            model[sl] = (p @ vv) / p.sum(dim=-1, keepdim=True)
    return (exact.transpose(1, 2).reshape(b, nq, c), model.transpose(1, 2).reshape(b, nq, c))


def within(got, ref, dtype):
    """-> (ok, message): |got - ref| <= atol + rtol |ref| elementwise with the project's numbers for ``dtype``."""
    atol, rtol = TOL[dtype]
    got, ref = got.double(), ref.double().to(got.device)
    err = (got - ref).abs()
    bad = ~(err <= atol + rtol * ref.abs())          # NaN counts as bad
    if not bool(bad.any()):
        return True, ""
    i = int(torch.where(bad.flatten())[0][0])
    return False, (f"{int(bad.sum())}/{bad.numel()} off, max err {float(err.nan_to_num(float('inf')).max()):.4e}; first at "
                   f"{i}: got {float(got.flatten()[i]):.5e} ref {float(ref.flatten()[i]):.5e}")


# ------------------------------------------------------------------------------------------------ flash inputs
def amplitude(L, d):
    """a with  (a u) . (a u) / sqrt(d) = L  for u = ones(d)."""
    return math.sqrt(L / math.sqrt(d))


def _tile_levels(nk, delta, descending):
    """Target maximum (log2 units) of each 64-key tile: tile t is t * delta above (staircase) or below (descending)
    tile 0; centred on zero so that the operands stay small."""
    nt = (nk + TILE - 1) // TILE
    lv = (torch.arange(nt, dtype=F64) - (nt - 1) / 2.0) * delta
    return -lv if descending else lv


def step_positions(nk):
    """The one key per tile that carries the tile's maximum (inside the valid part of a ragged last tile)."""
    nt = (nk + TILE - 1) // TILE
    return [t * TILE + (7 * t + 3) % min(TILE, nk - t * TILE) for t in range(nt)]


def _placed_keys(target, qs_entry, d, dtype, gen, noise):
    """Keys [..., d] in ``dtype`` whose entries sum to target / qs_entry: against a query with d equal entries
    ``qs_entry`` (the rounded, pre-scaled q) the exponent is ``target`` up to the rounding of ONE small entry - the
    last one absorbs what rounding the others left over."""
    want = target / qs_entry                                         # float64 sums
    r = 0.5 * torch.randn(*target.shape, d, generator=gen).double() * noise[..., None]
    r = r - r.mean(dim=-1, keepdim=True)
    k = (r + want[..., None] / d).float().to(dtype)
    rest = want - k[..., :-1].double().sum(dim=-1)
    k[..., -1] = rest.float().to(dtype)
    return k


PATTERNS = ("first_tile_floor", "all_floor", "one_hot", "staircase", "descending", "flat", "random_spiky")


def build(pattern, arg, b, heads, d, nq, nk, dtype, seed=0):
    """-> (q [b, nq, heads*d], k, v [b, nk, heads*d]) in ``dtype``.  ``arg``: L (natural units) for the floors, the key
    index for one_hot (negative: from the end), delta (log2 units) for staircase / descending."""
    gen = torch.Generator().manual_seed(1000 + seed)
    rn = lambda n: torch.randn(b, n, heads, d, generator=gen)        # noqa: E731
    if pattern == "random_spiky":                                    # what test_self_attention draws
        q, k, v = rn(nq), rn(nk), rn(nk)
        k[0, nk // 3] *= 4.0
    elif pattern in ("staircase", "descending"):
        q = torch.ones(b, nq, heads, d)                              # a u with a = 1: no random part
        qs = float(scaled_q(q[:1, :1, :1, :1].to(dtype), d).double())
        lv = _tile_levels(nk, float(arg), pattern == "descending")
        target = lv[torch.arange(nk) // TILE] - (1.0 + 5.0 * torch.rand(nk, generator=gen).double())
        noise = torch.ones(nk, dtype=F64)
        pos = step_positions(nk)
        target[pos] = lv
        noise[pos] = 0.0
        target = target[None, :, None].expand(b, nk, heads)
        noise = noise[None, :, None].expand(b, nk, heads)
        k, v = _placed_keys(target, qs, d, dtype, gen, noise), rn(nk)
    else:
        q, k, v = 0.5 * rn(nq), 0.5 * rn(nk), rn(nk)
        if pattern == "flat":
            q.zero_()
        elif pattern == "first_tile_floor":
            a = amplitude(float(arg), d)
            q += a
            k[:, :TILE] -= a
        elif pattern == "all_floor":
            a = amplitude(float(arg), d)
            q += a
            k -= a
        elif pattern == "one_hot":
            a = amplitude(150.0, d)
            q += a
            k[:, int(arg) % nk] += a
        else:
            raise ValueError(pattern)
    return tuple(t.to(dtype).reshape(t.shape[0], t.shape[1], heads * d) for t in (q, k, v))


def flash_patterns(nk):
    """(pattern, arg) pairs for ``nk`` keys.  one_hot positions beyond the last key do not exist for the short key
    counts; the last key is always there (on a ragged nk it puts the re-centring into the masked tile)."""
    pats = [("first_tile_floor", L) for L in (80, 100, 150, 300)] + [("all_floor", 150)]
    pats += [("one_hot", p) for p in sorted({p for p in (0, 63, 64, nk - 1) if p < nk})]
    pats += [("staircase", 7.5), ("staircase", 8.5), ("descending", 10.0), ("flat", 0), ("random_spiky", 0)]
    return pats


# ------------------------------------------------------------------------------------------------ tri_xattn
XATTN_PATTERNS = ("flat", "one_hot", "all_floor", "one_floor")


def build_xattn(pattern, b, n, heads, d, mode, dtype, seed=0):
    """-> (q [b, n, C], kv) for xattn_kernel.  mode 0 (split): kv [b, 48, 4C], tokens 16..31 anatomy (K cols 0..C, V
    C..2C), tokens 0..15 disease and 32..47 delta (K 2C..3C, V 3C..4C), one softmax per sixteen keys; mode 1
    (baseline): kv [b, 32, 2C], one softmax over the 32 keys.  ``one_floor``: the disease pathway (mode 1: keys
    0..15) at ~ -150, the others random."""
    gen = torch.Generator().manual_seed(2000 + seed)
    c = heads * d
    t_tok, ld = (48, 4 * c) if mode == 0 else (32, 2 * c)
    q, kv = 0.5 * torch.randn(b, n, c, generator=gen), 0.5 * torch.randn(b, t_tok, ld, generator=gen)
    kcols = [(slice(16, 32), slice(0, c)), (slice(0, 16), slice(2 * c, 3 * c)), (slice(32, 48), slice(2 * c, 3 * c))] \
        if mode == 0 else [(slice(0, 16), slice(0, c)), (slice(16, 32), slice(0, c))]
    vcol = slice(c, 2 * c)
    kv[:, :, vcol] *= 2.0
    if mode == 0:
        kv[:, :, 3 * c:] *= 2.0
    a = amplitude(150.0, d)
    if pattern == "flat":
        q.zero_()
    elif pattern == "one_hot":               # one key per sixteen at ~ +150
        q += a
        for i, (tok, col) in enumerate(kcols):
            kv[:, tok.start + (5 * i + 3) % 16, col] += a
    elif pattern == "all_floor":
        q += a
        for tok, col in kcols:
            kv[:, tok, col] -= a
    elif pattern == "one_floor":
        q += a
        tok, col = kcols[1] if mode == 0 else kcols[0]
        kv[:, tok, col] -= a
    else:
        raise ValueError(pattern)
    return q.to(dtype), kv.to(dtype)


def xattn_reference(q, kv, gates, lam, mode, heads):
    """float64 restatement of TorchRefBackend.tri_xattn."""
    b, n, c = q.shape
    d = c // heads
    qh = _split(q, heads).double()

    def path(tok0, ntok, kcol, vcol):
        k = _split(kv[:, tok0:tok0 + ntok, kcol:kcol + c], heads).double()
        v = _split(kv[:, tok0:tok0 + ntok, vcol:vcol + c], heads).double()
        return torch.softmax(qh @ k.transpose(-1, -2) / math.sqrt(d), dim=-1) @ v

    if mode == 0:
        z = float(gates[0]) * path(16, 16, 0, c) + float(gates[1]) * path(0, 16, 2 * c, 3 * c)
        if lam != 0.0:
            z = z + lam * path(32, 16, 2 * c, 3 * c)
    else:
        z = path(0, 32, 0, c)
    return z.transpose(1, 2).reshape(b, n, c)
