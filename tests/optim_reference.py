"""Float64 restatement of the optimizer step of csrc/optim.hip (include/dadd_hip_optim.h), a CPU model of the kernel's
rounding points in fp32, and the bounds the GPU suite holds the kernel to.  The bounds are derived, not fitted.

One step, per element, with c the clip / unscale coefficient and the group's lr, beta1, beta2, eps, wd at step t:
    g' = g c;  p = p (1 - lr wd);  m = m + (g' - m)(1 - beta1);  v = v beta2 + g' g' (1 - beta2)
    p = p - lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps);  ema = ema + (p - ema)(1 - ema_decay)
``ref_step64`` evaluates this in float64 on the fp32 inputs with the hyper-parameters as Python doubles.
``model_step32`` evaluates it in torch fp32 in the kernel's order with the kernel's fp32 constants (``kernel_consts``).

Elementwise bounds against float64 (u = 2^-24, the unit roundoff of fp32):
    |p - p64|     <= 2 ulp32(|p64|) + 16 u step_size (|m_old| + |c g|) / (sqrt(v64) rsqrt_bc2 + eps)
                     two roundings of p (the decay product and the final subtraction) plus the rounded constant decay;
                     about a dozen roundings on the update term (g', the difference, the product, the sum of m; the five
                     of v halved by the square root; sqrt, product, sum, quotient, product; the constants lr, step_size,
                     rsqrt_bc2), the cancellation in m bounded by the magnitudes of its terms
    |m - m64|     <= 4 u (|m_old| + |c g|)                four roundings, each below the magnitudes of the terms
    |v - v64|     <= 8 u v64                              five roundings and the constants beta2, 1 - beta2; all terms >= 0
    |ema - ema64| <= 2 ulp32(|ema64|) + 2 u |p64 - ema_old| + (1 - ema_decay) * (the bound of p)
                     the sum and the product's share of it; difference, product and the rounded weight; the error of p
    p16 bit-equal to p.to(dtype) of the kernel's own p.
Norm: |grad_norm - norm64| <= 32 u norm64.  The terms are non-negative; a chunk partial is SUM_DEPTH = 24 fp32 additions
deep (15 in a lane over its 16 squares, 6 across the wave, 3 across the four waves) plus the rounding of each square, the
partials combine in double, the square root halves the relative error and adds one rounding to fp32: (24 + 1) / 2 + 1
= 13.5 u at worst, bound 32 u.  coef: relative 40 u against the float64 rule (the norm's 32 u plus the final rounding).
"""
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import torch

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
CHUNK = 4096
SUM_DEPTH = 24            # 15 + 6 + 3 additions per chunk partial at CHUNK = 4096 with 256 lanes
NORM_REL = 32 * U
COEF_REL = 40 * U
EMA_DECAY = 0.999
SIZES = (1, 7, 8, 9, 4095, 4096, 4097)      # tensor sizes of the layout and chunk-edge cases


@dataclass
class Hyper:
    lr: float
    wd: float
    b1: float = 0.9
    b2: float = 0.999
    eps: float = 1e-8


def f32r(x: float) -> float:
    """x rounded to fp32, as a Python float."""
    return float(torch.tensor(x, dtype=F64).to(F32))


def true_consts(h: Hyper, t: int) -> Dict[str, float]:
    return dict(decay=1 - h.lr * h.wd, omb1=1 - h.b1, beta2=h.b2, omb2=1 - h.b2, eps=h.eps,
                step_size=h.lr / (1 - h.b1 ** t), rsqrt_bc2=1 / math.sqrt(1 - h.b2 ** t))


def kernel_consts(h: Hyper, t: int) -> Dict[str, float]:
    """The fp32 constants dadd_optim_finalize leaves in the state block: the host's values rounded to fp32, the derived
    ones computed in double from those and rounded once."""
    lr, wd, omb1, omb2 = f32r(h.lr), f32r(h.wd), f32r(1 - h.b1), f32r(1 - h.b2)
    return dict(decay=f32r(1 - lr * wd), omb1=omb1, beta2=f32r(h.b2), omb2=omb2, eps=f32r(h.eps),
                step_size=f32r(lr / (1 - (1 - omb1) ** t)), rsqrt_bc2=f32r(1 / math.sqrt(1 - (1 - omb2) ** t)))


def expand(consts: Sequence[Dict[str, float]], sizes: Sequence[int], dtype) -> Dict[str, torch.Tensor]:
    """Per-element constants of an arena whose group k holds sizes[k] elements."""
    return {k: torch.cat([torch.full((n,), c[k], dtype=dtype) for c, n in zip(consts, sizes)]) for k in consts[0]}


def ref_step64(p, g, m, v, ema, c, K, ema_w=None):
    """-> dict p, m, v, ema (float64) and what the bounds need: cg = |c g|, den.  K: ``true_consts`` (or ``expand`` of)."""
    p, g, m, v = (x.double() for x in (p, g, m, v))
    gs = g * float(c)
    m2 = m + (gs - m) * K["omb1"]
    v2 = v * K["beta2"] + gs * gs * K["omb2"]
    den = v2.sqrt() * K["rsqrt_bc2"] + K["eps"]
    p2 = p * K["decay"] - K["step_size"] * m2 / den
    out = dict(p=p2, m=m2, v=v2, cg=gs.abs(), den=den, m_old=m.abs(), step_size=K["step_size"], ema=None)
    if ema is not None:
        e = ema.double()
        out.update(ema=e + (p2 - e) * ema_w, ema_old=e, ema_w=ema_w)
    return out


def model_step32(p, g, m, v, ema, c, K, ema_w=None):
    """The kernel's arithmetic in torch fp32, one rounding per operation, in the kernel's order.  K: ``kernel_consts``
    (or ``expand`` of, in fp32); c: an fp32-representable float."""
    assert all(x.dtype == F32 for x in (p, g, m, v))
    gs = g * f32r(c)
    p = p * K["decay"]
    m = m + (gs - m) * K["omb1"]
    v = v * K["beta2"] + (gs * gs) * K["omb2"]
    den = v.sqrt() * K["rsqrt_bc2"] + K["eps"]
    p = p - K["step_size"] * (m / den)
    e = None if ema is None else ema + (p - ema) * f32r(ema_w)
    return dict(p=p, m=m, v=v, ema=e)


def ulp32(x64: torch.Tensor) -> torch.Tensor:
    return 2.0 ** -23 * 2.0 ** torch.floor(torch.log2(x64.abs().clamp_min(2.0 ** -126)))


def bounds(ref) -> Dict[str, torch.Tensor]:
    bp = 2 * ulp32(ref["p"]) + 16 * U * ref["step_size"] * (ref["m_old"] + ref["cg"]) / ref["den"]
    b = dict(p=bp, m=4 * U * (ref["m_old"] + ref["cg"]), v=8 * U * ref["v"])
    if ref["ema"] is not None:
        b["ema"] = 2 * ulp32(ref["ema"]) + 2 * U * (ref["p"] - ref["ema_old"]).abs() + ref["ema_w"] * bp
    return b


def worst_ratios(got, ref) -> Dict[str, float]:
    """max |got - ref| / bound per array; inf where an element with a zero bound is not exact."""
    out = {}
    for k, b in bounds(ref).items():
        err = (got[k].double() - ref[k]).abs()
        ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf),
                                                                         torch.zeros_like(err)))
        assert not torch.isnan(ratio).any(), k
        out[k] = float(ratio.max())
    return out


def check_step(got, ref, what) -> Dict[str, float]:
    r = worst_ratios(got, ref)
    print(f"{what}: worst error / bound " + ", ".join(f"{k} {x:.3f}" for k, x in r.items()))
    for k, x in r.items():
        assert x <= 1.0, f"{what}: {k} is {x:.3f} times its bound"
    return r


# ---- norm and coefficient ---------------------------------------------------------------------------------------------
def norm64(g: torch.Tensor, scale: float = 0.0) -> float:
    return math.sqrt(float(g.double().pow(2).sum())) * (1.0 if scale == 0 else 1.0 / scale)


def coef64(norm: float, max_norm: float, scale: float = 0.0) -> float:
    inv = 1.0 if scale == 0 else 1.0 / scale
    return inv * (min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0)


def model_partials(g: torch.Tensor) -> torch.Tensor:
    """Chunk partials of sum g^2 in the kernel's order in fp32: lane l of 256 adds the squares of elements
    4 (256 j + l) + e for j, e in 0..3 in that order, a butterfly over the 64 lanes of a wave (offsets 32 .. 1), then the
    four waves left to right."""
    x = g.reshape(-1, 4, 256, 4)                       # [chunk][j][lane][e]
    sq = (x * x).permute(0, 2, 1, 3).reshape(-1, 256, 16)
    s = sq[..., 0]
    for i in range(1, 16):
        s = s + sq[..., i]
    s = s.reshape(-1, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., torch.arange(64) ^ o]
    w = s[..., 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


# ---- inputs ------------------------------------------------------------------------------------------------------------
def sweep_case(n, sg, t, seed):
    """n elements at gradient scale sg for step t: weights of mixed magnitude with a zero row, gradients with a zero row,
    warm moments (zero for t = 1) with a row where m = -g cancels."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen) * 0.05
    k = max(1, n // 400)
    p[:k] *= 100
    p[k:2 * k] = 0
    g = torch.randn(n, generator=gen) * sg * torch.rand(n, generator=gen)
    g[2 * k:3 * k] = 0
    if t > 1:
        m = torch.randn(n, generator=gen) * sg * 0.3
        v = torch.rand(n, generator=gen) * sg * sg
        m[3 * k:4 * k] = -g[3 * k:4 * k]
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    ema = p + torch.randn(n, generator=gen) * 1e-3
    return p, g, m, v, ema


def layout_tensors(seed=0, scale=0.05):
    """The seven sizes of SIZES twice over four groups (14 tensors, every group with a chunk-edge size)."""
    gen = torch.Generator().manual_seed(seed)
    tensors, group_of = {}, {}
    for i, n in enumerate(SIZES + SIZES[::-1]):
        name = f"g{i % 4}.t{i}"
        tensors[name] = torch.randn(n, generator=gen) * scale if n != 8 else torch.randn(2, 4, generator=gen) * scale
        group_of[name] = i % 4
    return tensors, group_of


HYPERS4 = [Hyper(1e-4, 1e-3), Hyper(1e-4, 0.0), Hyper(2e-4, 1e-3), Hyper(2e-4, 1e-2)]


def as_groups(hypers: Sequence[Hyper]) -> List[dict]:
    return [{"lr": h.lr, "weight_decay": h.wd, "betas": (h.b1, h.b2), "eps": h.eps} for h in hypers]


# ---- trajectories ------------------------------------------------------------------------------------------------------
def torch_trajectory(p0: torch.Tensor, grads: Sequence[torch.Tensor], lrs: Sequence[Sequence[float]], sizes, hypers,
                     max_norm, ema_decay, ema_every):
    """``torch.optim.AdamW`` in float64 over one flat tensor per group + ``clip_grad_norm_`` + the lerp EMA, on CPU.
    -> (p, ema) flat float64."""
    params = [torch.nn.Parameter(x.double().clone()) for x in torch.split(p0, list(sizes))]
    opt = torch.optim.AdamW([{"params": [q], "lr": h.lr, "weight_decay": h.wd, "betas": (h.b1, h.b2), "eps": h.eps}
                             for q, h in zip(params, hypers)])
    ema = [q.detach().clone() for q in params]
    for i, (g, lr) in enumerate(zip(grads, lrs)):
        for q, gq, grp, x in zip(params, torch.split(g.double(), list(sizes)), opt.param_groups, lr):
            q.grad = gq.clone()
            grp["lr"] = x
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        if (i + 1) % ema_every == 0:
            with torch.no_grad():
                for e, q in zip(ema, params):
                    e.lerp_(q, 1.0 - ema_decay)
    return torch.cat([q.detach() for q in params]), torch.cat(ema)


def model_trajectory(p0, grads, lrs, sizes, hypers, max_norm, ema_decay, ema_every):
    """The same trajectory on ``model_step32`` with the exact float64 clip coefficient rounded to fp32."""
    p, m, v, ema = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), p0.clone()
    for i, (g, lr) in enumerate(zip(grads, lrs)):
        K = expand([kernel_consts(Hyper(x, h.wd, h.b1, h.b2, h.eps), i + 1) for x, h in zip(lr, hypers)], sizes, F32)
        out = model_step32(p, g, m, v, None, f32r(coef64(norm64(g), max_norm)), K)
        p, m, v = out["p"], out["m"], out["v"]
        if (i + 1) % ema_every == 0:
            ema = ema + (p - ema) * f32r(1.0 - ema_decay)
    return p, ema


def displacement_error(x, x0, ref, bounds_of: Sequence[slice]) -> List[float]:
    """Relative L2 error of the displacement x - x0 against ref - x0, per tensor (slice)."""
    d, r = x.double() - x0.double(), ref.double() - x0.double()
    return [float((d[s] - r[s]).norm() / r[s].norm().clamp_min(1e-300)) for s in bounds_of]
