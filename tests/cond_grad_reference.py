"""TEST-ONLY helper (no tests here): float64 models, bounds, cases and a CPU stand-in backend for the training kernels
of the conditioning front-end (csrc/cond_grad.hip, include/dadd_hip_cond_grad.h) and for the blocks of
``conditioning_grad``.

Models (float64 from the 16-bit operands, at the kernels' rounding points):
  gelu_model       : 0.5 x (1 + erf_AS(x / sqrt 2)), erf_AS the polynomial of Abramowitz & Stegun 7.1.26 that dadd_gelu
                     evaluates, its magnitude rounded to fp32 where the kernel forms it next to 1; rounded once to the
                     storage type by the caller.
  gelu_grad_model  : dy (Phi_AS(x) + x phi(x)), Phi_AS from the same erf, phi exact.
  gate_tail_model  : LayerNorm(img - sigmoid(z) * dis) * gamma + beta.
  gate_tail_grad_model : the formulas of the header -> dimg, ddis, dz, dgamma, dbeta and the sums of absolute terms
                     E_gamma = sum_m |dout xhat|, E_beta = sum_m |dout| that the (M + 16) 2^-24 E bound takes.
``tests/test_cond_grad_cpu.py`` pins them to float64 autograd of ``oracle.conditioning``'s formulas.

Bounds.  A&S 7.1.26 states |erf_AS - erf| <= 1.5e-7 (``ERF_ERR``).  Phi = (1 + erf) / 2, so |Phi_AS - Phi| <= ERF_ERR / 2
and, phi being exact, |gelu'_AS(x) - gelu'(x)| <= ERF_ERR / 2 = 7.5e-8 for every x (``GELU_GRAD_ERR``);
|gelu_AS(x) - gelu(x)| <= |x| ERF_ERR / 2 (+ |x| 2^-26 with the fp32 rounding of erf in the model).
GPU, elementwise: gelu within one spacing of the storage type at the model's value (``gelu_bound``); gelu_grad within
2 ULP |ref| + ULP 2^-4 of the float64 model (one rounding of dx, ULP / 2 relative, with as much again for the fp32
arithmetic, and an absolute floor for results next to the zero of gelu' and in the subnormal range); the purifier tail's fp32
output within the absolute 2e-5 of ``norm_cases.PURIFIER_ATOL``; dimg / ddis / dz with the 16-bit tolerance of
``norm_grad_reference.TOL16``; dgamma / dbeta within ``norm_grad_reference.sum_bound`` = (M + 16) 2^-24 E.
Blocks: relative L2 per tensor <= 4e-3 against float64 autograd of the oracle on 16-bit-rounded weight matrices.

``CpuCondBackend`` extends ``attn_grad_reference.CpuAttnBackend`` with the methods ``grad_ops.linear``, ``layer_norm``,
``gelu`` and ``purifier_gate_tail`` call: the same names and argument lists as ``HipBackend``, float64 inside, outputs
rounded to the tensors' type.  It lets the CPU suite run ``conditioning_grad``'s own code.
"""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

from oracle import conditioning as OC
from tests import attn_grad_reference as R
from tests import norm_grad_reference as N
from tests.attention_cases import ULP

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
ERF_ERR = 1.5e-7                    # Abramowitz & Stegun 7.1.26, absolute
GELU_GRAD_ERR = 0.5 * ERF_ERR       # |gelu'_AS - gelu'|, see above
PURIFIER_ATOL = 2e-5                # tests/norm_cases.py, the fp32 output of purifier_tail
BLOCK_BOUND = 4e-3
STANDIN_BOUND = 2e-3                # what the CPU stand-in must keep, so that the reference path fits the block bound
MANT = {F16: 10, BF16: 7}
MIN_EXP = {F16: -14, BF16: -126}

GELU_CASES = [(5, 8, F16), (33, 3072, F16), (32, 768, BF16)]
TAIL_CASES = [(3, 8), (32, 768), (37, 2048)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=gen(seed))


def spacing(ref, dtype):
    """The distance between neighbouring values of ``dtype`` at |ref| (the subnormal spacing below the smallest normal)."""
    a = ref.detach().double().abs().clamp_min(2.0 ** MIN_EXP[dtype])
    return torch.exp2(torch.floor(torch.log2(a)) - MANT[dtype])


# ---- attention backward at d = 96 and ragged key counts ----------------------------------------------------------------------
# (b, heads, d, nq, nk)
RAGGED_CASES = [(2, 8, 96, 16, 257),    # the resampler: five key tiles, one key in the last
                (2, 2, 96, 16, 16),     # the purifier
                (1, 2, 96, 64, 65), (1, 2, 96, 16, 63), (1, 2, 96, 16, 17),
                (2, 2, 40, 64, 72),     # ragged Nk on an old head dim
                (1, 2, 160, 16, 129),
                (1, 2, 96, 16, 1)]      # one key only: dq = dk = 0 exactly
RAGGED_BF16 = (0, 2, 5)
RAGGED_RUNS = [(i, F16) for i in range(len(RAGGED_CASES))] + [(i, BF16) for i in RAGGED_BF16]


def ragged_id(run):
    i, dtype = run
    b, h, d, nq, nk = RAGGED_CASES[i]
    return f"b{b}h{h}d{d}q{nq}k{nk}-{'bf16' if dtype == BF16 else 'f16'}"


@functools.lru_cache(maxsize=None)
def ragged_inputs(i, dtype):
    """-> (q, k, v, dout) as ``attn_grad_reference.inputs`` makes them: 0.5 randn operands in ``dtype``."""
    b, h, d, nq, nk = RAGGED_CASES[i]
    g = gen(4100 + i)
    return tuple((0.5 * torch.randn(b, n, h * d, generator=g)).to(dtype) for n in (nq, nk, nk, nq))


@functools.lru_cache(maxsize=None)
def ragged_reference(i, dtype):
    """-> attn_grad_reference.Reference(exact, E_model per tensor, bound per tensor); computed once per process.  With one
    key the exact dq and dk are zero and their E_model is undefined (nan): the tests cap those tensors instead."""
    heads = RAGGED_CASES[i][1]
    q, k, v, do = ragged_inputs(i, dtype)
    ex, mo = R.exact(q, k, v, do, heads), R.model(q, k, v, do, heads)
    e = tuple(R.rel_l2(a, b) if float(b.abs().max()) > 0 else float("nan") for a, b in zip(mo, ex))
    return R.Reference(ex, e, tuple(max(2.0 * x, ULP[dtype]) if x == x else float("nan") for x in e))


def one_key_cap(q, k, v, dout):
    """max |dq|, |dk| allowed where the exact gradient is zero: ULP * max|dout| * max(max|q|, max|k|, max|v|)."""
    return ULP[q.dtype] * float(dout.float().abs().max()) * max(float(t.float().abs().max()) for t in (q, k, v))


# ---- GELU ----------------------------------------------------------------------------------------------------------------
def erf_as(x):
    """erf by Abramowitz & Stegun 7.1.26 in float64, the coefficients of dadd_gelu."""
    z = x.abs()
    t = 1.0 / (1.0 + 0.3275911 * z)
    p = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
    return torch.sign(x) * (1.0 - p * torch.exp(-z * z))


def gelu_model(x, fp32_point=True):
    """0.5 x (1 + erf_AS(x / sqrt 2)) in float64 with the kernel's one rounding point that matters: dadd_gelu forms
    erf_AS(|x| / sqrt 2) = 1 - p t e in fp32, next to 1, so ``fp32_point`` rounds that value to fp32 before Phi is formed
    (1 - erf is then exact, by Sterbenz).  Deep in the negative tail the rounded value is 1 and gelu is 0, as the kernel and
    the GEMM epilogue give it.  ``fp32_point=False``: the plain A&S formula."""
    x = x.double()
    e = erf_as(x / math.sqrt(2.0)).abs()
    if fp32_point:
        e = e.float().double()
    return 0.5 * x * (1.0 + torch.sign(x) * e)


def gelu_grad_model(x, dy):
    x = x.double()
    Phi = 0.5 * (1.0 + erf_as(x / math.sqrt(2.0)))
    phi = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return dy.double() * (Phi + x * phi)


def gelu_bound(model, dtype):
    """|kernel - model rounded to ``dtype``| allowed elementwise: one spacing of the storage type at the model's value, the
    issue's 1 ulp (a 16-bit rounding that falls the other way).  Nothing is added for the fp32 arithmetic: its one rounding
    that matters is in ``gelu_model``."""
    return spacing(model, dtype)


def gelu_grad_bound(ref, dtype):
    return 2.0 * ULP[dtype] * ref.abs() + ULP[dtype] * 2.0 ** -4


@functools.lru_cache(maxsize=None)
def gelu_case(m, f, dtype):
    """x spanning +-6 (a ramp over the whole range plus noise, shuffled), dy ~ N(0, 1) -> (x, dy) in ``dtype``."""
    n = m * f
    x = torch.linspace(-6.0, 6.0, n, dtype=F64) + 0.01 * torch.randn(n, generator=gen(7100 + n), dtype=F64)
    x = x[torch.randperm(n, generator=gen(7101 + n))].reshape(m, f).clamp(-6.0, 6.0)
    return x.to(dtype), randn((m, f), 7102 + n).to(dtype)


# ---- the purifier's tail -------------------------------------------------------------------------------------------------
def gate_tail_model(img, dis, z, gamma, beta, eps=1e-5):
    u = img.double() - torch.sigmoid(z.double()) * dis.double()
    return F.layer_norm(u, (u.shape[-1],), gamma.double(), beta.double(), eps)


def gate_tail_grad_model(img, dis, z, dout, gamma, eps=1e-5):
    """-> dict(dimg, ddis, dz, dgamma, dbeta, e_gamma, e_beta, m), float64, by the formulas of the header."""
    img, dis, z, dout, gamma = (t.double() for t in (img, dis, z, dout, gamma))
    c = img.shape[-1]
    g = torch.sigmoid(z)
    u = (img - g * dis).reshape(-1, c)
    do = dout.reshape(-1, c)
    mean = u.mean(-1, keepdim=True)
    d = u - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    xh = d * rstd
    a = do * gamma
    du = (rstd * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True))).reshape(img.shape)
    return dict(dimg=du, ddis=-g * du, dz=-du * dis * g * (1.0 - g), dgamma=(do * xh).sum(0), dbeta=do.sum(0),
                e_gamma=(do * xh).abs().sum(0), e_beta=do.abs().sum(0), m=u.shape[0])


@functools.lru_cache(maxsize=None)
def tail_case(m, c, dtype=F16, shifted=False):
    """-> (img, dis, z, dout fp32, gamma, beta).  ``shifted``: the rows of img - g * dis sit at 50 with a spread of 0.1."""
    s = 9000 + 7 * m + c + (1 if shifted else 0)
    if shifted:
        img, dis = 50.0 + randn((m, c), s, 0.1), randn((m, c), s + 1, 0.1)
    else:
        img, dis = randn((m, c), s, 1.0) + 0.3, randn((m, c), s + 1, 0.5)
    z = randn((m, c), s + 2, 2.0)
    gamma, beta = 1.0 + randn((c,), s + 3, 0.2), randn((c,), s + 4, 0.2)
    return img.to(dtype), dis.to(dtype), z.to(dtype), randn((m, c), s + 5), gamma, beta


# ---- the blocks ----------------------------------------------------------------------------------------------------------
E, HEADS, TOKENS, CTX, CLIP_W, DEPTH, BATCH = 192, 2, 16, 257, 128, 2, 2
PROJ_IN, PROJ_D = 128, 64           # image_projection: Linear(128 -> 16 * 64)


def _affine(sd, key, c, seed):
    sd[key + ".weight"], sd[key + ".bias"] = 1.0 + randn((c,), seed, 0.2), randn((c,), seed + 1, 0.2)


def _linear(sd, key, n, c, seed):
    sd[key + ".weight"], sd[key + ".bias"] = randn((n, c), seed, c ** -0.5), randn((n,), seed + 1, 0.1)


def _mha(sd, key, e, seed):
    sd[key + ".in_proj_weight"], sd[key + ".in_proj_bias"] = randn((3 * e, e), seed, e ** -0.5), randn((3 * e,), seed + 1, 0.1)
    _linear(sd, key + ".out_proj", e, e, seed + 2)


def purifier_params(e=E, ff_mult=2, p="feature_purifier"):
    """fp32 masters under the reference's key names (feature_purifier.py: ff_mult = 2 is its default)."""
    sd = {}
    _affine(sd, p + ".norm_img", e, 100)
    _affine(sd, p + ".norm_aoe", e, 110)
    _mha(sd, p + ".cross_attn", e, 120)
    _linear(sd, p + ".gate.0", ff_mult * e, 2 * e, 130)
    _linear(sd, p + ".gate.2", e, ff_mult * e, 140)
    _affine(sd, p + ".norm_out", e, 150)
    return sd


def resampler_params(e=E, depth=DEPTH, clip_w=CLIP_W, tokens=TOKENS, p="image_projection"):
    sd = {p + ".latents": randn((1, tokens, e), 200, 1.0)}
    _linear(sd, p + ".proj_in", e, clip_w, 210)
    for i in range(depth):
        lp, s = p + f".layers.{i}", 300 + 50 * i
        _mha(sd, lp + ".cross_attn", e, s)
        _linear(sd, lp + ".ff.0", 4 * e, e, s + 10)
        _linear(sd, lp + ".ff.2", e, 4 * e, s + 20)
        _affine(sd, lp + ".norm1", e, s + 30)
        _affine(sd, lp + ".norm2", e, s + 40)
    _affine(sd, p + ".norm_out", e, 290)
    return sd


def projection_params(p="image_projection"):
    sd = {}
    _linear(sd, p + ".projection", TOKENS * PROJ_D, PROJ_IN, 500)
    _affine(sd, p + ".norm", PROJ_D, 510)
    return sd


def block_inputs(kind):
    """-> (fp16 inputs by name, dout) of one block at the test shapes."""
    if kind == "purifier":
        return dict(image_embeds=(randn((BATCH, TOKENS, E), 600) + 0.3).half(), source_aoe=randn((BATCH, TOKENS, E), 601).half()), \
            randn((BATCH, TOKENS, E), 602)
    if kind == "resampler":
        return dict(hidden=randn((BATCH, CTX, CLIP_W), 610).half()), randn((BATCH, TOKENS, E), 611)
    return dict(image_embeds=randn((BATCH, PROJ_IN), 620).half()), randn((BATCH, TOKENS, PROJ_D), 621)


BLOCKS = {"purifier": purifier_params, "resampler": resampler_params, "projection": projection_params}


def oracle_grads(kind, params, inputs, dout):
    """float64 autograd of the oracle function on the masters with their weight MATRICES rounded to fp16 (what the kernels
    multiply with) -> {name: gradient} over every parameter and every input."""
    sd = {k: (v.half() if v.dim() == 2 else v).double().requires_grad_(True) for k, v in params.items()}
    xs = {k: v.double().requires_grad_(True) for k, v in inputs.items()}
    if kind == "purifier":
        out = OC.feature_purifier(sd, xs["image_embeds"], xs["source_aoe"], HEADS)
    elif kind == "resampler":
        out = OC.image_projection_plus(sd, xs["hidden"], HEADS)
    else:
        out = OC.image_projection(sd, xs["image_embeds"], TOKENS)
    out.backward(dout.double())
    return {**{k: v.grad for k, v in sd.items()}, **{k: v.grad for k, v in xs.items()}}


def run_block(be, CG, kind, params, inputs, dout):
    """``conditioning_grad``'s function on leaves made from ``params`` / ``inputs`` (already on the backend's device)
    -> ({name: gradient}, output)."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    xs = {k: v.detach().clone().requires_grad_(True) for k, v in inputs.items()}
    if kind == "purifier":
        out = CG.feature_purifier(be, leaves, xs["image_embeds"], xs["source_aoe"], HEADS)
    elif kind == "resampler":
        out = CG.image_projection_plus(be, leaves, xs["hidden"], HEADS)
    else:
        out = CG.image_projection(be, leaves, xs["image_embeds"], TOKENS)
    out.backward(dout.to(out.dtype))
    return {**{k: v.grad for k, v in leaves.items()}, **{k: v.grad for k, v in xs.items()}}, out


def check_block(what, got, ref, bound=BLOCK_BOUND):
    """Prints the relative L2 error of every tensor, then asserts each against ``bound``; -> the worst."""
    errs = {}
    for name in ref:
        assert got[name] is not None, (what, name, "no gradient arrived")
        errs[name] = R.rel_l2(got[name], ref[name])
        print(f"{what} d {name}: relative L2 error {errs[name]:.3e}")
    worst = max(errs, key=errs.get)
    print(f"{what}: worst relative L2 error {errs[worst]:.3e} ({worst}; bound {bound:.0e})")
    bad = {k: v for k, v in errs.items() if not v <= bound}
    assert not bad, (what, bad)
    return errs[worst]


# ---- CPU stand-in backend ------------------------------------------------------------------------------------------------
class CpuCondBackend(R.CpuAttnBackend):
    """``CpuAttnBackend`` plus the products, LayerNorm, GELU and the purifier's tail: float64 inside, outputs rounded by
    the copy into the tensor the operator allocated."""

    # products (taps = 1 only: the front-end has no convs)
    def igemm(self, x, w, out, *, bias=None, taps=1, stride=1, ups=0, pad=0, flags=0, **kw):
        assert taps == 1 and stride == 1 and not ups and not kw, (taps, stride, ups, kw)
        y = x.double().reshape(-1, x.shape[-1]) @ w.double().t()
        if bias is not None:
            y = y + bias.double()
        out.copy_(y.reshape(out.shape))

    def dgrad(self, dy, wt, dx, *, taps=1):
        assert taps == 1 and wt.shape == (dx.shape[-1], dy.shape[-1])
        dx.copy_((dy.double().reshape(-1, dy.shape[-1]) @ wt.double().t()).reshape(dx.shape))

    @staticmethod
    def wgrad_splitm(m, n, c, taps=1):
        return 1

    @staticmethod
    def wgrad_partial_numel(splitm, n, c, taps=1):
        return 0

    def wgrad(self, dy, x, dw, *, dbias=None, taps=1, stride=1, ups=0, pad=0, splitm=None, partial=None, ld_tap=None):
        assert taps == 1
        d2, x2 = dy.double().reshape(-1, dy.shape[-1]), x.double().reshape(-1, x.shape[-1])
        dw.copy_(d2.t() @ x2)
        if dbias is not None:
            dbias.copy_(d2.sum(0))

    # norms
    def layernorm(self, x, gamma, beta, out, eps=1e-5):
        out.copy_(F.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), eps))

    @staticmethod
    def layernorm_grad_ws_numel(m, c):
        return 2 * c

    def layernorm_grad(self, x, dy, gamma, *, dx=None, dgamma=None, dbeta=None, ws=None, eps=1e-5):
        c = x.shape[-1]
        zero = torch.zeros_like(x)
        r = gate_tail_grad_model(x, zero, zero, dy, gamma, eps)      # dis = 0: the plain LayerNorm backward
        for dst, key in ((dx, "dimg"), (dgamma, "dgamma"), (dbeta, "dbeta")):
            if dst is not None:
                dst.copy_(r[key].reshape(dst.shape))
        assert (dgamma is None) or ws.numel() >= self.layernorm_grad_ws_numel(x.numel() // c, c)

    # the conditioning kernels
    def gelu(self, x, y):
        y.copy_(gelu_model(x))

    def gelu_grad(self, x, dy, dx):
        dx.copy_(gelu_grad_model(x, dy))

    def purifier_gate_tail(self, img, dis, z, gamma, beta, out, eps=1e-5):
        assert out.dtype == F32
        out.copy_(gate_tail_model(img, dis, z, gamma, beta, eps))

    @staticmethod
    def purifier_gate_tail_grad_ws_numel(m, c):
        return 2 * c

    def purifier_gate_tail_grad(self, img, dis, z, dout, gamma, *, dimg=None, ddis=None, dz=None, dgamma=None, dbeta=None,
                                ws=None, eps=1e-5):
        assert dout.dtype == F32 and (dgamma is None) == (dbeta is None)
        r = gate_tail_grad_model(img, dis, z, dout, gamma, eps)
        for dst, key in ((dimg, "dimg"), (ddis, "ddis"), (dz, "dz"), (dgamma, "dgamma"), (dbeta, "dbeta")):
            if dst is not None:
                dst.copy_(r[key].reshape(dst.shape))


def sum_bound(m, e):
    return N.sum_bound(m, e)


TOL16 = N.TOL16
