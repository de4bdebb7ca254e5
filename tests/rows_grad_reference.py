"""TEST-ONLY helper (no tests here): float64 models, bounds, cases and a CPU stand-in backend for the backward of the fp32
row path (csrc/rows_grad.hip, include/dadd_hip_rows_grad.h) and for ``conditioning_grad.ordinal_embedder`` /
``time_embedding``.

Models (float64 from the operands the kernels get, by the formulas of the header):
  linear_rows_grad_model : a = act_in(x); dw = dy^T a, db = sum_m dy, dx = act_in'(x) (dy w), with the exact SiLU / GELU
                           and their exact derivatives, and the sums of absolute terms E_dw = |dy|^T |a|, E_db = sum |dy|,
                           E_dx = |act_in'(x)| (|dy| |w|).
  aoe_interp_grad_model  : the scatter of (1 - frac) dout / frac dout into the class table, dbase = sum_c, ddeltas[j] =
                           sum_{c > j}; E = the same with absolute values.
  rowvec_grad_model      : drow = sum_p dy, E = sum_p |dy|.
``tests/test_rows_grad_cpu.py`` pins them to float64 autograd of ``oracle.conditioning`` / ``oracle.sd_unet`` formulas.

Bounds (``norm_grad_reference.sum_bound``: an fp32 sum of T terms in any order is within T 2^-24 E of the exact sum, + 16
for the fp32 evaluation of each term):
  dw, db : (M + 16) 2^-24 E;   dx : (N + 16) 2^-24 E_dx + 4 2^-24 |ref| (the derivative's own fp32 evaluation);
  dbase, ddeltas : (B + classes + 16) 2^-24 E;   drow : (HW + 16) 2^-24 E.
On integer-valued operands (and act_in = 0) every product and partial sum is an integer below 2^24: the kernels must
give the float64 result bit for bit.
Blocks: the embedder is fp32 throughout, so its gradients are held to 10 x the error of torch's own fp32 autograd of the
oracle on the CPU against float64 (``EMBEDDER_F32_ERR``, measured by ``embedder_f32_error``; the factor covers another
summation order over N = 256 ... 12288 terms); the purifier attachment and the resnet block with the time path keep
the 16-bit block bound 4e-3.

``CpuRowsBackend`` extends ``cond_grad_reference.CpuCondBackend`` with the row path and a ``rowvec``-aware ``igemm`` (with
the 3x3 conv, its data and weight gradients): float64 inside, outputs rounded to the tensors' type.
"""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

from oracle import conditioning as OC
from oracle import sd_unet as OU
from tests import cond_grad_reference as K
from tests import norm_grad_reference as N

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
EPS32 = 2.0 ** -24
BLOCK_BOUND = K.BLOCK_BOUND

# (M, K, N): one chunk; N not a multiple of 4 and fewer chunks than lanes; 65 chunks (a second, ragged K-tile); a ragged
# second row pass over several strips (the ws order matters); the maximum K
LINEAR_CASES = [(1, 8, 1), (3, 24, 5), (8, 520, 67), (11, 1536, 130), (9, 2048, 8)]
LINEAR_OUTPUTS = {"all": ("dx", "dw", "db"), "dx": ("dx",), "dw+db": ("dw", "db"), "no db": ("dx", "dw")}
# (B, D, classes)
AOE_CASES = [(1, 8, 2), (7, 100, 3), (9, 768, 4)]
AOE_LABELS = (-0.5, 0.0, 0.25, 1.0, 2.75, 3.0, 7.0)      # both clamps, lo == hi, an integer label, two samples in one cell
# (B, HW, C)
ROWVEC_CASES = [(1, 1, 8), (2, 64, 64), (3, 130, 320), (2, 1024, 1280)]
# the embedder block and the time path
EMB_D, EMB_HIDDEN, EMB_TOKENS, EMB_CLASSES, EMB_B = 64, 128, 4, 4, 5
# relative L2 per tensor of torch fp32 autograd of the oracle's AOE against float64 at these shapes, measured on the CPU
# (``embedder_f32_error``; rounded up): the reference's own fp32 error, ten times which is the block's bound
EMBEDDER_F32_ERR = {"base": 5.2e-7, "deltas": 3.4e-7, "projector.0.weight": 3.6e-7, "projector.0.bias": 3.9e-7,
                    "projector.2.weight": 1.9e-7, "projector.2.bias": 4.8e-8}
EMBEDDER_BOUND = {k: 10.0 * v for k, v in EMBEDDER_F32_ERR.items()}
TIME_DIM, TIME_HIDDEN, TIME_WIDTHS = 64, 128, (128, 64)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=gen(seed))


def randint(shape, seed, lo=-4, hi=5):
    return torch.randint(lo, hi, shape, generator=gen(seed)).float()


def labels(b):
    return torch.tensor((AOE_LABELS * (b // len(AOE_LABELS) + 1))[:b], dtype=F32)


# ---- activations ------------------------------------------------------------------------------------------------------------
def act(x, a):
    return x if a == 0 else F.silu(x) if a == 1 else F.gelu(x)


def act_grad(x, a):
    x = x.double()
    if a == 0:
        return torch.ones_like(x)
    if a == 1:
        s = torch.sigmoid(x)
        return s * (1.0 + x * (1.0 - s))
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ---- linear_rows backward ---------------------------------------------------------------------------------------------------
def linear_rows_model(x, w, bias, act_in):
    y = act(x.double(), act_in) @ w.double().t()
    return y if bias is None else y + bias.double()


def linear_rows_grad_model(x, w, dy, act_in):
    """-> dict(dx, dw, db, e_dx, e_dw, e_db, m, n), float64; ``w`` as the kernel multiplies with it (fp16 or fp32)."""
    x, w, dy = x.double(), w.double(), dy.double()
    a, g = act(x, act_in), act_grad(x, act_in)
    return dict(dx=g * (dy @ w), dw=dy.t() @ a, db=dy.sum(0), e_dx=g.abs() * (dy.abs() @ w.abs()), e_dw=dy.abs().t() @ a.abs(),
                e_db=dy.abs().sum(0), m=x.shape[0], n=w.shape[0])


def linear_bounds(r):
    """name -> elementwise bound of dx, dw, db from a ``linear_rows_grad_model`` result."""
    return dict(dx=(r["n"] + 16) * EPS32 * r["e_dx"] + 4 * EPS32 * r["dx"].abs(), dw=N.sum_bound(r["m"], r["e_dw"]),
                db=N.sum_bound(r["m"], r["e_db"]))


@functools.lru_cache(maxsize=None)
def linear_case(m, k, n, w_dtype=F32, integer=False):
    """-> (x fp32 [M][K], w [N][K] in ``w_dtype``, dy fp32 [M][N]); x spans the activations' curved range."""
    s = 3000 + 131 * m + 7 * k + n
    if integer:
        return randint((m, k), s), randint((n, k), s + 1).to(w_dtype), randint((m, n), s + 2)
    return randn((m, k), s, 1.5), randn((n, k), s + 1, k ** -0.5).to(w_dtype), randn((m, n), s + 2)


# ---- AOE interpolation backward ---------------------------------------------------------------------------------------------
def aoe_cells(lab, classes):
    y = lab.double().clamp(0.0, float(classes - 1))
    lo = torch.floor(y)
    hi = torch.clamp(lo + 1, max=classes - 1)
    return lo.long(), hi.long(), y - lo


def aoe_interp_model(lab, base, deltas):
    return OC.aoe_lerp({"e.base": base.double(), "e.deltas": deltas.double()}, lab.double(), "e")


def aoe_interp_grad_model(lab, dout, classes):
    """-> dict(dbase, ddeltas, e_base, e_deltas, b), float64."""
    lo, hi, frac = aoe_cells(lab, classes)
    dout = dout.double()
    out = {}
    for key, g in (("d", dout), ("e", dout.abs())):
        table = torch.zeros(classes, dout.shape[1], dtype=F64)
        table.index_add_(0, lo, (1.0 - frac)[:, None] * g)
        table.index_add_(0, hi, frac[:, None] * g)
        suffix = torch.flip(torch.cumsum(torch.flip(table, (0,)), 0), (0,))       # suffix[c] = sum_{c' >= c}
        out[key] = (suffix[0], suffix[1:])
    return dict(dbase=out["d"][0], ddeltas=out["d"][1], e_base=out["e"][0], e_deltas=out["e"][1], b=lab.shape[0])


def aoe_bound(b, classes, e):
    return (b + classes + 16) * EPS32 * e


@functools.lru_cache(maxsize=None)
def aoe_case(b, d, classes, integer=False):
    """-> (labels [B], base [D], deltas [classes - 1][D], dout [B][D]), fp32."""
    s = 5000 + 17 * b + d + classes
    return labels(b), randn((d,), s), randn((classes - 1, d), s + 1, 0.3), randint((b, d), s + 2) if integer else randn((b, d), s + 2)


# ---- rowvec backward --------------------------------------------------------------------------------------------------------
def rowvec_grad_model(dy):
    d = dy.double().reshape(dy.shape[0], -1, dy.shape[-1])
    return dict(drow=d.sum(1), e=d.abs().sum(1), hw=d.shape[1])


@functools.lru_cache(maxsize=None)
def rowvec_case(b, hw, c, dtype=F16, integer=False):
    s = 6000 + 13 * b + hw + c
    return (randint((b, hw, c), s) if integer else randn((b, hw, c), s)).to(dtype)


def share(got, ref, bound):
    """Worst |got - ref| / bound; inf for a non-finite value or a miss where the bound is zero."""
    got, ref = got.detach().double().cpu(), ref.double()
    if got.shape != ref.shape or not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max())


# ---- the embedder block -------------------------------------------------------------------------------------------------------
def embedder_params(d=EMB_D, hidden=EMB_HIDDEN, tokens=EMB_TOKENS, classes=EMB_CLASSES, p="ordinal_embedder"):
    """fp32 masters under the reference's key names; ``norm.*`` and ``null_embedding`` exist and stay unused."""
    return {p + ".base": randn((d,), 700, 0.5), p + ".deltas": 0.3 + randn((classes - 1, d), 701, 0.2),
            p + ".projector.0.weight": randn((hidden, d), 702, d ** -0.5), p + ".projector.0.bias": randn((hidden,), 703, 0.1),
            p + ".projector.2.weight": randn((tokens * d, hidden), 704, hidden ** -0.5),
            p + ".projector.2.bias": randn((tokens * d,), 705, 0.1),
            p + ".norm.weight": torch.ones(tokens * d), p + ".norm.bias": torch.zeros(tokens * d),
            p + ".null_embedding": torch.zeros(1, d)}


EMBEDDER_TRAINED = ("base", "deltas", "projector.0.weight", "projector.0.bias", "projector.2.weight", "projector.2.bias")


def embedder_oracle_grads(params, lab, dout, dtype=F64, tokens=EMB_TOKENS, p="ordinal_embedder"):
    """Autograd of ``oracle.conditioning.aoe_forward`` in ``dtype`` -> {key: gradient} over the trained masters."""
    sd = {k: v.to(dtype).requires_grad_(True) for k, v in params.items()}
    OC.aoe_forward(sd, lab.to(dtype), tokens, p).backward(dout.to(dtype))
    return {p + "." + k: sd[p + "." + k].grad for k in EMBEDDER_TRAINED}


def embedder_f32_error():
    """{key: relative L2 of torch fp32 autograd of the oracle's AOE on the CPU against float64} at the block's shapes."""
    params, lab, dout = embedder_params(), labels(EMB_B), randn((EMB_B, EMB_TOKENS, EMB_D), 710)
    ref, f32 = embedder_oracle_grads(params, lab, dout), embedder_oracle_grads(params, lab, dout, F32)
    return {k: N.rel_l2(f32[k], ref[k]) for k in ref}


# ---- the time path ------------------------------------------------------------------------------------------------------------
TIME_PREFIX = "unet.unet.time_embedding"
TIME_PROJ_KEYS = ("unet.unet.down_blocks.0.resnets.0.time_emb_proj", "unet.unet.down_blocks.0.resnets.1.time_emb_proj")


def time_params(dim=TIME_DIM, hidden=TIME_HIDDEN, widths=TIME_WIDTHS):
    sd = {TIME_PREFIX + ".linear_1.weight": randn((hidden, dim), 800, dim ** -0.5), TIME_PREFIX + ".linear_1.bias": randn((hidden,), 801, 0.1),
          TIME_PREFIX + ".linear_2.weight": randn((hidden, hidden), 802, hidden ** -0.5),
          TIME_PREFIX + ".linear_2.bias": randn((hidden,), 803, 0.1)}
    for i, (key, wd) in enumerate(zip(TIME_PROJ_KEYS, widths)):
        sd[key + ".weight"], sd[key + ".bias"] = randn((wd, hidden), 810 + 2 * i, hidden ** -0.5), randn((wd,), 811 + 2 * i, 0.1)
    return sd


def time_rows64(sd, t, dim=TIME_DIM):
    """float64 rows of the oracle's time path over the (already rounded, float64) state dict: Timesteps -> linear_1 -> SiLU
    -> linear_2 (= temb) -> per resnet ``F.linear(F.silu(temb), time_emb_proj)`` (``oracle.sd_unet.resnet``), concatenated."""
    feat = OU.timestep_embedding(t, dim).double()
    temb = F.linear(F.silu(F.linear(feat, sd[TIME_PREFIX + ".linear_1.weight"], sd[TIME_PREFIX + ".linear_1.bias"])),
                    sd[TIME_PREFIX + ".linear_2.weight"], sd[TIME_PREFIX + ".linear_2.bias"])
    return torch.cat([F.linear(F.silu(temb), sd[k + ".weight"], sd[k + ".bias"]) for k in TIME_PROJ_KEYS], -1)


def round_matrices(params):
    """float64 leaves of the masters with the weight MATRICES rounded to fp16 (what the kernels multiply with)."""
    return {k: (v.half() if v.dim() == 2 else v).double().requires_grad_(True) for k, v in params.items()}


def time_block_case():
    """The resnet block of test_gpu_norm_grad.test_resnet_block_gradients (B = 2, 8x8, 64 -> 128, the same operands) with
    timesteps instead of a given time row -> (block masters, x fp16, t int64, dy fp16)."""
    b, hw, ci, co = 2, 8, 64, 128
    r = N.R.rnd
    x, dy = (1.5 * r((b, hw, hw, ci), 41, dtype=F32) + 0.3).half(), r((b, hw, hw, co), 42)
    p = dict(g1=1 + 0.2 * r((ci,), 44, dtype=F32), b1=r((ci,), 45, 0.2, F32), w1=r((co, 9 * ci), 46, (9 * ci) ** -0.5, F32),
             c1=r((co,), 47, 0.1, F32), g2=1 + 0.2 * r((co,), 48, dtype=F32), b2=r((co,), 49, 0.2, F32),
             w2=r((co, 9 * co), 50, (9 * co) ** -0.5, F32), c2=r((co,), 51, 0.1, F32),
             ws=r((co, ci), 52, ci ** -0.5, F32), cs=r((co,), 53, 0.1, F32))
    return p, x, torch.tensor([17, 640], dtype=torch.int64), dy


def time_block_oracle(p, tparams, x, t, dy):
    """float64 autograd of the block with the oracle's time path in front, matrices rounded to fp16 -> {name: gradient}
    over the block masters, the time-path masters and x."""
    q = {k: (v.half() if k.startswith("w") else v).double().requires_grad_(True) for k, v in p.items()}
    tp = round_matrices(tparams)
    x64 = x.double().requires_grad_(True)
    rows = time_rows64(tp, t)
    N.resnet_block64(x64, rows[:, :TIME_WIDTHS[0]], q).backward(dy.double())
    zero = {k: torch.zeros_like(v) for k, v in tp.items() if v.grad is None}
    return dict({k: v.grad for k, v in q.items()}, x=x64.grad, **{k: (v.grad if v.grad is not None else zero[k]) for k, v in tp.items()})


def run_time_block(be, G, CG, p, tparams, x, t, dy):
    """The same block on the operators: ``time_embedding`` -> rows, whose first columns enter the first conv as
    ``rowvec`` (a strided slice).  Operands already on the backend's device -> {name: gradient}."""
    d = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    tp = {k: v.detach().clone().requires_grad_(True) for k, v in tparams.items()}
    xd = x.detach().clone().requires_grad_(True)
    rows = CG.time_embedding(be, tp, t, TIME_PROJ_KEYS, dim=TIME_DIM, prefix=TIME_PREFIX)
    assert rows.shape == (x.shape[0], sum(TIME_WIDTHS)) and rows.dtype == F32
    hdn = G.group_norm(be, xd, d["g1"], d["b1"], silu=True)
    hdn = G.conv3x3(be, hdn, d["w1"], d["c1"], rowvec=rows[:, :TIME_WIDTHS[0]])
    hdn = G.group_norm(be, hdn, d["g2"], d["b2"], silu=True)
    hdn = G.conv3x3(be, hdn, d["w2"], d["c2"])
    (hdn + G.linear(be, xd, d["ws"], d["cs"])).backward(dy)
    return dict({k: v.grad for k, v in d.items()}, x=xd.grad, **{k: v.grad for k, v in tp.items()})


# ---- CPU stand-in backend -------------------------------------------------------------------------------------------------------
class CpuRowsBackend(K.CpuCondBackend):
    """``CpuCondBackend`` plus the fp32 row path, the row gradient and a ``rowvec``-aware ``igemm`` that also takes the
    stride-1 3x3 conv: float64 inside, outputs rounded by the copy into the tensor the operator allocated."""

    def timestep_features(self, t, out):
        out.copy_(OU.timestep_embedding(t, out.shape[1]))

    def linear_rows(self, x, w, bias, out, act_in=0, act_out=0):
        assert x.dtype == F32 and w.dtype in (F16, F32) and out.dtype == F32
        out.copy_(act(linear_rows_model(x, w, bias, act_in), act_out))

    @staticmethod
    def linear_rows_grad_ws_numel(m, k, n):
        if k % 8 or not 0 < k <= 2048 or m < 1 or n < 1:
            raise ValueError("linear_rows_grad: K a multiple of 8 up to 2048")
        return m * k

    def linear_rows_grad(self, x, w, dy, *, dx=None, dw=None, db=None, ws=None, act_in=0):
        if dx is None and dw is None:
            raise ValueError("linear_rows_grad: no output")
        if dw is None and db is not None:
            raise ValueError("linear_rows_grad: db comes with dw")
        assert dx is None or ws.numel() >= self.linear_rows_grad_ws_numel(x.shape[0], x.shape[1], w.shape[0])
        r = linear_rows_grad_model(x, w, dy, act_in)
        for dst, key in ((dx, "dx"), (dw, "dw"), (db, "db")):
            if dst is not None:
                assert dst.dtype == F32
                dst.copy_(r[key])

    def aoe_interp(self, lab, base, deltas, out):
        out.copy_(aoe_interp_model(lab, base, deltas))

    def aoe_interp_grad(self, lab, dout, dbase, ddeltas):
        classes = ddeltas.shape[0] + 1
        if not 2 <= classes <= 16:
            raise ValueError("aoe_interp_grad: 2..16 classes")
        r = aoe_interp_grad_model(lab, dout, classes)
        dbase.copy_(r["dbase"])
        ddeltas.copy_(r["ddeltas"])

    def rowvec_grad(self, dy, drow, ws=None):
        assert dy.dtype in (F16, BF16) and drow.dtype == F32
        drow.copy_(rowvec_grad_model(dy)["drow"])

    def igemm(self, x, w, out, *, bias=None, rowvec=None, taps=1, stride=1, ups=0, pad=0, flags=0, **kw):
        assert stride == 1 and not ups and not kw and taps in (1, 9), (taps, stride, ups, kw)
        assert (rowvec is not None) == bool(flags & 2) and (bias is not None) == bool(flags & 1), flags
        if taps == 1:
            y = (x.double().reshape(-1, x.shape[-1]) @ w.double().t()).reshape(out.shape)
        else:
            y = N.conv3x3_nhwc(x.double(), w.double(), None)
        if bias is not None:
            y = y + bias.double()
        if rowvec is not None:
            assert rowvec.dtype == F32 and rowvec.shape == (x.shape[0], w.shape[0]) and taps == 9
            y = y + rowvec.double()[:, None, None, :]
        out.copy_(y.reshape(out.shape))

    def dgrad(self, dy, wt, dx, *, taps=1):
        if taps == 1:
            return super().dgrad(dy, wt, dx, taps=taps)
        dx.copy_(N.conv3x3_nhwc(dy.double(), wt.double(), None))      # the forward on dy with the re-laid weight

    def wgrad(self, dy, x, dw, *, dbias=None, taps=1, stride=1, ups=0, pad=0, splitm=None, partial=None, ld_tap=None):
        if taps == 1:
            return super().wgrad(dy, x, dw, dbias=dbias, taps=taps)
        assert stride == 1 and not ups
        with torch.enable_grad():      # (called from inside an autograd backward)
            w0 = torch.zeros(dw.shape, dtype=F64, requires_grad=True)
            N.conv3x3_nhwc(x.double(), w0, None).backward(dy.double())
        dw.copy_(w0.grad)
        if dbias is not None:
            dbias.copy_(dy.double().sum((0, 1, 2)))
