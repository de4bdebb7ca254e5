"""-m gpu: every path of the shared GEMM / conv epilogue (csrc/igemm_epilogue.h) on every kernel form that ends in it.

The epilogue issues a tile's operand loads in batches ahead of the stores (per tile, per row fragment or per column block,
by instantiation) at addresses clamped into the tensor.  What can go wrong with that, and what each case here checks:
  * a wrong operand, a clamped duplicate used as data, a ragged row / column tile, a sample boundary inside a wave's
    rows: the output against ``TorchRefBackend`` in float64.  Linear paths (bias / time-embedding row / residual, with
    or without statistics) within the bound of tests/launch_audit.py for linear launches, 2 u |r| + K 2^-24 (|x| conv |w|
    + |operands|); LayerNorm fold, GEGLU and activations within ``launch_audit.TOL`` of that path;
  * a load or store outside a tensor: the output and EVERY operand live inside sentinel bands, which must be intact;
  * the hoisted residual loads when ``residual`` is ``out`` itself: that run must equal the separate-buffer run bit for
    bit;
  * anything order- or placement-dependent: a second run must be bit-identical.
Shapes are the smallest that hit the edges: K = 256 (4 K tiles), 4 samples of 6 x 6 pixels (M = 144: full 64- and 128-row
tiles plus a ragged one, 36 rows per sample so that a wave's rows span samples), N = 200 (ragged against 64, 128 and 160
columns, ending in half a fragment).  The statistics cases keep their host contracts (full tiles, whole-wave row blocks
inside one sample; N a multiple of the wave's columns).
"""
import functools
import math

import pytest
import torch

from tests.launch_audit import TOL, U, U32
from tests.torch_backend import TorchRefBackend

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
REF64 = TorchRefBackend(compute=F64)
SENT = 77.0          # exactly representable in fp16, bf16 and fp32; far outside the value range of every case
BAND = 256           # elements of sentinel before and after every buffer (a multiple of 16 bytes for every type)
K = 256


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(torch.device("cuda:0"))


def rnd(shape, seed, scale=1.0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


class Banded:
    """Device copy of ``t`` between two sentinel bands."""

    def __init__(self, hip, t):
        self.n = t.numel()
        self.buf = hip.zeros((self.n + 2 * BAND,), t.dtype)
        self.t = self.buf[BAND:BAND + self.n].view(t.shape)
        with hip.ctx():
            self.buf.fill_(SENT)
            self.t.copy_(t.to(self.buf.device))

    def intact(self):
        b = self.buf.float().cpu()
        return bool((b[:BAND] == SENT).all() and (b[BAND + self.n:] == SENT).all())


# ---- forms: name -> (igemm keyword arguments, x shape for M = 144 cases).  Tile requests and tuning bits select the kernel.
def _forms():
    from progressive_stable_diffusion_amd import lib as L
    lin = dict(shape=(4, 6, 6, K), conv={})
    return {
        "dma64x64": dict(lin, kw=dict(tile_m=64, tile_n=64)),
        "dma64x160": dict(lin, kw=dict(tile_m=64, tile_n=160)),
        "dma128x128": dict(lin, kw=dict(tile_m=128, tile_n=128)),
        "dma128x160": dict(lin, kw=dict(tile_m=128, tile_n=160)),
        "reg64x160": dict(lin, kw=dict(tile_m=64, tile_n=160), tune=L.TUNE_NODMA),
        "reg128x128": dict(lin, kw=dict(tile_m=128, tile_n=128), tune=L.TUNE_NODMA),
        # 3x3 convs: the halo kernel at W = 16 (one sample, 256 rows) and W = 32, the 2x-upsample gather (6x6 -> 12x12 = 144 rows)
        "halo16": dict(shape=(1, 16, 16, 64), conv=dict(taps=9, pad=1), kw=dict(tile_m=128, tile_n=160)),
        "halo32": dict(shape=(1, 32, 32, 64), conv=dict(taps=9, pad=1), kw=dict(tile_m=128, tile_n=160)),
        "ups128x160": dict(shape=(1, 6, 6, 64), conv=dict(taps=9, pad=1, ups=1), kw=dict(tile_m=128, tile_n=160)),
    }


FORMS = ["dma64x64", "dma64x160", "dma128x128", "dma128x160", "reg64x160", "reg128x128", "halo16", "halo32", "ups128x160"]
FLAGSETS = ["b", "bv", "br", "bvr"]        # bias; + time-embedding row (v); + residual (r)


@functools.lru_cache(maxsize=None)
def operands(shape, conv, n, flagset, dtype, extra=""):
    """CPU operands of one case, the float64 reference and its bound: shared by every form that runs the same shape
    (never modified).  ``extra``: 'gelu', 'lnstat', 'gnstat' ride on the linear flags."""
    from progressive_stable_diffusion_amd import lib as L
    conv = dict(conv)
    b, hi, wi, cin = shape
    ho, wo = (2 * hi, 2 * wi) if conv.get("ups") else (hi, wi)
    kk = conv.get("taps", 1) * cin
    x, w = rnd(shape, 1, dtype=dtype), rnd((n, kk), 2, 1 / math.sqrt(kk), dtype)
    t, flags = dict(bias=rnd((n,), 3, 0.1)), L.EPI_BIAS
    if "v" in flagset:
        t["rowvec"], flags = rnd((b, n), 5, 0.3), flags | L.EPI_ROWVEC
    if "r" in flagset:
        t["residual"], flags = rnd((b, ho, wo, n), 4, dtype=dtype), flags | L.EPI_RESIDUAL
    if extra == "gelu":
        flags |= L.EPI_GELU
    r = torch.zeros((b, ho, wo, n), dtype=F64)
    REF64.igemm(x, w, r, flags=flags, **t, **conv)
    if extra == "gelu":
        atol, rtol, _ = TOL[(dtype, "igemm.act")]
        bound = atol * max(1.0, r.pow(2).mean().sqrt().item()) + rtol * r.abs()
    else:           # the audit's bound for linear launches
        amag = torch.zeros_like(r)
        REF64.igemm(x.abs(), w.abs(), amag, flags=flags, **{k: v.abs() for k, v in t.items()}, **conv)
        fi = torch.finfo(dtype)
        bound = 2 * U[dtype] * r.abs() + kk * U32 * amag + fi.smallest_normal * fi.eps
    return x, w, t, flags, r, bound


def run(hip, x, w, t, flags, out_shape, dtype, kw, side=None):
    """Three launches of one case -> (first output on the CPU, its side outputs).  Asserts the bands, the repeat and the
    aliased run.  ``side``: name -> (shape, dtype) of side outputs (statistics), compared bitwise between the runs too."""
    dx, dw = Banded(hip, x), Banded(hip, w)
    dt = {k: Banded(hip, v) for k, v in t.items()}
    outs, sides = [], []
    for rep in range(3 if "residual" in t else 2):
        do = Banded(hip, torch.full(out_shape, SENT, dtype=dtype))
        ds = {k: Banded(hip, torch.zeros(s, dtype=d)) for k, (s, d) in (side or {}).items()}
        args = {k: v.t for k, v in dt.items()}
        if rep == 2:                    # residual == out: the residual is read from the buffer the launch writes
            with hip.ctx():
                do.t.copy_(dt["residual"].t)
            args["residual"] = do.t
        hip.igemm(dx.t, dw.t, do.t, flags=flags, **args, **{k: v.t for k, v in ds.items()}, **kw)
        hip.synchronize()
        assert do.intact(), f"run {rep}: wrote outside the output"
        assert all(v.intact() for v in ds.values()), f"run {rep}: wrote outside a side output"
        outs.append(do.t.cpu())
        sides.append({k: v.t.cpu() for k, v in ds.items()})
    assert dx.intact() and dw.intact() and all(v.intact() for v in dt.values()), "an operand's band was written"
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "second run differs"
    assert all(torch.equal(sides[0][k], sides[1][k]) for k in sides[0]), "second run's statistics differ"
    if len(outs) == 3:
        assert torch.equal(outs[0].view(torch.int16), outs[2].view(torch.int16)), "residual == out differs from separate buffers"
        assert all(torch.equal(sides[0][k], sides[2][k]) for k in sides[0]), "residual == out: statistics differ"
    return outs[0], sides[0]


def check(got, r, bound, what):
    err = (got.to(F64) - r).abs()
    ratio = (err / bound.clamp_min(1e-300)).flatten()
    i = int(ratio.argmax())
    print(f"{what}: worst error {err.flatten()[i].item():.3e} at {ratio[i].item():.3f} of its bound")
    assert ratio[i].item() <= 1.0, f"{what}: error {err.flatten()[i].item():.3e} is {ratio[i].item():.2f} x the bound at ref {r.flatten()[i].item():.4e}"


def tol_bound(key, r, dtype):
    atol, rtol, _ = TOL[(dtype, key)]
    return atol * max(1.0, r.pow(2).mean().sqrt().item()) + rtol * r.abs()


# ---- linear paths -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("flagset", FLAGSETS)
@pytest.mark.parametrize("form", FORMS)
def test_plain_path(hip, form, flagset, dtype):
    f = _forms()[form]
    n = 200
    x, w, t, flags, r, bound = operands(f["shape"], tuple(sorted(f["conv"].items())), n, flagset, dtype)
    got, _ = run(hip, x, w, t, flags | f.get("tune", 0), tuple(r.shape), dtype, dict(f["kw"], **f["conv"]))
    check(got, r, bound, f"{form} {flagset}")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_plain_path_on_the_persistent_ring(hip, dtype):
    """DADD_TUNE_PERSIST, 128 x 128 tiles, more tiles than CUs: every workgroup walks several tiles, the residual taken per
    row fragment.  36 rows per sample: most waves span two or three samples; ragged last row tile."""
    from progressive_stable_diffusion_amd import lib as L
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    b = (128 * (ncu // 2 + 1)) // 36 + 1               # x 2 column tiles > CUs
    x, w, t, flags, r, bound = operands((b, 6, 6, K), (), 200, "bvr", dtype)
    got, _ = run(hip, x, w, t, flags | L.TUNE_PERSIST, tuple(r.shape), dtype, dict(tile_m=128, tile_n=128))
    check(got, r, bound, "persistent ring bvr")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("form", ["dma64x160", "reg128x128"])
def test_activation(hip, form, dtype):
    f = _forms()[form]
    x, w, t, flags, r, bound = operands(f["shape"], (), 200, "br", dtype, "gelu")
    got, _ = run(hip, x, w, t, flags | f.get("tune", 0), tuple(r.shape), dtype, f["kw"])
    check(got, r, bound, f"{form} gelu")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("form", ["dma64x64", "dma64x160", "dma128x128", "dma128x160", "reg64x160", "reg128x128"])
def test_layernorm_statistics_out(hip, form, dtype):
    """DADD_EPI_LNSTAT (N = 320: a multiple of every wave width) with bias + residual: the row partials against float64
    sums over the output the same launch stored, within n 2^-24 sum|term|."""
    from progressive_stable_diffusion_amd import lib as L
    f = _forms()[form]
    n, m = 320, 144
    parts = n // (f["kw"]["tile_n"] // 2)
    x, w, t, flags, r, bound = operands(f["shape"], (), n, "br", dtype)
    got, side = run(hip, x, w, t, flags | L.EPI_LNSTAT | f.get("tune", 0), tuple(r.shape), dtype, f["kw"],
                    side=dict(ln_stats_out=((parts, m, 2), F32)))
    check(got, r, bound, f"{form} lnstat")
    o = got.to(F64).reshape(m, parts, -1)
    want = torch.stack([o.sum(-1), (o * o).sum(-1)], dim=-1).permute(1, 0, 2)
    slack = (n // parts) * U32 * torch.stack([o.abs().sum(-1), (o * o).sum(-1)], dim=-1).permute(1, 0, 2) + 1e-30
    assert bool(((side["ln_stats_out"].to(F64) - want).abs() <= slack).all()), form


GN_FORMS = {   # full tiles, whole-wave row blocks inside one sample, whole groups per wave: name -> (x shape, conv, N, tile)
    "halo16": ((2, 16, 16, 64), dict(taps=9, pad=1), 320, (128, 160)),
    "halo32": ((1, 32, 32, 64), dict(taps=9, pad=1), 320, (128, 160)),
    "dma128x160": ((2, 8, 8, K), {}, 320, (128, 160)),
    "dma64x128": ((2, 8, 8, K), {}, 256, (64, 128)),
}


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("flagset", FLAGSETS)
@pytest.mark.parametrize("form", list(GN_FORMS))
def test_groupnorm_statistics_out(hip, form, flagset, dtype):
    """DADD_EPI_GNSTAT: the output as on the plain path, the chunk partials against float64 sums over the stored output."""
    from progressive_stable_diffusion_amd import lib as L
    shape, conv, n, tile = GN_FORMS[form]
    x, w, t, flags, r, bound = operands(shape, tuple(sorted(conv.items())), n, flagset, dtype)
    b, ho, wo, _ = r.shape
    nchunk = ho * wo // (tile[0] // 2)
    got, side = run(hip, x, w, t, flags | L.EPI_GNSTAT, tuple(r.shape), dtype,
                    dict(tile_m=tile[0], tile_n=tile[1], gn_nchunk=nchunk, **conv), side=dict(gn_ws=((b * nchunk * 64,), F32)))
    check(got, r, bound, f"{form} gnstat {flagset}")
    o = got.to(F64).reshape(b, nchunk, -1, 32, n // 32)
    want = torch.stack([o.sum(dim=(2, 4)), (o * o).sum(dim=(2, 4))], dim=-1)
    terms = o.shape[2] * o.shape[4]
    slack = terms * U32 * torch.stack([o.abs().sum(dim=(2, 4)), (o * o).sum(dim=(2, 4))], dim=-1) + 1e-30
    assert bool(((side["gn_ws"].to(F64).reshape(want.shape) - want).abs() <= slack).all()), form


# ---- LayerNorm fold and GEGLU --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fold_operands(m_shape, n, geglu, fold, dtype, residual):
    """x with a per-row offset (so that the mean term matters), gamma o W / c1 / composed bias of engine.fold_layernorm in
    the GEGLU row order when asked, the producer's row partials in 4 parts, the float64 reference and its TOL bound."""
    from progressive_stable_diffusion_amd import engine as E
    from progressive_stable_diffusion_amd import lib as L
    b, hi, wi, k = m_shape
    m = b * hi * wi
    x = (rnd(m_shape, 11) + 2.0 * rnd((b, hi, wi, 1), 12)).to(dtype)
    g = torch.Generator().manual_seed(13)
    w = torch.randn(n, k, generator=g) / math.sqrt(k)
    bias = torch.randn(n, generator=g) * 0.1
    t, kw, flags = {}, {}, L.EPI_BIAS
    if fold:
        gamma, beta = 1.0 + 0.2 * torch.randn(k, generator=g), 0.2 * torch.randn(k, generator=g)
        w16, c1, bias = E.fold_layernorm(w, bias, gamma, beta, dtype=dtype)
        flags |= L.EPI_LNFOLD
    else:
        w16, c1 = w.to(dtype), None
    if geglu:
        idx = E.geglu_interleave(torch.arange(n)[:, None].float(), torch.zeros(n))[0][:, 0].long()
        w16, bias, c1 = w16[idx].contiguous(), bias[idx].contiguous(), (None if c1 is None else c1[idx].contiguous())
        flags |= L.EPI_GEGLU
    t["bias"] = bias.float()
    if fold:
        kw["ln_c1"] = c1
    n_out = n // 2 if geglu else n
    if residual:
        t["residual"], flags = rnd((b, hi, wi, n_out), 14, dtype=dtype), flags | L.EPI_RESIDUAL
    xp = x.to(F64).reshape(m, 4, k // 4)
    stats = torch.stack([xp.sum(-1), (xp * xp).sum(-1)], dim=-1).permute(1, 0, 2).float().contiguous()
    r = torch.zeros((b, hi, wi, n_out), dtype=F64)
    REF64.igemm(x, w16, r, flags=flags, **t, **kw)
    key = "igemm.lnfold" if fold else "igemm.geglu"
    return x, w16, t, kw, flags, stats, r, tol_bound(key, r, dtype)


def run_fold(hip, form_kw, tune, n, geglu, fold, stats_in, dtype, residual, what, m_shape=(4, 6, 6, K)):
    x, w16, t, kw, flags, stats, r, bound = fold_operands(m_shape, n, geglu, fold, dtype, residual)
    t = dict(t, **kw)                   # c1 (and the partials) are operands too: banded like the rest
    if stats_in:
        t["ln_stats_in"] = stats
    got, _ = run(hip, x, w16, t, flags | tune, tuple(r.shape), dtype, form_kw)
    check(got, r, bound, what)


LN_ROUTES = [   # (name, form, statistics from the producer?)
    ("in-loop 64x160", "dma64x160", False), ("in-loop 128x160", "dma128x160", False), ("in-loop 64x64", "dma64x64", False),
    ("global 64x160", "dma64x160", True), ("global reg64x160", "reg64x160", True),
    ("lds 128x160", "dma128x160", True), ("lds 128x128", "dma128x128", True), ("lds reg128x128", "reg128x128", True),
]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("route", LN_ROUTES, ids=[r[0].replace(" ", "-") for r in LN_ROUTES])
def test_layernorm_fold(hip, route, dtype):
    """The three routes of a folded LayerNorm's row statistics: summed in the K loop, the producer's partials read from
    global memory by the epilogue (64-row tiles), the partials, c1 and the bias staged in LDS (128-row tiles).  Bias +
    residual, N = 200."""
    name, form, stats_in = route
    f = _forms()[form]
    run_fold(hip, f["kw"], f.get("tune", 0), 200, False, True, stats_in, dtype, True, f"ln fold {name}")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_layernorm_fold_on_the_persistent_ring(hip, dtype):
    """128 x 160 persistent tiles with the operands staged in LDS: the instantiation that batches by column block."""
    from progressive_stable_diffusion_amd import lib as L
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    b = (128 * (ncu // 2 + 1)) // 36 + 1               # x 2 column tiles > CUs
    run_fold(hip, dict(tile_m=128, tile_n=160), L.TUNE_PERSIST, 200, False, True, True, dtype, True, "ln fold ring",
             m_shape=(b, 6, 6, K))


GEGLU_CASES = [   # (name, form, folded?, statistics from the producer?)   N = 256: 128 outputs, two hidden fragments per wave
    ("plain 64x128", dict(tile_m=64, tile_n=128), False, False), ("plain 128x128", dict(tile_m=128, tile_n=128), False, False),
    ("fold in-loop 64x128", dict(tile_m=64, tile_n=128), True, False), ("fold global 64x128", dict(tile_m=64, tile_n=128), True, True),
    ("fold lds 128x128", dict(tile_m=128, tile_n=128), True, True),
]


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", GEGLU_CASES, ids=[c[0].replace(" ", "-") for c in GEGLU_CASES])
def test_geglu(hip, case, dtype):
    name, kw, fold, stats_in = case
    run_fold(hip, kw, 0, 256, True, fold, stats_in, dtype, False, f"geglu {name}")
    if not fold:                        # the register-staged kernel, plain
        from progressive_stable_diffusion_amd import lib as L
        run_fold(hip, kw, L.TUNE_NODMA, 256, True, False, False, dtype, False, f"geglu {name} reg")
