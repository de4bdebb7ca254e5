"""-m gpu: the attention kernels where the LARGE logits sit in chosen places (tests/attention_cases.py), on every
registered flash_kernel instantiation of both storage types, against float64 references from the same rounded operands.

Bounds are the project's existing ones (fp16 3e-3 + 3e-3 |ref| as test_self_attention, bf16 2e-2 + 2e-2 |ref| as
test_self_attention_bf16), taken against the `model` reference: float64 with the kernel's two documented rounding points
(pre-scaled Q and P rounded to the storage type).  `|out - exact|` and `|model - exact|` are measured and printed, not
bounded (profiles/r04_c_attention_edges.txt): they show what pre-scaling Q in 16 bits costs at |logit| ~ 100..300.
"""
import math

import pytest
import torch

from tests import attention_cases as AC
from tests.torch_backend import TorchRefBackend

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
REF = TorchRefBackend()
NKS = (37, 64, 300, 1041)       # one ragged tile; one full tile; several with a ragged tail; 17 tiles (odd count, DEEP)
MEASURED = {}                   # (pattern, dtype, d) -> [max |out - exact|, max |model - exact|, max |out - model|]


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    be = HipBackend(torch.device("cuda:0"))
    yield be
    if MEASURED:
        print("\n# measured, not bounded: max over the cases of one (pattern, storage type, head dim)")
        print(f"# {'pattern':24s} {'type':5s} {'d':>4s} {'|out-exact|':>12s} {'|model-exact|':>14s} {'|out-model|':>12s}")
        for (pat, dt, d), (oe, me, om) in sorted(MEASURED.items(), key=lambda kv: (kv[0][0], str(kv[0][1]), kv[0][2])):
            print(f"  {pat:24s} {'bf16' if dt == BF16 else 'f16':5s} {d:4d} {oe:12.3e} {me:14.3e} {om:12.3e}")


def _note(pattern, dtype, d, out, exact, model):
    o = out.double()
    new = [float((o - exact).abs().nan_to_num(float("inf")).max()), float((model - exact).abs().max()),
           float((o - model).abs().nan_to_num(float("inf")).max())]
    old = MEASURED.setdefault((pattern, dtype, d), [0.0, 0.0, 0.0])
    MEASURED[(pattern, dtype, d)] = [max(a, b) for a, b in zip(old, new)]
    return new


def _launch_flash(hip, q, k, v, heads, dtype):
    """Two launches; the first between prof_begin / prof_end -> (out, second out, recorded kernel names)."""
    o1, o2 = hip.zeros(q.shape, dtype), hip.zeros(q.shape, dtype)
    hip.prof_begin()
    hip.attention(q, k, v, o1, heads)
    rec = hip.prof_end()
    hip.attention(q, k, v, o2, heads)
    hip.synchronize()
    return o1, o2, [r[0] for r in rec]


_FLASH_CASES = [pytest.param(dt, var, nk, pat, arg, id=f"{var.label(dt)}-nk{nk}-{pat}{arg if pat not in ('flat', 'random_spiky') else ''}")
                for dt in (F16, BF16) for var in AC.VARIANTS[dt] for nk in NKS for pat, arg in AC.flash_patterns(nk)]


@pytest.mark.parametrize("dtype,var,nk,pattern,arg", _FLASH_CASES)
def test_flash_placed_logits(hip, dtype, var, nk, pattern, arg):
    """Every registered instantiation x key count x pattern: the launch is the promised instantiation, the output is
    finite, within the project's bound of the model reference (one_hot / flat: of the exact one too, one_hot: the row
    IS v[p]), and a second launch gives the same bits."""
    seed = NKS.index(nk) * 16 + AC.PATTERNS.index(pattern)
    q, k, v = (hip.to_device(t) for t in AC.build(pattern, arg, var.b, var.heads, var.d, var.nq, nk, dtype, seed))
    out, out2, names = _launch_flash(hip, q, k, v, var.heads, dtype)
    assert names == [var.kernel_name(dtype)], names
    exact, model = AC.references(q, k, v, var.heads)
    oe, me, om = _note(f"{pattern}({arg})" if pattern not in ("flat", "random_spiky") else pattern, dtype, var.d, out, exact, model)
    print(f"{var.label(dtype)} nk={nk} {pattern}({arg}): |out-exact| {oe:.3e} |model-exact| {me:.3e} |out-model| {om:.3e}")
    assert bool(torch.isfinite(out).all()), f"{int((~torch.isfinite(out)).any(dim=-1).sum())} of {out.shape[0] * out.shape[1]} rows not finite"
    ok, msg = AC.within(out, model, dtype)
    assert ok, "against model: " + msg
    if pattern in ("one_hot", "flat"):
        ok, msg = AC.within(out, exact, dtype)
        assert ok, "against exact: " + msg
    if pattern == "one_hot":
        want = v[:, int(arg) % nk][:, None, :].double().expand(-1, var.nq, -1)
        err = (out.double() - want).abs()
        assert bool((err <= AC.ULP[dtype] * want.abs() + 2.0 ** -24).all()), f"row != v[p]: max err {float(err.max()):.3e}"
    assert torch.equal(out, out2), "second launch differs"


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("pattern,arg", [("random_spiky", 0), ("first_tile_floor", 150)])
def test_self_attention_product_shape(hip, dtype, pattern, arg):
    """The shape the benchmark runs (B = 4, 8 heads, d = 40, 64 x 64 latent) through hip.self_attn: the eight-wave
    kernel, against float64 per (batch, head)."""
    b, heads, d, n = 4, 8, 40, 4096
    c = heads * d
    q, k, v = AC.build(pattern, arg, b, heads, d, n, n, dtype, seed=99)
    qkv = hip.to_device(torch.cat([q, k, v], dim=-1))
    out = hip.zeros((b, n, c), dtype)
    hip.prof_begin()
    hip.self_attn(qkv, out, heads)
    names = [r[0] for r in hip.prof_end()]
    hip.synchronize()
    assert names == [AC.Variant(40, 2, True, 8, b, heads, n).kernel_name(dtype)], names
    qd, kd, vd = qkv.split(c, dim=-1)
    exact, model = AC.references(qd, kd, vd, heads)
    oe, me, om = _note(f"product {pattern}", dtype, d, out, exact, model)
    print(f"product shape {pattern} {dtype}: |out-exact| {oe:.3e} |model-exact| {me:.3e} |out-model| {om:.3e}")
    assert bool(torch.isfinite(out).all())
    ok, msg = AC.within(out, model, dtype)
    assert ok, "against model: " + msg
    if pattern == "random_spiky":
        ok, msg = AC.within(out, exact, dtype)
        assert ok, "against exact: " + msg


# ------------------------------------------------------------------------------------------------ xattn_kernel
XTOL = {F16: (4e-3, 4e-3), BF16: (2.5e-2, 2.5e-2)}       # test_tri_xattn, test_tri_xattn_bf16


def _xclose(got, ref, dtype, what):
    atol, rtol = XTOL[dtype]
    err = (got.double() - ref).abs()
    bad = ~(err <= atol + rtol * ref.abs())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.nan_to_num(float('inf')).max()):.4e}"


def _run_xattn(hip, q, kv, gates, lam, mode, heads, dtype):
    out = hip.zeros(q.shape, dtype)
    hip.tri_xattn(q, kv, out, gates if mode == 0 else None, lam, mode, heads)
    hip.synchronize()
    return out


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [40, 80, 160])
@pytest.mark.parametrize("mode,lam", [(0, 3.0), (0, 0.0), (1, 0.0)])
@pytest.mark.parametrize("pattern", AC.XATTN_PATTERNS)
def test_tri_xattn_placed_logits(hip, dtype, d, mode, lam, pattern):
    b, n, heads = 2, 300, 8
    q, kv = (hip.to_device(t) for t in AC.build_xattn(pattern, b, n, heads, d, mode, dtype, seed=d + mode))
    gates = hip.to_device(torch.tensor([0.3, 0.7]))
    out = _run_xattn(hip, q, kv, gates, lam, mode, heads, dtype)
    assert bool(torch.isfinite(out).all())
    _xclose(out, AC.xattn_reference(q, kv, gates, lam, mode, heads), dtype, f"tri_xattn {pattern} d{d} mode{mode} lam{lam}")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("lam", [0.0, 3.0])
def test_tri_xattn_256_queries_per_workgroup(hip, dtype, lam):
    """B * heads * ceil(N / 256) = 4 * 8 * 16 = 512: the launch with 256 queries per workgroup (four 16-query fragments
    per wave); N = 4091 is ragged against 16 and against 256.  The same rows through the B = 1 launch (64 queries per
    workgroup) must carry the same bits."""
    b, n, heads, d = 4, 4091, 8, 40
    q, kv = (hip.to_device(t) for t in AC.build_xattn("one_floor", b, n, heads, d, 0, dtype, seed=7))
    gates = hip.to_device(torch.tensor([0.3, 0.7]))
    out = _run_xattn(hip, q, kv, gates, lam, 0, heads, dtype)
    assert bool(torch.isfinite(out).all())
    _xclose(out, AC.xattn_reference(q, kv, gates, lam, 0, heads), dtype, f"tri_xattn qpb 256 lam{lam}")
    for bi in (0, 3):
        one = _run_xattn(hip, hip.to_device(q[bi:bi + 1]), hip.to_device(kv[bi:bi + 1]), gates, lam, 0, heads, dtype)
        assert torch.equal(one[0], out[bi]), f"sample {bi}: 64 and 256 queries per workgroup differ"


# ------------------------------------------------------------------------------------------------ attn2_fused
@pytest.mark.parametrize("b,hw", [(2, 256), (8, 4096)])          # attn2_fused_kernel<64> and <128>
@pytest.mark.parametrize("pattern", ["one_hot", "flat"])
def test_attn2_fused_logit_range(hip, b, hw, pattern):
    """Scores of +-100 log2 units and beyond (P one-hot per sixteen-key group), and x = 0 (P = 1/16 exactly), against
    TorchRefBackend.attn2_fused at test_attn2_fused's bound."""
    c = 320
    gen = torch.Generator().manual_seed(300 + hw)
    rn = lambda *s: torch.randn(*s, generator=gen)                   # noqa: E731
    x = (torch.zeros(b, hw, c) if pattern == "flat" else rn(b, hw, c)).to(F16)
    res = rn(b, hw, c).to(F16)
    mcat = (rn(b, 384, c) * (50.0 / math.sqrt(c))).to(F16)           # scores ~ N(0, 50^2)
    vw = (rn(b, c, 384) * 0.5).to(F16)
    bias = rn(c) * 0.1
    o_ref = torch.zeros(b, hw, c, dtype=F16)
    REF.attn2_fused(x, mcat, vw, bias, res, o_ref)
    if pattern == "one_hot":
        s = torch.einsum("mc,kc->mk", x[0].float(), mcat[0].float())
        assert float(s.abs().max()) > 100.0
    o = hip.zeros((b, hw, c), F16)
    hip.prof_begin()
    hip.attn2_fused(*(hip.to_device(t) for t in (x, mcat, vw, bias, res)), o)
    names = [r[0] for r in hip.prof_end()]
    hip.synchronize()
    assert names == ["attn2_fused_kernel<128>" if b * hw >= 8 * 4096 else "attn2_fused_kernel<64>"], names
    assert bool(torch.isfinite(o).all())
    err = (o.float().cpu() - o_ref.float()).abs()
    bad = err > 4e-3 + 3e-3 * o_ref.float().abs()
    assert not bool(bad.any()), f"attn2_fused {pattern} {b}x{hw}: {int(bad.sum())}/{bad.numel()} off, max err {float(err.max()):.4e}"
