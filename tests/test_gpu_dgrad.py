"""-m gpu: the data gradient of the stride-2 and the upsampled 3x3 conv on the HIP kernel (csrc/dgrad.hip) through
``HipBackend.dgrad_resample`` and the operators ``grad_ops.downsample2d`` / ``upsample2d``, against float64 autograd on
the same 16-bit operands (tests/dgrad_reference.py).

Tolerances: dx is a 16-bit output - fp16 the project's conv tolerance 3e-3 + 2e-3 |ref|, bf16 2e-2 + 1.6e-2 |ref|
(derivation and the share the kernel's rounding points use of it: tests/dgrad_reference.py, tests/test_dgrad_cpu.py); on
integer operands dx is exact.  The composed stages take the per-tensor relative L2 bound of the other composed blocks.
Shapes are the smallest that reach each hazard: ragged K, four unequal parity classes below one tile, the oy + 1 == Ho
edge, a batch edge inside a tile, a ragged second tile, two c tiles, M = 15."""
import pytest
import torch

from progressive_stable_diffusion_amd import grad_ops
from tests import dgrad_reference as D
from tests import grad_reference as R
from tests import norm_grad_reference as N

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
NAN = float("nan")
BLOCK_BOUND = 4e-3      # relative L2 per tensor of a composed block (tests/test_gpu_norm_grad.py)
IDS = [f"{c.mode}-{c.b}x{c.h}x{c.w}-C{c.c}-N{c.n}" for c in D.CASES]


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(torch.device("cuda:0"))


def filled(hip, shape, value, dtype=F16):
    t = hip.empty(shape, dtype)
    with hip.ctx():
        t.fill_(value)
    return t


def mode_kw(case):
    return dict(ups=1) if case.mode == "ups" else dict(stride=2)


def run_dgrad(hip, case, dy, w, dyd=None, wt=None):
    """One launch on a NaN-filled dx -> dx [B,H,W,C], synchronised."""
    dyd = hip.to_device(dy) if dyd is None else dyd
    wt = hip.to_device(D.relaid(w, case.mode)) if wt is None else wt
    dx = filled(hip, (case.b, case.h, case.w, case.c), NAN, dy.dtype)
    hip.dgrad_resample(dyd, wt, dx, **mode_kw(case))
    hip.synchronize()
    return dx


# ---- the kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_dgrad_against_float64(hip, case):
    dy, w, dx_ref = D.case_operands(case)
    dx = run_dgrad(hip, case, dy, w)
    print(f"{case}: worst err/bound {D.bound_ratio(dx, dx_ref, *N.TOL16[F16]):.3f}")
    N.close16(dx, dx_ref, f"dgrad {case}")


@pytest.mark.parametrize("case", D.BF16_CASES, ids=["stride2", "ups"])
def test_dgrad_bf16(hip, case):
    dy, w, dx_ref = D.case_operands(case, BF16)
    dx = run_dgrad(hip, case, dy, w)
    assert dx.dtype == BF16
    print(f"{case} bf16: worst err/bound {D.bound_ratio(dx, dx_ref, *N.TOL16[BF16]):.3f}")
    N.close16(dx, dx_ref, f"dgrad bf16 {case}")


@pytest.mark.parametrize("case", D.EXACT_CASES, ids=["stride2", "ups"])
def test_dgrad_is_exact_on_integers(hip, case):
    """dy in {-2..2}, w in {-1, 0, 1}, asymmetric: a wrong fragment map, tap or slab cannot hide in a tolerance."""
    dy, w, dx_ref = D.exact_operands(case)
    dx = run_dgrad(hip, case, dy, w)
    bad = dx.double().cpu() != dx_ref
    assert not bool(bad.any()), f"{int(bad.sum())}/{bad.numel()} values differ, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("case", [D.CASES[0], D.CASES[4]], ids=["stride2", "ups"])
def test_dgrad_stays_inside_its_column_slice(hip, case):
    """dx is the middle column slice of a wider sentinel-filled tensor, dy a column slice of a wider one."""
    dy, w, dx_ref = D.case_operands(case)
    c, n = case.c, case.n
    dyw = filled(hip, dy.shape[:-1] + (128,), NAN)
    dxw = filled(hip, (case.b, case.h, case.w, 3 * c), 1234.0)
    with hip.ctx():
        dyw[..., 8:8 + n] = dy.cuda()
        dxw[..., c:2 * c] = NAN
    hip.dgrad_resample(dyw[..., 8:8 + n], hip.to_device(D.relaid(w, case.mode)), dxw[..., c:2 * c], **mode_kw(case))
    hip.synchronize()
    assert bool((dxw[..., :c] == 1234.0).all()) and bool((dxw[..., 2 * c:] == 1234.0).all()), "wrote outside the slice"
    N.close16(dxw[..., c:2 * c], dx_ref, f"sliced {case}")       # finite: no NaN left inside


@pytest.mark.parametrize("case", [D.CASES[3], D.CASES[6]], ids=["stride2", "ups"])
def test_dgrad_is_deterministic_and_capturable(hip, case):
    """Two calls: equal bit for bit; captured into a graph and launched twice: equal to the eager result bit for bit."""
    dy, w, _ = D.case_operands(case)
    dyd, wt = hip.to_device(dy), hip.to_device(D.relaid(w, case.mode))
    dx1 = run_dgrad(hip, case, dy, w, dyd, wt)
    dx2 = run_dgrad(hip, case, dy, w, dyd, wt)
    assert torch.equal(dx1, dx2)
    dx = filled(hip, tuple(dx1.shape), NAN)
    hip.synchronize()
    hip.graph_begin()
    hip.dgrad_resample(dyd, wt, dx, **mode_kw(case))
    g = hip.graph_end()
    try:
        for _ in range(2):
            hip.zero_(dx)
            hip.graph_launch(g)
            hip.synchronize()
            assert torch.equal(dx, dx1)
    finally:
        hip.graph_destroy(g)


@pytest.mark.parametrize("bad", ["C=96", "N=70", "Ho", "Wo ups", "both modes", "no mode", "mixed types", "wt shape"])
def test_dgrad_contract(hip, bad):
    b, h, c, n = 2, 16, 64, 72
    kw = dict(stride=2)
    dy_shape, dtype = (b, 8, 8, n), F16
    if bad == "C=96":
        c = 96
    elif bad == "N=70":
        n, dy_shape = 70, (b, 8, 8, 70)
    elif bad == "Ho":
        dy_shape = (b, 9, 8, n)
    elif bad == "Wo ups":
        kw, dy_shape = dict(ups=1), (b, 32, 30, n)
    elif bad == "both modes":
        kw = dict(stride=2, ups=1)
    elif bad == "no mode":
        kw = dict()
    elif bad == "mixed types":
        dtype = BF16
    t = 16 if kw.get("ups") else 9
    wt = hip.zeros((c, t * n + (8 if bad == "wt shape" else 0)), F16)
    dy, dx = hip.zeros(dy_shape, F16), filled(hip, (b, h, h, c), NAN, dtype)
    with pytest.raises(ValueError):
        hip.dgrad_resample(dy, wt, dx, **kw)
    hip.synchronize()
    assert bool(torch.isnan(dx).all()), "a refused call launched something"


# ---- operators -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [D.CASES[0], D.CASES[4]], ids=["downsample2d", "upsample2d"])
def test_operator_forward_and_backward(hip, case):
    dy, w16, _ = D.case_operands(case)
    stride, ups = (1, True) if case.mode == "ups" else (2, False)
    op = grad_ops.upsample2d if ups else grad_ops.downsample2d
    x = R.rnd((case.b, case.h, case.w, case.c), 7700)
    w, bias = w16.float(), R.rnd((case.n,), 7701, 0.1, F32)            # the master rounds to w16 exactly
    y_ref, dx_ref, _, _ = R.conv_autograd(x, w16, dy, 9, stride, ups, bias)
    xd = x.cuda().requires_grad_(True)
    wd, bd = w.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
    y = op(hip, xd, wd, bd)
    assert y.dtype == F16 and y.shape == dy.shape
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    R.close(y, y_ref, f"{case.mode} y")
    R.close(xd.grad, dx_ref, f"{case.mode} x.grad")
    assert xd.grad.dtype == F16 and wd.grad.shape == w.shape and bd.grad.shape == bias.shape
    R.WgradRef(x, dy, 9, stride, ups).check(wd.grad, bd.grad, f"{case.mode} operator")
    x2 = x.cuda()                                                       # no data gradient wanted: none computed
    w2 = w.cuda().requires_grad_(True)
    op(hip, x2, w2).backward(dy.cuda())
    torch.cuda.synchronize()
    assert x2.grad is None and torch.equal(w2.grad, wd.grad)


# ---- two composed stages -------------------------------------------------------------------------------------------
def _leaves(params, cuda=False):
    return {k: (v.cuda() if cuda else v.double()).requires_grad_(True) for k, v in params.items()}


def _check_block(what, got, ref):
    errs = {name: N.rel_l2(got[name], ref[name]) for name in ref}
    for name, err in errs.items():
        print(f"{what} d{name}: relative L2 error {err:.3e}")
    print(f"{what}: worst relative L2 error {max(errs.values()):.3e} (bound {BLOCK_BOUND:.0e})")
    for name, err in errs.items():
        assert err <= BLOCK_BOUND, (what, name, err)


def _conv_params(r, name, seed, n, c):
    return {"w" + name: r((n, 9 * c), seed, (9 * c) ** -0.5, F32), "c" + name: r((n,), seed + 1, 0.1, F32)}


def test_down_stage_gradients(hip):
    """GroupNorm+SiLU -> conv3x3 -> downsample2d -> conv3x3, B = 2, 8x8 -> 4x4, 64 -> 64: every gradient against float64
    autograd of the same stage with the weights rounded to fp16; the gradient of x and of the first conv cross the
    stride-2 data gradient.  Measured on MI355X: worst tensor 4.2e-4 (dx), weights 3.5-3.6e-4, dg / db 3.8-3.9e-4
    (DESIGN.md 7.1)."""
    b, hw, ch = 2, 8, 64
    r = R.rnd
    x, dy = (1.5 * r((b, hw, hw, ch), 71, dtype=F32) + 0.3).half(), r((b, hw // 2, hw // 2, ch), 72)
    p = dict(g=1 + 0.2 * r((ch,), 73, dtype=F32), b=r((ch,), 74, 0.2, F32), **_conv_params(r, "1", 75, ch, ch),
             **_conv_params(r, "d", 77, ch, ch), **_conv_params(r, "2", 79, ch, ch))
    q = _leaves({k: (v.half() if k.startswith("w") else v) for k, v in p.items()})
    x64 = x.double().requires_grad_(True)
    D.down_stage64(x64, q).backward(dy.double())
    ref = dict({k: v.grad for k, v in q.items()}, x=x64.grad)
    d = _leaves(p, cuda=True)
    xd = x.cuda().requires_grad_(True)
    hdn = grad_ops.conv3x3(hip, grad_ops.group_norm(hip, xd, d["g"], d["b"], silu=True), d["w1"], d["c1"])
    out = grad_ops.conv3x3(hip, grad_ops.downsample2d(hip, hdn, d["wd"], d["cd"]), d["w2"], d["c2"])
    out.backward(dy.cuda())
    torch.cuda.synchronize()
    _check_block("down stage", dict({k: v.grad for k, v in d.items()}, x=xd.grad), ref)


def test_up_stage_gradients(hip):
    """upsample2d(x) -> group_norm([h | skip], SiLU) -> conv3x3, B = 2, 4x4 -> 8x8, 64 + 64 -> 64: the gradients of x
    (through the upsampled data gradient), of skip and of every weight.  Measured on MI355X: worst tensor 4.2e-4 (dx),
    dskip 2.9e-4, weights 2.7-3.0e-4."""
    b, hw, ch = 2, 4, 64
    r = R.rnd
    x, skip = r((b, hw, hw, ch), 81), (1.5 * r((b, 2 * hw, 2 * hw, ch), 82, dtype=F32) + 0.3).half()
    dy = r((b, 2 * hw, 2 * hw, ch), 83)
    p = dict(g=1 + 0.2 * r((2 * ch,), 84, dtype=F32), b=r((2 * ch,), 85, 0.2, F32), **_conv_params(r, "u", 86, ch, ch),
             **_conv_params(r, "1", 88, ch, 2 * ch))
    q = _leaves({k: (v.half() if k.startswith("w") else v) for k, v in p.items()})
    x64, s64 = x.double().requires_grad_(True), skip.double().requires_grad_(True)
    D.up_stage64(x64, s64, q).backward(dy.double())
    ref = dict({k: v.grad for k, v in q.items()}, x=x64.grad, skip=s64.grad)
    d = _leaves(p, cuda=True)
    xd, sd = x.cuda().requires_grad_(True), skip.cuda().requires_grad_(True)
    hdn = grad_ops.upsample2d(hip, xd, d["wu"], d["cu"])
    out = grad_ops.conv3x3(hip, grad_ops.group_norm(hip, hdn, d["g"], d["b"], silu=True, x2=sd), d["w1"], d["c1"])
    out.backward(dy.cuda())
    torch.cuda.synchronize()
    _check_block("up stage", dict({k: v.grad for k, v in d.items()}, x=xd.grad, skip=sd.grad), ref)
