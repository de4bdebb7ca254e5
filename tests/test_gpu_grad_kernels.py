"""-m gpu: the gradients of Linear / conv3x3 on the HIP kernels - the M-reduction GEMM of the weight gradient
(csrc/wgrad.hip) through ``HipBackend.wgrad``, the data gradient through ``HipBackend.dgrad`` and the autograd
operators of ``grad_ops`` - against float64 autograd on the same 16-bit operands (tests/grad_reference.py).

Tolerances: ``dW`` / ``dbias`` elementwise (M + 2) * 2^-24 * (|dy|^T |x|), derived in tests/grad_reference.py (16-bit
products are exact in fp32; only the fp32 accumulation of M terms errs) - a dropped or doubled term is tens of times over
it at these M (<= 513).  ``dx`` and ``y`` are rounded to 16 bits: the project's conv tolerance 3e-3 + 2e-3 |ref|.
Shapes are the smallest that reach each hazard: ragged M and N, M below one staged tile, image rows wrapping inside a
tile with padding on all four sides, ragged slices of the split reduction, stride 2, the upsample map."""
import pytest
import torch

from progressive_stable_diffusion_amd import grad_ops
from tests import grad_reference as R

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
NAN = float("nan")


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(torch.device("cuda:0"))


def filled(hip, shape, value, dtype=F32):
    t = hip.empty(shape, dtype)
    with hip.ctx():
        t.fill_(value)
    return t


def run_wgrad(hip, dy, x, taps=1, stride=1, ups=0, splitm=1, bias=True, xd=None, dyd=None):
    """One launch on NaN-filled outputs and scratch -> (dw [N, taps, C], dbias or None), synchronised."""
    n, c = dy.shape[-1], x.shape[-1]
    xd = hip.to_device(x) if xd is None else xd
    dyd = hip.to_device(dy) if dyd is None else dyd
    dw = filled(hip, (n, taps, c), NAN)
    db = filled(hip, (n,), NAN) if bias else None
    partial = filled(hip, (hip.wgrad_partial_numel(splitm, n, c, taps),), NAN) if splitm > 1 else None
    hip.wgrad(dyd, xd, dw, dbias=db, taps=taps, stride=stride, ups=ups, pad=1 if taps == 9 else 0, splitm=splitm,
              partial=partial)
    hip.synchronize()
    return dw, db


# ---- weight gradient -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,c,splitm", [(200, 192, 128, 1), (513, 320, 64, 1), (513, 320, 64, 4), (64, 72, 64, 1),
                                          (40, 64, 64, 1)])
def test_wgrad_linear(hip, m, n, c, splitm):
    x, dy, ref = R.linear_case(m, n, c)
    dw, db = run_wgrad(hip, dy, x, splitm=splitm)
    ref.check(dw, db, f"linear M{m} N{n} C{c} splitm{splitm}")      # dbias: the (513, 320, 64) cases among them


@pytest.mark.parametrize("b,h,c,n,stride,ups,splitm", [(2, 12, 64, 128, 1, 0, 1), (2, 8, 128, 64, 1, 0, 4),
                                                       (2, 16, 64, 72, 2, 0, 1), (2, 4, 64, 64, 1, 1, 1)])
def test_wgrad_conv3x3(hip, b, h, c, n, stride, ups, splitm):
    x, dy, ref = R.conv_case(b, h, c, n, stride, bool(ups))
    dw, db = run_wgrad(hip, dy, x, taps=9, stride=stride, ups=ups, splitm=splitm)
    ref.check(dw, db, f"conv3x3 B{b} H{h} C{c} N{n} s{stride} u{ups} splitm{splitm}")


def test_wgrad_bf16(hip):
    x, dy, ref = R.conv_case(1, 12, 64, 128, 1, False, BF16)
    dw, db = run_wgrad(hip, dy, x, taps=9)
    ref.check(dw, db, "conv3x3 bf16")


def test_wgrad_two_sources_fill_one_weight_gradient(hip):
    """Skip-concat [x1 | x2]: two calls into the column views of one dW [64][9][192]; a call leaves the other source's
    columns alone."""
    c1, c2 = 128, 64
    x, dy, ref = R.conv_case(2, 8, c1 + c2, 64)
    x1, x2, dyd = hip.to_device(x[..., :c1].contiguous()), hip.to_device(x[..., c1:].contiguous()), hip.to_device(dy)
    dw = filled(hip, (64, 9, c1 + c2), NAN)
    hip.wgrad(dyd, x1, dw[:, :, :c1], taps=9, pad=1, splitm=1)
    hip.synchronize()
    assert bool(torch.isnan(dw[:, :, c1:]).all()) and bool(torch.isfinite(dw[:, :, :c1]).all())
    ref.check(dw[:, :, :c1], None, "two sources, first", cols=slice(0, c1))
    hip.wgrad(dyd, x2, dw[:, :, c1:], taps=9, pad=1, splitm=1)
    hip.synchronize()
    ref.check(dw, None, "two sources, both")


def test_wgrad_two_sources_flat_weight_with_ld_tap(hip):
    """The same through the 2-D form of dW and an explicit ``ld_tap``: the second source at a column offset."""
    c1, c2 = 128, 64
    x, dy, ref = R.conv_case(2, 8, c1 + c2, 64)
    dyd = hip.to_device(dy)
    dw = filled(hip, (64, 9 * (c1 + c2)), NAN)
    hip.wgrad(dyd, hip.to_device(x[..., :c1].contiguous()), dw, taps=9, pad=1, splitm=1, ld_tap=c1 + c2)
    hip.wgrad(dyd, hip.to_device(x[..., c1:].contiguous()), dw[:, c1:], taps=9, pad=1, splitm=1, ld_tap=c1 + c2)
    hip.synchronize()
    ref.check(dw, None, "two sources, flat dW")


def test_wgrad_strided_views(hip):
    """x is the channel slice [..., 64:128] of a 192-wide tensor, dy the slice [..., 0:64] of a 128-wide one."""
    xw, dyw = R.rnd((2, 8, 8, 192), 31), R.rnd((2, 8, 8, 128), 32)
    x, dy = xw[..., 64:128], dyw[..., 0:64]
    ref = R.WgradRef(x, dy, 9)
    dw, db = run_wgrad(hip, dy, x, taps=9, splitm=2, xd=hip.to_device(xw)[..., 64:128], dyd=hip.to_device(dyw)[..., 0:64])
    ref.check(dw, db, "strided views")


def test_wgrad_overwrites_and_stays_inside_its_output(hip):
    """dw, dbias and partial start as NaN (run_wgrad) and come out finite; 64 sentinel floats behind dW stay."""
    x, dy, ref = R.linear_case(513, 320, 64)
    n, c, splitm = 320, 64, 4
    buf = filled(hip, (n * c + 64,), NAN)
    with hip.ctx():
        buf[n * c:] = 12345.0
    db = filled(hip, (n,), NAN)
    partial = filled(hip, (hip.wgrad_partial_numel(splitm, n, c),), NAN)
    hip.wgrad(hip.to_device(dy), hip.to_device(x), buf[:n * c].view(n, c), dbias=db, splitm=splitm, partial=partial)
    hip.synchronize()
    assert bool(torch.isfinite(buf).all()) and bool(torch.isfinite(db).all())
    assert bool((buf[n * c:] == 12345.0).all()), "wrote past the end of dW"
    ref.check(buf[:n * c], db, "overwrite")


def test_wgrad_is_deterministic_and_capturable(hip):
    """The same splitm-4 call twice: equal bit for bit; captured into a graph (one chain) and launched twice: equal to
    the eager result bit for bit."""
    x, dy, _ = R.conv_case(2, 8, 128, 64)
    xd, dyd = hip.to_device(x), hip.to_device(dy)
    dw1, db1 = run_wgrad(hip, dy, x, taps=9, splitm=4, xd=xd, dyd=dyd)
    dw2, db2 = run_wgrad(hip, dy, x, taps=9, splitm=4, xd=xd, dyd=dyd)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)
    dw, db = filled(hip, (64, 9, 128), NAN), filled(hip, (64,), NAN)
    partial = filled(hip, (hip.wgrad_partial_numel(4, 64, 128, 9),), NAN)
    hip.synchronize()
    hip.graph_begin()
    hip.wgrad(dyd, xd, dw, dbias=db, taps=9, pad=1, splitm=4, partial=partial)
    g = hip.graph_end()
    try:
        for _ in range(2):
            hip.zero_(dw)
            hip.graph_launch(g)
            hip.synchronize()
            assert torch.equal(dw, dw1) and torch.equal(db, db1)
    finally:
        hip.graph_destroy(g)


def test_wgrad_default_splitm_follows_the_documented_rule(hip):
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert hip.wgrad_splitm(32768, 320, 320, 9) == -(-2 * cu // (5 * 9 * 5))
    assert hip.wgrad_splitm(100, 64, 64) == 2                         # at least 64 rows per slice
    assert hip.wgrad_splitm(1 << 20, 2560, 1280) == 1                 # already more tiles than 2 per CU
    x, dy, ref = R.linear_case(513, 320, 64)
    n, c = 320, 64
    splitm = hip.wgrad_splitm(513, n, c)
    dw, partial = filled(hip, (n, c), NAN), filled(hip, (hip.wgrad_partial_numel(splitm, n, c),), NAN)
    hip.wgrad(hip.to_device(dy), hip.to_device(x), dw, partial=partial)      # splitm=None
    hip.synchronize()
    ref.check(dw, None, f"default splitm {splitm}")
    with pytest.raises(ValueError):
        hip.wgrad(hip.to_device(dy), hip.to_device(x), dw)                   # default splitm > 1 without scratch


@pytest.mark.parametrize("bad", ["C=96", "N=70", "splitm=0", "taps=9,pad=0"])
def test_wgrad_contract(hip, bad):
    m, n, c, kw = 128, 64, 64, dict(splitm=1)
    if bad == "C=96":
        c = 96
    elif bad == "N=70":
        n = 70
    elif bad == "splitm=0":
        kw = dict(splitm=0)
    x, dy = hip.zeros((1, 8, m // 8, c), F16), hip.zeros((1, 8, m // 8, n), F16)
    if bad == "taps=9,pad=0":
        kw.update(taps=9, pad=0)
    dw = filled(hip, (n, kw.get("taps", 1) * c), NAN)
    with pytest.raises(ValueError):
        hip.wgrad(dy, x, dw, **kw)
    hip.synchronize()
    assert bool(torch.isnan(dw).all()), "a refused call launched something"


# ---- data gradient -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["conv", "linear"])
def test_dgrad(hip, kind):
    x, w, _, dy, taps, (_, dx_ref, _, _) = R.op_case(kind)
    wt = hip.to_device(grad_ops.dgrad_weight(w.half(), taps))
    dx = filled(hip, tuple(x.shape), NAN, F16)
    hip.dgrad(hip.to_device(dy), wt, dx, taps=taps)
    hip.synchronize()
    R.close(dx, dx_ref, f"dgrad {kind}")


def test_dgrad_two_sources(hip):
    """dx of a skip-concat input: two calls on the row slices [0, C1) and [C1, C1+C2) of the re-laid weight."""
    c1 = 128
    x, w, _, dy, taps, (_, dx_ref, _, _) = R.op_case("two_source")
    wt = hip.to_device(grad_ops.dgrad_weight(w.half(), taps))
    dyd = hip.to_device(dy)
    for lo, hi in ((0, c1), (c1, x.shape[-1])):
        dx = filled(hip, tuple(x.shape[:-1]) + (hi - lo,), NAN, F16)
        hip.dgrad(dyd, wt[lo:hi], dx, taps=taps)
        hip.synchronize()
        R.close(dx, dx_ref[..., lo:hi], f"dgrad two sources, columns {lo}:{hi}")


def test_dgrad_refuses_thin_outputs(hip):
    with pytest.raises(ValueError):
        hip.dgrad(hip.zeros((1, 8, 8, 8), F16), hip.zeros((64, 72), F16), hip.zeros((1, 8, 8, 64), F16), taps=9)


# ---- operators -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["conv", "linear"])
def test_operator_forward_and_backward(hip, kind):
    x, w, bias, dy, taps, (y_ref, dx_ref, _, _) = R.op_case(kind)
    if kind == "linear":
        x, dy, y_ref, dx_ref = x[0, 0], dy[0, 0], y_ref[0, 0], dx_ref[0, 0]
    xd = x.cuda().requires_grad_(True)
    wd, bd = w.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
    y = grad_ops.conv3x3(hip, xd, wd, bd) if kind == "conv" else grad_ops.linear(hip, xd, wd, bd)
    assert y.dtype == F16
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    R.close(y, y_ref, f"{kind} y")
    R.close(xd.grad, dx_ref, f"{kind} x.grad")
    assert xd.grad.dtype == F16 and wd.grad.shape == w.shape and bd.grad.shape == bias.shape
    R.WgradRef(x, dy, taps).check(wd.grad, bd.grad, f"{kind} operator")


def test_operator_stride2_has_weight_gradient_only(hip):
    x, w, bias, dy, taps, _ = R.op_case("conv_s2")
    wd, bd = w.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="data gradient"):
        grad_ops.conv3x3(hip, x.cuda().requires_grad_(True), wd, bd, stride=2)
    y = grad_ops.conv3x3(hip, x.cuda(), wd, bd, stride=2)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    R.WgradRef(x, dy, 9, 2).check(wd.grad, bd.grad, "stride-2 operator")
