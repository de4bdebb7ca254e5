"""-m gpu: the backward of GroupNorm(+SiLU), LayerNorm and GEGLU on the HIP kernels (csrc/norm_grad.hip) through
``HipBackend.groupnorm_grad`` / ``layernorm_grad`` / ``geglu`` / ``geglu_grad`` and the autograd operators of
``grad_ops``, against float64 autograd on the same 16-bit operands (tests/norm_grad_reference.py, where the bounds are
derived): 16-bit outputs 3e-3 + 2e-3 |ref| (bf16: 2e-2 + 1.6e-2 |ref|), dgamma / dbeta elementwise (M + 16) 2^-24 E.
Outputs and scratch are NaN-filled before every call.  Shapes are the smallest that reach each hazard: groups that
straddle the 8-channel vectors, ragged row chunks, two sources, two vectors per thread, many chunks, rows strided over
a bounded grid.  The two composed blocks (a ResnetBlock2D and a transformer feed-forward, written from ``grad_ops`` and
torch adds) are checked per tensor in relative L2 against float64 autograd of the same block: bound 4e-3."""
import pytest
import torch

from progressive_stable_diffusion_amd import grad_ops
from tests import norm_grad_reference as N

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
NAN = float("nan")
BLOCK_BOUND = 4e-3


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(torch.device("cuda:0"))


def filled(hip, shape, value, dtype=F32):
    t = hip.empty(shape, dtype)
    with hip.ctx():
        t.fill_(value)
    return t


class GnCall:
    """Device operands of one GroupNorm backward with NaN-filled outputs and scratch."""

    def __init__(self, hip, x, dy, gamma, beta, c1, silu, eps, groups=N.GROUPS):
        b, h, w, c = x.shape
        self.hip, self.kw = hip, dict(groups=groups, eps=eps, silu=bool(silu))
        self.x1 = hip.to_device(x[..., :c1].contiguous())
        self.x2 = hip.to_device(x[..., c1:].contiguous()) if c1 < c else None
        self.dy, self.gamma, self.beta = hip.to_device(dy), hip.to_device(gamma), hip.to_device(beta)
        self.dx1 = filled(hip, (b, h, w, c1), NAN, x.dtype)
        self.dx2 = filled(hip, (b, h, w, c - c1), NAN, x.dtype) if c1 < c else None
        self.dgamma, self.dbeta = filled(hip, (c,), NAN), filled(hip, (c,), NAN)
        self.ws = filled(hip, (hip.groupnorm_grad_ws_numel(b, h * w, c, groups),), NAN)

    def run(self):
        self.hip.groupnorm_grad(self.x1, self.x2, self.dy, self.gamma, self.beta, dx1=self.dx1, dx2=self.dx2,
                                dgamma=self.dgamma, dbeta=self.dbeta, ws=self.ws, **self.kw)
        self.hip.synchronize()
        return self

    @property
    def dx(self):
        return self.dx1 if self.dx2 is None else torch.cat([self.dx1, self.dx2], -1)


def run_ln(hip, x, dy, gamma, eps=1e-5):
    m, c = x.shape
    dx, dgamma, dbeta = filled(hip, (m, c), NAN, x.dtype), filled(hip, (c,), NAN), filled(hip, (c,), NAN)
    ws = filled(hip, (hip.layernorm_grad_ws_numel(m, c),), NAN)
    hip.layernorm_grad(hip.to_device(x), hip.to_device(dy), hip.to_device(gamma), dx=dx, dgamma=dgamma, dbeta=dbeta, ws=ws,
                       eps=eps)
    hip.synchronize()
    return dx, dgamma, dbeta


def run_geglu(hip, h, dy):
    m, f = dy.shape
    y, dh = filled(hip, (m, f), NAN, h.dtype), filled(hip, (m, 2 * f), NAN, h.dtype)
    hd = hip.to_device(h)
    hip.geglu(hd, y)
    hip.geglu_grad(hd, hip.to_device(dy), dh)
    hip.synchronize()
    return y, dh


# ---- GroupNorm backward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.GN_CASES)
def test_groupnorm_grad(hip, case):
    b, c1, c2, h, w, silu, eps = case
    x, dy, gamma, beta, ref = N.gn_case(*case)
    call = GnCall(hip, x, dy, gamma, beta, c1, silu, eps).run()
    ref.check(call.dx, call.dgamma, call.dbeta, f"groupnorm_grad {case}")


def test_groupnorm_grad_bf16(hip):
    case = N.GN_CASES[0]
    x, dy, gamma, beta, ref = N.gn_case(*case, dtype=BF16)
    call = GnCall(hip, x, dy, gamma, beta, case[1], case[5], case[6]).run()
    assert call.dx.dtype == BF16
    ref.check(call.dx, call.dgamma, call.dbeta, "groupnorm_grad bf16")


def test_groupnorm_grad_zero_variance(hip):
    """One (sample, group) of x is the constant 0.5: var = 0, rstd = eps^-1/2, everything finite and within tolerance."""
    case = N.GN_CASES[0]
    x, dy, gamma, beta, ref = N.gn_case(*case, constant_group=True)
    call = GnCall(hip, x, dy, gamma, beta, case[1], case[5], case[6]).run()
    assert bool(torch.isfinite(call.dx.float()).all())
    ref.check(call.dx, call.dgamma, call.dbeta, "groupnorm_grad zero variance")


def test_groupnorm_grad_outputs_may_be_left_out(hip):
    """dx only and dgamma / dbeta only give the bits of the full call."""
    case = N.GN_CASES[2]
    x, dy, gamma, beta, _ = N.gn_case(*case)
    full = GnCall(hip, x, dy, gamma, beta, case[1], case[5], case[6]).run()
    a = GnCall(hip, x, dy, gamma, beta, case[1], case[5], case[6])
    a.dgamma = a.dbeta = None
    a.run()
    assert torch.equal(a.dx, full.dx)
    p = GnCall(hip, x, dy, gamma, beta, case[1], case[5], case[6])
    p.dx1 = p.dx2 = None
    p.run()
    assert torch.equal(p.dgamma, full.dgamma) and torch.equal(p.dbeta, full.dbeta)


def test_groupnorm_grad_stays_inside_repeats_and_captures(hip):
    """64 sentinels behind dx and behind dgamma survive; two calls agree bit for bit; a captured call launched twice
    equals the eager result bit for bit."""
    case = N.GN_CASES[0]
    b, c1, _, h, w, silu, eps = case
    x, dy, gamma, beta, ref = N.gn_case(*case)
    first = GnCall(hip, x, dy, gamma, beta, c1, silu, eps).run()
    call = GnCall(hip, x, dy, gamma, beta, c1, silu, eps)
    n = x.numel()
    dxbuf, gbuf = filled(hip, (n + 64,), NAN, F16), filled(hip, (c1 + 64,), NAN)
    with hip.ctx():
        dxbuf[n:] = 123.0
        gbuf[c1:] = 12345.0
    call.dx1, call.dgamma = dxbuf[:n].view(x.shape), gbuf[:c1]
    call.run()
    assert bool((dxbuf[n:] == 123.0).all()), "wrote past the end of dx"
    assert bool((gbuf[c1:] == 12345.0).all()), "wrote past the end of dgamma"
    assert torch.equal(call.dx, first.dx) and torch.equal(call.dgamma, first.dgamma) and torch.equal(call.dbeta, first.dbeta)
    ref.check(call.dx, call.dgamma, call.dbeta, "groupnorm_grad into views")
    cap = GnCall(hip, x, dy, gamma, beta, c1, silu, eps)
    hip.synchronize()
    hip.graph_begin()
    hip.groupnorm_grad(cap.x1, cap.x2, cap.dy, cap.gamma, cap.beta, dx1=cap.dx1, dx2=cap.dx2, dgamma=cap.dgamma,
                       dbeta=cap.dbeta, ws=cap.ws, **cap.kw)
    g = hip.graph_end()
    try:
        for _ in range(2):
            hip.zero_(cap.dx1)
            hip.zero_(cap.dgamma)
            hip.graph_launch(g)
            hip.synchronize()
            assert torch.equal(cap.dx, first.dx) and torch.equal(cap.dgamma, first.dgamma) \
                and torch.equal(cap.dbeta, first.dbeta)
    finally:
        hip.graph_destroy(g)


@pytest.mark.parametrize("bad", ["C=36", "groups=3", "mixed types"])
def test_groupnorm_grad_contract(hip, bad):
    c, groups = (36, 4) if bad == "C=36" else (320, 3 if bad == "groups=3" else 32)
    x, dy = hip.zeros((2, 4, 4, c), F16), hip.zeros((2, 4, 4, c), BF16 if bad == "mixed types" else F16)
    gamma, beta = hip.zeros((c,), F32), hip.zeros((c,), F32)
    dx, dgamma, dbeta = filled(hip, (2, 4, 4, c), NAN, F16), filled(hip, (c,), NAN), filled(hip, (c,), NAN)
    ws = filled(hip, (1 << 16,), NAN)
    with pytest.raises(ValueError):
        hip.groupnorm_grad(x, None, dy, gamma, beta, dx1=dx, dgamma=dgamma, dbeta=dbeta, ws=ws, groups=groups, eps=1e-5,
                           silu=True)
    hip.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (dx, dgamma, dbeta, ws)), "a refused call launched something"


# ---- LayerNorm backward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,c", N.LN_CASES)
def test_layernorm_grad(hip, m, c):
    x, dy, gamma, beta, ref = N.ln_case(m, c)
    ref.check(*run_ln(hip, x, dy, gamma), f"layernorm_grad {m}x{c}")


def test_layernorm_grad_bf16(hip):
    x, dy, gamma, beta, ref = N.ln_case(100, 640, BF16)
    dx, dgamma, dbeta = run_ln(hip, x, dy, gamma)
    assert dx.dtype == BF16
    ref.check(dx, dgamma, dbeta, "layernorm_grad bf16")


def test_layernorm_grad_stays_inside_repeats_and_captures(hip):
    m, c = 1030, 320
    x, dy, gamma, beta, ref = N.ln_case(m, c)
    dx1, dg1, db1 = run_ln(hip, x, dy, gamma)
    xd, dyd, gd = hip.to_device(x), hip.to_device(dy), hip.to_device(gamma)
    dxbuf, gbuf, dbeta = filled(hip, (m * c + 64,), NAN, F16), filled(hip, (c + 64,), NAN), filled(hip, (c,), NAN)
    with hip.ctx():
        dxbuf[m * c:] = 123.0
        gbuf[c:] = 12345.0
    ws = filled(hip, (hip.layernorm_grad_ws_numel(m, c),), NAN)
    dx, dgamma = dxbuf[:m * c].view(m, c), gbuf[:c]
    hip.layernorm_grad(xd, dyd, gd, dx=dx, dgamma=dgamma, dbeta=dbeta, ws=ws)
    hip.synchronize()
    assert bool((dxbuf[m * c:] == 123.0).all()), "wrote past the end of dx"
    assert bool((gbuf[c:] == 12345.0).all()), "wrote past the end of dgamma"
    assert torch.equal(dx, dx1) and torch.equal(dgamma, dg1) and torch.equal(dbeta, db1)
    only = filled(hip, (m, c), NAN, F16)
    hip.layernorm_grad(xd, dyd, gd, dx=only)                              # data gradient only: no scratch
    hip.synchronize()
    assert torch.equal(only, dx1)
    hip.graph_begin()
    hip.layernorm_grad(xd, dyd, gd, dx=dx, dgamma=dgamma, dbeta=dbeta, ws=ws)
    g = hip.graph_end()
    try:
        for _ in range(2):
            hip.zero_(dxbuf[:m * c])
            hip.zero_(dbeta)
            hip.graph_launch(g)
            hip.synchronize()
            assert torch.equal(dx, dx1) and torch.equal(dgamma, dg1) and torch.equal(dbeta, db1)
    finally:
        hip.graph_destroy(g)


@pytest.mark.parametrize("bad", ["C=2056", "C=12", "mixed types"])
def test_layernorm_grad_contract(hip, bad):
    c = 2056 if bad == "C=2056" else 12 if bad == "C=12" else 320
    x, dy = hip.zeros((8, c), F16), hip.zeros((8, c), BF16 if bad == "mixed types" else F16)
    dx, dgamma, dbeta, ws = filled(hip, (8, c), NAN, F16), filled(hip, (c,), NAN), filled(hip, (c,), NAN), filled(hip, (1 << 16,), NAN)
    with pytest.raises(ValueError):
        hip.layernorm_grad(x, dy, hip.zeros((c,), F32), dx=dx, dgamma=dgamma, dbeta=dbeta, ws=ws)
    hip.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (dx, dgamma, dbeta, ws)), "a refused call launched something"


# ---- GEGLU -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,f,dtype", [(5, 8, F16), (130, 1280, F16), (64, 1280, BF16)])
def test_geglu_forward_and_backward(hip, m, f, dtype):
    h, dy, (y_ref, dh_ref) = N.geglu_case(m, f, dtype)
    y, dh = run_geglu(hip, h, dy)
    assert y.dtype == dh.dtype == dtype
    N.close16(y, y_ref, f"geglu {m}x{f} y")
    N.close16(dh, dh_ref, f"geglu {m}x{f} dh")


def test_geglu_stays_inside_repeats_and_captures(hip):
    m, f = 130, 1280
    h, dy, _ = N.geglu_case(m, f)
    y1, dh1 = run_geglu(hip, h, dy)
    hd, dyd = hip.to_device(h), hip.to_device(dy)
    ybuf, dhbuf = filled(hip, (m * f + 64,), NAN, F16), filled(hip, (2 * m * f + 64,), NAN, F16)
    with hip.ctx():
        ybuf[m * f:] = 123.0
        dhbuf[2 * m * f:] = 123.0
    y, dh = ybuf[:m * f].view(m, f), dhbuf[:2 * m * f].view(m, 2 * f)
    hip.geglu(hd, y)
    hip.geglu_grad(hd, dyd, dh)
    hip.synchronize()
    assert bool((ybuf[m * f:] == 123.0).all()) and bool((dhbuf[2 * m * f:] == 123.0).all()), "wrote past an output"
    assert torch.equal(y, y1) and torch.equal(dh, dh1)
    hip.graph_begin()
    hip.geglu(hd, y)
    hip.geglu_grad(hd, dyd, dh)
    g = hip.graph_end()
    try:
        for _ in range(2):
            hip.zero_(ybuf[:m * f])
            hip.zero_(dhbuf[:2 * m * f])
            hip.graph_launch(g)
            hip.synchronize()
            assert torch.equal(y, y1) and torch.equal(dh, dh1)
    finally:
        hip.graph_destroy(g)


@pytest.mark.parametrize("bad", ["F=12", "mixed types"])
def test_geglu_contract(hip, bad):
    f = 12 if bad == "F=12" else 64
    h, dy = hip.zeros((4, 2 * f), F16), hip.zeros((4, f), BF16 if bad == "mixed types" else F16)
    y, dh = filled(hip, (4, f), NAN, dy.dtype), filled(hip, (4, 2 * f), NAN, F16)
    with pytest.raises(ValueError):
        hip.geglu(h, y)
    with pytest.raises(ValueError):
        hip.geglu_grad(h, dy, dh)
    hip.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(dh).all()), "a refused call launched something"


# ---- operators ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [N.GN_CASES[0], N.GN_CASES[2]])
def test_group_norm_operator(hip, case):
    b, c1, c2, h, w, silu, eps = case
    x, dy, gamma, beta, ref = N.gn_case(*case)
    x1 = x[..., :c1].contiguous().cuda().requires_grad_(True)
    x2 = x[..., c1:].contiguous().cuda().requires_grad_(True) if c2 else None
    gd, bd = gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
    y = grad_ops.group_norm(hip, x1, gd, bd, eps=eps, silu=bool(silu), x2=x2)
    assert y.dtype == F16 and y.shape == x.shape
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    N.close16(y, N.gn_nhwc(x.double(), gamma.double(), beta.double(), eps, bool(silu)), "group_norm y")
    assert x1.grad.dtype == F16 and gd.grad.dtype == bd.grad.dtype == F32
    dx = x1.grad if x2 is None else torch.cat([x1.grad, x2.grad], -1)
    ref.check(dx, gd.grad, bd.grad, "group_norm operator")
    g2, b2 = gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
    xdet = x1.detach()
    grad_ops.group_norm(hip, xdet, g2, b2, eps=eps, silu=bool(silu), x2=None if x2 is None else x2.detach()).backward(dy.cuda())
    torch.cuda.synchronize()
    assert xdet.grad is None and torch.equal(g2.grad, gd.grad) and torch.equal(b2.grad, bd.grad)


def test_layer_norm_operator(hip):
    x, dy, gamma, beta, ref = N.ln_case(130, 320)
    xd, gd, bd = x.cuda().requires_grad_(True), gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
    y = grad_ops.layer_norm(hip, xd, gd, bd)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    N.close16(y, torch.nn.functional.layer_norm(x.double(), (320,), gamma.double(), beta.double(), 1e-5), "layer_norm y")
    assert xd.grad.dtype == F16 and gd.grad.dtype == bd.grad.dtype == F32
    ref.check(xd.grad, gd.grad, bd.grad, "layer_norm operator")
    g2, b2 = gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
    xdet = xd.detach()
    grad_ops.layer_norm(hip, xdet, g2, b2).backward(dy.cuda())
    torch.cuda.synchronize()
    assert xdet.grad is None and torch.equal(g2.grad, gd.grad) and torch.equal(b2.grad, bd.grad)
    x3 = x.cuda().requires_grad_(True)
    grad_ops.layer_norm(hip, x3, gamma.cuda(), beta.cuda()).backward(dy.cuda())
    torch.cuda.synchronize()
    assert torch.equal(x3.grad, xd.grad)


def test_geglu_operator(hip):
    h, dy, (y_ref, dh_ref) = N.geglu_case(130, 1280)
    hd = h.cuda().requires_grad_(True)
    y = grad_ops.geglu(hip, hd)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    assert y.dtype == F16 and hd.grad.dtype == F16
    N.close16(y, y_ref, "geglu operator y")
    N.close16(hd.grad, dh_ref, "geglu operator dh")
    with pytest.raises(ValueError):
        grad_ops.geglu(hip, torch.zeros(4, 24, dtype=F16, device="cuda"))


# ---- two composed blocks -----------------------------------------------------------------------------------------------
def _leaves(params, dtype=None):
    return {k: (v.double() if dtype is None else v.cuda()).requires_grad_(True) for k, v in params.items()}


def _check_block(what, got, ref):
    worst = 0.0
    for name in ref:
        err = N.rel_l2(got[name], ref[name])
        worst = max(worst, err)
        print(f"{what} d{name}: relative L2 error {err:.3e}")
    for name in ref:
        assert N.rel_l2(got[name], ref[name]) <= BLOCK_BOUND, (what, name, N.rel_l2(got[name], ref[name]))
    print(f"{what}: worst relative L2 error {worst:.3e} (bound {BLOCK_BOUND:.0e})")


def test_resnet_block_gradients(hip):
    """norm -> SiLU -> conv3x3 -> + time row -> norm -> SiLU -> conv3x3 -> + 1x1 shortcut, B = 2, 8x8, 64 -> 128: every
    gradient against float64 autograd of the same block with the weights rounded to fp16.
    Measured on MI355X: worst tensor 4.6e-4 (db1), dx 3.3e-4, dtemb 3.9e-4, dw1 / dw2 4.1e-4 / 4.3e-4."""
    b, hw, ci, co = 2, 8, 64, 128
    r = N.R.rnd
    x, dy = (1.5 * r((b, hw, hw, ci), 41, dtype=F32) + 0.3).half(), r((b, hw, hw, co), 42)
    temb = r((b, co), 43, 0.5, F32)
    p = dict(g1=1 + 0.2 * r((ci,), 44, dtype=F32), b1=r((ci,), 45, 0.2, F32), w1=r((co, 9 * ci), 46, (9 * ci) ** -0.5, F32),
             c1=r((co,), 47, 0.1, F32), g2=1 + 0.2 * r((co,), 48, dtype=F32), b2=r((co,), 49, 0.2, F32),
             w2=r((co, 9 * co), 50, (9 * co) ** -0.5, F32), c2=r((co,), 51, 0.1, F32),
             ws=r((co, ci), 52, ci ** -0.5, F32), cs=r((co,), 53, 0.1, F32))
    # float64, weights rounded to the 16-bit type the kernels multiply with
    q = _leaves({k: (v.half() if k.startswith("w") else v) for k, v in p.items()})
    x64, t64 = x.double().requires_grad_(True), temb.double().requires_grad_(True)
    N.resnet_block64(x64, t64, q).backward(dy.double())
    ref = dict({k: v.grad for k, v in q.items()}, x=x64.grad, temb=t64.grad)
    d = _leaves(p, F32)
    xd, td = x.cuda().requires_grad_(True), temb.cuda().requires_grad_(True)
    hdn = grad_ops.group_norm(hip, xd, d["g1"], d["b1"], silu=True)
    hdn = grad_ops.conv3x3(hip, hdn, d["w1"], d["c1"])
    hdn = (hdn.float() + td[:, None, None, :]).half()
    hdn = grad_ops.group_norm(hip, hdn, d["g2"], d["b2"], silu=True)
    hdn = grad_ops.conv3x3(hip, hdn, d["w2"], d["c2"])
    out = hdn + grad_ops.linear(hip, xd, d["ws"], d["cs"])
    out.backward(dy.cuda())
    torch.cuda.synchronize()
    _check_block("resnet block", dict({k: v.grad for k, v in d.items()}, x=xd.grad, temb=td.grad), ref)


def test_feed_forward_gradients(hip):
    """LayerNorm -> Linear -> GEGLU -> Linear -> + x, M = 130, C = 320, F = 1280.  Measured on MI355X: worst tensor 5.0e-4 (dg), dx 3.8e-4, dw1 / dw2 4.9e-4 / 4.8e-4
    (DESIGN.md 7.1)."""
    m, c, f = 130, 320, 1280
    r = N.R.rnd
    x, dy = (1.5 * r((m, c), 61, dtype=F32) + 0.3).half(), r((m, c), 62)
    p = dict(g=1 + 0.2 * r((c,), 63, dtype=F32), b=r((c,), 64, 0.2, F32), w1=r((2 * f, c), 65, c ** -0.5, F32),
             c1=r((2 * f,), 66, 0.1, F32), w2=r((c, f), 67, f ** -0.5, F32), c2=r((c,), 68, 0.1, F32))
    q = _leaves({k: (v.half() if k.startswith("w") else v) for k, v in p.items()})
    x64 = x.double().requires_grad_(True)
    N.feed_forward64(x64, q).backward(dy.double())
    ref = dict({k: v.grad for k, v in q.items()}, x=x64.grad)
    d = _leaves(p, F32)
    xd = x.cuda().requires_grad_(True)
    hdn = grad_ops.layer_norm(hip, xd, d["g"], d["b"])
    hdn = grad_ops.geglu(hip, grad_ops.linear(hip, hdn, d["w1"], d["c1"]))
    out = grad_ops.linear(hip, hdn, d["w2"], d["c2"]) + xd
    out.backward(dy.cuda())
    torch.cuda.synchronize()
    _check_block("feed-forward", dict({k: v.grad for k, v in d.items()}, x=xd.grad), ref)
