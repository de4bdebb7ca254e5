"""-m gpu: the backward of attention on the HIP kernels (csrc/attn_grad.hip) through ``HipBackend.attn_grad`` and the
operators ``grad_ops.self_attention`` / ``attention`` / ``tri_cross_attention``, against float64 autograd on the same
16-bit operands (tests/attn_grad_reference.py).  Bound per tensor: rel_l2(kernel, exact) <= max(2 E_model, ULP[dtype]),
E_model the error of the CPU model of the kernels' rounding points - never a number taken from a kernel.  Outputs and
scratch are NaN-filled before every call.  The shapes are the smallest that reach each branch (the case table of the
helper).  The composed BasicTransformerBlock is checked per tensor in relative L2 against float64 autograd: bound 4e-3."""
import math

import pytest
import torch
import torch.nn.functional as F

from progressive_stable_diffusion_amd import grad_ops
from progressive_stable_diffusion_amd import lib as L
from tests import attention_cases as A
from tests import attn_grad_reference as R
from tests import norm_grad_reference as N

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
NAN = float("nan")
BLOCK_BOUND = 4e-3
CASE_DTYPES = [(c.name, F16) for c in R.CASES] + [(n, BF16) for n in R.BF16_CASES]


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(torch.device("cuda:0"))


def filled(hip, shape, value, dtype=F32):
    t = hip.empty(shape, dtype)
    with hip.ctx():
        t.fill_(value)
    return t


class Call:
    """Device operands of one ``attn_grad`` call of a case, outputs and scratch NaN-filled.  ``pad`` > 0: every output
    row is ``pad`` columns wider than heads * d and ``pad`` rows follow the last token, all holding a sentinel."""
    SENTINEL = 123.0

    def __init__(self, hip, name, dtype, pad=0):
        c = R.BY_NAME[name]
        self.hip, self.case, self.cc, self.pad = hip, c, c.heads * c.d, pad
        q, k, v, do = R.inputs(name, dtype)
        cc = self.cc
        if c.layout == "self":       # q | k | v and dq | dk | dv as column blocks of one [B,N,3C] buffer each
            assert pad == 0
            qkv = hip.to_device(torch.cat([q, k, v], -1))
            self.q, self.k, self.v = qkv[..., :cc], qkv[..., cc:2 * cc], qkv[..., 2 * cc:]
            self.bufs = [filled(hip, qkv.shape, NAN, dtype)]
            self.dq, self.dk, self.dv = (self.bufs[0][..., i * cc:(i + 1) * cc] for i in range(3))
        else:
            self.q, self.k, self.v = hip.to_device(q), hip.to_device(k), hip.to_device(v)
            self.bufs = [filled(hip, (c.b * n + pad, cc + pad), NAN, dtype) for n in (c.nq, c.nk, c.nk)]
            with hip.ctx():
                for buf, n in zip(self.bufs, (c.nq, c.nk, c.nk)):
                    if pad:
                        buf[:, cc:] = self.SENTINEL
                        buf[c.b * n:] = self.SENTINEL
            self.dq, self.dk, self.dv = (buf[:c.b * n, :cc].view(c.b, n, cc) if not pad else
                                         buf[:c.b * n].view(c.b, n, cc + pad)[..., :cc]
                                         for buf, n in zip(self.bufs, (c.nq, c.nk, c.nk)))
        self.dout = hip.to_device(do)
        self.scale_dev = None if c.do_scale_dev is None else hip.to_device(torch.tensor([c.do_scale_dev], dtype=F32))
        self.ws = filled(hip, (hip.attn_grad_ws_numel(c.b, c.heads, c.nq),), NAN)

    def launch(self, dq=True, dk=True, dv=True):
        self.hip.attn_grad(self.q, self.k, self.v, self.dout, dq=self.dq if dq else None, dk=self.dk if dk else None,
                           dv=self.dv if dv else None, ws=self.ws, heads=self.case.heads, do_scale=self.case.do_scale,
                           do_scale_dev=self.scale_dev)

    def run(self, **kw):
        self.launch(**kw)
        self.hip.synchronize()
        return self

    def sentinels_intact(self):
        c, cc = self.case, self.cc
        return all(bool((buf[:, cc:] == self.SENTINEL).all()) and bool((buf[c.b * n:] == self.SENTINEL).all())
                   for buf, n in zip(self.bufs, (c.nq, c.nk, c.nk)))


def check_case(call, name, dtype, what):
    ref = R.reference(name, dtype)
    errs = [R.rel_l2(got, ex) for got, ex in zip((call.dq, call.dk, call.dv), ref.exact)]
    for tname, err, e_model, bound in zip(("dq", "dk", "dv"), errs, ref.e_model, ref.bound):
        print(f"{what} [{name}, {dtype}] {tname}: rel L2 {err:.3e}  (E_model {e_model:.3e}, bound {bound:.3e})")
    for tname, got, err, bound in zip(("dq", "dk", "dv"), (call.dq, call.dk, call.dv), errs, ref.bound):
        assert bool(torch.isfinite(got.float()).all()), (name, tname, "non-finite values")
        assert err <= bound, (name, str(dtype), tname, err, bound)


# ---- the kernels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", CASE_DTYPES)
def test_attn_grad(hip, name, dtype):
    call = Call(hip, name, dtype).run()
    assert call.dq.dtype == dtype
    check_case(call, name, dtype, "attn_grad")


def test_attn_grad_outputs_may_be_left_out(hip):
    """dq only, then dk + dv only: what is present has the bits of the full call, what is absent is not written."""
    name = "tails both sides"
    full = Call(hip, name, F16).run()
    a = Call(hip, name, F16).run(dk=False, dv=False)
    assert torch.equal(a.dq, full.dq) and bool(torch.isnan(a.dk).all()) and bool(torch.isnan(a.dv).all())
    b = Call(hip, name, F16).run(dq=False)
    assert torch.equal(b.dk, full.dk) and torch.equal(b.dv, full.dv) and bool(torch.isnan(b.dq).all())
    c = Call(hip, name, F16).run(dq=False, dk=False)
    assert torch.equal(c.dv, full.dv) and bool(torch.isnan(c.dk).all())


def test_attn_grad_stays_inside_repeats_and_captures(hip):
    """Sentinel columns beyond heads * d (ld larger than needed) and sentinel rows after the last token survive; a second
    call agrees bit for bit; a captured call launched twice equals the eager result bit for bit."""
    name = "tails both sides"
    first = Call(hip, name, F16).run()
    call = Call(hip, name, F16, pad=24).run()
    assert call.dq.stride(1) == call.cc + 24
    assert call.sentinels_intact(), "wrote outside the heads * d columns of the output rows"
    assert torch.equal(call.dq, first.dq) and torch.equal(call.dk, first.dk) and torch.equal(call.dv, first.dv)
    check_case(call, name, F16, "attn_grad into padded rows")
    call.run()
    assert call.sentinels_intact()
    assert torch.equal(call.dq, first.dq) and torch.equal(call.dk, first.dk) and torch.equal(call.dv, first.dv)
    cap = Call(hip, name, F16, pad=24)
    hip.synchronize()
    hip.graph_begin()
    cap.launch()
    g = hip.graph_end()
    try:
        for _ in range(2):
            with hip.ctx():
                cap.dq.zero_()
                cap.dk.zero_()
                cap.dv.zero_()
            hip.graph_launch(g)
            hip.synchronize()
            assert torch.equal(cap.dq, first.dq) and torch.equal(cap.dk, first.dk) and torch.equal(cap.dv, first.dv)
            assert cap.sentinels_intact()
    finally:
        hip.graph_destroy(g)


@pytest.mark.parametrize("bad", ["d=64", "Nq=72", "ld_q=324", "mixed types", "no outputs"])
def test_attn_grad_contract(hip, bad):
    heads, d = 2, (64 if bad == "d=64" else 40)
    cc = heads * d
    nq, nk = (72 if bad == "Nq=72" else 64), 64
    q = hip.zeros((2, nq, 324), F16)[..., :cc] if bad == "ld_q=324" else hip.zeros((2, nq, cc), F16)
    k, v = hip.zeros((2, nk, cc), F16), hip.zeros((2, nk, cc), F16)
    dout = hip.zeros((2, nq, cc), BF16 if bad == "mixed types" else F16)
    dq, dk, dv = filled(hip, (2, nq, cc), NAN, F16), filled(hip, (2, nk, cc), NAN, F16), filled(hip, (2, nk, cc), NAN, F16)
    ws = filled(hip, (2 * heads * nq * 2,), NAN)
    outs = {} if bad == "no outputs" else dict(dq=dq, dk=dk, dv=dv)
    with pytest.raises(ValueError):
        hip.attn_grad(q, k, v, dout, ws=ws, heads=heads, **outs)
    hip.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (dq, dk, dv, ws)), "a refused call launched something"


# ---- operators ---------------------------------------------------------------------------------------------------------
def _check_against(what, got, ref, bound):
    err = R.rel_l2(got, ref)
    print(f"{what}: rel L2 {err:.3e} (bound {bound:.3e})")
    assert bool(torch.isfinite(got.float()).all()) and err <= bound, (what, err, bound)


def test_self_attention_operator(hip):
    name = "self layout"
    c = R.BY_NAME[name]
    q, k, v, do = R.inputs(name, F16)
    ref = R.reference(name, F16)
    qkv = torch.cat([q, k, v], -1).cuda().requires_grad_(True)
    out = grad_ops.self_attention(hip, qkv, c.heads)
    out.backward(do.cuda())
    torch.cuda.synchronize()
    exact_out, _ = A.references(q, k, v, c.heads)
    ok, msg = A.within(out, exact_out, F16)
    assert ok, msg
    assert qkv.grad.dtype == F16 and qkv.grad.shape == qkv.shape
    cc = c.heads * c.d
    for i, tname in enumerate(("dq", "dk", "dv")):
        _check_against(f"self_attention {tname}", qkv.grad[..., i * cc:(i + 1) * cc], ref.exact[i], ref.bound[i])
    with pytest.raises(ValueError):
        grad_ops.self_attention(hip, qkv.detach().float(), c.heads)


def test_attention_operator(hip):
    """Separate Nq / Nk ("pathway shape" operands, scale 1); ``needs_input_grad`` selects the outputs."""
    name = "pathway shape"
    c = R.BY_NAME[name]
    q, k, v, do = R.inputs(name, F16)
    ex = R.exact(q, k, v, do, c.heads)
    mo = R.model(q, k, v, do, c.heads)
    bounds = [max(2 * R.rel_l2(m, e), A.ULP[F16]) for m, e in zip(mo, ex)]
    qd, kd, vd = (t.cuda().requires_grad_(True) for t in (q, k, v))
    out = grad_ops.attention(hip, qd, kd, vd, c.heads)
    out.backward(do.cuda())
    torch.cuda.synchronize()
    ok, msg = A.within(out, A.references(q, k, v, c.heads)[0], F16)
    assert ok, msg
    for tname, got, e, bound in zip(("dq", "dk", "dv"), (qd.grad, kd.grad, vd.grad), ex, bounds):
        _check_against(f"attention {tname}", got, e, bound)
    q2, v2 = q.cuda().requires_grad_(True), v.cuda().requires_grad_(True)
    k2 = k.cuda()
    grad_ops.attention(hip, q2, k2, v2, c.heads).backward(do.cuda())
    torch.cuda.synchronize()
    assert k2.grad is None and torch.equal(q2.grad, qd.grad) and torch.equal(v2.grad, vd.grad)


@pytest.mark.parametrize("mode,lam", [(L.XATTN_SPLIT, 0.0), (L.XATTN_SPLIT, 0.3), (L.XATTN_BASELINE, 0.0)])
def test_tri_cross_attention_operator(hip, mode, lam):
    """B = 2, N = 128, 8 heads of 40 ("pathway shape").  Bounds from the pathway bound Bp = max(2 E_model, ULP): the
    slices of dkv are disjoint, each within Bp of its own norm, so dkv is within Bp; dq is the rounded fp32 sum of the
    pathways' dq, each within Bp of ITS norm: Bp * sum_p |dq_p| / |dq| plus half an ulp for the final rounding."""
    c = R.BY_NAME["pathway shape"]
    cc = c.heads * c.d
    gen = torch.Generator().manual_seed(91)
    q = (0.5 * torch.randn(c.b, c.nq, cc, generator=gen)).half()
    kv = (0.5 * torch.randn(c.b, 48 if mode == L.XATTN_SPLIT else 32, (4 if mode == L.XATTN_SPLIT else 2) * cc,
                            generator=gen)).half()
    dy = torch.randn(c.b, c.nq, cc, generator=gen).half()
    gates = torch.tensor([0.8, 0.35], dtype=F32)
    bp = max(R.reference("pathway shape", F16).bound)
    dq_ref, dkv_ref = R.tri_exact(q, kv, dy, gates, lam, mode, c.heads)
    parts = [R.exact(q, kv[:, t0:t0 + nt, kc:kc + cc], kv[:, t0:t0 + nt, kc + cc:kc + 2 * cc], dy, c.heads, s)[0]
             for t0, nt, kc, s in R.tri_paths(cc, gates, lam, mode)]
    dq_bound = bp * sum(float(p.norm()) for p in parts) / float(dq_ref.norm()) + 0.5 * A.ULP[F16]
    qd, kvd = q.cuda().requires_grad_(True), kv.cuda().requires_grad_(True)
    out = grad_ops.tri_cross_attention(hip, qd, kvd, gates.cuda() if mode == L.XATTN_SPLIT else None, lam, c.heads, mode)
    out.backward(dy.cuda())
    torch.cuda.synchronize()
    ok, msg = A.within(out, A.xattn_reference(q, kv, gates, lam, mode, c.heads), F16)
    assert ok, msg
    assert qd.grad.dtype == kvd.grad.dtype == F16 and kvd.grad.shape == kv.shape
    _check_against(f"tri_cross_attention mode {mode} lambda {lam} dq", qd.grad, dq_ref, dq_bound)
    _check_against(f"tri_cross_attention mode {mode} lambda {lam} dkv", kvd.grad, dkv_ref, bp)
    if mode == L.XATTN_SPLIT:
        g = kvd.grad
        assert not g[:, 16:32, 2 * cc:].any() and not g[:, :16, :2 * cc].any() and not g[:, 32:, :2 * cc].any()
        if lam == 0.0:
            assert not g[:, 32:48].any(), "lambda = 0: the delta tokens get no gradient"
        else:
            assert bool(g[:, 32:48, 2 * cc:].any())


# ---- a composed BasicTransformerBlock ----------------------------------------------------------------------------------
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


def _transformer_block64(x, cond, p, gates, lam, heads):
    c = x.shape[-1]
    d = c // heads

    def split(t):
        return t.reshape(t.shape[0], t.shape[1], heads, d).transpose(1, 2)

    h = F.layer_norm(x, (c,), p["g1"], p["b1"], 1e-5) @ p["wqkv"].t()
    q, k, v = h.chunk(3, dim=-1)
    a = torch.softmax(split(q) @ split(k).transpose(-1, -2) / math.sqrt(d), dim=-1) @ split(v)
    x1 = a.transpose(1, 2).reshape(x.shape) @ p["wo1"].t() + p["co1"] + x
    q = F.layer_norm(x1, (c,), p["g2"], p["b2"], 1e-5) @ p["wq"].t()
    kv = cond @ p["wkv"].t()
    x2 = A.xattn_reference(q, kv, gates, lam, 0, heads) @ p["wo2"].t() + p["co2"] + x1
    return N.feed_forward64(x2, dict(g=p["g3"], b=p["b3"], w1=p["w1"], c1=p["c1"], w2=p["w2"], c2=p["c2"]))


def test_transformer_block_gradients(hip):
    """LayerNorm -> qkv Linear -> self_attention -> out Linear -> + x;  LayerNorm -> q Linear -> tri_cross_attention
    against kv = Linear(cond tokens [B,48,768] -> 4C) (gates 0.8 / 0.35, lambda 0.3) -> out Linear -> + x;  LayerNorm ->
    Linear -> GEGLU -> Linear -> + x.  B = 2, N = 144, C = 320, 8 heads: every gradient (x, cond, weights, biases, gamma /
    beta) against float64 autograd of the same block with the weights rounded to fp16, relative L2 per tensor.
    Measured on MI355X: worst tensor 9.2e-4 (dg1); dx 5.5e-4, dcond 7.7e-4; dwqkv 7.7e-4, dwo1 6.7e-4, dwq 8.2e-4, dwkv 7.4e-4,
    dwo2 6.7e-4, dw1 7.0e-4, dw2 6.8e-4; dg2 / dg3 8.2e-4 / 6.8e-4; db1 / db2 / db3 5.8e-4 / 6.9e-4 / 6.6e-4; dco1 / dco2 / dc1
    5.3e-4 / 4.4e-4 / 5.9e-4; dc2 2e-8 (a column sum of dy)."""
    b, n, c, heads, f, t, cd = 2, 144, 320, 8, 1280, 48, 768
    r = N.R.rnd
    x, dy = (1.5 * r((b, n, c), 71, dtype=F32) + 0.3).half(), r((b, n, c), 72)
    cond = r((b, t, cd), 73)
    gates, lam = torch.tensor([0.8, 0.35], dtype=F32), 0.3
    p = dict(g1=1 + 0.2 * r((c,), 74, dtype=F32), b1=r((c,), 75, 0.2, F32), wqkv=r((3 * c, c), 76, c ** -0.5, F32),
             wo1=r((c, c), 77, c ** -0.5, F32), co1=r((c,), 78, 0.1, F32),
             g2=1 + 0.2 * r((c,), 79, dtype=F32), b2=r((c,), 80, 0.2, F32), wq=r((c, c), 81, c ** -0.5, F32),
             wkv=r((4 * c, cd), 82, cd ** -0.5, F32), wo2=r((c, c), 83, c ** -0.5, F32), co2=r((c,), 84, 0.1, F32),
             g3=1 + 0.2 * r((c,), 85, dtype=F32), b3=r((c,), 86, 0.2, F32), w1=r((2 * f, c), 87, c ** -0.5, F32),
             c1=r((2 * f,), 88, 0.1, F32), w2=r((c, f), 89, f ** -0.5, F32), c2=r((c,), 90, 0.1, F32))
    q64 = _leaves({k: (v.half() if k.startswith("w") else v) for k, v in p.items()})
    x64, cond64 = x.double().requires_grad_(True), cond.double().requires_grad_(True)
    _transformer_block64(x64, cond64, q64, gates, lam, heads).backward(dy.double())
    ref = dict({k: v.grad for k, v in q64.items()}, x=x64.grad, cond=cond64.grad)
    d = _leaves(p, F32)
    xd, condd, gd = x.cuda().requires_grad_(True), cond.cuda().requires_grad_(True), gates.cuda()
    h = grad_ops.linear(hip, grad_ops.layer_norm(hip, xd, d["g1"], d["b1"]), d["wqkv"])
    x1 = grad_ops.linear(hip, grad_ops.self_attention(hip, h, heads), d["wo1"], d["co1"]) + xd
    q = grad_ops.linear(hip, grad_ops.layer_norm(hip, x1, d["g2"], d["b2"]), d["wq"])
    kv = grad_ops.linear(hip, condd, d["wkv"])
    a = grad_ops.tri_cross_attention(hip, q, kv, gd, lam, heads)
    x2 = grad_ops.linear(hip, a, d["wo2"], d["co2"]) + x1
    h = grad_ops.geglu(hip, grad_ops.linear(hip, grad_ops.layer_norm(hip, x2, d["g3"], d["b3"]), d["w1"], d["c1"]))
    out = grad_ops.linear(hip, h, d["w2"], d["c2"]) + x2
    out.backward(dy.cuda())
    torch.cuda.synchronize()
    _check_block("transformer block", dict({k: v.grad for k, v in d.items()}, x=xd.grad, cond=condd.grad), ref)
