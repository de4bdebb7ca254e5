"""-m gpu: the training kernels of the conditioning front-end (csrc/cond_grad.hip) through ``HipBackend.gelu`` /
``gelu_grad`` / ``purifier_gate_tail`` / ``purifier_gate_tail_grad``, the operators ``grad_ops.gelu`` /
``purifier_gate_tail`` and the three blocks of ``conditioning_grad``, against the float64 references of
tests/cond_grad_reference.py (where the bounds are derived): gelu within one spacing of the storage type of
the model with dadd_gelu's fp32 rounding of erf in it, gelu_grad within
2 ULP |ref| + ULP 2^-4, the tail's fp32 output within 2e-5, dimg / ddis / dz 3e-3 + 2e-3 |ref| (bf16: 2e-2 + 1.6e-2 |ref|),
dgamma / dbeta (M + 16) 2^-24 E, the blocks 4e-3 relative L2 per tensor against float64 autograd of the oracle on
fp16-rounded weight matrices.  Outputs and scratch are NaN-filled before every call and followed by sentinels.

Measured on MI355X: see DESIGN.md 7.1 (worst share of each bound)."""
import itertools

import pytest
import torch

from progressive_stable_diffusion_amd import conditioning_grad as CG
from progressive_stable_diffusion_amd import grad_ops
from progressive_stable_diffusion_amd import optim as O
from tests import cond_grad_reference as K

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
NAN = float("nan")
SENT16, SENT32, PAD = 123.0, 12345.0, 64
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(DEV)


def filled(hip, shape, value, dtype=F32):
    t = hip.empty(shape, dtype)
    with hip.ctx():
        t.fill_(value)
    return t


def guarded(hip, shape, dtype):
    """A NaN-filled tensor of ``shape`` at the front of a buffer whose last PAD elements hold a sentinel -> (view, buffer)."""
    n = 1
    for s in shape:
        n *= s
    buf = filled(hip, (n + PAD,), NAN, dtype)
    with hip.ctx():
        buf[n:] = SENT32 if dtype == F32 else SENT16
    return buf[:n].view(shape), buf


def intact(buf, dtype):
    return bool((buf[-PAD:] == (SENT32 if dtype == F32 else SENT16)).all())


def share(got, ref, bound):
    """Worst |got - ref| / bound; inf for a non-finite value."""
    got, ref = got.detach().double().cpu(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref.reshape(got.shape)).abs() / bound.reshape(got.shape)).max())


# ---- GELU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,f,dtype", K.GELU_CASES)
def test_gelu_forward_and_backward(hip, m, f, dtype):
    x, dy = K.gelu_case(m, f, dtype)
    xd, dyd = hip.to_device(x), hip.to_device(dy)
    (y, ybuf), (dx, dxbuf) = guarded(hip, (m, f), dtype), guarded(hip, (m, f), dtype)
    hip.gelu(xd, y)
    hip.gelu_grad(xd, dyd, dx)
    hip.synchronize()
    assert intact(ybuf, dtype) and intact(dxbuf, dtype), "wrote past an output"
    model = K.gelu_model(x)
    s_y = share(y, model.to(dtype), K.gelu_bound(model, dtype))
    ref = K.gelu_grad_model(x, dy)
    s_dx = share(dx, ref, K.gelu_grad_bound(ref, dtype))
    print(f"gelu {m}x{f} {dtype}: y {s_y:.3f} spacings from the rounded model, dx {s_dx:.3f} of its bound")
    assert s_y <= 1.0 and s_dx <= 1.0, (s_y, s_dx)


def test_gelu_repeats_replays_and_refuses(hip):
    m, f, dtype = K.GELU_CASES[1]
    x, dy = K.gelu_case(m, f, dtype)
    xd, dyd = hip.to_device(x), hip.to_device(dy)
    y1, dx1, y2, dx2 = (filled(hip, (m, f), NAN, dtype) for _ in range(4))
    hip.gelu(xd, y1)
    hip.gelu_grad(xd, dyd, dx1)
    hip.synchronize()
    hip.graph_begin()
    hip.gelu(xd, y2)
    hip.gelu_grad(xd, dyd, dx2)
    g = hip.graph_end()
    try:
        for _ in range(2):
            hip.zero_(y2)
            hip.zero_(dx2)
            hip.graph_launch(g)
            hip.synchronize()
            assert torch.equal(y2, y1) and torch.equal(dx2, dx1)
    finally:
        hip.graph_destroy(g)
    for bad in ("F=12", "mixed types"):
        fb = 12 if bad == "F=12" else 64
        xb, dyb = hip.zeros((4, fb), F16), hip.zeros((4, fb), BF16 if bad == "mixed types" else F16)
        yb, dxb = filled(hip, (4, fb), NAN, dyb.dtype), filled(hip, (4, fb), NAN, F16)
        with pytest.raises(ValueError):
            hip.gelu(xb, yb)
        with pytest.raises(ValueError):
            hip.gelu_grad(xb, dyb, dxb)
        hip.synchronize()
        assert bool(torch.isnan(yb).all()) and bool(torch.isnan(dxb).all()), "a refused call launched something"


def test_gelu_operator(hip):
    m, f, dtype = K.GELU_CASES[1]
    x, dy = K.gelu_case(m, f, dtype)
    xd = x.cuda().requires_grad_(True)
    y = grad_ops.gelu(hip, xd)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    model, ref = K.gelu_model(x), K.gelu_grad_model(x, dy)
    assert y.dtype == dtype and xd.grad.dtype == dtype
    assert share(y, model.to(dtype), K.gelu_bound(model, dtype)) <= 1.0
    assert share(xd.grad, ref, K.gelu_grad_bound(ref, dtype)) <= 1.0


# ---- the purifier's tail -----------------------------------------------------------------------------------------------------
class TailCall:
    """Device operands of one gate-tail forward and backward; outputs NaN-filled with sentinels behind them."""
    NAMES = ("dimg", "ddis", "dz")

    def __init__(self, hip, m, c, dtype=F16, shifted=False, want=("dimg", "ddis", "dz", "params")):
        self.hip, self.m, self.c, self.dtype = hip, m, c, dtype
        self.host = K.tail_case(m, c, dtype, shifted)
        self.img, self.dis, self.z, self.dout, self.gamma, self.beta = (hip.to_device(t) for t in self.host)
        self.out, self.outbuf = guarded(hip, (m, c), F32)
        self.d, self.bufs = {}, {}
        for name in self.NAMES:
            if name in want:
                self.d[name], self.bufs[name] = guarded(hip, (m, c), dtype)
        self.dgamma = self.dbeta = self.ws = None
        if "params" in want:
            (self.dgamma, self.bufs["dgamma"]), (self.dbeta, self.bufs["dbeta"]) = guarded(hip, (c,), F32), guarded(hip, (c,), F32)
            self.ws = filled(hip, (hip.purifier_gate_tail_grad_ws_numel(m, c),), NAN)

    def forward(self):
        self.hip.purifier_gate_tail(self.img, self.dis, self.z, self.gamma, self.beta, self.out)

    def backward(self):
        self.hip.purifier_gate_tail_grad(self.img, self.dis, self.z, self.dout, self.gamma, dimg=self.d.get("dimg"),
                                         ddis=self.d.get("ddis"), dz=self.d.get("dz"), dgamma=self.dgamma, dbeta=self.dbeta,
                                         ws=self.ws)

    def run(self):
        self.forward()
        self.backward()
        self.hip.synchronize()
        return self

    def intact(self):
        return intact(self.outbuf, F32) and all(intact(b, b.dtype) for b in self.bufs.values())

    def tensors(self):
        return dict(self.d, **({} if self.dgamma is None else dict(dgamma=self.dgamma, dbeta=self.dbeta)))


def check_tail(call, what):
    img, dis, z, dout, gamma, beta = call.host
    ref_out = K.gate_tail_model(img, dis, z, gamma, beta)
    r = K.gate_tail_grad_model(img, dis, z, dout, gamma)
    atol, rtol = K.TOL16[call.dtype]
    shares = {"out": share(call.out, ref_out, torch.full_like(ref_out, K.PURIFIER_ATOL))}
    for name in TailCall.NAMES:
        shares[name] = share(call.d[name], r[name], atol + rtol * r[name].abs())
    shares["dgamma"] = share(call.dgamma, r["dgamma"], K.sum_bound(r["m"], r["e_gamma"]))
    shares["dbeta"] = share(call.dbeta, r["dbeta"], K.sum_bound(r["m"], r["e_beta"]))
    print(f"{what}: share of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    assert all(v <= 1.0 for v in shares.values()), (what, shares)
    assert call.intact(), f"{what}: wrote past an output"


@pytest.mark.parametrize("m,c", K.TAIL_CASES)
def test_purifier_gate_tail(hip, m, c):
    check_tail(TailCall(hip, m, c).run(), f"purifier_gate_tail {m}x{c} f16")


def test_purifier_gate_tail_bf16(hip):
    call = TailCall(hip, 32, 768, BF16).run()
    assert call.d["dimg"].dtype == BF16
    check_tail(call, "purifier_gate_tail 32x768 bf16")


def test_purifier_gate_tail_rows_far_from_zero(hip):
    """Rows at 50 with a spread of 0.1 (rstd about 9): the statistics are formed about the row's first element."""
    check_tail(TailCall(hip, 32, 768, F16, shifted=True).run(), "purifier_gate_tail 32x768 f16, mean 50 spread 0.1")


def test_purifier_gate_tail_outputs_may_be_left_out(hip):
    """Every legal combination of outputs once: what is present has the bits of the full call."""
    m, c = 32, 768
    full = TailCall(hip, m, c).run().tensors()
    every = ("dimg", "ddis", "dz", "params")
    combos = [w for n in range(1, 4) for w in itertools.combinations(every, n)]
    assert len(combos) == 14
    for want in combos:
        part = TailCall(hip, m, c, want=want)
        part.backward()
        hip.synchronize()
        got = part.tensors()
        assert set(got) == {n for n in want if n != "params"} | ({"dgamma", "dbeta"} if "params" in want else set())
        assert all(torch.equal(got[k], full[k]) for k in got), want
        assert all(intact(b, b.dtype) for b in part.bufs.values()), want


def test_purifier_gate_tail_repeats_and_replays_bit_for_bit(hip):
    m, c = 37, 2048
    first = TailCall(hip, m, c).run()
    again = TailCall(hip, m, c).run().run()
    assert torch.equal(again.out, first.out) and all(torch.equal(v, first.tensors()[k]) for k, v in again.tensors().items())
    cap = TailCall(hip, m, c)
    hip.synchronize()
    hip.graph_begin()
    cap.forward()
    cap.backward()
    g = hip.graph_end()
    try:
        for _ in range(2):
            with hip.ctx():
                cap.out.zero_()
                cap.ws.fill_(NAN)
                for t in cap.tensors().values():
                    t.zero_()
            hip.graph_launch(g)
            hip.synchronize()
            assert torch.equal(cap.out, first.out) and cap.intact()
            assert all(torch.equal(v, first.tensors()[k]) for k, v in cap.tensors().items())
    finally:
        hip.graph_destroy(g)


@pytest.mark.parametrize("bad", ["C=12", "C=2056", "mixed types", "no outputs"])
def test_purifier_gate_tail_contract(hip, bad):
    c = 12 if bad == "C=12" else 2056 if bad == "C=2056" else 64
    img, z = hip.zeros((8, c), F16), hip.zeros((8, c), F16)
    dis = hip.zeros((8, c), BF16 if bad == "mixed types" else F16)
    gamma, beta, dout = hip.zeros((c,), F32), hip.zeros((c,), F32), hip.zeros((8, c), F32)
    out = filled(hip, (8, c), NAN)
    outs = dict(dimg=filled(hip, (8, c), NAN, F16), ddis=filled(hip, (8, c), NAN, F16), dz=filled(hip, (8, c), NAN, F16),
                dgamma=filled(hip, (c,), NAN), dbeta=filled(hip, (c,), NAN))
    ws = filled(hip, (1 << 16,), NAN)
    if bad != "no outputs":
        with pytest.raises(ValueError):
            hip.purifier_gate_tail(img, dis, z, gamma, beta, out)
    with pytest.raises(ValueError):
        hip.purifier_gate_tail_grad(img, dis, z, dout, gamma, ws=ws, **({} if bad == "no outputs" else outs))
    hip.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (out, ws, *outs.values())), "a refused call launched something"


def test_purifier_gate_tail_operator(hip):
    m, c = 32, 768
    img, dis, z, dout, gamma, beta = K.tail_case(m, c)
    leaves = [t.cuda().requires_grad_(True) for t in (img, dis, z, gamma, beta)]
    out = grad_ops.purifier_gate_tail(hip, *leaves)
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    assert out.dtype == F32 and [t.grad.dtype for t in leaves] == [F16, F16, F16, F32, F32]
    direct = TailCall(hip, m, c).run()
    assert torch.equal(out.detach(), direct.out)
    for leaf, key in zip(leaves, ("dimg", "ddis", "dz", "dgamma", "dbeta")):
        assert torch.equal(leaf.grad.reshape(-1), direct.tensors()[key].reshape(-1)), key
    # the gate's inputs alone: no parameter gradient is computed, the data gradients keep their bits
    only = [t.cuda().requires_grad_(i < 3) for i, t in enumerate((img, dis, z, gamma, beta))]
    grad_ops.purifier_gate_tail(hip, *only).backward(dout.cuda())
    torch.cuda.synchronize()
    assert only[3].grad is None and all(torch.equal(a.grad, b.grad) for a, b in zip(only[:3], leaves[:3]))


# ---- the blocks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(K.BLOCKS))
def test_block_gradients(hip, kind):
    """B = 2, heads = 2, E = 192 (d = 96); purifier: 16 image tokens against 16 AOE tokens, ff_mult 2; resampler: 257
    context tokens of width 128 through proj_in, 16 latents, depth 2; projection: Linear(128 -> 16 x 64) + LN."""
    params = K.BLOCKS[kind]()
    inputs, dout = K.block_inputs(kind)
    ref = K.oracle_grads(kind, params, inputs, dout)
    got, out = K.run_block(hip, CG, kind, {k: v.cuda() for k, v in params.items()}, {k: v.cuda() for k, v in inputs.items()},
                           dout.cuda())
    torch.cuda.synchronize()
    assert out.dtype == (F32 if kind == "purifier" else F16)
    assert set(ref) == set(params) | set(inputs)
    K.check_block(f"{kind} block", got, ref)


def test_both_blocks_into_an_arena_and_one_fused_step(hip):
    """Masters as views of a ParamArena over the reference's parameter groups: backward through the purifier and the
    resampler accumulates into the arena's flat gradient, then one FusedAdamW step (not skipped) moves every master of
    the two 2 x lr groups."""
    tensors = {**K.resampler_params(), **K.purifier_params()}
    groups = [g for g in O.reference_param_groups(list(tensors), 1e-3, weight_decay=1e-3) if g["params"]]
    assert [g["name"] for g in groups] == ["image_projection", "feature_purifier"] and all(g["lr"] == 2e-3 for g in groups)
    arena = O.arena_from_groups(tensors, groups, device=DEV, working_dtype=F16)
    fused = O.FusedAdamW(hip, arena, groups, max_grad_norm=1.0)
    params = {k: torch.nn.Parameter(torch.empty(t.shape, device=DEV)) for k, t in tensors.items()}
    arena.attach(params)
    (pin, pdo), (rin, rdo) = K.block_inputs("purifier"), K.block_inputs("resampler")
    out_p = CG.feature_purifier(hip, params, pin["image_embeds"].cuda(), pin["source_aoe"].cuda(), K.HEADS)
    out_r = CG.image_projection_plus(hip, params, rin["hidden"].cuda(), K.HEADS)
    ((out_p * pdo.cuda()).sum() + (out_r.float() * rdo.cuda()).sum()).backward()
    torch.cuda.synchronize()
    assert all(float(arena.grad(k).abs().sum()) > 0 for k in tensors), [k for k in tensors if not float(arena.grad(k).abs().sum()) > 0]
    before = {k: arena.param(k).clone() for k in tensors}
    fused.step()
    st = fused.stats()
    assert st["step"] == 1 and not st["found_inf"], st
    stuck = [k for k in tensors if torch.equal(arena.param(k), before[k])]
    assert not stuck and not arena.g.any(), stuck
    assert bool(torch.isfinite(arena.p).all())
