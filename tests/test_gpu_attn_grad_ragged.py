"""-m gpu: the attention backward at d = 96 and at key counts that are no multiple of 16 (csrc/attn_grad.hip: the
Perceiver resampler's 257 CLIP tokens, the purifier's 16 AOE tokens) through ``HipBackend.attn_grad`` and
``grad_ops.attention``, against float64 autograd on the same 16-bit operands.  Bound per tensor, as in
tests/test_gpu_attn_grad.py: rel_l2(kernel, exact) <= max(2 E_model, ULP[dtype]) with E_model from the CPU model
(tests/cond_grad_reference.ragged_reference; tests/test_cond_grad_cpu.py prints the numbers).  With ONE key the exact dq
and dk are zero: there the kernel's values are capped at ULP * max|dout| * max(max|q|, max|k|, max|v|), which catches an
unmasked key or a NaN and measures nothing.

In every case k, v, dk and dv are the ``[:, :nk]`` views of buffers with 7 more rows per sample: the guard rows of k and v
hold NaN (a read of one poisons the result), those of dk and dv a sentinel that must survive; ``ws`` is NaN-filled.

Measured on MI355X (worst tensor per case, share of its bound): see DESIGN.md 7.1."""
import pytest
import torch

from progressive_stable_diffusion_amd import grad_ops
from tests import attention_cases as A
from tests import attn_grad_reference as R
from tests import cond_grad_reference as K

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
NAN = float("nan")
GUARD = 7
SENTINEL = 123.0


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
    """Device operands of one ragged case.  ``wide`` > 0: the rows of k, v, dk, dv (and dq) are ``wide`` columns wider
    than heads * d; the extra columns of the outputs hold the sentinel, those of k and v NaN."""

    def __init__(self, hip, i, dtype, wide=0):
        b, heads, d, nq, nk = K.RAGGED_CASES[i]
        self.hip, self.i, self.dtype, self.heads, self.cc = hip, i, dtype, heads, heads * d
        cc, w = self.cc, heads * d + wide
        q, k, v, do = K.ragged_inputs(i, dtype)
        self.q, self.dout = hip.to_device(q), hip.to_device(do)
        self.kbuf, self.vbuf = filled(hip, (b, nk + GUARD, w), NAN, dtype), filled(hip, (b, nk + GUARD, w), NAN, dtype)
        self.dkbuf, self.dvbuf = (filled(hip, (b, nk + GUARD, w), SENTINEL, dtype) for _ in range(2))
        self.dqbuf = filled(hip, (b, nq, w), SENTINEL, dtype)
        self.k, self.v = self.kbuf[:, :nk, :cc], self.vbuf[:, :nk, :cc]
        self.dk, self.dv, self.dq = self.dkbuf[:, :nk, :cc], self.dvbuf[:, :nk, :cc], self.dqbuf[:, :, :cc]
        with hip.ctx():
            self.k.copy_(hip.to_device(k))
            self.v.copy_(hip.to_device(v))
            for t in (self.dk, self.dv, self.dq):
                t.fill_(NAN)
        self.nk = nk
        self.ws = filled(hip, (hip.attn_grad_ws_numel(b, heads, nq),), NAN)

    def launch(self):
        self.hip.attn_grad(self.q, self.k, self.v, self.dout, dq=self.dq, dk=self.dk, dv=self.dv, ws=self.ws, heads=self.heads)

    def run(self):
        self.launch()
        self.hip.synchronize()
        return self

    def guards_intact(self):
        cc, nk = self.cc, self.nk
        rows = all(bool((buf[:, nk:] == SENTINEL).all()) for buf in (self.dkbuf, self.dvbuf))
        cols = all(bool((buf[..., cc:] == SENTINEL).all()) for buf in (self.dkbuf, self.dvbuf, self.dqbuf))
        return rows and cols

    def outputs(self):
        return self.dq, self.dk, self.dv


def check(call, what):
    i, dtype = call.i, call.dtype
    nk = K.RAGGED_CASES[i][4]
    ref = K.ragged_reference(i, dtype)
    q, k, v, do = K.ragged_inputs(i, dtype)
    cap = K.one_key_cap(q, k, v, do)
    results = []
    for name, got, ex, e, bound in zip(("dq", "dk", "dv"), call.outputs(), ref.exact, ref.e_model, ref.bound):
        finite = bool(torch.isfinite(got.float()).all())
        if nk == 1 and name != "dv":
            worst = float(got.float().abs().nan_to_num(float("inf")).max())
            print(f"{what} {name}: max |value| {worst:.3e} where the exact gradient is 0 (cap {cap:.3e})")
            results.append((name, finite and worst <= cap, worst, cap))
        else:
            err = R.rel_l2(got, ex)
            print(f"{what} {name}: rel L2 {err:.3e}  (E_model {e:.3e}, bound {bound:.3e}, share {err / bound:.2f})")
            results.append((name, finite and err <= bound, err, bound))
    assert all(ok for _, ok, _, _ in results), (what, results)
    assert call.guards_intact(), f"{what}: wrote into a guard row or a guard column"


@pytest.mark.parametrize("run", K.RAGGED_RUNS, ids=K.ragged_id)
def test_attn_grad_ragged(hip, run):
    i, dtype = run
    call = Call(hip, i, dtype).run()
    assert call.dq.dtype == dtype
    check(call, f"attn_grad {K.ragged_id(run)}")


def test_attn_grad_ragged_into_wider_rows(hip):
    """The resampler shape with 24 more columns per row: sentinel columns of the outputs survive, NaN columns of k and v
    are not read, and the bits are those of the dense call."""
    dense = Call(hip, 0, F16).run()
    wide = Call(hip, 0, F16, wide=24).run()
    assert wide.dk.stride(1) == wide.cc + 24 and wide.k.stride(1) == wide.cc + 24
    check(wide, "attn_grad resampler shape, wider rows")
    assert all(torch.equal(a, b) for a, b in zip(wide.outputs(), dense.outputs()))


def test_attn_grad_ragged_repeats_and_replays_bit_for_bit(hip):
    first = Call(hip, 0, F16).run()
    again = Call(hip, 0, F16).run().run()
    assert all(torch.equal(a, b) for a, b in zip(again.outputs(), first.outputs())) and again.guards_intact()
    ref = Call(hip, 2, F16).run()
    cap = Call(hip, 2, F16)
    hip.synchronize()
    hip.graph_begin()
    cap.launch()
    g = hip.graph_end()
    try:
        for _ in range(2):
            with hip.ctx():
                for t in cap.outputs():
                    t.zero_()
                cap.ws.fill_(NAN)
            hip.graph_launch(g)
            hip.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(cap.outputs(), ref.outputs())) and cap.guards_intact()
    finally:
        hip.graph_destroy(g)


@pytest.mark.parametrize("bad", ["nk=0", "d=96 nq=24"])
def test_attn_grad_ragged_contract(hip, bad):
    heads, d = 2, 96
    cc = heads * d
    nq, nk = (24 if bad == "d=96 nq=24" else 16), (0 if bad == "nk=0" else 17)
    q, dout = hip.zeros((2, nq, cc), F16), hip.zeros((2, nq, cc), F16)
    kbuf, vbuf = hip.zeros((2, 24, cc), F16), hip.zeros((2, 24, cc), F16)
    dq, dkbuf, dvbuf = filled(hip, (2, nq, cc), NAN, F16), filled(hip, (2, 24, cc), NAN, F16), filled(hip, (2, 24, cc), NAN, F16)
    ws = filled(hip, (2 * heads * nq * 2,), NAN)
    with pytest.raises(ValueError):
        hip.attn_grad(q, kbuf[:, :nk], vbuf[:, :nk], dout, dq=dq, dk=dkbuf[:, :nk], dv=dvbuf[:, :nk], ws=ws, heads=heads)
    hip.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (dq, dkbuf, dvbuf, ws)), "a refused call launched something"


def test_attention_operator_at_the_resampler_shape(hip):
    i = 0
    b, heads, d, nq, nk = K.RAGGED_CASES[i]
    q, k, v, do = K.ragged_inputs(i, F16)
    qd, kd, vd = (t.cuda().requires_grad_(True) for t in (q, k, v))
    out = grad_ops.attention(hip, qd, kd, vd, heads)
    out.backward(do.cuda())
    torch.cuda.synchronize()
    exact, _ = A.references(q, k, v, heads)
    ok, msg = A.within(out.detach().cpu(), exact, F16)
    assert ok, msg
    ref = K.ragged_reference(i, F16)
    for name, got, ex, bound in zip(("dq", "dk", "dv"), (qd.grad, kd.grad, vd.grad), ref.exact, ref.bound):
        err = R.rel_l2(got, ex)
        print(f"attention operator {name}: rel L2 {err:.3e} (bound {bound:.3e})")
        assert got.dtype == F16 and err <= bound, (name, err, bound)
