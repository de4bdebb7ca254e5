"""-m gpu: the backward of the fp32 row path (csrc/rows_grad.hip) through ``HipBackend.linear_rows_grad`` /
``aoe_interp_grad`` / ``rowvec_grad``, the operators ``grad_ops.linear_rows`` / ``aoe_interp`` / ``conv3x3(rowvec=)`` and
the blocks ``conditioning_grad.ordinal_embedder`` / ``time_embedding``, against the float64 references of
tests/rows_grad_reference.py (where the bounds are derived): dw / db (M + 16) 2^-24 E, dx (N + 16) 2^-24 E + 4 2^-24 |ref|,
dbase / ddeltas (B + classes + 16) 2^-24 E, drow (HW + 16) 2^-24 E, bit-equal to float64 on integer-valued operands; the
embedder block ten times torch's own fp32 error on the CPU per tensor, the purifier attachment and the resnet block with
the time path 4e-3 relative L2 per tensor.  Every kernel call has its outputs and scratch NaN-filled and fenced by
sentinels on both sides, is repeated, and is replayed from a captured graph, bit for bit.

Measured on MI355X: see DESIGN.md 7.1 (worst share of each bound)."""
import pytest
import torch

from progressive_stable_diffusion_amd import conditioning_grad as CG
from progressive_stable_diffusion_amd import grad_ops
from progressive_stable_diffusion_amd import optim as O
from tests import cond_grad_reference as KC
from tests import norm_grad_reference as N
from tests import rows_grad_reference as K

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
NAN = float("nan")
SENT, PAD = 12345.0, 64
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


def guarded(hip, shape):
    """A NaN-filled fp32 tensor of ``shape`` in the middle of a buffer with PAD sentinels before and behind it."""
    n = 1
    for s in shape:
        n *= s
    buf = filled(hip, (n + 2 * PAD,), NAN)
    with hip.ctx():
        buf[:PAD] = SENT
        buf[PAD + n:] = SENT
    return buf[PAD:PAD + n].view(shape), buf


def intact(buf):
    return bool((buf[:PAD] == SENT).all()) and bool((buf[-PAD:] == SENT).all())


class Call:
    """One kernel call with NaN-filled, fenced outputs: ``launch`` issues it on the backend stream."""

    def run(self):
        self.launch()
        self.hip.synchronize()
        return self

    def intact(self):
        return all(intact(b) for b in self.bufs.values())


def repeats_and_replays(hip, make, what):
    """A second call on fresh buffers, a repeated call on the same buffers and two replays of a captured graph (outputs
    and scratch spoiled in between) give the first call's bits."""
    first, again = make().run(), make().run().run()
    assert all(torch.equal(again.outs[k], v) for k, v in first.outs.items()), f"{what}: a repeated call differs"
    cap = make()
    hip.synchronize()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=hip.stream):
        cap.launch()
    for _ in range(2):
        with hip.ctx():
            for t in cap.outs.values():
                t.zero_()
            if cap.ws is not None:
                cap.ws.fill_(NAN)
        hip.synchronize()
        with hip.ctx():
            graph.replay()
        hip.synchronize()
        assert all(torch.equal(cap.outs[k], v) for k, v in first.outs.items()), f"{what}: a graph replay differs"
        assert cap.intact(), f"{what}: a graph replay wrote past an output"
    return first


# ---- linear_rows backward ---------------------------------------------------------------------------------------------------
class LinearCall(Call):
    def __init__(self, hip, m, k, n, act_in, w_dtype, want=("dx", "dw", "db"), integer=False):
        self.hip, self.act_in = hip, act_in
        self.host = K.linear_case(m, k, n, w_dtype, integer)
        self.x, self.w, self.dy = (hip.to_device(t) for t in self.host)
        self.outs, self.bufs = {}, {}
        for name, shape in (("dx", (m, k)), ("dw", (n, k)), ("db", (n,))):
            if name in want:
                self.outs[name], self.bufs[name] = guarded(hip, shape)
        self.ws = filled(hip, (hip.linear_rows_grad_ws_numel(m, k, n),), NAN) if "dx" in want else None

    def launch(self):
        self.hip.linear_rows_grad(self.x, self.w, self.dy, dx=self.outs.get("dx"), dw=self.outs.get("dw"),
                                  db=self.outs.get("db"), ws=self.ws, act_in=self.act_in)


@pytest.mark.parametrize("w_dtype", [F32, F16], ids=["w32", "w16"])
@pytest.mark.parametrize("act_in", [0, 1, 2])
@pytest.mark.parametrize("m,k,n", K.LINEAR_CASES)
def test_linear_rows_grad(hip, m, k, n, act_in, w_dtype):
    what = f"linear_rows_grad {m}x{k}x{n} act {act_in} {w_dtype}"
    full = repeats_and_replays(hip, lambda: LinearCall(hip, m, k, n, act_in, w_dtype), what)
    r = K.linear_rows_grad_model(*full.host, act_in)
    bounds = K.linear_bounds(r)
    shares = {name: K.share(full.outs[name], r[name], bounds[name]) for name in ("dx", "dw", "db")}
    print(f"{what}: share of the bound " + ", ".join(f"{k_} {v:.3f}" for k_, v in shares.items()))
    assert full.intact(), f"{what}: wrote past an output"
    assert all(v <= 1.0 for v in shares.values()), (what, shares)
    for key, want in K.LINEAR_OUTPUTS.items():
        if key == "all":
            continue
        part = LinearCall(hip, m, k, n, act_in, w_dtype, want=want).run()
        assert set(part.outs) == set(want) and part.intact(), (what, key)
        assert all(torch.equal(part.outs[name], full.outs[name]) for name in want), (what, key)


@pytest.mark.parametrize("w_dtype", [F32, F16], ids=["w32", "w16"])
@pytest.mark.parametrize("m,k,n", K.LINEAR_CASES)
def test_linear_rows_grad_is_exact_on_integers(hip, m, k, n, w_dtype):
    call = LinearCall(hip, m, k, n, 0, w_dtype, integer=True).run()
    r = K.linear_rows_grad_model(*call.host, 0)
    assert float(r["e_dx"].max()) < 2 ** 24 and float(r["e_dw"].max()) < 2 ** 24
    for name in ("dx", "dw", "db"):
        assert torch.equal(call.outs[name].double().cpu(), r[name]), name
    assert call.intact()


@pytest.mark.parametrize("bad", ["K=12", "K=2056", "act_in=3", "no outputs", "db without dw"])
def test_linear_rows_grad_contract(hip, bad):
    k = 12 if bad == "K=12" else 2056 if bad == "K=2056" else 16
    x, w, dy = hip.zeros((4, k), F32), hip.zeros((8, k), F32), hip.zeros((4, 8), F32)
    outs = dict(dx=filled(hip, (4, k), NAN), dw=filled(hip, (8, k), NAN), db=filled(hip, (8,), NAN))
    ws = filled(hip, (1 << 16,), NAN)
    kw = {} if bad == "no outputs" else dict(dx=outs["dx"], db=outs["db"]) if bad == "db without dw" else outs
    with pytest.raises(ValueError):
        hip.linear_rows_grad(x, w, dy, ws=ws, act_in=3 if bad == "act_in=3" else 0, **kw)
    args = [hip.lib.dadd_linear_rows_grad_f32, x.data_ptr(), w.data_ptr(), dy.data_ptr()]
    ptr = {n_: (t.data_ptr() if n_ in kw else None) for n_, t in outs.items()}
    rc = args[0](*args[1:], ptr["dx"], ptr["dw"], ptr["db"], ws.data_ptr(), 4, k, 8, 3 if bad == "act_in=3" else 0, 1, hip.s)
    assert rc == -1, "the C entry point itself refuses"
    hip.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (ws, *outs.values())), "a refused call launched something"


def test_linear_rows_operator_and_the_place_of_the_activation(hip):
    """The operator's gradients are the kernel's bits, with fp32 and with fp16 weights; and a layer's activation applied
    as the next layer's act_in gives the bits of the inference path's act_out."""
    m, k, n = 11, 1536, 130
    x, w, dy = K.linear_case(m, k, n)
    bias = K.randn((n,), 77, 0.1)
    for wt in (F32, F16):
        leaves = [t.cuda().requires_grad_(True) for t in (x, w, bias)]
        out = grad_ops.linear_rows(hip, *leaves, act_in=2, weight_dtype=wt)
        out.backward(dy.cuda())
        torch.cuda.synchronize()
        wk = w.to(wt)
        ref = K.linear_rows_model(x, wk, bias, 2)
        assert out.dtype == F32 and N.rel_l2(out, ref) <= 1e-6
        direct = LinearCall(hip, m, k, n, 2, wt).run()
        assert torch.equal(direct.w.cpu(), wk)
        for leaf, name in zip(leaves, ("dx", "dw", "db")):
            assert leaf.grad.dtype == F32 and torch.equal(leaf.grad, direct.outs[name]), (wt, name)
    only_x = [x.cuda().requires_grad_(True), w.cuda(), bias.cuda()]      # the data gradient alone keeps its bits
    grad_ops.linear_rows(hip, *only_x, act_in=2, weight_dtype=F16).backward(dy.cuda())
    torch.cuda.synchronize()
    assert only_x[1].grad is None and only_x[2].grad is None and torch.equal(only_x[0].grad, leaves[0].grad)
    # act_out = a, then act_in = 0  ==  act_out = 0, then act_in = a
    n1 = 136                                                               # (the second layer's K: a multiple of 8)
    w2, b2 = hip.to_device(K.randn((24, n1), 78, n1 ** -0.5)), hip.to_device(K.randn((24,), 79, 0.1))
    xd, wd, bd = hip.to_device(x), hip.to_device(K.randn((n1, k), 80, k ** -0.5)), hip.to_device(K.randn((n1,), 81, 0.1))
    for a in (1, 2):
        h1, h2, o1, o2 = (filled(hip, s, NAN) for s in ((m, n1), (m, n1), (m, 24), (m, 24)))
        hip.linear_rows(xd, wd, bd, h1, 0, a)
        hip.linear_rows(h1, w2, b2, o1, 0, 0)
        hip.linear_rows(xd, wd, bd, h2, 0, 0)
        hip.linear_rows(h2, w2, b2, o2, a, 0)
        hip.synchronize()
        assert bool(torch.isfinite(o1).all()) and torch.equal(o1, o2), a


# ---- AOE interpolation backward ---------------------------------------------------------------------------------------------
class AoeCall(Call):
    ws = None

    def __init__(self, hip, b, d, classes, integer=False):
        self.hip = hip
        self.host = K.aoe_case(b, d, classes, integer)
        self.lab, self.base, self.deltas, self.dout = (hip.to_device(t) for t in self.host)
        self.outs, self.bufs = {}, {}
        for name, shape in (("dbase", (d,)), ("ddeltas", (classes - 1, d))):
            self.outs[name], self.bufs[name] = guarded(hip, shape)

    def launch(self):
        self.hip.aoe_interp_grad(self.lab, self.dout, self.outs["dbase"], self.outs["ddeltas"])


@pytest.mark.parametrize("b,d,classes", K.AOE_CASES)
def test_aoe_interp_grad(hip, b, d, classes):
    what = f"aoe_interp_grad B {b} D {d} classes {classes}"
    call = repeats_and_replays(hip, lambda: AoeCall(hip, b, d, classes), what)
    lab, base, deltas, dout = call.host
    r = K.aoe_interp_grad_model(lab, dout, classes)
    s_b = K.share(call.outs["dbase"], r["dbase"], K.aoe_bound(b, classes, r["e_base"]))
    s_d = K.share(call.outs["ddeltas"], r["ddeltas"], K.aoe_bound(b, classes, r["e_deltas"]))
    print(f"{what}: share of the bound dbase {s_b:.3f}, ddeltas {s_d:.3f}")
    assert call.intact() and s_b <= 1.0 and s_d <= 1.0, (what, s_b, s_d)
    # the operator: the forward kernel's output and this kernel's bits
    leaves = [base.cuda().requires_grad_(True), deltas.cuda().requires_grad_(True)]
    out = grad_ops.aoe_interp(hip, lab.cuda(), *leaves)
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    assert N.rel_l2(out, K.aoe_interp_model(lab, base, deltas)) <= 1e-6
    assert torch.equal(leaves[0].grad, call.outs["dbase"]) and torch.equal(leaves[1].grad, call.outs["ddeltas"])


def test_aoe_interp_grad_contract(hip):
    lab, dout = hip.zeros((2,), F32), hip.zeros((2, 8), F32)
    dbase, ddeltas = filled(hip, (8,), NAN), filled(hip, (16, 8), NAN)
    with pytest.raises(ValueError):
        hip.aoe_interp_grad(lab, dout, dbase, ddeltas)                  # 17 classes
    rc = hip.lib.dadd_aoe_interp_grad_f32(lab.data_ptr(), dout.data_ptr(), dbase.data_ptr(), ddeltas.data_ptr(), 2, 8, 17, hip.s)
    assert rc == -1
    hip.synchronize()
    assert bool(torch.isnan(dbase).all()) and bool(torch.isnan(ddeltas).all()), "a refused call launched something"


# ---- rowvec backward ----------------------------------------------------------------------------------------------------------
class RowvecCall(Call):
    def __init__(self, hip, b, hw, c, dtype, integer=False):
        self.hip = hip
        self.host = K.rowvec_case(b, hw, c, dtype, integer)
        self.dy = hip.to_device(self.host)
        self.outs, self.bufs = {}, {}
        self.outs["drow"], self.bufs["drow"] = guarded(hip, (b, c))
        self.ws = filled(hip, (hip.rowvec_grad_ws_numel(b, hw, c),), NAN)

    def launch(self):
        self.hip.rowvec_grad(self.dy, self.outs["drow"], self.ws)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("b,hw,c", K.ROWVEC_CASES)
def test_rowvec_grad(hip, b, hw, c, dtype):
    what = f"rowvec_grad B {b} HW {hw} C {c} {dtype}"
    call = repeats_and_replays(hip, lambda: RowvecCall(hip, b, hw, c, dtype), what)
    r = K.rowvec_grad_model(call.host)
    s = K.share(call.outs["drow"], r["drow"], N.sum_bound(hw, r["e"]))
    print(f"{what}: share of the bound {s:.3f}")
    assert call.intact() and s <= 1.0, (what, s)
    exact = RowvecCall(hip, b, hw, c, dtype, integer=True).run()
    assert torch.equal(exact.outs["drow"].double().cpu(), K.rowvec_grad_model(exact.host)["drow"]) and exact.intact()


def test_rowvec_grad_contract(hip):
    dy, drow, ws = hip.zeros((2, 4, 12), F16), filled(hip, (2, 12), NAN), filled(hip, (1 << 10,), NAN)
    with pytest.raises(ValueError):
        hip.rowvec_grad(dy, drow, ws)                                   # C = 12
    rc = hip.lib.dadd_rowvec_grad_f16(dy.data_ptr(), drow.data_ptr(), ws.data_ptr(), 2, 4, 12, hip.s)
    assert rc == -1
    hip.synchronize()
    assert bool(torch.isnan(drow).all()) and bool(torch.isnan(ws).all()), "a refused call launched something"


# ---- the blocks --------------------------------------------------------------------------------------------------------------
def test_embedder_block_gradients(hip):
    """D = 64, hidden 128, 4 tokens, 4 classes, B = 5, labels -0.5, 0, 0.25, 1, 2.75: every trained master of the
    ``ordinal_embedder.`` group in relative L2 against float64 autograd of the oracle's AOE.  The path is fp32 throughout:
    the bound per tensor is ten times the error of torch's own fp32 autograd of the same block on the CPU against float64
    (base 5.2e-7, deltas 3.4e-7, projector.0 weight / bias 3.6e-7 / 3.9e-7, projector.2 weight / bias 1.9e-7 / 4.8e-8;
    tests/rows_grad_reference.py, pinned by the CPU suite)."""
    params, lab = K.embedder_params(), K.labels(K.EMB_B)
    dout = K.randn((K.EMB_B, K.EMB_TOKENS, K.EMB_D), 710)
    ref = K.embedder_oracle_grads(params, lab, dout)
    leaves = {k: v.cuda().requires_grad_(True) for k, v in params.items()}
    out = CG.ordinal_embedder(hip, leaves, lab.cuda(), num_tokens=K.EMB_TOKENS)
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    assert out.dtype == F32 and out.shape == (K.EMB_B, K.EMB_TOKENS, K.EMB_D)
    bad = {}
    for key in ref:
        err, bound = N.rel_l2(leaves[key].grad, ref[key]), K.EMBEDDER_BOUND[key.split(".", 1)[1]]
        print(f"embedder block d {key}: relative L2 error {err:.3e} (bound {bound:.1e}, {err / bound:.3f} of it)")
        if not err <= bound:
            bad[key] = (err, bound)
    assert not bad, bad
    assert leaves["ordinal_embedder.norm.weight"].grad is None and leaves["ordinal_embedder.null_embedding"].grad is None


def test_embedder_into_the_purifier_an_arena_and_one_fused_step(hip):
    """``ordinal_embedder`` -> .half() -> ``feature_purifier`` as source_aoe, E = 192, 2 heads, B = 2: the embedder's masters
    within the 16-bit block bound 4e-3 against float64 autograd; then, with the masters in a ParamArena, one FusedAdamW step
    is not skipped and moves every master that received a gradient."""
    e, tokens = KC.E, KC.TOKENS
    emb = K.embedder_params(d=e, hidden=2 * e, tokens=tokens)
    pur = KC.purifier_params()
    lab = torch.tensor([0.25, 2.75])
    inputs, dout = KC.block_inputs("purifier")
    img = inputs["image_embeds"]
    # float64: fp32 embedder weights as they are, the purifier's matrices rounded to fp16
    sd = {**{k: v.double().requires_grad_(True) for k, v in emb.items()}, **K.round_matrices(pur)}
    aoe64 = K.OC.aoe_forward(sd, lab.double(), tokens)
    K.OC.feature_purifier(sd, img.double(), aoe64, KC.HEADS).backward(dout.double())
    trained = ["ordinal_embedder." + k for k in K.EMBEDDER_TRAINED]
    leaves = {k: v.cuda().requires_grad_(True) for k, v in {**emb, **pur}.items()}
    aoe = CG.ordinal_embedder(hip, leaves, lab.cuda(), num_tokens=tokens)
    CG.feature_purifier(hip, leaves, img.cuda(), aoe.half(), KC.HEADS).backward(dout.cuda())
    torch.cuda.synchronize()
    KC.check_block("embedder -> purifier", {k: leaves[k].grad for k in trained}, {k: sd[k].grad for k in trained})
    # the arena and one step
    tensors = {**{k: emb[k] for k in trained}, **pur}
    groups = [g for g in O.reference_param_groups(list(tensors), 1e-3, weight_decay=1e-3) if g["params"]]
    assert [g["name"] for g in groups] == ["ordinal_embedder", "feature_purifier"] and [g["lr"] for g in groups] == [1e-3, 2e-3]
    arena = O.arena_from_groups(tensors, groups, device=DEV, working_dtype=F16)
    fused = O.FusedAdamW(hip, arena, groups, max_grad_norm=1.0)
    params = {k: torch.nn.Parameter(torch.empty(t.shape, device=DEV)) for k, t in tensors.items()}
    arena.attach(params)
    aoe = CG.ordinal_embedder(hip, params, lab.cuda(), num_tokens=tokens)
    out = CG.feature_purifier(hip, params, img.cuda(), aoe.half(), KC.HEADS)
    (out * dout.cuda()).sum().backward()
    torch.cuda.synchronize()
    got = [k for k in tensors if float(arena.grad(k).abs().sum()) > 0]
    assert set(trained) <= set(got), sorted(set(trained) - set(got))
    before = {k: arena.param(k).clone() for k in tensors}
    fused.step()
    st = fused.stats()
    assert st["step"] == 1 and not st["found_inf"], st
    stuck = [k for k in got if torch.equal(arena.param(k), before[k])]
    assert not stuck and not arena.g.any(), stuck
    assert bool(torch.isfinite(arena.p).all())


def test_time_path_into_a_resnet_block(hip):
    """The block of test_resnet_block_gradients (B = 2, 8x8, 64 -> 128) with the time path in front: timesteps -> 64
    sinusoids -> 128 -> SiLU -> 128 -> SiLU -> rows of width 128 + 64, whose first 128 columns (a strided slice) enter the
    first conv through ``conv3x3(rowvec=)``.  Every gradient, the time path's weights and biases included, against float64
    autograd with the matrices rounded to fp16; the columns the block does not take get a zero gradient."""
    p, x, t, dy = K.time_block_case()
    tparams = K.time_params()
    ref = K.time_block_oracle(p, tparams, x, t, dy)
    got = K.run_time_block(hip, grad_ops, CG, {k: v.cuda() for k, v in p.items()}, {k: v.cuda() for k, v in tparams.items()},
                           x.cuda(), t.cuda(), dy.cuda())
    torch.cuda.synchronize()
    unused = K.TIME_PROJ_KEYS[1]
    for key in (unused + ".weight", unused + ".bias"):
        assert not ref.pop(key).any() and got[key] is not None and not got[key].any(), key
    assert set(ref) == set(p) | set(tparams) - {unused + ".weight", unused + ".bias"} | {"x"}
    KC.check_block("time path -> resnet block", got, ref, bound=K.BLOCK_BOUND)


def test_conv3x3_rowvec_is_the_epilogue_row_and_nothing_else_changes(hip):
    """With ``rowvec`` the conv's output is that of the backend's EPI_ROWVEC call and drow the bits of ``rowvec_grad``;
    without it the operator's output and gradients keep the bits of the plain product."""
    b, hw, c, n = 2, 8, 64, 128
    r = N.R.rnd
    x, w, bias, dy = r((b, hw, hw, c), 900), r((n, 9 * c), 901, (9 * c) ** -0.5, F32), r((n,), 902, 0.1, F32), r((b, hw, hw, n), 903)
    rows = r((b, n + 64), 904, 0.5, F32)
    xd, wd, bd, rd = (t.cuda().requires_grad_(True) for t in (x, w, bias, rows))
    y = grad_ops.conv3x3(hip, xd, wd, bd, rowvec=rd[:, :n])
    y.backward(dy.cuda())
    x0, w0, b0 = (t.cuda().requires_grad_(True) for t in (x, w, bias))
    y0 = grad_ops.conv3x3(hip, x0, w0, b0)
    y0.backward(dy.cuda())
    torch.cuda.synchronize()
    ref = N.conv3x3_nhwc(x.double(), w.half().double(), bias.double()) + rows.double()[:, :n][:, None, None, :]
    N.close16(y, ref, "conv3x3(rowvec) y")
    assert not torch.equal(y, y0)
    drow = filled(hip, (b, n), NAN)
    hip.rowvec_grad(hip.to_device(dy), drow)
    hip.synchronize()
    assert torch.equal(rd.grad[:, :n], drow) and not rd.grad[:, n:].any()
    assert torch.equal(xd.grad, x0.grad) and torch.equal(wd.grad, w0.grad) and torch.equal(bd.grad, b0.grad)
