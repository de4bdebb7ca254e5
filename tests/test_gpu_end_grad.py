"""-m gpu: the gradients of the UNet's 4-channel end convolutions and of the loss on the HIP kernels of csrc/end_grad.hip
- ``HipBackend.end_wgrad`` (both modes), ``mse_rows_grad``, ``dgrad_cout4`` and the operators ``grad_ops.conv_in`` /
``conv_out`` / ``mse_rows`` - against float64 references on the same 16-bit operands (tests/end_grad_reference.py,
tests/grad_reference.py), and the UNet's shell end to end: latents -> conv_in -> ... -> conv_out -> Min-SNR MSE -> backward
-> one FusedAdamW step.

Tolerances: ``dW`` / ``dbias`` elementwise (M + 2) * 2^-24 * (|wide|^T |r(thin)|), derived in tests/grad_reference.py: the
kernel rounds thin to the storage type before the product, so every product is exact in fp32 and only the accumulation of
M terms errs, in any order; integer-valued operands must therefore come out bit-equal to float64.  16-bit outputs and the
conv forwards: the project's conv tolerance, 3e-3 + 2e-3 |ref| (fp16) and 2e-2 + 1.6e-2 |ref| (bf16).  ``mse_rows_grad``:
8 * 2^-24 |ref| (one subtraction, the rounded constant 2 / P, two multiplies: under 5 roundings).  Shell stage: relative L2
per tensor <= 4e-3, the block bound of DESIGN.md 7.1.
Shapes are the smallest that reach each hazard: maps whose rows wrap inside a 32-pixel step with padding on all four
sides, M below one step, slices that end mid-row, one to four thin channels, five tiles of wide channels; a slice of 18
stages with a ragged tail (M = 1150 at splitm 1: the main kernel's steady state, both register sets reloaded inside the
loop - a slice of at most 128 pixels never reloads); and 20 / 36 slices, so that a lane group of the finish kernel adds a
run of 3 / 5 slabs, the last run is short and one group is empty."""
from collections import OrderedDict

import pytest
import torch

from progressive_stable_diffusion_amd import grad_ops
from progressive_stable_diffusion_amd import lib as L
from progressive_stable_diffusion_amd import optim as O
from tests import end_grad_reference as E
from tests import grad_reference as R
from tests import norm_grad_reference as N

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
GUARD = 12345.0
BLOCK_BOUND = 4e-3
TOL = {F16: (3e-3, 2e-3), BF16: (2e-2, 1.6e-2)}
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


def dw_shape(mode, ct, cw):
    return (cw, 9, 8) if mode == E.IN else (ct, 9, cw)


def run_end_wgrad(hip, thin, wide, mode, splitm=1, bias=True, wide_dev=None):
    """One call on NaN-filled outputs and scratch -> (dw, dbias or None), synchronised.  ``splitm`` None: the default."""
    ct, cw = thin.shape[1], wide.shape[-1]
    td = hip.to_device(thin)
    wd = hip.to_device(wide) if wide_dev is None else wide_dev
    dw = filled(hip, dw_shape(mode, ct, cw), NAN)
    db = filled(hip, (cw if mode == E.IN else ct,), NAN) if bias else None
    s = hip.end_wgrad_splitm(thin.shape[0] * thin.shape[2] * thin.shape[3], cw) if splitm is None else splitm
    partial = filled(hip, (hip.end_wgrad_partial_numel(s, ct, cw, mode),), NAN) if s > 1 else None
    hip.end_wgrad(td, wd, dw, dbias=db, mode=mode, splitm=splitm, partial=partial)
    hip.synchronize()
    return dw, db


def check_end_wgrad(ref, dw, db, mode, ct, what):
    if mode == E.IN:
        assert not bool(dw[:, :, ct:].any()), f"{what}: pad channels are not zero"
        dw = dw[:, :, :ct]
    ref.check(dw, db, what)


# ---- weight gradient -----------------------------------------------------------------------------------------------
CASES = [(2, 8, 8, 4, 64, 1), (2, 7, 9, 4, 320, 1), (2, 7, 9, 3, 64, 4), (1, 3, 3, 4, 64, 1), (2, 12, 12, 4, 128, None),
         (2, 23, 25, 4, 64, 1), (2, 23, 25, 3, 128, 2), (2, 23, 25, 2, 64, 20), (2, 23, 25, 1, 64, 36)]


@pytest.mark.parametrize("mode", [E.IN, E.OUT], ids=["in", "out"])
@pytest.mark.parametrize("b,h,w,ct,cw,splitm", CASES)
def test_end_wgrad(hip, b, h, w, ct, cw, splitm, mode):
    what = f"end_wgrad mode{mode} B{b} {h}x{w} Ct{ct} Cw{cw} splitm{splitm}"
    thin, wide, ref = E.wgrad_case(b, h, w, ct, cw, mode)
    dw, db = run_end_wgrad(hip, thin, wide, mode, splitm)
    check_end_wgrad(ref, dw, db, mode, ct, what)
    # integer-valued operands: every product and every partial sum is exact, whatever the order
    thin, wide, ref = E.wgrad_case(b, h, w, ct, cw, mode, integer=True)
    dw, db = run_end_wgrad(hip, thin, wide, mode, splitm)
    got = dw[:, :, :ct] if mode == E.IN else dw
    assert torch.equal(got.double().cpu(), ref.dw), f"{what}: integer operands are not exact"
    assert torch.equal(db.double().cpu(), ref.db), f"{what}: integer dbias is not exact"
    # the raw output, pad channels of IN mode included, against the index-level model of the kernel (the model the CPU
    # suite pins to autograd)
    dw_model, db_model = E.end_wgrad_model(thin, wide, mode)
    assert dw.shape == dw_model.shape and torch.equal(dw.double().cpu(), dw_model), f"{what}: raw layout differs from the model"
    assert torch.equal(db.double().cpu(), db_model)


@pytest.mark.parametrize("mode", [E.IN, E.OUT], ids=["in", "out"])
def test_end_wgrad_bf16(hip, mode):
    thin, wide, ref = E.wgrad_case(2, 7, 9, 4, 64, mode, BF16)
    dw, db = run_end_wgrad(hip, thin, wide, mode, 2)
    check_end_wgrad(ref, dw, db, mode, 4, f"end_wgrad bf16 mode{mode}")


@pytest.mark.parametrize("mode", [E.IN, E.OUT], ids=["in", "out"])
def test_end_wgrad_wide_is_a_column_slice(hip, mode):
    """wide is the channel slice [..., 64:128] of a 192-wide tensor: the row stride travels."""
    g = torch.Generator().manual_seed(77)
    thin, wide192 = torch.randn((2, 3, 7, 9), generator=g), torch.randn((2, 7, 9, 192), generator=g).half()
    wide = wide192[..., 64:128]
    thin16 = E.nhwc(thin.half())
    ref = R.WgradRef(thin16, wide, 9) if mode == E.IN else R.WgradRef(wide, thin16, 9)
    dw, db = run_end_wgrad(hip, thin, wide, mode, 2, wide_dev=hip.to_device(wide192)[..., 64:128])
    check_end_wgrad(ref, dw, db, mode, 3, f"column slice mode{mode}")


def test_end_wgrad_without_bias(hip):
    thin, wide, ref = E.wgrad_case(2, 7, 9, 3, 64, E.OUT)
    dw, db = run_end_wgrad(hip, thin, wide, E.OUT, 4, bias=False)
    assert db is None
    check_end_wgrad(ref, dw, None, E.OUT, 3, "no bias")


# ---- overwrite, determinism, contract ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [E.IN, E.OUT], ids=["in", "out"])
def test_end_wgrad_overwrites_and_stays_inside_its_outputs(hip, mode):
    """dw, dbias and partial start as NaN and every element comes out finite (the zero pad channels of IN mode among
    them); 64 sentinel floats behind dw and behind dbias stay."""
    b, h, w, ct, cw, splitm = 2, 7, 9, 3, 64, 4
    thin, wide, ref = E.wgrad_case(b, h, w, ct, cw, mode)
    shape = dw_shape(mode, ct, cw)
    nw, nb = shape[0] * shape[1] * shape[2], (cw if mode == E.IN else ct)
    bw, bb = filled(hip, (nw + 64,), NAN), filled(hip, (nb + 64,), NAN)
    with hip.ctx():
        bw[nw:] = GUARD
        bb[nb:] = GUARD
    partial = filled(hip, (hip.end_wgrad_partial_numel(splitm, ct, cw, mode),), NAN)
    dw, db = bw[:nw].view(shape), bb[:nb]
    hip.end_wgrad(hip.to_device(thin), hip.to_device(wide), dw, dbias=db, mode=mode, splitm=splitm, partial=partial)
    hip.synchronize()
    assert bool(torch.isfinite(bw).all()) and bool(torch.isfinite(bb).all())
    assert bool((bw[nw:] == GUARD).all()) and bool((bb[nb:] == GUARD).all()), "wrote past the end of dw / dbias"
    check_end_wgrad(ref, dw, db, mode, ct, f"overwrite mode{mode}")


@pytest.mark.parametrize("mode", [E.IN, E.OUT], ids=["in", "out"])
def test_end_wgrad_is_deterministic_and_capturable(hip, mode):
    """The same splitm-4 call twice: equal bit for bit; captured into a graph and launched twice: equal to the eager
    result bit for bit."""
    b, h, w, ct, cw, splitm = 2, 12, 12, 4, 128, 4
    thin, wide, _ = E.wgrad_case(b, h, w, ct, cw, mode)
    wd = hip.to_device(wide)
    dw1, db1 = run_end_wgrad(hip, thin, wide, mode, splitm, wide_dev=wd)
    dw2, db2 = run_end_wgrad(hip, thin, wide, mode, splitm, wide_dev=wd)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)
    td = hip.to_device(thin)
    dw, db = filled(hip, dw_shape(mode, ct, cw), NAN), filled(hip, tuple(db1.shape), NAN)
    partial = filled(hip, (hip.end_wgrad_partial_numel(splitm, ct, cw, mode),), NAN)
    hip.synchronize()
    hip.graph_begin()
    hip.end_wgrad(td, wd, dw, dbias=db, mode=mode, splitm=splitm, partial=partial)
    g = hip.graph_end()
    try:
        for _ in range(2):
            hip.zero_(dw)
            hip.zero_(db)
            hip.graph_launch(g)
            hip.synchronize()
            assert torch.equal(dw, dw1) and torch.equal(db, db1)
    finally:
        hip.graph_destroy(g)


def test_end_wgrad_default_splitm_follows_the_documented_rule(hip):
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert hip.end_wgrad_splitm(32768, 320) == -(-2 * cu // 5)
    assert hip.end_wgrad_splitm(100, 64) == 2                          # at least 64 pixels per slice
    assert hip.end_wgrad_splitm(40, 64) == 1
    assert hip.end_wgrad_partial_numel(1, 4, 64, E.IN) == 0
    assert hip.end_wgrad_partial_numel(3, 4, 64, E.IN) == 3 * (64 * 72 + 64)


@pytest.mark.parametrize("mode", [E.IN, E.OUT], ids=["in", "out"])
@pytest.mark.parametrize("bad", ["Cw=96", "Ct=5", "splitm=0", "mode=2", "no partial", "splitm>ceil(M/32)", "ld_wide=100",
                                 "wide unaligned", "dw unaligned"])
def test_end_wgrad_contract(hip, bad, mode):
    """Each violation is refused (ValueError) and nothing is launched.  Cw, Ct, splitm, the missing partial, ld_wide and
    the alignments are refused by the library itself (DADD_EINVAL)."""
    b, h, w, ct, cw, kw = 1, 8, 8, 4, 64, dict(splitm=1)
    if bad == "Cw=96":
        cw = 96
    elif bad == "Ct=5":
        ct = 5
    elif bad == "splitm=0":
        kw = dict(splitm=0)
    elif bad == "no partial":
        kw = dict(splitm=2)
    elif bad == "splitm>ceil(M/32)":
        kw = dict(splitm=3, partial=filled(hip, (hip.end_wgrad_partial_numel(3, ct, cw, mode),), NAN))
    thin, wide = hip.zeros((b, ct, h, w), F32), hip.zeros((b, h, w, cw), F16)
    if bad == "ld_wide=100":
        wide = hip.zeros((b, h, w, 100), F16)[..., :cw]
    elif bad == "wide unaligned":
        wide = hip.zeros((b, h, w, cw + 8), F16)[..., 4:cw + 4]
    shape = dw_shape(mode, ct, cw)
    n = shape[0] * shape[1] * shape[2]
    buf = filled(hip, (n + 4,), NAN)
    dw = (buf[1:n + 1] if bad == "dw unaligned" else buf[:n]).view(shape)
    db = filled(hip, (cw if mode == E.IN else ct,), NAN)
    with pytest.raises(ValueError):
        hip.end_wgrad(thin, wide, dw, dbias=db, mode=2 if bad == "mode=2" else mode, **kw)
    hip.synchronize()
    assert bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all()), "a refused call launched something"


# ---- the loss gradient -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 4, 5, 7), (3, 3, 5, 7)], ids=["vector", "scalar"])
def test_mse_rows_grad(hip, shape):
    """per_sample = 140 takes the 16-byte path, 105 the scalar one."""
    g = torch.Generator().manual_seed(5)
    pred, target = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    rowgrad = torch.tensor([0.37, 0.0, -1234.5])
    per = pred.numel() // shape[0]
    out = filled(hip, shape, NAN)
    hip.mse_rows_grad(hip.to_device(pred), hip.to_device(target), hip.to_device(rowgrad), out)
    hip.synchronize()
    ref = rowgrad.double().view(-1, 1, 1, 1) * (2.0 / per) * (pred.double() - target.double())
    err = (out.double().cpu() - ref).abs()
    bound = 8 * 2.0 ** -24 * ref.abs()
    print(f"mse_rows_grad per {per}: worst err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert bool((err <= bound).all()), int((err > bound).sum())
    assert bool((out[1] == 0).all()), "a zero row gradient must give exact zeros"
    inplace = hip.to_device(pred)                                      # out may be pred itself
    hip.mse_rows_grad(inplace, hip.to_device(target), hip.to_device(rowgrad), inplace)
    hip.synchronize()
    assert torch.equal(inplace, out), "the in-place call differs"


def test_mse_rows_operator(hip):
    g = torch.Generator().manual_seed(6)
    pred, target = torch.randn((3, 4, 5, 7), generator=g), torch.randn((3, 4, 5, 7), generator=g)
    wrow = torch.tensor([0.5, 2.0, 1.25])
    pd = pred.cuda().requires_grad_(True)
    base = grad_ops.mse_rows(hip, pd, target.cuda())
    assert base.shape == (3,) and base.dtype == F32
    ((wrow.cuda() * base).mean() * 4096.0).backward()
    torch.cuda.synchronize()
    p64 = pred.double().requires_grad_(True)
    b64 = ((p64 - target.double()) ** 2).mean((1, 2, 3))
    ((wrow.double() * b64).mean() * 4096.0).backward()
    assert (base.detach().double().cpu() - b64.detach()).abs().max().item() <= 140 * 2.0 ** -24 * b64.max().item()
    err = (pd.grad.double().cpu() - p64.grad).abs()
    assert pd.grad.dtype == F32 and bool((err <= 16 * 2.0 ** -24 * p64.grad.abs()).all())   # + the roundings of rowgrad


# ---- conv_out's data gradient --------------------------------------------------------------------------------------------
def conv_out_operands(c, dtype):
    g = torch.Generator().manual_seed(300 + c)
    b, h, w, co = 2, 7, 9, 4
    x = torch.randn((b, h, w, c), generator=g).to(dtype)
    wm = torch.randn((co, 9 * c), generator=g) * (9 * c) ** -0.5        # fp32 master
    bias = torch.randn((co,), generator=g) * 0.1
    dy = torch.randn((b, co, h, w), generator=g)                          # fp32 NCHW, rounded by the kernels
    w16 = wm.to(dtype)
    dx_ref, _, _ = E.conv2d_grads(E.nchw(x), w16.reshape(co, 3, 3, c).permute(0, 3, 1, 2), dy.to(dtype))
    return x, wm, bias, dy, w16, E.nhwc(dx_ref)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("c", [64, 320])
def test_dgrad_cout4(hip, c, dtype):
    x, _, _, dy, w16, dx_ref = conv_out_operands(c, dtype)
    wt = hip.to_device(grad_ops.dgrad_weight_cout4(w16))
    dx = filled(hip, tuple(x.shape), NAN, dtype)
    hip.dgrad_cout4(hip.to_device(dy), wt, dx)
    hip.synchronize()
    R.close(dx, dx_ref, f"dgrad_cout4 C{c} {dtype}", *TOL[dtype])


def test_dgrad_still_refuses_thin_outputs_and_names_the_way(hip):
    with pytest.raises(ValueError, match="dgrad_cout4"):
        hip.dgrad(hip.zeros((1, 8, 8, 8), F16), hip.zeros((64, 72), F16), hip.zeros((1, 8, 8, 64), F16), taps=9)


# ---- operators -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_conv_in_operator(hip, dtype):
    g = torch.Generator().manual_seed(410)
    b, ct, h, w, n = 2, 4, 7, 9, 64
    x = torch.randn((b, ct, h, w), generator=g)
    wm, bias = torch.randn((n, 9 * ct), generator=g) * (9 * ct) ** -0.5, torch.randn((n,), generator=g) * 0.1
    dy = torch.randn((b, h, w, n), generator=g).to(dtype)
    x16 = E.nhwc(x.to(dtype))
    y_ref, _, _, _ = R.conv_autograd(x16, wm.to(dtype), dy, 9, 1, False, bias)
    wd, bd = wm.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="data gradient"):
        grad_ops.conv_in(hip, x.cuda().requires_grad_(True), wd, bd, dtype=dtype)
    y = grad_ops.conv_in(hip, x.cuda(), wd, bd, dtype=dtype)
    assert y.dtype == dtype and y.shape == (b, h, w, n)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    R.close(y, y_ref, f"conv_in y {dtype}", *TOL[dtype])
    assert wd.grad.dtype == F32 and wd.grad.shape == wm.shape and bd.grad.dtype == F32 and bd.grad.shape == bias.shape
    R.WgradRef(x16, dy, 9).check(wd.grad, bd.grad, f"conv_in operator {dtype}")


def test_operators_refuse_untrainable_widths_in_the_forward(hip):
    """The weight-gradient kernel takes wide channels in multiples of 64: a trainable conv_in with N = 72 or conv_out with
    C = 72 is refused by the forward, not from inside backward(); with detached parameters the forward runs."""
    x = torch.zeros((1, 4, 8, 8), device=DEV)
    w, bias = torch.zeros((72, 36), device=DEV), torch.zeros((72,), device=DEV)
    with pytest.raises(ValueError, match="multiple of 64"):
        grad_ops.conv_in(hip, x, w.clone().requires_grad_(True), bias)
    assert grad_ops.conv_in(hip, x, w, bias).shape == (1, 8, 8, 72)
    xo, wo = torch.zeros((1, 8, 8, 72), device=DEV, dtype=F16), torch.zeros((4, 9 * 72), device=DEV)
    with pytest.raises(ValueError, match="multiple of 64"):
        grad_ops.conv_out(hip, xo, wo.clone().requires_grad_(True))
    assert grad_ops.conv_out(hip, xo, wo).shape == (1, 4, 8, 8)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_conv_out_operator(hip, dtype):
    c, co = 64, 4
    x, wm, bias, dy, w16, dx_ref = conv_out_operands(c, dtype)
    y_ref, _, _, _ = R.conv_autograd(x, w16, E.nhwc(dy.to(dtype)), 9, 1, False, bias)
    xd = x.cuda().requires_grad_(True)
    wd, bd = wm.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
    y = grad_ops.conv_out(hip, xd, wd, bd)
    assert y.dtype == F32 and y.shape == dy.shape
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    R.close(E.nhwc(y), y_ref, f"conv_out y {dtype}", *TOL[dtype])
    assert xd.grad.dtype == dtype and xd.grad.shape == x.shape
    R.close(xd.grad, dx_ref, f"conv_out x.grad {dtype}", *TOL[dtype])
    assert wd.grad.dtype == F32 and wd.grad.shape == wm.shape and bd.grad.dtype == F32 and bd.grad.shape == bias.shape
    R.WgradRef(x, E.nhwc(dy.to(dtype)), 9).check(wd.grad, bd.grad, f"conv_out operator {dtype}")
    x2, w2 = x.cuda(), wm.cuda().requires_grad_(True)                   # no data gradient wanted: none computed
    grad_ops.conv_out(hip, x2, w2).backward(dy.cuda())
    torch.cuda.synchronize()
    assert x2.grad is None and torch.equal(w2.grad, wd.grad)


# ---- the UNet's shell, end to end ------------------------------------------------------------------------------------
def test_shell_stage_gradients_and_optimizer_step(hip):
    """Latents B = 2, 4 x 8 x 8 -> conv_in (4 -> 64) -> GroupNorm+SiLU -> conv3x3 (64 -> 64) -> GroupNorm+SiLU -> conv_out
    (64 -> 4) -> mse_rows -> (w_b * base).mean() * scale, masters in a ParamArena, scale = FusedAdamW's loss scale 2^12:
    every parameter gradient, divided by the scale, against float64 autograd of the same stage with the weights rounded to
    fp16, relative L2 per tensor <= 4e-3; then one optimizer step that is not skipped and moves every master.
    Measured on MI355X: worst tensor 5.6e-4 (the middle conv's weight), conv_in weight 5.4e-4, conv_out weight 4.9e-4,
    gamma / beta 2.4-4.7e-4, biases 1.8-4.2e-4."""
    b, hw, ch = 2, 8, 64
    r = R.rnd
    lat = r((b, 4, hw, hw), 901).float()                                 # fp16-representable: conv_in's rounding is exact
    target = r((b, 4, hw, hw), 902, dtype=F32)
    wrow = torch.tensor([0.8, 2.5])                                      # a fixed Min-SNR-like row
    p = OrderedDict([
        ("unet.conv_in.weight", r((ch, 36), 903, 36 ** -0.5, F32)), ("unet.conv_in.bias", r((ch,), 904, 0.1, F32)),
        ("unet.norm1.weight", 1 + 0.2 * r((ch,), 905, dtype=F32)), ("unet.norm1.bias", r((ch,), 906, 0.2, F32)),
        ("unet.conv_mid.weight", r((ch, 9 * ch), 907, (9 * ch) ** -0.5, F32)), ("unet.conv_mid.bias", r((ch,), 908, 0.1, F32)),
        ("unet.norm2.weight", 1 + 0.2 * r((ch,), 909, dtype=F32)), ("unet.norm2.bias", r((ch,), 910, 0.2, F32)),
        ("unet.conv_out.weight", r((4, 9 * ch), 911, (9 * ch) ** -0.5, F32)), ("unet.conv_out.bias", r((4,), 912, 0.1, F32))])
    short = dict(zip(p, ("w_in", "c_in", "g1", "b1", "w_mid", "c_mid", "g2", "b2", "w_out", "c_out")))
    q = {short[k]: (v.half() if short[k].startswith("w") else v).double().requires_grad_(True) for k, v in p.items()}
    E.shell_stage64(lat.double(), target.double(), wrow.double(), q).backward()
    ref = {k: q[short[k]].grad for k in p}

    groups = O.reference_param_groups(list(p), 1e-3, weight_decay=1e-2)[:1]
    arena = O.arena_from_groups(p, groups, device=DEV)
    fused = O.FusedAdamW(hip, arena, groups, init_scale=2.0 ** 12)
    params = {k: torch.nn.Parameter(torch.empty(t.shape, device=DEV)) for k, t in p.items()}
    arena.attach(params)
    hip.synchronize()                                                    # the state block (the scale) is uploaded
    d = {short[k]: v for k, v in params.items()}
    h = grad_ops.conv_in(hip, lat.cuda(), d["w_in"], d["c_in"])
    h = grad_ops.conv3x3(hip, grad_ops.group_norm(hip, h, d["g1"], d["b1"], silu=True), d["w_mid"], d["c_mid"])
    pred = grad_ops.conv_out(hip, grad_ops.group_norm(hip, h, d["g2"], d["b2"], silu=True), d["w_out"], d["c_out"])
    base = grad_ops.mse_rows(hip, pred, target.cuda())
    loss = (wrow.cuda() * base).mean() * fused.scale()[0]
    loss.backward()
    torch.cuda.synchronize()
    scale = fused.stats()["scale"]
    assert scale == 2.0 ** 12
    errs = {k: N.rel_l2(arena.grad(k) / scale, ref[k]) for k in p}
    for k, err in errs.items():
        print(f"shell stage d{k}: relative L2 error {err:.3e}")
    worst = max(errs, key=errs.get)
    print(f"shell stage: worst relative L2 error {errs[worst]:.3e} ({worst}) (bound {BLOCK_BOUND:.0e})")
    for k, err in errs.items():
        assert err <= BLOCK_BOUND, (k, err)
    before = {k: arena.param(k).clone() for k in p}
    fused.step()
    torch.cuda.synchronize()
    st = fused.stats()
    assert st["step"] == 1 and not st["found_inf"], st
    for k in p:
        assert not torch.equal(arena.param(k), before[k]), f"{k} did not move"
