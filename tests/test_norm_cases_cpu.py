"""CPU checks of tests/norm_cases.py: that its inputs have the statistics they claim (ratio), that a correct fp32
two-pass implementation passes on them (fairness), and that degraded statistics fail on them (teeth).

ratio     after the 16-bit rounding every (sample, group) slab / row measures |mu| / sigma within 5 % of the nominal r,
          and the constant slabs are bit-constant.  The producer routes place the offsets exactly (bias, residual) on a
          random product: there the spread is a sample estimate over n values, whose relative standard error is
          1 / sqrt(2 n), and the check allows 5 % + 4 / sqrt(2 n).
fairness  F.group_norm / F.layer_norm in fp32 on the CPU (two-pass; the operator the reference model itself calls) stays
          within the route's tolerance of the float64 reference on every listed (r, dtype) and on the constant case; and
          every route of the table runs end to end on ``TorchRefBackend`` (fp32 arithmetic, rounding where the kernels
          round) inside its bounds - the same code path the GPU suite runs on ``HipBackend``.
teeth     on the r = 512 fp16 input the numpy one-pass fp32 models of the helper miss the tolerance, while at r = 8 and
          32 they hold it: a kernel with degraded statistics is something these inputs can see.  r = 512 is used only here.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import norm_cases as NC
from tests import norm_grad_reference as N
from tests.torch_backend import TorchRefBackend

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DTYPES = [F16, BF16]
IDS = ["f16", "bf16"]
# the maps and rows the routes of the table are built from: (b, h, w, c) and (m, c)
GN_SHAPES = [(2, 16, 16, 320), (2, 8, 8, 640), (2, 32, 32, 320), (2, 32, 32, 960), (1, 16, 16, 256), (1, 32, 32, 1280),
             (1, 8, 8, 320), (2, 8, 8, 320), (2, 4, 4, 2560)]
LN_SHAPES = [(200, 640), (512, 320), (37, 640), (64, 320), (32, 768), (3, 8)]
LN_TWO_PASS_SHAPES = [(37, 640), (64, 320), (32, 768), (3, 8)]


def _rs(shape, dtype):
    return (NC.R_TWO_PASS_BF16 if dtype == BF16 else NC.R_TWO_PASS) if shape in LN_TWO_PASS_SHAPES else NC.R_ONE_PASS


# ---- ratio -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", GN_SHAPES)
def test_groupnorm_maps_have_the_placed_ratio(shape, dtype):
    for r in NC.R_ONE_PASS:
        x = NC.gn_map(*shape, r, dtype)
        ratio = NC.gn_ratio(x)
        assert bool(((ratio / r - 1.0).abs() <= 0.05).all()), (shape, r, float((ratio / r - 1.0).abs().max()))
        mu = x.double().reshape(shape[0], -1, NC.GROUPS, shape[3] // NC.GROUPS).mean(dim=(1, 3))
        assert bool((torch.sign(mu) == NC.signs(NC.GROUPS)).all()), "the sign alternates by group"
    x = NC.gn_map(*shape, NC.R_CONST, dtype, constant=True)
    cg = shape[3] // NC.GROUPS
    slab = x[shape[0] - 1, :, :, NC.CONST_GROUP * cg:(NC.CONST_GROUP + 1) * cg]
    assert bool((slab == NC.CONST).all())
    ratio = NC.gn_ratio(x)
    assert math.isinf(float(ratio[shape[0] - 1, NC.CONST_GROUP]))
    ratio[shape[0] - 1, NC.CONST_GROUP] = NC.R_CONST
    assert bool(((ratio / NC.R_CONST - 1.0).abs() <= 0.05).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", LN_SHAPES)
def test_layernorm_rows_have_the_placed_ratio(shape, dtype):
    m, c = shape
    for r in _rs(shape, dtype):
        x = NC.ln_rows(m, c, r, dtype)
        ratio = NC.ln_ratio(x)
        assert bool(((ratio / r - 1.0).abs() <= 0.05).all()), (shape, r, float((ratio / r - 1.0).abs().max()))
        assert bool((torch.sign(x.double().mean(dim=1)) == NC.signs(m)).all()), "the sign alternates by row"
    x = NC.ln_rows(m, c, NC.R_CONST, dtype, constant=True)
    assert bool((x[NC.const_rows(m)] == NC.CONST).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_producer_offsets_are_exact_and_give_the_ratio(dtype):
    """The bias is +/- r sigma per group, the residual +/- r sigma per row, both exact; the float64 product they ride on
    has spread sigma within the sampling error of its estimate."""
    for r in NC.R_ONE_PASS:
        bias = NC.gn_bias(640, r)
        assert bool((bias.reshape(NC.GROUPS, -1) == (NC.signs(NC.GROUPS) * r * NC.SIGMA_GN).float()[:, None]).all())
        res = NC.row_offsets(NC.LNFOLD_M, 640, r, dtype)
        assert bool((res.double() == (NC.signs(NC.LNFOLD_M) * r * NC.SIGMA_LN)[:, None]).all())
    be = TorchRefBackend(compute=F64)
    for r in NC.R_ONE_PASS:
        recs = NC.run(be, "gnstat.dma128x160", dtype, r)               # 32 x 32 pixels x 20 channels per slab
        ratio = NC.gn_ratio(recs[0].got)
        n = 32 * 32 * 20
        assert bool(((ratio / r - 1.0).abs() <= 0.05 + 4.0 / math.sqrt(2 * n)).all()), (r, float((ratio / r - 1.0).abs().max()))
        recs = NC.run(be, "lnstat.lds", dtype, r)                      # rows of 640
        ratio = NC.ln_ratio(recs[0].got)
        assert bool(((ratio / r - 1.0).abs() <= 0.05 + 4.0 / math.sqrt(2 * 640)).all()), (r, float((ratio / r - 1.0).abs().max()))


# ---- fairness ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", GN_SHAPES)
def test_fp32_two_pass_groupnorm_is_within_tolerance(shape, dtype):
    gamma, beta = NC.affine(shape[3], 1)
    for r, const in [(r, False) for r in NC.R_ONE_PASS] + [(NC.R_CONST, True)]:
        x = NC.gn_map(*shape, r, dtype, constant=const)
        ref = NC.gn_ref64(x, gamma, beta, 1e-5, 1)
        got = F.silu(F.group_norm(x.float().permute(0, 3, 1, 2), NC.GROUPS, gamma, beta, 1e-5)).permute(0, 2, 3, 1).to(dtype)
        NC.check([NC.Rec("fp32 two-pass", got, ref, NC.tol_bound("groupnorm", ref, dtype))], f"groupnorm {shape} r {r} const {const}")
        if const:       # the float64 answer of the constant slab is silu(beta)
            cg = shape[3] // NC.GROUPS
            sl = slice(NC.CONST_GROUP * cg, (NC.CONST_GROUP + 1) * cg)
            assert torch.allclose(ref[shape[0] - 1, :, :, sl], F.silu(beta.double()[sl]).expand(shape[1], shape[2], cg), rtol=0, atol=1e-12)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", LN_SHAPES)
def test_fp32_two_pass_layernorm_is_within_tolerance(shape, dtype):
    m, c = shape
    gamma, beta = NC.affine(c, 2)
    for r, const in [(r, False) for r in _rs(shape, dtype)] + [(NC.R_CONST, True)]:
        x = NC.ln_rows(m, c, r, dtype, constant=const)
        ref = NC.ln_ref64(x, gamma, beta)
        got = F.layer_norm(x.float(), (c,), gamma, beta, 1e-5).to(dtype)
        NC.check([NC.Rec("fp32 two-pass", got, ref, NC.tol_bound("layernorm", ref, dtype))], f"layernorm {shape} r {r} const {const}")
        if const:
            assert torch.allclose(ref[NC.const_rows(m)], beta.double().expand(len(NC.const_rows(m)), c), rtol=0, atol=1e-12)


_CPU_CASES = [c for c in NC.cases() if c[0] not in NC.NEEDS]


@pytest.mark.parametrize("name,dtype,r", _CPU_CASES, ids=[f"{n}-{NC.name_of(d)}-r{r}" for n, d, r in _CPU_CASES])
def test_routes_pass_on_the_fp32_reference_backend(name, dtype, r):
    """Every route of the table, as the GPU suite runs it, on ``TorchRefBackend``: fp32 arithmetic on the same operands is
    inside every bound, so the (r, dtype) pair is a fair thing to ask of a kernel."""
    NC.check(NC.run(TorchRefBackend(), name, dtype, r), f"{name} {NC.name_of(dtype)} r={r}")


def _two_pass_grad_fp32(x, dy, gamma, beta, eps, silu, dims):
    """The backward of a norm written out in fp32, two-pass: mean, then the spread about it, over ``dims`` of x
    [..., C] viewed as given; -> dx (x.dtype), dgamma, dbeta (fp32, summed over everything but the last axis)."""
    xf, dyf = x.float(), dy.float()
    mean = xf.mean(dim=dims, keepdim=True)
    d = xf - mean
    rstd = torch.rsqrt((d * d).mean(dim=dims, keepdim=True) + eps)
    xhat = d * rstd
    g, bt = gamma.reshape(xf.shape[-2:] if xf.dim() == 4 else (-1,)), beta.reshape(xf.shape[-2:] if xf.dim() == 4 else (-1,))
    dz = dyf
    if silu:
        s = torch.sigmoid(xhat * g + bt)
        dz = dyf * (s * (1.0 + (xhat * g + bt) * (1.0 - s)))
    a = dz * g
    dx = rstd * (a - a.mean(dim=dims, keepdim=True) - xhat * (a * xhat).mean(dim=dims, keepdim=True))
    lead = tuple(range(xf.dim() - (2 if xf.dim() == 4 else 1)))
    return dx.to(x.dtype), (dz * xhat).sum(dim=lead).reshape(-1), dz.sum(dim=lead).reshape(-1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("route", ["groupnorm_grad", "groupnorm_grad.concat_silu", "layernorm_grad"])
def test_fp32_two_pass_backward_is_within_the_asserted_bounds(route, dtype):
    """Fairness of the backward cases: a plain fp32 two-pass backward meets every record the GPU suite asserts - dx, and
    dgamma / dbeta with their (M + 16) 2^-24 E - at every listed r and in the constant case.  (torch's own fp32 CPU
    autograd of group_norm does not: its statistics are not two-pass.)"""
    for r, const in [(r, False) for r in NC.rs_of(route, dtype)] + [(NC.R_CONST, True)]:
        if route == "layernorm_grad":
            x, dy, gamma, beta, ref = NC.ln_grad_operands(dtype, r, const)
            got = _two_pass_grad_fp32(x, dy, gamma, beta, 1e-5, False, (1,))
        else:
            case = N.GN_CASES[0] if route == "groupnorm_grad" else N.GN_CASES[3]
            x, dy, gamma, beta, ref = NC.gn_grad_operands(case, dtype, r, const)
            b, h, w, c = x.shape
            v = lambda t: t.reshape(b, h * w, NC.GROUPS, c // NC.GROUPS)      # noqa: E731
            dx, dg, db = _two_pass_grad_fp32(v(x), v(dy), gamma, beta, case[6], bool(case[5]), (1, 3))
            got = (dx.reshape(x.shape), dg, db)
        NC.check(NC.grad_recs(ref, *got), f"{route} r {r} const {const}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_groupnorm_backward_model_holds_the_sums_at_r_32(dtype):
    """``norm_grad_reference.gn_model`` restates the kernels' passes in fp32, the statistics summed about the slab's first
    element: it meets the bounds of dgamma / dbeta at r = 32.  (With plain sums of x and x^2 the same model came to 5.6 and
    11.5 times the bound of dgamma on these two cases in fp16: the 1e-4 of rstd that a one-pass variance loses at r = 32.)"""
    for case in (N.GN_CASES[0], N.GN_CASES[3]):
        for r in NC.R_ONE_PASS:
            x, dy, gamma, beta, ref = NC.gn_grad_operands(case, dtype, r)
            NC.check(NC.grad_recs(ref, *N.gn_model(x, dy, gamma, beta, case[6], bool(case[5]))), f"gn_model {case} r {r}")


def test_every_route_is_listed_for_both_types_where_it_has_them():
    listed = {(n, d) for n, d, _ in NC.cases()}
    for name, rt in NC.ROUTES.items():
        assert all((name, d) in listed for d in rt.dtypes)
        assert all(set(NC.rs_of(name, d)) <= set(NC.R_ENVELOPE) and NC.R_TEETH not in NC.rs_of(name, d) for d in rt.dtypes)


# ---- teeth -------------------------------------------------------------------------------------------------------------
def _gn_model_share(r, dtype):
    shape = (2, 16, 16, 320)
    gamma, beta = NC.affine(shape[3], 1)
    x = NC.gn_map(*shape, r, dtype)
    ref = NC.gn_ref64(x, gamma, beta, 1e-5, 1)
    got = NC.one_pass_groupnorm_model(x, gamma, beta, 1e-5, 1)
    return NC.share(NC.Rec("model", got, ref, NC.tol_bound("groupnorm", ref, dtype)))


def _fold_model_share(r, dtype):
    m, k, n = NC.LNFOLD_M, NC.LNFOLD_K, 1024
    x = NC.ln_rows(m, k, r, dtype)
    w, b, gamma, beta, w16, c1, bias = NC._fold_weights(n, k, False, dtype, 81)
    ref = NC._fold_ref(x, w, b, gamma, beta, False)
    got = NC.one_pass_lnfold_model(x, w16, c1, bias)
    return NC.share(NC.Rec("model", got, ref, NC.tol_bound("igemm.lnfold", ref, dtype)))


@pytest.mark.parametrize("model", [_gn_model_share, _fold_model_share], ids=["groupnorm", "lnfold"])
def test_one_pass_model_misses_the_tolerance_at_r_512(model):
    shares = {r: model(r, F16) for r in (*NC.R_ONE_PASS, NC.R_TEETH)}
    print({r: round(s, 3) for r, s in shares.items()})
    assert all(shares[r] <= 1.0 for r in NC.R_ONE_PASS), shares          # the model is a sane restatement
    assert shares[NC.R_TEETH] > 1.0, shares                               # ... and these inputs can see it degrade
