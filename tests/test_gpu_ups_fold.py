"""GPU: the upsample conv as four 2x2 phase convs on pre-summed weights (DADD_TUNE_UPS_FOLD, csrc/igemm_ups_fold.hip).

Every case is compared with
  (a) the float64 phase conv on the ROUNDED folded weights and the 16-bit inputs, under the launch audit's bound
      2 u16 |r| + K u32 (|x| conv |w4| + |bias|), K = 4 Cin: the kernel computes what the fold states;
  (b) the float64 UNFOLDED conv on the same inputs, under ``close(o, o_ref, 3e-3, 2e-3)`` of
      test_gpu_kernels.py::test_igemm_conv3x3: the fold states the conv.  The bf16 case draws x with a quarter of the
      spread: at |out| >= 2 one bf16 rounding of the output alone (2^-8 |out|) is as large as that fp16 tolerance.
The output is filled with NaN first (every pixel of all four phases must be written) and a guard band behind it must
stay as it was.  The rms error of the fold and of the 9-tap gather against (b)'s reference are printed side by side: the
fold carries one more independent 16-bit rounding per weight, so its rms may be the larger; a ratio above 2 is a defect."""
import math

import pytest
import torch

from progressive_stable_diffusion_amd import engine as E
from progressive_stable_diffusion_amd import lib as L
from tests import plan_cases
from tests.launch_audit import U, U32
from tests.ups_fold_reference import phase_conv, unfolded

pytestmark = pytest.mark.gpu
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
GUARD = 4096
FOLD_KERNEL = "igemm_ups_fold_kernel"


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(torch.device("cuda:0"))


def rnd(shape, seed, scale=1.0, dtype=F16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def rms(t):
    return float(torch.sqrt((t.double() ** 2).mean()))


def guarded(hip, shape, dtype):
    """(out view filled with NaN, guard band behind it filled with 1.5) in one allocation"""
    n = math.prod(shape)
    buf = hip.empty((n + GUARD,), dtype)
    with hip.ctx():
        buf[:n].fill_(float("nan"))
        buf[n:].fill_(1.5)
    return buf[:n].view(shape), buf[n:]


def launch(hip, xd, wd, bd, shape, dtype, **kw):
    out, guard = guarded(hip, shape, dtype)
    hip.igemm(xd, wd, out, bias=bd, taps=9, ups=1, pad=1, tile_m=128, **kw)
    hip.synchronize()
    o = out.cpu()
    assert not bool(torch.isnan(o.float()).any()), "output pixels left unwritten"
    assert bool((guard.cpu().float() == 1.5).all()), "guard band behind the output overwritten"
    return o


CASES = {                    # B, Hi, Wi, Cin, N, tile_n, dtype, spread of x, runs the fold (else: the gather fallback)
    "one_tile_per_phase_nonsquare": (1, 8, 16, 64, 160, 160, F16, 1.0, True),
    "tile_spans_two_samples_ragged_columns": (2, 8, 8, 128, 192, 160, F16, 1.0, True),
    "ragged_phase_192_rows_falls_back": (3, 8, 8, 64, 128, 128, F16, 1.0, False),
    "bf16_twin": (1, 8, 16, 64, 160, 160, BF16, 0.25, True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_fold_against_both_references(hip, case):
    b, hi, wi, cin, n, tile_n, dtype, spread, folds = CASES[case]
    x, w9 = rnd((b, hi, wi, cin), 21, spread, dtype), rnd((n, 9 * cin), 22, 1 / math.sqrt(9 * cin), dtype)
    bias = rnd((n,), 23, 0.1, F32)
    w4 = E.fold_ups_weight(w9)
    xd, w9d, w4d, bd = (hip.to_device(t) for t in (x, w9, w4, bias))
    hip.register_ups_fold(w9d, w4d)
    shape = (b, 2 * hi, 2 * wi, n)
    hip.prof_begin()
    o = launch(hip, xd, w9d, bd, shape, dtype, flags=L.EPI_BIAS | L.TUNE_UPS_FOLD, tile_n=tile_n)
    names = [r[0] for r in hip.prof_end()]
    assert len(names) == 1 and (FOLD_KERNEL in names[0]) == folds and ("_bf16" in names[0]) == (dtype == BF16), names
    gather = launch(hip, xd, w9d, bd, shape, dtype, flags=L.EPI_BIAS, tile_n=tile_n)
    x64, b64 = x.to(F64), bias.to(F64)
    ref_b = unfolded(x64, w9.to(F64)) + b64
    e_fold, e_gather = rms(o.to(F64) - ref_b), rms(gather.to(F64) - ref_b)
    print(f"\n{case}: rms error against the float64 unfolded conv: fold {e_fold:.4e}, gather {e_gather:.4e}, "
          f"ratio {e_fold / e_gather:.3f}")
    if not folds:
        assert torch.equal(o.view(torch.int16), gather.view(torch.int16))      # the fallback IS the flagless launch
    else:
        # (a) what the fold states, to accumulation accuracy
        ref_a = phase_conv(x64, w4.to(F64)) + b64
        amag = phase_conv(x64.abs(), w4.to(F64).abs()) + b64.abs()
        fi = torch.finfo(dtype)
        bound = 2 * U[dtype] * ref_a.abs() + 4 * cin * U32 * amag + fi.smallest_normal * fi.eps
        err = (o.to(F64) - ref_a).abs()
        worst = float((err / bound).max())
        print(f"{case}: worst element at {worst:.3f} of the audit bound")
        assert worst <= 1.0, (case, worst)
        assert e_fold <= 2 * e_gather, (case, e_fold, e_gather)
    # (b) the conv itself
    bad = (o.to(F64) - ref_b).abs() > 3e-3 + 2e-3 * ref_b.abs()
    assert not bool(bad.any()), (case, int(bad.sum()), float((o.to(F64) - ref_b).abs().max()))


def test_fold_writes_groupnorm_partials(hip):
    """The VAE form: 128 x 128 tiles, N = 128 (cg = 4), DADD_EPI_GNSTAT.  A wave's 64 rows are one chunk of one phase; summed
    per (sample, group) the partials are the sum and sum of squares of the stored output, within the audit's statistics
    bound (n terms: n 2^-24 sum |term|)."""
    b, hi, wi, cin, n = 1, 16, 16, 128, 128
    x, w9, bias = rnd((b, hi, wi, cin), 31), rnd((n, 9 * cin), 32, 1 / math.sqrt(9 * cin)), rnd((n,), 33, 0.1, F32)
    w4 = E.fold_ups_weight(w9)
    xd, w9d, w4d, bd = (hip.to_device(t) for t in (x, w9, w4, bias))
    hip.register_ups_fold(w9d, w4d)
    nchunk = 4 * hi * wi // 64
    ws = hip.zeros((b * nchunk * 64,), F32)
    hip.prof_begin()
    o = launch(hip, xd, w9d, bd, (b, 2 * hi, 2 * wi, n), F16, flags=L.EPI_BIAS | L.EPI_GNSTAT | L.TUNE_UPS_FOLD, tile_n=128,
               gn_ws=ws, gn_nchunk=nchunk)
    names = [r[0] for r in hip.prof_end()]
    assert names == [FOLD_KERNEL + "<128, 128>"], names
    x64, b64 = x.to(F64), bias.to(F64)
    ref_a = phase_conv(x64, w4.to(F64)) + b64
    bound = 2 * U[F16] * ref_a.abs() + 4 * cin * U32 * (phase_conv(x64.abs(), w4.to(F64).abs()) + b64.abs()) \
        + torch.finfo(F16).smallest_normal * torch.finfo(F16).eps
    assert float(((o.to(F64) - ref_a).abs() / bound).max()) <= 1.0
    ref_b = unfolded(x64, w9.to(F64)) + b64
    assert not bool(((o.to(F64) - ref_b).abs() > 3e-3 + 2e-3 * ref_b.abs()).any())
    got = ws.cpu().to(F64).reshape(b, nchunk, 32, 2).sum(1)                       # [B][group][2]
    terms = o.to(F64).reshape(b, 4 * hi * wi, 32, n // 32)
    want = torch.stack([terms.sum((1, 3)), (terms * terms).sum((1, 3))], -1)
    lim = terms.shape[1] * terms.shape[3] * U32 * torch.stack([terms.abs().sum((1, 3)), (terms * terms).sum((1, 3))], -1)
    assert bool(((got - want).abs() <= lim).all()), float(((got - want).abs() / lim).max())
    # every chunk holds 64 pixels of one phase: its sum of squares is positive and no chunk is left at zero
    assert bool((ws.cpu().reshape(b, nchunk, 32, 2)[..., 1] > 0).all())


def test_fallbacks_are_bit_equal_to_the_flagless_launch(hip):
    b, hi, wi, cin, n = 2, 8, 8, 128, 160
    x, w9, bias = rnd((b, hi, wi, cin), 41), rnd((n, 9 * cin), 42, 1 / math.sqrt(9 * cin)), rnd((n,), 43, 0.1, F32)
    xd, w9d, bd = (hip.to_device(t) for t in (x, w9, bias))
    shape = (b, 2 * hi, 2 * wi, n)
    plain = launch(hip, xd, w9d, bd, shape, F16, flags=L.EPI_BIAS, tile_n=160)
    # the flag without a registered fold
    hip.prof_begin()
    o = launch(hip, xd, w9d, bd, shape, F16, flags=L.EPI_BIAS | L.TUNE_UPS_FOLD, tile_n=160)
    assert [r[0] for r in hip.prof_end()] == ["igemm_dma_kernel<128, 160, true, false, 0>"]
    assert torch.equal(o.view(torch.int16), plain.view(torch.int16))
    # the flag, a registered fold and split-K: the gather and its finish kernel
    hip.register_ups_fold(w9d, hip.to_device(E.fold_ups_weight(w9)))
    part = hip.zeros((2 * math.prod(shape),), F32)
    sk = launch(hip, xd, w9d, bd, shape, F16, flags=L.EPI_BIAS, tile_n=160, splitk=2, partial=part)
    hip.prof_begin()
    o = launch(hip, xd, w9d, bd, shape, F16, flags=L.EPI_BIAS | L.TUNE_UPS_FOLD, tile_n=160, splitk=2, partial=part)
    assert [r[0] for r in hip.prof_end()] == ["igemm_dma_kernel<128, 160, true, false, 0>", "splitk_finish_kernel"]
    assert torch.equal(o.view(torch.int16), sk.view(torch.int16))
    with pytest.raises(ValueError):                                  # a residual with a registered fold is refused, not launched
        out = hip.zeros(shape, F16)
        hip.igemm(xd, w9d, out, bias=bd, residual=hip.zeros(shape, F16), taps=9, ups=1, pad=1, tile_m=128, tile_n=160,
                  flags=L.EPI_BIAS | L.EPI_RESIDUAL | L.TUNE_UPS_FOLD)


def test_unet_plan_with_and_without_the_fold(hip):
    """The smallest UNet of tests/plan_cases.py whose upsample convs have whole 128-row phases, (B, side) = (2, 32): its
    8x8 -> 16x16 and 16x16 -> 32x32 sites, which the planner's rules would run split-K on the gather at this size, are put on
    the fold through the tile table's own hook.  eps with the fold agrees with eps without it within the tolerance
    test_gpu_parity.py::test_unet_call_matches_oracle applies to a UNet call, and the fold kernel is among the launches."""
    sd, _ = plan_cases.state_dicts()
    b, side = 2, 32
    g = torch.Generator().manual_seed(7)
    x, cond, t = torch.randn(b, 4, side, side, generator=g), torch.randn(b, 48, 768, generator=g) * 0.5, torch.tensor([999, 261])
    dev = hip.device
    over = {E.tiling_key(b * 16 * 16, 1280, 4 * 1280, 9, False, False, 1, 1): (128, 160, 1, L.TUNE_UPS_FOLD),
            E.tiling_key(b * 32 * 32, 640, 4 * 640, 9, False, False, 1, 1): (128, 160, 1, L.TUNE_UPS_FOLD)}
    eps, cache = {}, {}                              # (one packing of the weights serves both plans)
    for on in (False, True):
        with plan_cases.policy(E, dict(UPS_FOLD=on, TILING_OVERRIDE=over)):
            plan = E.UNetPlan(hip, sd, b, side, wcache=cache)
        plan.forward(x.to(dev), t.to(dev), cond.to(dev), lam=3.0)                    # (conditioning projections, warm-up)
        hip.synchronize()
        hip.prof_begin()
        eps[on] = plan.forward(x.to(dev), t.to(dev), None, lam=3.0)
        hip.synchronize()
        names = [r[0] for r in hip.prof_end()]
        assert sum(FOLD_KERNEL in k for k in names) == (2 if on else 0), sorted(set(names))
        eps[on] = eps[on].cpu()
    err = (eps[True] - eps[False]).abs().max().item()
    print(f"\nUNetPlan({b}, {side}): max |eps(fold) - eps(gather)| = {err:.3e}, max |eps| = {eps[False].abs().max().item():.3e}")
    assert err < 1e-2 * max(1.0, eps[False].abs().max().item()), err
