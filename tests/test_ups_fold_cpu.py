"""The upsample-conv fold without a GPU: "nearest 2x upsample -> conv3x3" as four 2x2 phase convs on pre-summed weights
(``engine.fold_ups_weight``, DADD_TUNE_UPS_FOLD, csrc/igemm_ups_fold.hip).

  * algebra: in float64, with unrounded folded weights, the four phase convs scattered to (2y + py, 2x + px) equal
    conv3x3(nearest2x(x), pad 1) to 1e-12 relative, borders included;
  * rounding: the fold of a 16-bit weight equals round16(float64 sum of the 16-bit values) exactly - one rounding;
  * resolve: what ``dadd_conv_igemm_*`` decides for a descriptor with and without the folded pointer."""
import ctypes as C

import pytest
import torch

from progressive_stable_diffusion_amd import engine as E
from progressive_stable_diffusion_amd import lib as L
from progressive_stable_diffusion_amd.backend import fill_igemm_desc
from tests.ups_fold_reference import phase_conv, unfolded

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64


@pytest.mark.parametrize("b,hi,wi", [(2, 3, 5), (1, 1, 1)])
def test_phase_convs_equal_the_upsampled_conv(b, hi, wi):
    cin, n = 2, 3
    g = torch.Generator().manual_seed(11)
    x = torch.randn(b, hi, wi, cin, generator=g, dtype=F64)
    w9 = torch.randn(n, 9 * cin, generator=g, dtype=F64)
    w4 = E.fold_ups_weight(w9)
    assert w4.dtype == F64 and tuple(w4.shape) == (4, n, 4 * cin)
    got, ref = phase_conv(x, w4), unfolded(x, w9)
    assert tuple(got.shape) == (b, 2 * hi, 2 * wi, n)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_fold_rounds_once(dtype):
    n, cin = 5, 8
    g = torch.Generator().manual_seed(12)
    w9 = (torch.randn(n, 9 * cin, generator=g) * 0.7).to(dtype)
    w4 = E.fold_ups_weight(w9)
    assert w4.dtype == dtype and w4.is_contiguous()
    w = w9.to(F64).reshape(n, 3, 3, cin)
    rows = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}       # (parity, d) -> the ky (kx) that land there
    want = torch.zeros(4, n, 2, 2, cin, dtype=F64)
    for py in range(2):
        for px in range(2):
            for dy in range(2):
                for dx in range(2):
                    for ky in rows[(py, dy)]:
                        for kx in rows[(px, dx)]:
                            want[2 * py + px, :, dy, dx] += w[:, ky, kx]
    assert torch.equal(w4, want.reshape(4, n, 4 * cin).to(dtype))
    # the sums are exact in float64, so a second rounding would show: most two- and four-term sums are no 16-bit numbers
    assert not torch.equal(want.reshape(4, n, 4 * cin).to(dtype).to(F64), want.reshape(4, n, 4 * cin))


# ---- resolve ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    L.build()
    return L.load()


def _t(shape, dtype=F16):
    return torch.zeros(shape, dtype=dtype)


def _ptr(t):
    return None if t is None else t.data_ptr()


def resolve(lib, sfx, x, w, out, **kw):
    d, c = L.IgemmDesc(), L.IgemmChoice()
    fill_igemm_desc(d, _ptr, x, w, out, **kw)
    L.check(getattr(lib, "dadd_conv_igemm_resolve_" + sfx)(C.byref(d), E.N_CU, C.byref(c)))
    return {f: (v.decode() if isinstance(v := getattr(c, f), bytes) else v) for f, _ in L.IgemmChoice._fields_}


def _site(b, hi, wi, cin, n):
    return _t((b, hi, wi, cin)), _t((n, 9 * cin)), _t((b, 2 * hi, 2 * wi, n)), _t((4, n, 4 * cin))


@pytest.mark.parametrize("tile_n", [160, 128])
def test_resolve_takes_the_fold(lib, tile_n):
    cin, n = 128, 640
    x, w9, o, w4 = _site(2, 16, 16, cin, n)
    kw = dict(taps=9, ups=1, pad=1, flags=L.EPI_BIAS | L.TUNE_UPS_FOLD, bias=_t((n,), F32), tile_m=128, tile_n=tile_n)
    c = resolve(lib, "f16", x, w9, o, w_fold=w4, **kw)
    assert c["kernel"] == f"igemm_ups_fold_kernel<128, {tile_n}>" and c["finish"] is None
    assert (c["nsplit"], c["grid_y"], c["persistent"]) == (1, 1, 0)
    assert c["kps"] * 64 == 4 * cin                                       # K = 4 Cin
    assert c["grid_x"] == (2 * 32 * 32 // 128) * -(-n // tile_n)          # four phases of B Hi Wi / 128 row tiles each
    twin = resolve(lib, "bf16", x, w9, o, w_fold=w4, **kw)
    assert twin["kernel"] == f"igemm_ups_fold_kernel_bf16<128, {tile_n}>"
    assert {k: v for k, v in twin.items() if k != "kernel"} == {k: v for k, v in c.items() if k != "kernel"}


def test_resolve_falls_back_to_the_gather(lib):
    cin, n = 128, 640
    x, w9, o, w4 = _site(2, 16, 16, cin, n)
    kw = dict(taps=9, ups=1, pad=1, tile_m=128, tile_n=160)
    plain = resolve(lib, "f16", x, w9, o, **kw)
    assert plain["kernel"] == "igemm_dma_kernel<128, 160, true, false, 0>" and plain["kps"] * 64 == 9 * cin
    # the flag without a folded pointer
    assert resolve(lib, "f16", x, w9, o, flags=L.TUNE_UPS_FOLD, **kw) == plain
    # split-K stays on the gather and its finish kernel
    part = _t((2 * 2 * 32 * 32 * n,), F32)
    sk = resolve(lib, "f16", x, w9, o, splitk=2, partial=part, **kw)
    assert sk["finish"] == "splitk_finish_kernel" and sk["nsplit"] == 2
    assert resolve(lib, "f16", x, w9, o, flags=L.TUNE_UPS_FOLD, w_fold=w4, splitk=2, partial=part, **kw) == sk
    # a phase that is no whole number of 128-row tiles (3 x 8 x 8 = 192 rows): the gather
    x3, w3, o3, f3 = _site(3, 8, 8, cin, n)
    assert resolve(lib, "f16", x3, w3, o3, flags=L.TUNE_UPS_FOLD, w_fold=f3, **kw) == resolve(lib, "f16", x3, w3, o3, **kw)
    # ... and one more sample makes it whole
    x4, w4b, o4, f4 = _site(4, 8, 8, cin, n)
    assert resolve(lib, "f16", x4, w4b, o4, flags=L.TUNE_UPS_FOLD, w_fold=f4, **kw)["kernel"] == "igemm_ups_fold_kernel<128, 160>"
    # 64-row tiles and the register-staged kernel have no fold
    assert resolve(lib, "f16", x, w9, o, flags=L.TUNE_UPS_FOLD | L.TUNE_NODMA, w_fold=w4, taps=9, ups=1, pad=1, tile_m=128,
                   tile_n=160)["kernel"].startswith("igemm_kernel<")


def test_resolve_refuses_operands_the_fold_does_not_take(lib):
    cin, n = 128, 640
    x, w9, o, w4 = _site(2, 16, 16, cin, n)
    kw = dict(taps=9, ups=1, pad=1, tile_m=128, tile_n=160, w_fold=w4)
    resolve(lib, "f16", x, w9, o, flags=L.TUNE_UPS_FOLD, **kw)
    with pytest.raises(ValueError):                            # a residual is read by output row: not in phase order
        resolve(lib, "f16", x, w9, o, flags=L.TUNE_UPS_FOLD | L.EPI_RESIDUAL, residual=_t(tuple(o.shape)), **kw)
    with pytest.raises(ValueError):                            # ... nor a time-embedding row
        resolve(lib, "f16", x, w9, o, flags=L.TUNE_UPS_FOLD | L.EPI_ROWVEC, rowvec=_t((2, n), F32), **kw)
    with pytest.raises(ValueError):                            # one source only
        resolve(lib, "f16", x, _t((n, 18 * cin)), o, x2=x, flags=L.TUNE_UPS_FOLD, taps=9, ups=1, pad=1, tile_m=128, tile_n=160,
                w_fold=_t((4, n, 8 * cin)))


def test_engine_requests_the_fold_where_the_gather_needs_no_split_k():
    assert E.UPS_FOLD is True
    assert E.ups_fold_tiling(4096, 1280, 1280) == (128, 160, 1, L.TUNE_UPS_FOLD)
    assert E.ups_fold_tiling(16384, 640, 640) == (128, 160, 1, L.TUNE_UPS_FOLD)
    assert E.ups_fold_tiling(1024, 1280, 1280) is None         # 8x8 -> 16x16: split-K on the gather
    assert E.ups_fold_tiling(3 * 16 * 16, 1280, 1280) is None  # 192 rows per phase
