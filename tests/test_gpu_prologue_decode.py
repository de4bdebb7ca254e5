"""-m gpu: the division-free prologue of the implicit-GEMM kernels (csrc/fastdiv.h, igemm_args.h row_decode /
tile_decode, the K cursor of igemm_dma.hip) against TorchRefBackend at the tolerance of test_igemm_conv3x3.

Output row -> (sample, y, x) is decoded by multiply and shift, a linear layer skips the decode, and the tap mask is
built from row and column bits; a wrong quotient moves a whole row of the gather, so errors are gross.  Shapes:
Ho * Wo = 144 makes the 64- and 128-row tiles straddle samples (B = 3: 432 rows, ragged last tile); the same map is
reached by a stride-2 3x3 from 24x24 and by the 2x nearest upsample from 6x6; a 1x1 over a skip-concat and a linear
with M = 200 take the decode-free path; split-K 2 starts the second slice's cursor at K tile 5 of 9 (tap 5).  Every
case runs on the LDS-DMA kernels (64- and 128-row tiles) and on the register-staged kernel (TUNE_NODMA).
"""
import math

import pytest
import torch

from tests.torch_backend import TorchRefBackend

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
REF = TorchRefBackend()
KERNELS = [(64, 0), (128, 0), (64, 32), (128, 32)]      # (tile_m, tune): 32 = TUNE_NODMA


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(torch.device("cuda:0"))


def rnd(shape, seed, scale=1.0, dtype=F16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def close(got, ref, atol, rtol, what=""):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())}/{bad.numel()} off, max err "
                                 f"{err.max().item():.4e} at ref {ref.flatten()[err.argmax()].item():.4e}")


def case(name):
    """(x, x2, w, output shape, tensors, keyword arguments) of one problem."""
    b, c, n = 3, 64, 64
    if name in ("conv", "conv_splitk"):
        hi, ho, kw = 12, 12, dict(taps=9, pad=1)
    elif name == "stride2":
        hi, ho, kw = 24, 12, dict(taps=9, pad=1, stride=2)
    elif name == "upsample":
        hi, ho, kw = 6, 12, dict(taps=9, pad=1, ups=1)
    elif name == "concat1x1":
        hi, ho, kw = 12, 12, dict()
    else:                                  # linear, M = 200
        x, w = rnd((1, 200, 1, 256), 1), rnd((136, 256), 2, 1 / 16.0)
        return x, None, w, (1, 200, 1, 136), dict(bias=rnd((136,), 3, 0.1, F32)), dict(flags=1)
    x = rnd((b, hi, hi, c), 4)
    x2 = rnd((b, hi, hi, 128), 5) if name == "concat1x1" else None
    k = kw.get("taps", 1) * (c + (128 if x2 is not None else 0))
    w = rnd((n, k), 6, 1 / math.sqrt(k))
    t = dict(bias=rnd((n,), 7, 0.1, F32), rowvec=rnd((b, n), 8, 0.3, F32), residual=rnd((b, ho, ho, n), 9))
    return x, x2, w, (b, ho, ho, n), t, dict(flags=7, **kw)


_REFS = {}


def reference(name):
    if name not in _REFS:                  # computed once per problem, shared by every kernel that runs it
        x, x2, w, shape, t, kw = case(name)
        ref = torch.zeros(shape, dtype=F16)
        REF.igemm(x, w, ref, x2=x2, **t, **kw)
        _REFS[name] = ref
    return _REFS[name]


@pytest.mark.parametrize("tile_m,tune", KERNELS)
@pytest.mark.parametrize("name", ["conv", "stride2", "upsample", "concat1x1", "linear"])
def test_gather_decode(hip, name, tile_m, tune):
    x, x2, w, shape, t, kw = case(name)
    kw = dict(kw, flags=kw["flags"] | tune)
    o = hip.zeros(shape, F16)
    hip.igemm(hip.to_device(x), hip.to_device(w), o, x2=None if x2 is None else hip.to_device(x2),
              **{k: hip.to_device(v) for k, v in t.items()}, tile_m=tile_m, **kw)
    hip.synchronize()
    close(o, reference(name), 3e-3, 2e-3, f"{name} tile_m {tile_m} tune {tune}")


@pytest.mark.parametrize("tile_m,tune", KERNELS)
@pytest.mark.parametrize("in_launch", [True, False])
def test_split_k_cursor_starts_inside_the_taps(hip, tile_m, tune, in_launch):
    """Split-K 2 over the nine K tiles of the 3x3: the second slice starts at K tile 5 (tap 5, ky = 1, kx = 2); slabs
    combined by the last arriver (tickets) or by the finish kernel."""
    x, x2, w, shape, t, kw = case("conv_splitk")
    kw = dict(kw, flags=kw["flags"] | tune)
    m = shape[0] * shape[1] * shape[2]
    o = hip.zeros(shape, F16)
    partial = hip.zeros((2 * m * w.shape[0],), F32)
    counters = hip.zeros((4096,), torch.int32) if in_launch else None
    hip.igemm(hip.to_device(x), hip.to_device(w), o, **{k: hip.to_device(v) for k, v in t.items()}, tile_m=tile_m,
              splitk=2, partial=partial, counters=counters, **kw)
    hip.synchronize()
    close(o, reference("conv_splitk"), 3e-3, 2e-3, f"split-K 2 tile_m {tile_m} tune {tune} in_launch {in_launch}")
    if counters is not None:
        assert int(counters.abs().sum().item()) == 0, "split-K tickets not reset"
