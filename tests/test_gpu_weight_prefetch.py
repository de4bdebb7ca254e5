"""-m gpu: the run-ahead weight prefetch of the LDS-DMA kernels (csrc/igemm_args.h dadd_pf_*, igemm_dma.hip,
conv_halo.hip).  Before their first barrier the MFMA waves touch the first K tiles of the weight strip, one dword per
128-byte line, and throw the loads away; the row-tile workgroups that share a strip deal its lines between them, and
dadd_igemm_resolve turns the prefetch on in igemm_dma.hip where at least sixteen of them do (M >= 16 row tiles) and the
ring is not the persistent one.  The halo conv measured no gain and has none.  A prefetch changes no arithmetic, so what can go wrong is the ring's wait accounting (a tile read
before it has landed gives grossly wrong values, and not the same ones twice) or an address that runs off the strip
(rows past N, K tiles past a short split-K slice).  Cases marked "off" run launches the rule leaves without prefetch:
they pin that those kernels are untouched.

Every case is one ``HipBackend.igemm`` launch audited by ``tests/launch_audit.py`` — the ``TorchRefBackend`` references
at the bound or ``TOL`` entry that module holds for the kind of launch — and then launched a second time into a fresh
output, which must be bit-equal.  Shapes are the smallest that reach each path: K tiles above and below the ring depth of
four, two workgroups per CU on the 64x64 tiles, a last column tile that is partly empty (N = 192 on 128-column tiles:
the row clamp), split-K slices whose last one is short (45 K tiles in slices of 7 -> 3 left; in slices of 4 -> 1 left,
below the ring depth), the persistent ring over more tiles than CUs, the three ways a folded LayerNorm gets its
statistics, the 2x-upsample gather, and the halo conv with and without GroupNorm on the way in and with the
GroupNorm-applying finish kernel.
"""
import math

import pytest
import torch

from tests import launch_audit as LA

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DEV = "cuda:0"
BIAS, RESIDUAL, GEGLU, PERSIST = 1, 4, 8, 64


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(torch.device(DEV))


def rnd(shape, seed, scale=1.0, dtype=F16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def chunk_partials(x, nch):
    """[B][nch][32][2] fp32 (sum, sum of squares) of an NHWC tensor: what a producer's GroupNorm-statistics epilogue writes."""
    b, c = x.shape[0], x.shape[-1]
    xc = x.float().reshape(b, nch, -1, 32, c // 32)
    return torch.stack([xc.sum(dim=(2, 4)), (xc * xc).sum(dim=(2, 4))], dim=-1).contiguous().reshape(-1)


def row_partials(x, parts):
    """[parts][M][2] fp32 (sum, sum of squares) over column blocks of the rows: a producer's LayerNorm-statistics epilogue."""
    xr = x.float().reshape(-1, parts, x.shape[-1] // parts)
    return torch.stack([xr.sum(dim=-1), (xr * xr).sum(dim=-1)], dim=-1).permute(1, 0, 2).contiguous()


def check(hip, x, w, shape, dtype=F16, fresh=None, **kw):
    """One audited launch, then the same launch again: inside the audit's criteria, and bit-equal run to run.
    ``fresh``: builders of the per-launch workspaces / side outputs, name -> callable."""
    be, fresh = LA.backend(hip, DEV), fresh or {}
    xd, wd = hip.to_device(x), hip.to_device(w)
    kw = {k: (hip.to_device(v) if isinstance(v, torch.Tensor) and not v.is_cuda else v) for k, v in kw.items()}
    outs = []
    for run in (be, hip):
        o = hip.zeros(shape, dtype)
        extra = {k: f() for k, f in fresh.items()}
        run.igemm(xd, wd, o, **kw, **extra)
        hip.synchronize()
        outs.append((o, extra))
    be.assert_clean()
    assert be.launches == 1
    assert torch.equal(outs[0][0], outs[1][0]), "two launches of the same problem differ"
    for k in fresh:
        if k == "gn_apply":
            assert torch.equal(outs[0][1][k][0], outs[1][1][k][0]), "normalised outputs of two launches differ"


def fold(n, k, seed, geglu=False):
    """A LayerNorm folded into a linear: (gamma o W, c1, composed bias), GEGLU rows interleaved."""
    from progressive_stable_diffusion_amd import engine as E
    g = torch.Generator().manual_seed(seed)
    w, b = torch.randn(n, k, generator=g) / math.sqrt(k), torch.randn(n, generator=g) * 0.1
    gamma, beta = 1.0 + 0.2 * torch.randn(k, generator=g), 0.2 * torch.randn(k, generator=g)
    w16, c1, bias = E.fold_layernorm(w, b, gamma, beta)
    if geglu:
        idx = E.geglu_interleave(torch.arange(n)[:, None].float(), torch.zeros(n))[0][:, 0].long()
        w16, c1, bias = w16[idx], c1[idx], bias[idx]
    return w16.contiguous(), c1.contiguous(), bias.contiguous()


@pytest.mark.parametrize("b,side,c,n,tile_m,tile_n,dtype", [
    (1, 32, 640, 640, 64, 160, F16),   # 10 K tiles: above the ring depth, all of them prefetched
    (1, 32, 640, 640, 64, 160, BF16),  # ... and its bf16 twin
    (1, 32, 320, 320, 64, 160, F16),   # 5 K tiles
    (4, 16, 1280, 1280, 64, 64, F16),  # 20 K tiles (more than are prefetched), two workgroups per CU
    (4, 32, 320, 192, 128, 128, F16),  # N = 192: the second column tile holds 64 rows of weights and 64 rows of nothing
    (1, 16, 320, 192, 128, 128, F16),  # ... with two row tiles: off
])
def test_plain_linear(hip, b, side, c, n, tile_m, tile_n, dtype):
    x, w = rnd((b, side, side, c), 1, dtype=dtype), rnd((n, c), 2, 1 / math.sqrt(c), dtype)
    check(hip, x, w, (b, side, side, n), dtype, bias=rnd((n,), 3, 0.1, F32), flags=BIAS, tile_m=tile_m, tile_n=tile_n)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("splitk,last", [(7, 3), (12, 1)])
def test_split_k_with_a_short_last_slice(hip, splitk, last, stride):
    """3x3, 320 -> 320: 45 K tiles.  Slices of 7 leave 3 for the last one, slices of 4 leave 1; the prefetch of the last
    slice must stop at the end of K, the others at the end of their slice.  B = 4 on the 8x8 map is two row tiles (off);
    the stride-2 conv 64x64 -> 32x32 is 32, each taking every 32nd line of its slice's strip."""
    b, side, c, n = 4, 8 if stride == 1 else 32, 320, 320
    nkt = 9 * c // 64
    kps = -(-nkt // splitk)
    assert nkt - (-(-nkt // kps) - 1) * kps == last
    x, w = rnd((b, side * stride, side * stride, c), 4), rnd((n, 9 * c), 5, 1 / math.sqrt(9 * c))
    m = b * side * side
    check(hip, x, w, (b, side, side, n), bias=rnd((n,), 6, 0.1, F32), residual=rnd((b, side, side, n), 7),
          flags=BIAS | RESIDUAL, taps=9, pad=1, stride=stride, tile_m=128, tile_n=160, splitk=splitk,
          fresh=dict(partial=lambda: hip.zeros((splitk * m * n,), F32)))


@pytest.mark.parametrize("ln", [False, True])
def test_persistent_geglu(hip, ln):
    """B = 4, 32x32, 320 -> 2560 interleaved: 32 x 20 = 640 tiles of 128 x 128 over the workgroups of the persistent ring
    (off: its workgroups walk runs of tiles), plain and with the LayerNorm fold from the producer's row partials staged
    in LDS (LNK = 2)."""
    from progressive_stable_diffusion_amd import lib as L
    from progressive_stable_diffusion_amd.engine import geglu_interleave
    b, side, c, n = 4, 32, 320, 2560
    x = (rnd((b, side, side, c), 8).float() + 2.0 * rnd((b, side, side, 1), 9).float()).to(F16)
    if ln:
        w, c1, bias = fold(n, c, 10, geglu=True)
        kw = dict(flags=BIAS | GEGLU | PERSIST | L.EPI_LNFOLD, ln_c1=c1, ln_stats_in=row_partials(x, 4))
    else:
        w32, bias = geglu_interleave(rnd((n, c), 10, 1 / math.sqrt(c), F32), rnd((n,), 11, 0.1, F32))
        w, kw = w32.to(F16), dict(flags=BIAS | GEGLU | PERSIST)
    check(hip, x, w, (b, side, side, n // 2), bias=bias, tile_m=128, tile_n=128, **kw)


def test_layernorm_fold_summed_in_the_loop(hip):
    """64-row tiles, the MFMA waves sum the rows of their A fragments (LNK = 1): B = 1, 32x32, 640 -> 640."""
    from progressive_stable_diffusion_amd import lib as L
    b, side, c, n = 1, 32, 640, 640
    x = (rnd((b, side, side, c), 12).float() + 2.0 * rnd((b, side, side, 1), 13).float()).to(F16)
    w, c1, bias = fold(n, c, 14)
    check(hip, x, w, (b, side, side, n), bias=bias, flags=BIAS | L.EPI_LNFOLD, ln_c1=c1, tile_m=64, tile_n=160)


@pytest.mark.parametrize("b,side", [(2, 8), (2, 16)])
def test_upsample_conv(hip, b, side):
    """2x nearest upsample + 3x3, 320 -> 320 (45 K tiles, the gather of the 128-row upsample kernel): 8x8 -> 16x16 with four
    row tiles (off) and 16x16 -> 32x32 with sixteen."""
    c, n = 320, 320
    x, w = rnd((b, side, side, c), 15), rnd((n, 9 * c), 16, 1 / math.sqrt(9 * c))
    check(hip, x, w, (b, 2 * side, 2 * side, n), bias=rnd((n,), 17, 0.1, F32), flags=BIAS, taps=9, pad=1, ups=1, tile_m=128, tile_n=160)


@pytest.mark.parametrize("b,side,gn_in,dtype", [(1, 16, False, F16), (1, 16, True, F16), (1, 32, False, F16), (1, 32, True, F16),
                                                (1, 16, False, BF16)])
def test_halo_conv(hip, b, side, gn_in, dtype):
    """3x3 / stride 1 on a 16- and a 32-wide map, B = 1, 320 -> 320: five channel chunks = 45 weight tiles, two column
    tiles, with and without GroupNorm (+ SiLU) on the way in.  Off: the halo conv carries the new argument and nothing
    else."""
    from progressive_stable_diffusion_amd import lib as L
    c, n = 320, 320
    x = (rnd((b, side, side, c), 18).float() * 1.7 + 0.6).to(dtype)
    w = rnd((n, 9 * c), 19, 1 / math.sqrt(9 * c), dtype)
    kw = dict(bias=rnd((n,), 20, 0.1, F32), flags=BIAS, taps=9, pad=1, tile_m=128, tile_n=160)
    if gn_in:
        nch = side * side // 64
        kw.update(flags=BIAS | L.PRE_GN | L.PRE_GN_SILU,
                  gn_in=(hip.to_device(chunk_partials(x, nch)), nch, hip.to_device(rnd((c,), 21, 0.2, F32) + 1.0),
                         hip.to_device(rnd((c,), 22, 0.2, F32)), 1e-5))
    check(hip, x, w, (b, side, side, n), dtype, **kw)


def test_halo_conv_split_k_with_groupnorm_finish(hip):
    """The halo conv split over its channel chunks (5 chunks in slices of 3 and 2), combined by the finish kernel that
    also writes GroupNorm + SiLU of the output.  Off, as every halo conv."""
    from progressive_stable_diffusion_amd import lib as L
    b, side, c, n, sk = 1, 16, 320, 320, 2
    x, w = rnd((b, side, side, c), 23), rnd((n, 9 * c), 24, 1 / math.sqrt(9 * c))
    gamma, beta = hip.to_device(rnd((n,), 25, 0.1, F32) + 1.0), hip.to_device(rnd((n,), 26, 0.1, F32))
    check(hip, x, w, (b, side, side, n), bias=rnd((n,), 27, 0.1, F32), flags=BIAS | L.EPI_GNAPPLY | L.EPI_GNAPPLY_SILU,
          taps=9, pad=1, tile_m=128, tile_n=160, splitk=sk,
          fresh=dict(partial=lambda: hip.zeros((sk * b * side * side * n,), F32),
                     gn_apply=lambda: (hip.zeros((b, side, side, n), F16), gamma, beta, 1e-5)))
