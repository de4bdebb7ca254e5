"""-m gpu: the bf16 operand mode (csrc/*_bf16.hip, ``UNetPlan(dtype=torch.bfloat16)``,
``DiffusionModuleWithIP(operand_dtype=torch.bfloat16)``).

Per kernel: the _bf16 entry point against the fp32 torch reference of the same op (tests/torch_backend.py) on the same
bf16-rounded inputs, rounded once to bf16: the expected difference is one bf16 rounding of the result (rel 2^-9) plus
accumulation-order noise, so the bounds are 8x the fp16 ones of test_gpu_kernels.py.  Whole UNet / per sampler step:
max|eps_bf16 - eps_oracle| <= 4e-2 * max|eps| (fp16 holds 1e-2); the measured values are printed.
"""
import math

import pytest
import torch

from oracle import sampler as OS
from oracle.sd_unet import unet_forward
from tests import golden_inputs as GI
from tests.torch_backend import TorchRefBackend

pytestmark = pytest.mark.gpu

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DEV = torch.device("cuda:0")
REF = TorchRefBackend()


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(DEV)


def rnd(shape, seed, scale=1.0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def dev(hip, t):
    return None if t is None else hip.to_device(t)


def close(got, ref, atol, rtol, what=""):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {err.max().item():.4e} "
                                 f"at ref {ref.flatten()[err.argmax()].item():.4e}")


def igemm_pair(hip, x, w, out_shape, splitk=1, **kw):
    """(HIP bf16 result, reference) of one igemm launch."""
    tens = {k: kw.pop(k, None) for k in ("x2", "bias", "rowvec", "residual", "ln_c1")}
    o_ref = torch.zeros(out_shape, dtype=BF)
    REF.igemm(x, w, o_ref, splitk=splitk, **tens, **kw)
    o = hip.zeros(out_shape, BF)
    m = out_shape[0] * out_shape[1] * out_shape[2]
    partial = hip.zeros((splitk * m * w.shape[0],), F32) if splitk > 1 else None
    hip.igemm(dev(hip, x), dev(hip, w), o, splitk=splitk, partial=partial, **{k: dev(hip, v) for k, v in tens.items()}, **kw)
    hip.synchronize()
    return o, o_ref


# ------------------------------------------------------------------------------------------------ GEMM / conv
GEMM_CASES = {   # name: (x shape, N, taps, stride, ups, pad, flags, splitk, tile_m, tile_n, x2 channels)
    "linear_bias_res_dma128x160": ((2, 16, 16, 320), 320, 1, 1, 0, 0, 5, 1, 128, 160, 0),
    "linear_dma64x128": ((1, 8, 8, 640), 1280, 1, 1, 0, 0, 1, 1, 64, 128, 0),
    "linear_dma64x64": ((2, 4, 4, 1280), 640, 1, 1, 0, 0, 1, 1, 64, 64, 0),
    "linear_regstaged": ((2, 16, 16, 320), 320, 1, 1, 0, 0, 5 | 32, 1, 64, 160, 0),
    "linear_persist_ring": ((2, 32, 32, 320), 960, 1, 1, 0, 0, 1 | 64, 1, 128, 160, 0),
    "conv3x3_rowvec_res_dma": ((2, 12, 12, 320), 640, 9, 1, 0, 1, 7, 1, 128, 128, 0),
    "conv3x3_stride2": ((2, 16, 16, 320), 320, 9, 2, 0, 1, 1, 1, 128, 160, 0),
    "conv3x3_upsample": ((2, 8, 8, 640), 640, 9, 1, 1, 1, 1, 1, 128, 160, 0),
    "conv3x3_skip_concat": ((2, 8, 8, 640), 640, 9, 1, 0, 1, 7, 1, 128, 160, 640),
    "conv1x1_skip_concat": ((2, 8, 8, 640), 320, 1, 1, 0, 0, 1, 1, 128, 160, 320),
    "splitk_finish": ((2, 8, 8, 1280), 1280, 9, 1, 0, 1, 7, 8, 128, 160, 0),
    "splitk_finish_linear": ((2, 4, 4, 1280), 1280, 1, 1, 0, 0, 5, 3, 128, 160, 0),
    "geglu": ((2, 16, 16, 320), 2560, 1, 1, 0, 0, 1 | 8, 1, 128, 128, 0),
    "geglu_regstaged": ((2, 16, 16, 320), 2560, 1, 1, 0, 0, 1 | 8 | 32 | 16, 1, 64, 128, 0),
}


@pytest.mark.parametrize("case", sorted(GEMM_CASES))
def test_igemm_bf16(hip, case):
    shape, n, taps, stride, ups, pad, flags, sk, tm, tn, c2 = GEMM_CASES[case]
    b, h, w_, c1 = shape
    x = rnd(shape, 1)
    x2 = rnd((b, h, w_, c2), 2) if c2 else None
    k = taps * (c1 + c2)
    w = rnd((n, k), 3, 1 / math.sqrt(k))
    if flags & 8:
        from progressive_stable_diffusion_amd.engine import geglu_interleave
        w = geglu_interleave(w.float(), torch.zeros(n))[0].to(BF)
    ho = (h * (2 if ups else 1)) // stride
    nout = n // 2 if flags & 8 else n
    out_shape = (b, ho, ho if w_ == h else w_, nout)
    kw = dict(x2=x2, taps=taps, stride=stride, ups=ups, pad=pad, flags=flags, tile_m=tm, tile_n=tn)
    kw["bias"] = rnd((n,), 4, 0.1, F32)
    if flags & 2:
        kw["rowvec"] = rnd((b, n), 5, 0.3, F32)
    if flags & 4:
        kw["residual"] = rnd(out_shape, 6)
    o, o_ref = igemm_pair(hip, x, w, out_shape, splitk=sk, **kw)
    close(o, o_ref, 2e-2, 1.6e-2, case)


@pytest.mark.parametrize("tile_m,tile_n,geglu", [(64, 160, False), (128, 160, False), (128, 128, True)])
def test_igemm_bf16_layernorm_fold_and_statistics(hip, tile_m, tile_n, geglu):
    """EPI_LNFOLD from the A fragments and from a producer's EPI_LNSTAT partials."""
    from progressive_stable_diffusion_amd import engine as E
    from progressive_stable_diffusion_amd import lib as L
    b, h, c = 2, 16, 320
    n = 2560 if geglu else 960
    x = (rnd((b, h, h, c), 7).float() * 1.5 + 0.4).to(BF)
    w, bias = torch.randn(n, c) / math.sqrt(c), torch.randn(n) * 0.1
    gamma, beta = torch.rand(c) + 0.5, torch.randn(c) * 0.2
    w16, c1, bb = E.fold_layernorm(w, bias, gamma, beta, BF)
    if geglu:
        w16, bb = E.geglu_interleave(w16.float(), bb)
        w16 = w16.to(BF)
        c1 = w16.double().sum(dim=1).float()
    fl = L.EPI_BIAS | L.EPI_LNFOLD | (L.EPI_GEGLU if geglu else 0)
    out_shape = (b, h, h, n // 2 if geglu else n)
    o, o_ref = igemm_pair(hip, x, w16, out_shape, flags=fl, bias=bb, ln_c1=c1, tile_m=tile_m, tile_n=tile_n)
    close(o, o_ref, 3e-2, 2e-2, f"lnfold {tile_m}x{tile_n} geglu={geglu}")
    # the partials written by a producer (EPI_LNSTAT) instead of the consumer's own sums
    wp = rnd((c, c), 8, 1 / math.sqrt(c))
    xp = hip.zeros((b, h, h, c), BF)
    st = hip.zeros((c // 80, b * h * h, 2), F32)
    hip.igemm(dev(hip, x), dev(hip, wp), xp, flags=L.EPI_LNSTAT, ln_stats_out=st, tile_m=128, tile_n=160)
    o2 = hip.zeros(out_shape, BF)
    hip.igemm(xp, dev(hip, w16), o2, flags=fl, bias=dev(hip, bb), ln_c1=dev(hip, c1), ln_stats_in=st, tile_m=tile_m,
              tile_n=tile_n)
    o3 = hip.zeros(out_shape, BF)
    hip.igemm(xp, dev(hip, w16), o3, flags=fl, bias=dev(hip, bb), ln_c1=dev(hip, c1), tile_m=tile_m, tile_n=tile_n)
    hip.synchronize()
    close(o2, o3, 3e-2, 2e-2, "lnstat partials vs own sums")


@pytest.mark.parametrize("h", [16, 32, 64])
@pytest.mark.parametrize("pre_gn", [False, True])
def test_halo_conv_bf16(hip, h, pre_gn):
    """conv3x3_halo_kernel_bf16 on 16 / 32 / 64-pixel rows, with and without GroupNorm + SiLU on the loader waves, and
    the GroupNorm statistics of its output (EPI_GNSTAT)."""
    from progressive_stable_diffusion_amd import lib as L
    b, c, n = 2, 320, 320
    x = (rnd((b, h, h, c), 9).float() * 1.7 + 0.6).to(BF)
    w = rnd((n, 9 * c), 10, 1 / math.sqrt(9 * c))
    bias, rowvec, res = rnd((n,), 11, 0.1, F32), rnd((b, n), 12, 0.3, F32), rnd((b, h, h, n), 13)
    gamma, beta = rnd((c,), 14, 0.2, F32) + 1.0, rnd((c,), 15, 0.2, F32)
    nch = max(1, min(128, h * h // 64))
    xc = x.float().reshape(b, nch, -1, 32, c // 32)
    part = torch.stack([xc.sum(dim=(2, 4)), (xc * xc).sum(dim=(2, 4))], dim=-1).contiguous().reshape(-1)
    xin = x
    if pre_gn:
        xin = torch.zeros_like(x)
        REF.groupnorm(x, None, gamma, beta, xin, part, 32, 1e-5, 1, ws_chunks=nch)
    o_ref = torch.zeros(b, h, h, n, dtype=BF)
    REF.igemm(xin, w, o_ref, bias=bias, rowvec=rowvec, residual=res, taps=9, pad=1, flags=7)
    nch_o = h * h // 64
    ws_o = hip.zeros((b * nch_o * 64,), F32)
    fl = 7 | L.EPI_GNSTAT | ((L.PRE_GN | L.PRE_GN_SILU) if pre_gn else 0)
    kw = dict(gn_in=(dev(hip, part), nch, dev(hip, gamma), dev(hip, beta), 1e-5)) if pre_gn else {}
    o = hip.zeros((b, h, h, n), BF)
    hip.igemm(dev(hip, x), dev(hip, w), o, bias=dev(hip, bias), rowvec=dev(hip, rowvec), residual=dev(hip, res), taps=9,
              pad=1, flags=fl, tile_m=128, tile_n=160, gn_ws=ws_o, gn_nchunk=nch_o, **kw)
    hip.synchronize()
    close(o, o_ref, 3e-2 if pre_gn else 2e-2, 2e-2, f"halo {h} pre_gn={pre_gn}")
    of = o.float().cpu().reshape(b, nch_o, -1, 32, n // 32)
    want = torch.stack([of.sum(dim=(2, 4)), (of * of).sum(dim=(2, 4))], dim=-1).reshape(-1)
    close(ws_o, want, 1e-2, 1e-3, "GroupNorm partials of the output")


@pytest.mark.parametrize("case", ["conv8x8", "linear4x4"])
def test_splitk_finish_gn_and_gnapply_bf16(hip, case):
    """splitk_finish_gn_kernel_bf16 (GNSTAT under split-K) and splitk_finish_gnapply_kernel_bf16 (the finish writes
    GroupNorm + SiLU of its output), against the reference.  The GNAPPLY finish is bit-identical to finish +
    groupnorm_bf16, as in fp16; the GNSTAT finish sums the slices in its own order, so its outputs may differ from the
    plain finish by one bf16 rounding (measured: 2 of 327,680 elements)."""
    from progressive_stable_diffusion_amd import lib as L
    b, hw, cin, n, taps, sk, fl = (4, 8, 1280, 1280, 9, 9, 7) if case == "conv8x8" else (3, 4, 1280, 2560, 1, 3, 5)
    x, w = rnd((b, hw, hw, cin), 16), rnd((n, taps * cin), 17, 1 / math.sqrt(taps * cin))
    bias, rowvec, res = rnd((n,), 18, 0.1, F32), rnd((b, n), 19, 0.3, F32), rnd((b, hw, hw, n), 20)
    gamma, beta = rnd((n,), 21, 0.1, F32) + 1.0, rnd((n,), 22, 0.1, F32)
    kw = dict(bias=dev(hip, bias), taps=taps, pad=taps // 9, tile_m=128, tile_n=160 if n % 160 == 0 else 128, splitk=sk)
    if fl & 2:
        kw["rowvec"] = dev(hip, rowvec)
    if fl & 4:
        kw["residual"] = dev(hip, res)
    xd, wd = dev(hip, x), dev(hip, w)
    o1, o2, y1, y2 = (hip.zeros((b, hw, hw, n), BF) for _ in range(4))
    hip.igemm(xd, wd, o1, flags=fl, partial=hip.zeros((sk * b * hw * hw * n,), F32), **kw)
    hip.groupnorm(o1, None, dev(hip, gamma), dev(hip, beta), y1, hip.zeros((b * L.GN_MAX_CHUNKS * 64,), F32), 32, 1e-5, 1)
    hip.igemm(xd, wd, o2, flags=fl | L.EPI_GNAPPLY | L.EPI_GNAPPLY_SILU, partial=hip.zeros((sk * b * hw * hw * n,), F32),
              gn_apply=(y2, dev(hip, gamma), dev(hip, beta), 1e-5), **kw)
    hip.synchronize()
    o_ref, y_ref = torch.zeros(b, hw, hw, n, dtype=BF), torch.zeros(b, hw, hw, n, dtype=BF)
    REF.igemm(x, w, o_ref, flags=fl | L.EPI_GNAPPLY_SILU, bias=bias, rowvec=rowvec if fl & 2 else None,
              residual=res if fl & 4 else None, taps=taps, pad=taps // 9, gn_apply=(y_ref, gamma, beta, 1e-5))
    close(o2, o_ref, 2e-2, 1.6e-2, f"finish {case}")
    close(y2, y_ref, 4e-2, 3e-2, f"finish + GroupNorm {case}")
    assert torch.equal(o1.cpu(), o2.cpu()) and torch.equal(y1.cpu(), y2.cpu())
    if n % 160 == 0:                       # GNSTAT through the split-K finish (16-row chunks)
        nch = hw * hw // 16
        ws = hip.zeros((b * nch * 64,), F32)
        o3 = hip.zeros((b, hw, hw, n), BF)
        hip.igemm(xd, wd, o3, flags=fl | L.EPI_GNSTAT, partial=hip.zeros((sk * b * hw * hw * n,), F32), gn_ws=ws,
                  gn_nchunk=nch, **kw)
        hip.synchronize()
        close(o3, o1, 1e-3, 8e-3, "finish with GroupNorm statistics vs plain finish")
        of = o3.float().cpu().reshape(b, nch, -1, 32, n // 32)
        close(ws, torch.stack([of.sum(dim=(2, 4)), (of * of).sum(dim=(2, 4))], dim=-1).reshape(-1), 1e-2, 1e-3, "gnstat")


# ------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("c1,c2,hw,silu", [(320, 0, 256, 1), (640, 320, 64, 1), (1280, 0, 16, 0), (320, 0, 4096, 1)])
def test_groupnorm_bf16(hip, c1, c2, hw, silu):
    b, side = 2, int(math.isqrt(hw))
    x1 = (rnd((b, side, side, c1), 23, 1.5).float() + 0.3).to(BF)
    x2 = (rnd((b, side, side, c2), 24, 0.7).float() - 0.2).to(BF) if c2 else None
    c = c1 + c2
    gamma, beta = rnd((c,), 25, 0.2, F32) + 1.0, rnd((c,), 26, 0.2, F32)
    o_ref = torch.zeros(b, side, side, c, dtype=BF)
    REF.groupnorm(x1, x2, gamma, beta, o_ref, None, 32, 1e-5, silu)
    o = hip.zeros((b, side, side, c), BF)
    hip.groupnorm(dev(hip, x1), dev(hip, x2), dev(hip, gamma), dev(hip, beta), o, hip.zeros((b * 256 * 64,), F32), 32,
                  1e-5, silu)
    hip.synchronize()
    close(o, o_ref, 2e-2, 1.6e-2, f"groupnorm {c1}+{c2} hw{hw}")
    if c2 == 0 and hw >= 256:              # statistics from chunk partials (ws_chunks)
        nch = hw // 64
        xc = x1.float().reshape(b, nch, -1, 32, c // 32)
        part = torch.stack([xc.sum(dim=(2, 4)), (xc * xc).sum(dim=(2, 4))], dim=-1).reshape(-1)
        ws = hip.zeros((b * (nch + 64) * 64,), F32)
        hip.copy_(ws[:part.numel()], part)
        o2 = hip.zeros((b, side, side, c), BF)
        hip.groupnorm(dev(hip, x1), None, dev(hip, gamma), dev(hip, beta), o2, ws, 32, 1e-5, silu, ws_chunks=nch)
        hip.synchronize()
        close(o2, o_ref, 2e-2, 1.6e-2, "groupnorm from chunk partials")


@pytest.mark.parametrize("m,c", [(100, 320), (37, 640), (64, 1280)])
def test_layernorm_bf16(hip, m, c):
    x = (rnd((m, c), 27, 2.0).float() + 0.5).to(BF)
    gamma, beta = rnd((c,), 28, 0.2, F32) + 1.0, rnd((c,), 29, 0.2, F32)
    o_ref = torch.zeros(m, c, dtype=BF)
    REF.layernorm(x, gamma, beta, o_ref)
    o = hip.zeros((m, c), BF)
    hip.layernorm(dev(hip, x), dev(hip, gamma), dev(hip, beta), o)
    hip.synchronize()
    close(o, o_ref, 1.6e-2, 1.6e-2, f"layernorm {m}x{c}")


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("d", [40, 80, 160])
@pytest.mark.parametrize("n", [576, 144, 36, 9, 4096])
def test_self_attention_bf16(hip, d, n):
    """flash_kernel_bf16: ragged key counts of the 24x24 latent (576 / 144 / 36 / 9) and n = 4096.  At b = 2 the latter
    still runs the four-wave d = 40 kernel (2 * 8 * 16 = 256 < 512 workgroups); the eight-wave variant is compared in
    tests/test_gpu_attention_edges.py."""
    heads, b = 8, 2
    c = heads * d
    qkv = rnd((b, n, 3 * c), 30)
    qkv[0, n // 3, c:2 * c] *= 4.0
    o_ref = torch.zeros(b, n, c, dtype=BF)
    REF.self_attn(qkv, o_ref, heads)
    o = hip.zeros((b, n, c), BF)
    hip.self_attn(dev(hip, qkv), o, heads)
    hip.synchronize()
    close(o, o_ref, 2e-2, 2e-2, f"self_attn d{d} n{n}")


def test_attention_bf16_refuses_other_head_dims(hip):
    q = dev(hip, rnd((1, 16, 64), 31))
    with pytest.raises(ValueError):
        hip.attention(q, q, q, hip.zeros((1, 16, 64), BF), 1)


@pytest.mark.parametrize("d", [40, 80, 160])
@pytest.mark.parametrize("mode,lam", [(0, 0.0), (0, 3.0), (1, 0.0)])
def test_tri_xattn_bf16(hip, d, mode, lam):
    b, n, heads = 2, 300, 8
    c = heads * d
    t_tok, ld = (48, 4 * c) if mode == 0 else (32, 2 * c)
    q, kv = rnd((b, n, c), 32), rnd((b, t_tok, ld), 33)
    gates = torch.tensor([0.1, 0.9])
    o_ref = torch.zeros(b, n, c, dtype=BF)
    REF.tri_xattn(q, kv, o_ref, gates, lam, mode, heads)
    o = hip.zeros((b, n, c), BF)
    hip.tri_xattn(dev(hip, q), dev(hip, kv), o, dev(hip, gates) if mode == 0 else None, lam, mode, heads)
    hip.synchronize()
    close(o, o_ref, 2.5e-2, 2.5e-2, f"tri_xattn d{d} mode{mode} lam{lam}")
    if mode == 0 and lam == 0.0:           # lambda = 0 never reads the delta tokens (NaN there must not leak)
        kv2 = kv.clone()
        kv2[:, 32:] = float("nan")
        o2 = hip.zeros((b, n, c), BF)
        hip.tri_xattn(dev(hip, q), dev(hip, kv2), o2, dev(hip, gates), 0.0, 0, heads)
        o3 = hip.zeros((b, n, c), BF)
        hip.tri_xattn(dev(hip, q), dev(hip, kv2), o3, dev(hip, gates), 7.0, 0, heads, lam_dev=dev(hip, torch.zeros(1)))
        hip.synchronize()
        assert torch.equal(o2.cpu(), o.cpu()) and torch.equal(o3.cpu(), o.cpu())


# ------------------------------------------------------------------------------------------------ the UNet's ends
def test_conv_in_and_conv_out_bf16(hip):
    from progressive_stable_diffusion_amd import engine as E
    b, h = 2, 32
    x = torch.randn(b, 4, h, h, generator=torch.Generator().manual_seed(34))
    w_in = E.pack_conv_cin8(torch.randn(320, 4, 3, 3) * 0.2, BF)
    bias_in = torch.randn(320) * 0.1
    o = hip.zeros((b, h, h, 320), BF)
    nch = h * h // 256
    ws = hip.zeros((b * nch * 64,), F32)
    hip.conv_in_nchw(dev(hip, x), dev(hip, w_in), dev(hip, bias_in), o, ws, nch)
    x8 = torch.zeros(b, h, h, 8, dtype=BF)
    REF.pack_latents(x, x8)
    o_ref = torch.zeros(b, h, h, 320, dtype=BF)
    REF.conv_cin8(x8, w_in, bias_in, o_ref)
    hip.synchronize()
    close(o, o_ref, 1.6e-2, 1.6e-2, "conv_in_nchw")
    of = o.float().cpu().reshape(b, nch, -1, 32, 10)
    close(ws, torch.stack([of.sum(dim=(2, 4)), (of * of).sum(dim=(2, 4))], dim=-1).reshape(-1), 1e-2, 1e-3, "conv_in gn")
    xo = rnd((b, h, h, 320), 35)
    w_out = E.pack_conv_cout4(torch.randn(4, 320, 3, 3) / math.sqrt(9 * 320), BF)
    bias_out = torch.randn(4) * 0.1
    eps = hip.zeros((b, 4, h, h), F32)
    hip.conv_cout4(dev(hip, xo), dev(hip, w_out), dev(hip, bias_out), eps, 0)
    eps_ref = torch.zeros(b, 4, h, h)
    REF.conv_cout4(xo, w_out, bias_out, eps_ref, 0)
    lat = torch.randn(b, 4, h, h)
    coef = dev(hip, torch.tensor([0.8, 0.6, 0.9, 0.43589]))
    l_ref, l_fused = dev(hip, lat.clone()), dev(hip, lat.clone())
    hip.ddim_update(l_ref, eps, None, 1.0, coef)
    hip.conv_out_ddim(dev(hip, xo), dev(hip, w_out), dev(hip, bias_out), l_fused, coef)
    hip.synchronize()
    close(eps, eps_ref, 1e-3, 1e-3, "conv_cout4")
    assert torch.equal(l_fused.cpu(), l_ref.cpu())
    with pytest.raises(ValueError):        # one op, one 16-bit dtype
        hip.conv_cout4(dev(hip, xo), dev(hip, w_out.to(F16)), dev(hip, bias_out), eps, 0)


# ------------------------------------------------------------------------------------------------ range
def test_bf16_range_where_fp16_overflows(hip):
    """What the mode is for: activations around 1e6 (past fp16's 65504).  The bf16 GEMM and GroupNorm stay finite and
    within bf16 tolerance; the fp16 entry points on the same inputs do not."""
    m, c, n = 128, 320, 320
    x = (rnd((1, 8, 16, c), 36).float() * 3e3).to(BF)            # |x| up to ~1e4: the GEMM output reaches ~1e6
    w = rnd((n, c), 37, 20.0)
    o, o_ref = igemm_pair(hip, x, w, (1, 8, 16, n), flags=0, tile_m=128, tile_n=160)
    assert o_ref.float().abs().max().item() > 3e5
    assert torch.isfinite(o.float()).all()
    close(o, o_ref, 1e-2 * o_ref.float().abs().max().item(), 1.6e-2, "bf16 GEMM at 1e6")
    o16 = hip.zeros((1, 8, 16, n), F16)
    hip.igemm(dev(hip, x.to(F16)), dev(hip, w.to(F16)), o16, tile_m=128, tile_n=160)
    big = (rnd((2, 16, 16, c), 38).float() * 1e6 + 2e5).to(BF)    # GroupNorm over values ~1e6
    gamma, beta = torch.ones(c), torch.zeros(c)
    g = hip.zeros((2, 16, 16, c), BF)
    hip.groupnorm(dev(hip, big), None, dev(hip, gamma), dev(hip, beta), g, hip.zeros((2 * 256 * 64,), F32), 32, 1e-5, 0)
    g_ref = torch.zeros(2, 16, 16, c, dtype=BF)
    REF.groupnorm(big, None, gamma, beta, g_ref, None, 32, 1e-5, 0)
    g16 = hip.zeros((2, 16, 16, c), F16)
    hip.groupnorm(dev(hip, big.to(F16)), None, dev(hip, gamma), dev(hip, beta), g16, hip.zeros((2 * 256 * 64,), F32), 32,
                  1e-5, 0)
    hip.synchronize()
    assert torch.isfinite(g.float()).all()
    close(g, g_ref, 2e-2, 1.6e-2, "bf16 GroupNorm at 1e6")
    assert not torch.isfinite(o16.float().cpu()).all() and not torch.isfinite(g16.float().cpu()).all()


# ------------------------------------------------------------------------------------------------ UNet / sampler
@pytest.fixture(scope="module")
def full_sd():
    from progressive_stable_diffusion_amd import weights as W
    shapes = dict(W.unet_shapes())
    shapes.update(W.vae_shapes(encoder=False))
    shapes.update(W.conditioning_shapes())
    return W.init_state_dict(shapes, 0, gates=GI.GATES, warm_start_dis=False)


def _module(sd, image_size, batch, **cfg_over):
    from progressive_stable_diffusion_amd.config import default_config
    from progressive_stable_diffusion_amd.diffusion_module_ip import DiffusionModuleWithIP
    cfg = default_config(**{"dataset.image_size": image_size, **cfg_over})
    return DiffusionModuleWithIP(cfg, state_dict=sd, device=DEV, seed=0, batch_size=batch, operand_dtype=BF)


def _ocfg(mod):
    return OS.OracleCfg(image_size=mod.cfg.dataset.image_size, use_routing_gates=mod.diff_cfg.use_routing_gates)


@pytest.mark.parametrize("side,lam", [(16, 3.0), (24, 0.0), (16, 0.0), (24, 3.0)])
def test_unet_bf16_matches_oracle(hip, full_sd, side, lam):
    """One eps call of the bf16 plan, B = 2 (side 24: ragged attention lengths 576 / 144 / 36 / 9).  Measured on MI355X:
    0.91-1.06e-2 * max|eps| (fp16 plan on the same inputs: 1.1-1.5e-3)."""
    from progressive_stable_diffusion_amd.engine import UNetPlan
    b = 2
    plan = UNetPlan(hip, full_sd, b, side, dtype=BF)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(b, 4, side, side, generator=g)
    cond = torch.randn(b, 48, 768, generator=g) * 0.5
    t = torch.tensor([999, 261])
    with torch.no_grad():
        ref = unet_forward(full_sd, x, t, cond, delta_scale=lam)
    got = plan.forward(x.to(DEV), t.to(DEV), cond.to(DEV), lam=lam)
    got16 = UNetPlan(hip, full_sd, b, side).forward(x.to(DEV), t.to(DEV), cond.to(DEV), lam=lam)
    hip.synchronize()
    rel = (got.cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    rel16 = (got16.cpu() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print(f"UNet S={side} lam={lam}: bf16 {rel:.3e}, fp16 {rel16:.3e} of max|eps|")
    assert rel < 4e-2, rel
    assert not torch.equal(got.cpu(), got16.cpu())        # the bf16 kernels ran


@pytest.mark.parametrize("gates_on", [True, False])
def test_config1_teacher_forced_eps_per_step_bf16(full_sd, gates_on):
    """BASELINE config 1 (256x256, 10 steps; lambda = 3 with gates, CFG g = 3 without), teacher-forced: the oracle's x_t of
    every step into the bf16 module, eps compared per step and per branch at 4e-2 * max|eps|.  Measured on MI355X: worst
    step 1.23e-2 (gates on) and 1.30e-2 (CFG)."""
    from progressive_stable_diffusion_amd import inference_pipeline_ip as PIPE
    mod = _module(full_sd, 256, 1, **{"model.use_routing_gates": gates_on})
    target, source = torch.tensor([3.0]), torch.tensor([0.0])
    pix = torch.rand(1, 3, 224, 224, generator=torch.Generator().manual_seed(1)) * 2 - 1
    lat = torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(1234))
    kw = dict(steer_scale=3.0) if gates_on else dict(guidance_scale=3.0)
    with torch.no_grad():
        feats = mod.image_encoder.get_hidden_states(pix.to(DEV)).cpu()
        tr = []
        OS.ddim_sample(full_sd, _ocfg(mod), target, source, feats, 10, lat, trace=tr, **kw)
        cond = PIPE._prepare_conditioning(mod, target.to(DEV), source.to(DEV), pix.to(DEV))
        uncond = None if gates_on else PIPE._prepare_conditioning(mod, target.to(DEV), source.to(DEV), pix.to(DEV),
                                                                  zero_aoe=True)
        PIPE._set_delta_scale_on_processors(mod, 3.0 if gates_on else 0.0)
        ts = torch.linspace(999, 0, 10, dtype=torch.long, device=DEV)
        worst = 0.0
        for i, (eps_ref, _, x_t, parts) in enumerate(tr):
            t = ts[i].expand(1)
            refs = [(cond, eps_ref)] if gates_on else [(cond, parts[0]), (uncond, parts[1])]
            for c, ref in refs:
                got = mod(x_t.to(DEV), t, c).cpu()
                rel = (got - ref).abs().max().item() / max(1.0, ref.abs().max().item())
                worst = max(worst, rel)
                assert rel < 4e-2, (gates_on, i, int(ts[i]), rel)
    print(f"config1 teacher-forced bf16 gates={gates_on}: worst per-step eps error {worst:.3e} of max|eps|")


def test_bf16_sampler_properties(full_sd):
    """Captured graph == eager bit for bit; fused conv_out + DDIM == the traced two-launch run; steering acts (the
    lambda-0 row does not move); frames in [0, 1]."""
    from progressive_stable_diffusion_amd import inference_pipeline_ip as PIPE
    mod = _module(full_sd, 256, 2)
    assert mod.ddim_loop(2, 32).u.dtype == BF
    pix = (torch.rand(1, 3, 224, 224, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    lat = torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(5)).repeat(2, 1, 1, 1)
    tgt, src = torch.tensor([3.0, 2.0], device=DEV), torch.full((2,), 2.0, device=DEV)
    with torch.no_grad():
        z = PIPE._ddim_sample_ip(mod, tgt, src, pix, 6, DEV, steer_scale=3.0, latents=lat)
        z_eager = PIPE._ddim_sample_ip(mod, tgt, src, pix, 6, DEV, steer_scale=3.0, latents=lat, use_graph=False)
        tr = []
        z_tr = PIPE._ddim_sample_ip(mod, tgt, src, pix, 6, DEV, steer_scale=3.0, latents=lat, trace=tr)
        z0 = PIPE._ddim_sample_ip(mod, tgt, src, pix, 6, DEV, steer_scale=0.0, latents=lat)
        img = PIPE._latents_to_images(mod, z)
    assert torch.equal(z.cpu(), z_eager.cpu()), "graph replay must equal eager launches bit for bit"
    assert len(tr) == 6 and torch.equal(z_tr.cpu(), z.cpu()), "fused conv_out + DDIM must equal the two launches"
    assert torch.isfinite(z).all() and float(z.abs().max()) <= 4.0 + 1e-6
    assert (z[1] - z0[1]).abs().max().item() < 1e-5 and (z[0] - z0[0]).abs().max().item() > 1e-3
    assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0


def test_config5_geometry_768_bf16(full_sd):
    """BASELINE config 5's geometry (768x768, B = 2, 6 steps) in the bf16 mode: finite, clamped, deterministic,
    steering acts, frames in range."""
    from progressive_stable_diffusion_amd import inference_pipeline_ip as PIPE
    mod = _module(full_sd, 768, 2)
    pix = (torch.rand(1, 3, 224, 224, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(DEV)
    lat = torch.randn(1, 4, 96, 96, generator=torch.Generator().manual_seed(5)).repeat(2, 1, 1, 1)
    tgt, src = torch.tensor([3.0, 2.0], device=DEV), torch.full((2,), 2.0, device=DEV)
    with torch.no_grad():
        z = PIPE._ddim_sample_ip(mod, tgt, src, pix, 6, DEV, steer_scale=3.0, latents=lat)
        z2 = PIPE._ddim_sample_ip(mod, tgt, src, pix, 6, DEV, steer_scale=3.0, latents=lat)
        z0 = PIPE._ddim_sample_ip(mod, tgt, src, pix, 6, DEV, steer_scale=0.0, latents=lat)
        img = PIPE._latents_to_images(mod, z)
    assert z.shape == (2, 4, 96, 96) and torch.isfinite(z).all() and float(z.abs().max()) <= 4.0 + 1e-6
    assert torch.equal(z, z2)
    assert (z[1] - z0[1]).abs().max().item() < 1e-5 and (z[0] - z0[0]).abs().max().item() > 1e-3
    assert img.shape == (2, 3, 768, 768) and float(img.min()) >= 0.0 and float(img.max()) <= 1.0
