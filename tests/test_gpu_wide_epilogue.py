"""-m gpu: WHERE the GEMM / conv epilogues (csrc/igemm_epilogue.h) and the row-block kernels' private epilogues write.

Written for a 16-byte form of the output stores (two adjacent 16-column fragments of a wave exchanged between lane rows
with v_permlane16_swap, every lane storing 8 consecutive channels).  That form was measured and NOT kept (−26 us of
6.6 ms per UNet step, inside the end-to-end noise: profiles/r07_b_step_profile_*.txt); the tests stay,
because they pin what any other store layout has to respect.  The reference and the tolerances are those of the tests
of the same ops in test_gpu_kernels.py (TorchRefBackend; one fp16 rounding of the result plus accumulation order).
What these tests add: every output is a window of a larger buffer filled with a sentinel — columns to the right of N
(row stride > N), 16 rows below M — and everything outside [0, M) x [0, N) must still hold the sentinel after the
launch.  Shapes: M = 200 is ragged against 64- and 128-row tiles; N % 16 == 8 ends in half a fragment, N = 160 / 328
leave an odd fragment on the 160-column tiles; row strides of N + 4 and N + 8 halfs are 8- but not 16-byte and 16-byte
aligned rows.
"""
import functools
import math

import pytest
import torch

from tests.torch_backend import TorchRefBackend

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
REF = TorchRefBackend()
SENT = 77.0          # exactly representable in fp16 and bf16; far outside the value range of every case
GUARD_ROWS = 16
TILES = [(64, 64), (64, 160), (128, 128), (128, 160)]


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(torch.device("cuda:0"))


def rnd(shape, seed, scale=1.0, dtype=F16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def dev(hip, t):
    return None if t is None else hip.to_device(t)


def close(got, ref, atol, rtol, what=""):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())}/{bad.numel()} off, max err "
                                 f"{err.max().item():.4e} at ref {ref.flatten()[err.argmax()].item():.4e}")


class Window:
    """An output of `shape` = (B, Ho, Wo, N) with row stride `ld`, starting `off` halfs into a sentinel-filled buffer of
    rows + GUARD_ROWS rows."""

    def __init__(self, hip, shape, ld, off=0, dtype=F16):
        b, ho, wo, n = shape
        self.rows, self.n, self.ld, self.off = b * ho * wo, n, ld, off
        assert ld >= n + off
        self.buf = hip.zeros(((self.rows + GUARD_ROWS) * ld,), dtype)
        with hip.ctx():                      # on the backend's stream, ahead of the launch under test
            self.buf.fill_(SENT)
        self.out = self.buf.as_strided(shape, (ho * wo * ld, wo * ld, ld, 1), off)

    def check_untouched(self, what):
        img = self.buf.float().cpu().reshape(self.rows + GUARD_ROWS, self.ld).clone()
        img[: self.rows, self.off: self.off + self.n] = SENT
        bad = img != SENT
        assert not bool(bad.any()), (f"{what}: {int(bad.sum())} elements outside [0,M) x [0,N) were written, first at "
                                     f"(row, col) {tuple(bad.nonzero()[0].tolist())} (M={self.rows}, N={self.n}, ld={self.ld})")


M_LIN = 200


@functools.lru_cache(maxsize=None)
def linear_case(n, k, epi):
    """Operands and the reference of one linear, shared by every tile / stride that runs it (never modified)."""
    from progressive_stable_diffusion_amd import lib as L
    m = M_LIN
    x, w = rnd((1, m, 1, k), 1), rnd((n, k), 2, 1 / math.sqrt(k))
    t = dict(bias=rnd((n,), 3, 0.1, F32))
    flags = L.EPI_BIAS
    if epi == "residual":        # a residual whose row stride differs from the output's
        t["residual"] = rnd((1, m, 1, n + 24), 4)[..., 8:8 + n]
        flags |= L.EPI_RESIDUAL
    elif epi == "gelu":
        flags |= L.EPI_GELU
    elif epi == "rowvec":
        t["rowvec"] = rnd((1, n), 5, 0.3, F32)
        flags |= L.EPI_ROWVEC
    ref = torch.zeros((1, m, 1, n), dtype=F16)
    REF.igemm(x, w, ref, flags=flags, **t)
    return x, w, t, flags, ref


def run_linear(hip, n, k, epi, tile, ld, off=0, extra_flags=0, **kw):
    x, w, t, flags, ref = linear_case(n, k, "bias" if epi == "lnstat" else epi)
    win = Window(hip, (1, M_LIN, 1, n), ld, off)
    td = {key: dev(hip, v) for key, v in t.items()}
    if "residual" in t:          # keep the residual's own row stride on the device
        full = hip.to_device(rnd((1, M_LIN, 1, n + 24), 4))
        td["residual"] = full[..., 8:8 + n]
    hip.igemm(dev(hip, x), dev(hip, w), win.out, flags=flags | extra_flags, tile_m=tile[0], tile_n=tile[1], **td, **kw)
    hip.synchronize()
    what = f"linear N{n} K{k} {epi} tile{tile} ld{ld} off{off}"
    close(win.out, ref, 3e-3, 3e-3 if epi == "gelu" else 2e-3, what)      # test_igemm_linear / _activation_epilogues
    win.check_untouched(what)
    return win


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("n", [72, 136, 160, 328])
@pytest.mark.parametrize("k", [256, 128])
def test_linear_every_tile_and_stride(hip, k, n, tile):
    """bias epilogue; row strides N, N + 4 and N + 8.  K = 256 runs the LDS-DMA kernels; K = 128 asks for
    the register-staged igemm_kernel (TUNE_NODMA), which has no 64-column tile: (64, 64) stays on the LDS-DMA kernel."""
    from progressive_stable_diffusion_amd import lib as L
    nodma = L.TUNE_NODMA if (k == 128 and tile[1] != 64) else 0
    for ld in (n, n + 4, n + 8):
        run_linear(hip, n, k, "bias", tile, ld, extra_flags=nodma)


def test_linear_window_at_a_column_offset(hip):
    """The launcher takes 16-byte aligned outputs only, so a window 4 halfs into a row is refused before anything
    runs; 8 halfs in, it is a window like any other."""
    from progressive_stable_diffusion_amd import lib as L
    x, w, t, flags, _ = linear_case(136, 256, "bias")
    win = Window(hip, (1, M_LIN, 1, 136), 152, off=4)
    with pytest.raises(ValueError):
        hip.igemm(dev(hip, x), dev(hip, w), win.out, flags=flags, bias=dev(hip, t["bias"]))
    win.check_untouched("refused launch")
    for tile in ((64, 160), (128, 128)):
        run_linear(hip, 136, 256, "bias", tile, 152, off=8)
        run_linear(hip, 136, 128, "bias", tile, 152, off=8, extra_flags=L.TUNE_NODMA)


@pytest.mark.parametrize("tile", [(64, 160), (128, 128)])
@pytest.mark.parametrize("n", [72, 328])
@pytest.mark.parametrize("epi", ["residual", "gelu", "rowvec"])
def test_linear_epilogues(hip, epi, n, tile):
    from progressive_stable_diffusion_amd import lib as L
    run_linear(hip, n, 256, epi, tile, n + 8)
    run_linear(hip, n, 128, epi, tile, n + 4, extra_flags=L.TUNE_NODMA)


@pytest.mark.parametrize("tile", TILES)
def test_linear_row_partials_follow_the_stored_values(hip, tile):
    """DADD_EPI_LNSTAT: the partials are sums over the stored output (1e-5 relative, as in
    test_igemm_layernorm_statistics_from_producer)."""
    from progressive_stable_diffusion_amd import lib as L
    n = 320
    parts = n // (tile[1] // 2)
    for ld in (n + 8, n + 4):
        st = hip.zeros((parts, M_LIN, 2), F32)
        win = run_linear(hip, n, 256, "lnstat", tile, ld, extra_flags=L.EPI_LNSTAT, ln_stats_out=st)
        oc = win.out.float().cpu().reshape(M_LIN, parts, -1)
        want = torch.stack([oc.sum(-1), (oc * oc).sum(-1)], dim=-1).permute(1, 0, 2)
        err = (st.cpu() - want).abs().max().item()
        assert err <= 1e-5 * want.abs().max().item() + 1e-4, (err, tile, ld)


def _ln_operands(n, k, geglu, seed=80):
    from progressive_stable_diffusion_amd import engine as E
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) / math.sqrt(k)
    b = torch.randn(n, generator=g) * 0.1
    gamma, beta = 1.0 + 0.2 * torch.randn(k, generator=g), 0.2 * torch.randn(k, generator=g)
    w16, c1, bias = E.fold_layernorm(w, b, gamma, beta)
    if geglu:
        idx = E.geglu_interleave(torch.arange(n)[:, None].float(), torch.zeros(n))[0][:, 0].long()
        w16, c1, bias = w16[idx], c1[idx], bias[idx]
    return w, b, gamma, beta, w16.contiguous(), c1.contiguous(), bias.contiguous()


@pytest.mark.parametrize("tile,n", [((64, 64), 136), ((128, 160), 328), ((128, 128), 256)])
def test_layernorm_fold_statistics_from_the_a_fragments(hip, tile, n):
    """LNK 1 (the MFMA waves sum the rows): the global-operand path of the fold; tolerance of test_igemm_layernorm_fold."""
    from progressive_stable_diffusion_amd import lib as L
    import torch.nn.functional as Fn
    m, k = M_LIN, 256
    g = torch.Generator().manual_seed(82)
    x = (torch.randn(1, m, 1, k, generator=g) + 3.0 * torch.randn(1, m, 1, 1, generator=g)).to(F16)
    w, b, gamma, beta, w16, c1, bias = _ln_operands(n, k, False)
    ref = Fn.linear(Fn.layer_norm(x.float(), (k,), gamma, beta, 1e-5), w.to(F16).float(), b)
    for ld in (n + 8, n + 4):
        win = Window(hip, (1, m, 1, n), ld)
        hip.igemm(dev(hip, x), dev(hip, w16), win.out, bias=dev(hip, bias), flags=L.EPI_BIAS | L.EPI_LNFOLD, tile_m=tile[0],
                  tile_n=tile[1], ln_c1=dev(hip, c1))
        hip.synchronize()
        close(win.out, ref, 6e-3, 6e-3, f"ln fold {tile} N{n} ld{ld}")
        win.check_untouched(f"ln fold {tile} N{n} ld{ld}")


@pytest.mark.parametrize("geglu", [False, True])
def test_layernorm_fold_statistics_from_the_producer(hip, geglu):
    """LNK 2 on a 128-row tile: the producer's row partials, c1 and the bias staged in LDS (row-outer store order), with
    and without the GEGLU epilogue; tolerance of test_igemm_layernorm_statistics_from_producer."""
    from progressive_stable_diffusion_amd import lib as L
    import torch.nn.functional as Fn
    m, c = 512 + 72, 256                  # ragged last 128-row tile; nk = 4 K tiles
    n = 256 if geglu else 328
    tile = (128, 128) if geglu else (128, 160)
    h = (rnd((1, m, 1, c), 83).float() + 2.0 * rnd((1, m, 1, 1), 84).float()).to(F16)
    parts = 4
    hp = h.float().reshape(m, parts, c // parts)
    st = torch.stack([hp.sum(-1), (hp * hp).sum(-1)], dim=-1).permute(1, 0, 2).contiguous()
    w, b, gamma, beta, w16, c1, bias = _ln_operands(n, c, geglu, seed=85)
    ref = Fn.linear(Fn.layer_norm(h.float(), (c,), gamma, beta, 1e-5), w.to(F16).float(), b)
    if geglu:
        hid, gate = ref.chunk(2, dim=-1)
        ref = hid * Fn.gelu(gate)
    n_out = n // 2 if geglu else n
    flags = L.EPI_BIAS | L.EPI_LNFOLD | (L.EPI_GEGLU if geglu else 0)
    for ld in (n_out + 8, n_out + 4):
        win = Window(hip, (1, m, 1, n_out), ld)
        hip.igemm(dev(hip, h), dev(hip, w16), win.out, bias=dev(hip, bias), flags=flags, tile_m=tile[0], tile_n=tile[1],
                  ln_c1=dev(hip, c1), ln_stats_in=dev(hip, st))
        hip.synchronize()
        close(win.out, ref, 6e-3, 6e-3, f"ln stats-in geglu{geglu} ld{ld}")
        win.check_untouched(f"ln stats-in geglu{geglu} ld{ld}")


@pytest.mark.parametrize("fold", [False, True])
def test_geglu(hip, fold):
    """GEGLU with N = 256 (128 outputs: two hidden fragments per wave), plain and with LayerNorm folded
    from the A fragments; tolerances of test_igemm_geglu / test_igemm_layernorm_fold."""
    from progressive_stable_diffusion_amd import lib as L
    from progressive_stable_diffusion_amd.engine import geglu_interleave
    import torch.nn.functional as Fn
    m, k, n = M_LIN, 256, 256
    if fold:
        g = torch.Generator().manual_seed(86)
        x = (torch.randn(1, m, 1, k, generator=g) + 3.0 * torch.randn(1, m, 1, 1, generator=g)).to(F16)
        w, b, gamma, beta, w16, c1, bias = _ln_operands(n, k, True, seed=87)
        hid, gate = Fn.linear(Fn.layer_norm(x.float(), (k,), gamma, beta, 1e-5), w.to(F16).float(), b).chunk(2, dim=-1)
        ref, kw, tol = hid * Fn.gelu(gate), dict(ln_c1=dev(hip, c1)), 6e-3
        flags = L.EPI_BIAS | L.EPI_GEGLU | L.EPI_LNFOLD
    else:
        x = rnd((1, m, 1, k), 17)
        w32, b32 = rnd((n, k), 18, 1 / math.sqrt(k), F32), rnd((n,), 19, 0.1, F32)
        wp, bias = geglu_interleave(w32, b32)
        w16 = wp.to(F16)
        ref = torch.zeros((1, m, 1, n // 2), dtype=F16)
        REF.igemm(x, w16, ref, bias=bias, flags=1 | 8)
        kw, tol, flags = {}, 3e-3, L.EPI_BIAS | L.EPI_GEGLU
    for tile_m in (64, 128):
        for ld in (n // 2 + 8, n // 2 + 4):
            win = Window(hip, (1, m, 1, n // 2), ld)
            hip.igemm(dev(hip, x), dev(hip, w16), win.out, bias=dev(hip, bias), flags=flags, tile_m=tile_m, tile_n=128, **kw)
            hip.synchronize()
            close(win.out, ref, tol, tol, f"geglu fold{fold} tm{tile_m} ld{ld}")
            win.check_untouched(f"geglu fold{fold} tm{tile_m} ld{ld}")


def test_halo_conv_with_groupnorm_statistics(hip):
    """3x3 halo conv, B = 2, 16x16, 64 -> 320 with DADD_EPI_GNSTAT: output against the reference and the chunk partials
    against sums of the stored output (tolerances of test_igemm_groupnorm_statistics_epilogue)."""
    from progressive_stable_diffusion_amd import lib as L
    b, hw, cin, n, tm, tn = 2, 16, 64, 320, 128, 160
    x, w = rnd((b, hw, hw, cin), 90), rnd((n, 9 * cin), 91, 1 / math.sqrt(9 * cin))
    bias, rowvec, res = rnd((n,), 92, 0.1, F32), rnd((b, n), 93, 0.3, F32), rnd((b, hw, hw, n), 94)
    ref = torch.zeros(b, hw, hw, n, dtype=F16)
    REF.igemm(x, w, ref, bias=bias, rowvec=rowvec, residual=res, taps=9, pad=1, flags=7)
    nchunk = hw * hw // (tm // 2)
    for ld in (n + 8, n + 4):
        win = Window(hip, (b, hw, hw, n), ld)
        ws = hip.zeros((b * nchunk * 64,), F32)
        hip.igemm(dev(hip, x), dev(hip, w), win.out, bias=dev(hip, bias), rowvec=dev(hip, rowvec), residual=dev(hip, res),
                  taps=9, pad=1, flags=7 | L.EPI_GNSTAT, tile_m=tm, tile_n=tn, gn_ws=ws, gn_nchunk=nchunk)
        hip.synchronize()
        close(win.out, ref, 3e-3, 2e-3, f"halo gnstat ld{ld}")
        win.check_untouched(f"halo gnstat ld{ld}")
        oc = win.out.float().cpu().reshape(b, nchunk, -1, 32, n // 32)
        part = torch.stack([oc.sum(dim=(2, 4)), (oc * oc).sum(dim=(2, 4))], dim=-1)
        got = ws.cpu().reshape(b, nchunk, 32, 2)
        assert (got - part).abs().max().item() <= 1e-3 * part.abs().max().item() + 1e-3, ld


def test_persistent_ring_three_tiles_per_workgroup(hip):
    """DADD_TUNE_PERSIST with 3 x (CUs + 2) tiles of 128 x 128: every workgroup walks three or four output tiles, each
    with its own epilogue while the DMA cursor is already in the next one.  K = 256, bias + residual."""
    from progressive_stable_diffusion_amd import lib as L
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    m, k, n = 128 * (ncu + 2) - 56, 256, 384          # ragged last row tile
    x, w = rnd((1, m, 1, k), 70), rnd((n, k), 71, 1 / math.sqrt(k))
    bias, res = rnd((n,), 72, 0.1, F32), rnd((1, m, 1, n), 73)
    ref = torch.zeros((1, m, 1, n), dtype=F16)
    REF.igemm(x, w, ref, bias=bias, residual=res, flags=5)
    win = Window(hip, (1, m, 1, n), n + 8)
    hip.igemm(dev(hip, x), dev(hip, w), win.out, bias=dev(hip, bias), residual=dev(hip, res),
              flags=5 | L.TUNE_PERSIST, tile_m=128, tile_n=128)
    hip.synchronize()
    close(win.out, ref, 3e-3, 3e-3, "persistent ring")
    win.check_untouched("persistent ring")


@pytest.mark.parametrize("case", ["plain", "residual", "geglu"])
def test_bf16(hip, case):
    """The bf16 twins share the epilogue source: plain, residual and GEGLU, against the same reference computed from the
    bf16 operands with one bf16 rounding of the result (rel. 2^-8)."""
    from progressive_stable_diffusion_amd.engine import geglu_interleave
    m, k = M_LIN, 256
    n = 256 if case == "geglu" else 328
    x = rnd((1, m, 1, k), 30, dtype=BF16)
    if case == "geglu":
        w32, b32 = rnd((n, k), 31, 1 / math.sqrt(k), F32), rnd((n,), 32, 0.1, F32)
        wp, bias = geglu_interleave(w32, b32)
        w, tile, flags = wp.to(BF16), (128, 128), 1 | 8
    else:
        w, bias, tile, flags = rnd((n, k), 31, 1 / math.sqrt(k), BF16), rnd((n,), 32, 0.1, F32), (128, 160), 1
    n_out = n // 2 if case == "geglu" else n
    res = None
    if case == "residual":
        res, flags = rnd((1, m, 1, n), 33, dtype=BF16), flags | 4
    ref = torch.zeros((1, m, 1, n_out), dtype=F32)
    REF.igemm(x.float(), w.float(), ref, bias=bias, residual=None if res is None else res.float(), flags=flags)
    for ld in (n_out + 8, n_out + 4):
        win = Window(hip, (1, m, 1, n_out), ld, dtype=BF16)
        hip.igemm(dev(hip, x), dev(hip, w), win.out, bias=dev(hip, bias), residual=dev(hip, res), flags=flags,
                  tile_m=tile[0], tile_n=tile[1])
        hip.synchronize()
        close(win.out, ref, 2e-2, 1e-2, f"bf16 {case} ld{ld}")       # one bf16 rounding (2^-8 = 3.9e-3 rel.) + fp32 order
        win.check_untouched(f"bf16 {case} ld{ld}")


# ---- the row-block kernels: contiguous [B*HW + guard rows][C] outputs, smallest shapes of their tests in test_gpu_kernels.py

def _guarded_rows(hip, b, hw, c):
    buf = hip.zeros(((b * hw + GUARD_ROWS) * c,), F16)
    with hip.ctx():                          # on the backend's stream, ahead of the launch under test
        buf.fill_(SENT)
    return buf, buf[: b * hw * c].view(b, hw, c)


def _guard_intact(buf, rows, c, what):
    tail = buf[rows * c:].float().cpu()
    assert bool((tail == SENT).all()), f"{what}: rows behind the last row block were written"


def test_tf_head_outputs(hip):
    from progressive_stable_diffusion_amd.engine import pack_head_stream
    b, hw, nchunk, c = 1, 64, 1, 320
    x = (rnd((b, hw, c), 720).float() * (1.0 + 0.5 * torch.randn(1, 1, c, generator=torch.Generator().manual_seed(721)))
         + torch.randn(b, 1, c, generator=torch.Generator().manual_seed(722))).to(F16)
    wp = rnd((c, c, 1, 1), 723, 1.0 / math.sqrt(c))
    wq, wk, wv = (rnd((c, c), 724 + i, 1.0 / math.sqrt(c)) for i in range(3))
    bp = rnd((c,), 727, 0.2, F32)
    g = torch.Generator().manual_seed(728)
    gg, gb = 1.0 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    lg, lb = 1.0 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    xs = x.float().reshape(b, nchunk, hw // nchunk, 32, c // 32)
    ws = torch.stack([xs.sum(dim=(2, 4)), (xs * xs).sum(dim=(2, 4))], dim=-1).reshape(-1).contiguous()
    stream = pack_head_stream(wp, wq, wk, wv)
    hs_ref, qkv_ref = torch.zeros(b, hw, c, dtype=F16), torch.zeros(b, hw, 3 * c, dtype=F16)
    REF.tf_head(x, stream, ws, nchunk, gg, gb, bp, lg, lb, hs_ref, qkv_ref)
    args = [dev(hip, t) for t in (x, stream, ws)] + [nchunk] + [dev(hip, t) for t in (gg, gb, bp, lg, lb)]
    hbuf, hs = _guarded_rows(hip, b, hw, c)
    qbuf, qkv = _guarded_rows(hip, b, hw, 3 * c)
    hip.tf_head(*args, hs, qkv)
    hip.synchronize()
    close(hs, hs_ref, 3e-3, 3e-3, "tf_head hs")
    close(qkv, qkv_ref, 6e-3, 4e-3, "tf_head qkv")
    _guard_intact(hbuf, b * hw, c, "tf_head hs")
    _guard_intact(qbuf, b * hw, 3 * c, "tf_head qkv")


def test_ffn_block_output(hip):
    from progressive_stable_diffusion_amd.engine import pack_ffn_stream
    b, hw, c, hid = 1, 64, 320, 1280
    x = (rnd((b, hw, c), 700, 1.0).float() + 0.5 * torch.randn(b, hw, 1, generator=torch.Generator().manual_seed(701))).to(F16)
    xres = rnd((b, hw, c), 702)
    w1, w2 = rnd((2 * hid, c), 703, 1.0 / math.sqrt(c)), rnd((c, hid), 704, 1.0 / math.sqrt(hid))
    wp = rnd((c, c, 1, 1), 705, 1.0 / math.sqrt(c))
    b1, b2, bp = rnd((2 * hid,), 706, 0.2, F32), rnd((c,), 707, 0.2, F32), rnd((c,), 708, 0.2, F32)
    g = torch.Generator().manual_seed(709)
    gam, bet = 1.0 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    stream, b1p = pack_ffn_stream(w1, b1, w2, wp)
    nchunk = hw // 32
    o_ref, ws_ref = torch.zeros(b, hw, c, dtype=F16), torch.zeros(b * nchunk * 64)
    REF.ffn_block(x, stream, gam, bet, b1p, b2, bp, xres, o_ref, gn_ws=ws_ref, gn_nchunk=nchunk)
    args = [dev(hip, t) for t in (x, stream, gam, bet, b1p, b2, bp, xres)]
    obuf, o = _guarded_rows(hip, b, hw, c)
    ws = hip.zeros((b * nchunk * 64,), F32)
    hip.ffn_block(*args, o, gn_ws=ws, gn_nchunk=nchunk)
    hip.synchronize()
    close(o, o_ref, 6e-3, 4e-3, "ffn_block")
    _guard_intact(obuf, b * hw, c, "ffn_block")
    oc = o.float().cpu().reshape(b, nchunk, 32, 32, c // 32)
    want = torch.stack([oc.sum(dim=(2, 4)), (oc * oc).sum(dim=(2, 4))], dim=-1).reshape(-1)
    assert (ws.cpu() - want).abs().max().item() <= 1e-5 * want.abs().max().item() + 1e-4


def test_attn2_fused_output(hip):
    b, hw, c = 2, 256, 320
    x, res = rnd((b, hw, c), 90), rnd((b, hw, c), 91)
    mcat = rnd((b, 384, c), 92, 2.0 / math.sqrt(c))
    vw = rnd((b, c, 384), 93, 0.5)
    bias = rnd((c,), 94, 0.1, F32)
    o_ref = torch.zeros(b, hw, c, dtype=F16)
    REF.attn2_fused(x, mcat, vw, bias, res, o_ref)
    obuf, o = _guarded_rows(hip, b, hw, c)
    st = hip.zeros((c // 80, b * hw, 2), F32)
    hip.attn2_fused(dev(hip, x), dev(hip, mcat), dev(hip, vw), dev(hip, bias), dev(hip, res), o, ln_stats_out=st)
    hip.synchronize()
    close(o, o_ref, 4e-3, 3e-3, "attn2_fused")
    _guard_intact(obuf, b * hw, c, "attn2_fused")
    oc = o.float().cpu().reshape(b * hw, c // 80, 80)
    want = torch.stack([oc.sum(-1), (oc * oc).sum(-1)], dim=-1).permute(1, 0, 2)
    assert (st.cpu() - want).abs().max().item() <= 1e-5 * want.abs().max().item() + 1e-4
