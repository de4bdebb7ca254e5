"""Operator backend: torch tensors in, C-ABI kernel launches out.

``HipBackend`` is the only backend the product ships.  Every method takes device tensors whose
memory torch owns, validates what the kernels assume, and launches on the backend's stream.
(The engine takes the backend as a constructor argument so that the CPU test-suite can check the
*wiring* of the plan with a reference implementation that lives under ``tests/``; the product
never constructs anything but ``HipBackend`` and fails loudly when the library is missing.)
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import lib as L


def _p(t: Optional[torch.Tensor]):
    """Device pointer of a tensor argument.  A host tensor here would hand the kernel a host address (a GPU memory
    fault, which can take the whole node down): refuse it as an ordinary Python error instead."""
    if t is None:
        return None
    if t.device.type != "cuda":
        raise ValueError(f"kernel argument lives on {t.device}, not on the GPU (shape {tuple(t.shape)}, {t.dtype})")
    return t.data_ptr()


_SFX = {torch.float16: "f16", torch.bfloat16: "bf16"}


def _sfx(*ts) -> str:
    """Entry-point suffix for the 16-bit operands of one op: ``f16`` or ``bf16`` (the UNet's bf16 operand mode).  Every
    16-bit tensor of the op must carry the same dtype; mixing fp16 and bf16 in one launch is an error."""
    kinds = {t.dtype for t in ts if t is not None and t.dtype in _SFX}
    if len(kinds) != 1:
        raise ValueError(f"one op takes fp16 or bf16 operands, not {sorted(str(k) for k in kinds) or 'neither'}")
    return _SFX[kinds.pop()]


def fill_igemm_desc(d, ptr, x, w, out, *, x2=None, bias=None, rowvec=None, residual=None, taps=1, stride=1,
                    ups=0, pad=0, flags=0, splitk=1, partial=None, tile_n=0, tile_m=0, counters=None, ln_c1=None,
                    ln_eps=1e-5, gn_ws=None, gn_nchunk=0, ln_stats_out=None, ln_stats_in=None, gn_in=None, gn_apply=None,
                    w_fold=None):
    """Check the shapes of one ``igemm`` call (arguments of ``HipBackend.igemm``) and fill the ``IgemmDesc`` ``d`` with
    it; ``ptr`` turns a tensor (or None) into the address the descriptor carries."""
    b, hi, wi, c1 = x.shape
    c2 = 0 if x2 is None else x2.shape[-1]
    n = w.shape[0]
    ho, wo = out.shape[1], out.shape[2]
    assert w.shape[1] == taps * (c1 + c2), (w.shape, taps, c1, c2)
    assert out.shape[-1] == (n // 2 if flags & L.EPI_GEGLU else n) and out.shape[0] == b
    d.x, d.x2, d.w, d.out, d.partial = ptr(x), ptr(x2), ptr(w), ptr(out), ptr(partial)
    d.bias, d.rowvec, d.residual = ptr(bias), ptr(rowvec), ptr(residual)
    d.B, d.Hi, d.Wi, d.C1, d.C2, d.Ho, d.Wo, d.N = b, hi, wi, c1, c2, ho, wo, n
    d.taps, d.stride, d.ups, d.pad = taps, stride, ups, pad
    d.ldo, d.ldr = out.stride(-2), (residual.stride(-2) if residual is not None else 0)
    d.ld_rowvec = rowvec.stride(0) if rowvec is not None else 0
    d.splitk, d.flags, d.tile_n, d.tile_m = splitk, flags, tile_n, tile_m
    d.counters = ptr(counters)
    d.ln_c1, d.ln_eps = ptr(ln_c1), float(ln_eps)
    d.gn_ws, d.gn_nchunk, d.gn_cg = ptr(gn_ws), int(gn_nchunk), (n // 32 if gn_ws is not None else 0)
    if gn_ws is not None:
        assert flags & L.EPI_GNSTAT and gn_ws.numel() >= b * gn_nchunk * 64 and gn_ws.dtype == torch.float32
    if ln_c1 is not None:
        assert flags & L.EPI_LNFOLD and ln_c1.numel() == n and ln_c1.dtype == torch.float32
    m_rows = b * ho * wo
    d.ln_stats_out, d.ln_stats_in, d.ln_parts_out, d.ln_parts_in = ptr(ln_stats_out), ptr(ln_stats_in), 0, 0
    if ln_stats_out is not None:
        assert flags & L.EPI_LNSTAT and ln_stats_out.dtype == torch.float32 and ln_stats_out.dim() == 3 \
            and ln_stats_out.shape[1:] == (m_rows, 2) and ln_stats_out.is_contiguous()
        d.ln_parts_out = ln_stats_out.shape[0]
    if ln_stats_in is not None:
        assert flags & L.EPI_LNFOLD and ln_stats_in.dtype == torch.float32 and ln_stats_in.dim() == 3 \
            and ln_stats_in.shape[1:] == (b * hi * wi, 2) and ln_stats_in.is_contiguous()
        d.ln_parts_in = ln_stats_in.shape[0]
    d.gn_in_ws = d.gn_in_gamma = d.gn_in_beta = d.gn_in_ws2 = None
    d.gn_in_nchunk, d.gn_in_eps, d.gn_in_nchunk2 = 0, 0.0, 0
    if gn_in is not None:       # (partials, chunks, gamma, beta, eps[, partials of x2, chunks of x2])
        ws_in, nch_in, gam, bet, eps_in = gn_in[:5]
        assert flags & L.PRE_GN and ws_in.dtype == gam.dtype == bet.dtype == torch.float32 \
            and ws_in.numel() >= b * nch_in * 64 and gam.numel() == c1 + c2 and bet.numel() == c1 + c2
        d.gn_in_ws, d.gn_in_gamma, d.gn_in_beta = ptr(ws_in), ptr(gam), ptr(bet)
        d.gn_in_nchunk, d.gn_in_eps = int(nch_in), float(eps_in)
        if len(gn_in) > 5:
            ws2, nch2 = gn_in[5], gn_in[6]
            assert x2 is not None and ws2.dtype == torch.float32 and ws2.numel() >= b * nch2 * 64
            d.gn_in_ws2, d.gn_in_nchunk2 = ptr(ws2), int(nch2)
    d.gn_out = d.gn_out_gamma = d.gn_out_beta = None
    d.gn_out_eps = 0.0
    if gn_apply is not None:
        g_out, gam, bet, eps_o = gn_apply
        assert flags & L.EPI_GNAPPLY and g_out.shape == out.shape and g_out.dtype == out.dtype and g_out.is_contiguous() \
            and gam.dtype == bet.dtype == torch.float32 and gam.numel() == n and bet.numel() == n
        d.gn_out, d.gn_out_gamma, d.gn_out_beta, d.gn_out_eps = ptr(g_out), ptr(gam), ptr(bet), float(eps_o)
    if partial is not None:
        assert partial.numel() >= splitk * b * ho * wo * n
    d.w_fold = ptr(w_fold)
    if w_fold is not None:      # the four phase weights of an upsample conv (engine.fold_ups_weight), beside the 9-tap ``w``
        assert ups and taps == 9 and tuple(w_fold.shape) == (4, n, 4 * (c1 + c2)) and w_fold.dtype == w.dtype \
            and w_fold.is_contiguous()


class on_backend:
    """The stream bracket of every entry point, ``with on_backend(be):`` - inside it the backend's stream runs after what
    torch's current stream has produced, and after it (also when the body raises) torch's current stream waits for the
    backend's.  Everything that allocates or launches through ``be`` goes inside; leaving either end out is a cross-stream
    race that no test would catch.  Uses ``be.wait_current()`` and ``be.release_to_current()`` alone, so any backend with
    those two serves.  A plain class, not a ``contextlib`` generator: a step enters it a few thousand times, and this form
    costs 0.2 us more than the two bare calls where the generator costs 1 us."""
    __slots__ = ("be",)

    def __init__(self, be):
        self.be = be

    def __enter__(self):
        self.be.wait_current()

    def __exit__(self, *exc):
        self.be.release_to_current()


class HipBackend:
    name = "hip-gfx950"

    def __init__(self, device: torch.device):
        if not torch.cuda.is_available():
            raise RuntimeError("HipBackend needs a ROCm device (torch.cuda.is_available() is False)")
        self.lib = L.load()
        self.device = torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)
        self._desc = L.IgemmDesc()
        self._wdesc = L.WgradDesc()
        self._ddesc = L.DgradDesc()
        self._edesc = L.EndWgradDesc()
        self._gdesc = L.GnGradDesc()
        self._adesc = L.AttnGradDesc()
        self._ups_folds = {}        # address of a 9-tap upsample-conv weight -> (that weight, its folded copy); register_ups_fold
        self._n_cu = None
        self._capturing = False     # between graph_begin() and graph_end(): no cross-stream waits may be recorded
        self._prof_on = False
        with torch.cuda.device(self.device):
            L.check(self.lib.dadd_init())

    # ------------------------------------------------------------------ plumbing
    @property
    def s(self):
        return self.stream.cuda_stream

    def ctx(self):
        """All torch-side work of the engine (allocation, copy_, zero_) runs on the backend stream,
        so the caching allocator and the kernels agree on one stream order."""
        return torch.cuda.stream(self.stream)

    def empty(self, shape, dtype):
        with self.ctx():
            return torch.empty(shape, dtype=dtype, device=self.device)

    def zeros(self, shape, dtype):
        with self.ctx():
            return torch.zeros(shape, dtype=dtype, device=self.device)

    def _after_producer(self, src: torch.Tensor):
        """A device tensor handed in from outside was produced (or is still being produced) on torch's CURRENT
        stream; the backend stream must not read it earlier, and the caching allocator must not hand its block to
        another current-stream allocation while the backend stream still reads it."""
        if src.device.type == "cuda" and not self._capturing:
            cur = torch.cuda.current_stream(self.device)
            if cur != self.stream:
                self.stream.wait_stream(cur)
                src.record_stream(self.stream)

    def to_device(self, t: torch.Tensor, dtype=None):
        self._after_producer(t)
        with self.ctx():
            return t.to(device=self.device, dtype=dtype or t.dtype).contiguous()

    def copy_(self, dst: torch.Tensor, src: torch.Tensor):
        self._after_producer(src)
        with self.ctx():
            dst.copy_(src.reshape(dst.shape))

    def zero_(self, t: torch.Tensor):
        with self.ctx():
            t.zero_()

    def clone(self, t: torch.Tensor):
        """Copy made on the backend stream; the caller reads it on torch's current stream only after
        ``release_to_current()`` (or ``synchronize()``)."""
        with self.ctx():
            return t.detach().clone()

    def synchronize(self):
        self.stream.synchronize()

    def wait_current(self):
        """Order this backend's stream after torch's current stream (inputs produced by torch ops).  Nothing between
        ``graph_begin()`` and ``graph_end()``: a capture records launches, no cross-stream waits (``_after_producer``)."""
        if not self._capturing:
            self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def release_to_current(self):
        """Order torch's current stream after this backend's stream (outputs read by torch ops); nothing in a capture."""
        if not self._capturing:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)

    # ------------------------------------------------------------------ checks the training ops share
    @staticmethod
    def _scratch_numel(fn, args, message):
        """fp32 elements of an op's scratch from its ``dadd_*_floats`` query; the library answers -1 for sizes the op does
        not take, which raises ``ValueError(message.format(*args))``."""
        n = int(fn(*args))
        if n < 0:
            raise ValueError(message.format(*args))
        return n

    def _splitm(self, m, tiles):
        """Default slices of an ``m``-row reduction behind ``tiles`` output tiles: about 2 workgroups per CU, at least 64
        rows per slice: ``max(1, min(ceil(2 * CUs / tiles), ceil(m / 64)))``."""
        if self._n_cu is None:
            self._n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count
        return max(1, min(-(-2 * self._n_cu // tiles), -(-m // 64)))

    @staticmethod
    def _param_grad_checks(dgamma, dbeta, c, ws, need):
        """The parameter-gradient arguments of a norm backward, as three answers the caller raises on in its own words:
        dgamma and dbeta are both given or both None; each one given is contiguous fp32 [C]; ``ws`` is contiguous fp32
        with at least ``need`` elements."""
        together = (dgamma is None) == (dbeta is None)
        shaped = all(t is None or (t.dtype == torch.float32 and t.numel() == c and t.is_contiguous()) for t in (dgamma, dbeta))
        ws_ok = ws is not None and ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= need
        return together, shaped, ws_ok

    @staticmethod
    def _pointwise_width(op, f):
        if f % 8 or f == 0:
            raise ValueError(f"{op}: F = {f} must be a positive multiple of 8")

    # ------------------------------------------------------------------ ops
    def pack_latents(self, x, out, scale=1.0, mat=None, vec=None):
        b, c, h, w = x.shape
        assert x.dtype == torch.float32 and out.dtype == torch.float16 and out.shape == (b, h, w, 8)
        L.check(self.lib.dadd_pack_nchw_f32_to_nhwc8_f16(_p(x), _p(out), b, c, h, w, float(scale),
                                                         _p(mat), _p(vec), self.s))

    def conv_cin8(self, x, w, bias, out):
        b, h, wd, c8 = x.shape
        assert c8 == 8 and w.shape[1:] == (9, 8) and out.shape == (b, h, wd, w.shape[0])
        L.check(self.lib.dadd_conv3x3_cin8_f16(_p(x), _p(w), _p(bias), _p(out), b, h, wd, w.shape[0],
                                               self.s))

    def conv_in_nchw(self, x, w, bias, out, gn_ws=None, gn_nchunk=0):
        """fp32 NCHW latents (<= 4 channels) -> fp16 NHWC: pack_latents + conv_cin8 in one launch; with ``gn_ws`` also
        the GroupNorm chunk partials of the output (256 pixels per chunk)."""
        b, c, h, wd = x.shape
        assert x.dtype == torch.float32 and c <= 4 and w.shape[1:] == (9, 8) and out.shape == (b, h, wd, w.shape[0])
        assert gn_ws is None or (gn_ws.dtype == torch.float32 and gn_ws.numel() >= b * gn_nchunk * 64)
        fn = getattr(self.lib, "dadd_conv_in_nchw_" + _sfx(w, out))
        L.check(fn(_p(x), _p(w), _p(bias), _p(out), b, c, h, wd, w.shape[0], _p(gn_ws), gn_nchunk, self.s))

    def conv_cout4(self, x, w, bias, out, mode=0):
        b, h, wd, c = x.shape
        co = w.shape[0]
        assert w.shape == (co, 9, c) and out.shape == (b, co, h, wd) and out.dtype == torch.float32
        fn = getattr(self.lib, "dadd_conv3x3_cout4_" + _sfx(x, w))
        L.check(fn(_p(x), _p(w), _p(bias), _p(out), b, h, wd, c, co, int(mode), self.s))

    def conv_out_ddim(self, x, w, bias, latents, coef):
        """conv_out fused with the DDIM update: ``latents`` (fp32 NCHW) are stepped in place, eps is not stored."""
        b, h, wd, c = x.shape
        co = w.shape[0]
        assert w.shape == (co, 9, c) and latents.shape == (b, co, h, wd) and latents.dtype == torch.float32 \
            and coef.numel() == 4 and coef.dtype == torch.float32
        fn = getattr(self.lib, "dadd_conv_out_ddim_" + _sfx(x, w))
        L.check(fn(_p(x), _p(w), _p(bias), _p(latents), _p(coef), b, h, wd, c, co, self.s))

    def q_sample(self, x0, noise, t, alphas_cumprod, out):
        b = x0.shape[0]
        assert x0.dtype == torch.float32 and t.dtype == torch.int64 and t.shape == (b,) and noise.shape == x0.shape
        L.check(self.lib.dadd_q_sample_f32(_p(x0), _p(noise), _p(t), _p(alphas_cumprod), _p(out), b,
                                           x0.numel() // b, self.s))

    def mse_rows(self, pred, target, out):
        b = pred.shape[0]
        assert pred.shape == target.shape and out.shape == (b,) and pred.dtype == torch.float32
        L.check(self.lib.dadd_mse_rows_f32(_p(pred), _p(target), _p(out), b, pred.numel() // b, self.s))

    def frames_to_u8(self, frames, out):
        b, c, h, w = frames.shape
        assert c == 3 and frames.dtype == torch.float32 and out.dtype == torch.uint8 and out.shape == (b, h, w, 3)
        L.check(self.lib.dadd_frames_to_u8(_p(frames), _p(out), b, h, w, self.s))

    def gaussian_sample(self, mean, logvar, noise, out, scale=1.0):
        assert mean.shape == logvar.shape == noise.shape == out.shape and mean.dtype == torch.float32
        L.check(self.lib.dadd_gaussian_sample_f32(_p(mean), _p(logvar), _p(noise), float(scale), _p(out),
                                                  mean.numel(), self.s))

    def register_ups_fold(self, w9, w4):
        """``w4`` [4][N][4 Cin] is the phase-folded copy (``engine.fold_ups_weight``) of the packed upsample-conv weight
        ``w9`` [N][9 Cin]: an ``igemm(..., w9, ups=1, flags=TUNE_UPS_FOLD)`` then runs the four 2x2 phase convs on it.
        The registry holds both tensors, so neither address can be handed to another tensor while the entry exists; the
        plan that registers owns them."""
        if tuple(w4.shape) != (4, w9.shape[0], w9.shape[1] // 9 * 4) or w4.dtype != w9.dtype or not w4.is_contiguous() \
                or w4.device != w9.device:
            raise ValueError(f"register_ups_fold: w4 must be [4][N][4 Cin] of w9's type, got {tuple(w4.shape)} for {tuple(w9.shape)}")
        self._ups_folds[w9.data_ptr()] = (w9, w4)

    def igemm(self, x, w, out, *, x2=None, bias=None, rowvec=None, residual=None, taps=1, stride=1,
              ups=0, pad=0, flags=0, splitk=1, partial=None, tile_n=0, tile_m=0, counters=None, ln_c1=None,
              ln_eps=1e-5, gn_ws=None, gn_nchunk=0, ln_stats_out=None, ln_stats_in=None, gn_in=None, gn_apply=None):
        """x [B,Hi,Wi,C1] (x2 [B,Hi,Wi,C2]); w [N, taps*(C1+C2)]; out [B,Ho,Wo,N] (N/2 for GEGLU).
        ``gn_apply`` = (normalised output [B,Ho,Wo,N], gamma, beta, eps) with EPI_GNAPPLY: the split-K finish kernel also
        writes GroupNorm(out) (+ SiLU with EPI_GNAPPLY_SILU).
        ``gn_in`` = (partials [B*nchunk*64] fp32, nchunk, gamma, beta, eps) with PRE_GN: GroupNorm of x on the way in.
        ``ln_stats_out`` [P][M][2] fp32 (EPI_LNSTAT): row partials of the output, P = N / (tile_n/2);
        ``ln_stats_in`` [P'][M][2] (EPI_LNFOLD): the partials of x written by its producer."""
        fn = getattr(self.lib, "dadd_conv_igemm_" + _sfx(x, x2, w, out, residual, None if gn_apply is None else gn_apply[0]))
        d = self._desc
        fold = self._ups_folds.get(w.data_ptr()) if (flags & L.TUNE_UPS_FOLD) and ups else None
        fill_igemm_desc(d, _p, x, w, out, x2=x2, bias=bias, rowvec=rowvec, residual=residual, taps=taps, stride=stride,
                        ups=ups, pad=pad, flags=flags, splitk=splitk, partial=partial, tile_n=tile_n, tile_m=tile_m,
                        counters=counters, ln_c1=ln_c1, ln_eps=ln_eps, gn_ws=gn_ws, gn_nchunk=gn_nchunk,
                        ln_stats_out=ln_stats_out, ln_stats_in=ln_stats_in, gn_in=gn_in, gn_apply=gn_apply,
                        w_fold=None if fold is None else fold[1])
        L.check(fn(C.byref(d), self.s))

    # -- training backward of the matrix products (csrc/wgrad.hip; the data gradient is the forward kernel)
    def wgrad_splitm(self, m, n, c, taps=1):
        """Default number of reduction slices of ``wgrad``: the output has ceil(N/64) * taps * C/64 tiles of 64 x 64,
        usually far fewer than the device has CUs, and a reduction of M rows behind each; split it until the launch has
        about 2 workgroups per CU, every slice keeping at least 64 rows (the kernel itself takes slices down to one 32-row
        MFMA step, ``splitm <= ceil(M/32)``)."""
        return self._splitm(m, -(-n // 64) * taps * (c // 64))

    @staticmethod
    def wgrad_partial_numel(splitm, n, c, taps=1):
        """fp32 elements of the ``partial`` scratch of a ``wgrad`` call (nothing for ``splitm == 1``)."""
        return splitm * (n * taps * c + n) if splitm > 1 else 0

    @staticmethod
    def _pixel_ld(t):
        """Elements between two pixels of an NHWC / token-major tensor whose rows may be a column slice of a wider one."""
        ld = t.stride(-2)
        want, ok = ld, t.stride(-1) == 1
        for size, st in zip(reversed(t.shape[:-1]), reversed(t.stride()[:-1])):
            ok = ok and (size == 1 or st == want)
            want *= size
        if not ok:
            raise ValueError(f"expected dense pixels with one row stride, got shape {tuple(t.shape)} strides {t.stride()}")
        return ld

    def wgrad(self, dy, x, dw, *, dbias=None, taps=1, stride=1, ups=0, pad=0, splitm=None, partial=None, ld_tap=None):
        """Weight (and bias) gradient of ``igemm``: dw[n][tap][c] = sum_m dy[m][n] * x[gather(m, tap)][c] and
        dbias[n] = sum_m dy[m][n], fp32, overwritten.  dy [B,Ho,Wo,N] and x [B,Hi,Wi,C] (or [M,N] and [M,C] for a linear)
        are fp16 or bf16 and may be channel slices of wider tensors: the row strides travel.  dw is fp32 [N,taps,C] or
        [N,taps*C], possibly a column view of a wider weight gradient (skip-concat: one call per source into the
        [..., :C1] and [..., C1:] views of one [N,taps,C1+C2] tensor); for the 2-D form ``ld_tap`` gives the elements
        between taps (default C).
        ``splitm`` = number of slices of the M reduction; ``None`` takes ``wgrad_splitm``: enough slices for about two
        workgroups per CU, at least 64 rows per slice.  ``splitm > 1`` needs ``partial``, fp32 with
        ``wgrad_partial_numel`` = splitm * (N*taps*C + N) elements; the slabs are added in slice order, so the result is
        bit-reproducible."""
        if dy.dim() == 2:
            dy, x = dy.unsqueeze(0).unsqueeze(0), x.unsqueeze(0).unsqueeze(0)
        b, ho, wo, n = dy.shape
        bx, hi, wi, c = x.shape
        assert bx == b and dy.dim() == 4 and x.dim() == 4
        fn = getattr(self.lib, "dadd_conv_wgrad_" + _sfx(dy, x))
        assert dw.dtype == torch.float32 and dw.stride(-1) == 1 and dw.shape[0] == n
        if dw.dim() == 3:
            assert dw.shape[1:] == (taps, c) and ld_tap in (None, dw.stride(1))
            ld_tap = dw.stride(1)
        else:
            ld_tap = c if ld_tap is None else ld_tap
            assert dw.dim() == 2 and dw.shape[1] >= (taps - 1) * ld_tap + c
        assert dbias is None or (dbias.dtype == torch.float32 and dbias.numel() == n and dbias.is_contiguous())
        m = b * ho * wo
        if splitm is None:
            splitm = self.wgrad_splitm(m, n, c, taps)
        if splitm > 1:
            if partial is None:
                raise ValueError(f"wgrad with splitm = {splitm} needs a partial buffer")
            assert partial.dtype == torch.float32 and partial.is_contiguous() \
                and partial.numel() >= self.wgrad_partial_numel(splitm, n, c, taps), (partial.shape, splitm, n, taps, c)
        d = self._wdesc
        d.dy, d.x, d.dw, d.dbias, d.partial = _p(dy), _p(x), _p(dw), _p(dbias), _p(partial)
        d.B, d.Hi, d.Wi, d.C, d.Ho, d.Wo, d.N = b, hi, wi, c, ho, wo, n
        d.taps, d.stride, d.ups, d.pad = taps, stride, int(ups), pad
        d.ld_dy, d.ld_x, d.ld_dw, d.ld_tap = self._pixel_ld(dy), self._pixel_ld(x), dw.stride(0), ld_tap
        d.splitm = splitm
        L.check(fn(C.byref(d), self.s))

    def dgrad(self, dy, wt, dx, *, taps=1):
        """Data gradient of a stride-1 ``igemm``: the forward kernel on dy [B,H,W,N] with the re-laid weight
        wt [C, taps*N] (``grad_ops.dgrad_weight``: taps flipped, channel roles swapped) -> dx [B,H,W,C]; [M,N] -> [M,C] for
        a linear."""
        if dy.dim() == 2:
            dy, dx = dy.view(1, 1, *dy.shape), dx.view(1, 1, *dx.shape)
        n = dy.shape[-1]
        if n % 64 != 0:
            raise ValueError(f"dgrad contracts over the N = {n} output channels of the forward; the GEMM kernels need "
                             "a multiple of 64 (the data gradient of the 4-channel conv_out is dgrad_cout4)")
        assert taps in (1, 9) and wt.shape == (dx.shape[-1], taps * n) and dy.is_contiguous() and dx.is_contiguous()
        self.igemm(dy, wt, dx, taps=taps, pad=1 if taps == 9 else 0)

    # -- training backward of the 4-channel end convs and of the loss (csrc/end_grad.hip)
    def dgrad_cout4(self, dy_nchw_f32, wt, dx):
        """Data gradient of ``conv_cout4`` (the UNet's conv_out): dy fp32 NCHW [B,Co<=4,H,W] and the re-laid weight
        wt [C,9,8] (``grad_ops.dgrad_weight_cout4``: taps flipped, columns >= Co zero) -> dx [B,H,W,C] in wt's 16-bit
        type.  It is a 4 -> C convolution, so the kernel is ``conv_in_nchw`` without a bias: dy is rounded to the storage
        type in registers, as the forward rounds the latents."""
        if dy_nchw_f32.dim() != 4 or dy_nchw_f32.dtype != torch.float32 or not 1 <= dy_nchw_f32.shape[1] <= 4:
            raise ValueError(f"dgrad_cout4 takes dy fp32 NCHW with 1..4 channels, got {tuple(dy_nchw_f32.shape)} {dy_nchw_f32.dtype}")
        b, _, h, wd = dy_nchw_f32.shape
        if wt.dim() != 3 or wt.shape[1:] != (9, 8) or dx.shape != (b, h, wd, wt.shape[0]) or not (
                dy_nchw_f32.is_contiguous() and wt.is_contiguous() and dx.is_contiguous()):
            raise ValueError(f"dgrad_cout4: dy {tuple(dy_nchw_f32.shape)} takes contiguous wt [C,9,8] and dx [B,H,W,C], got "
                             f"{tuple(wt.shape)} and {tuple(dx.shape)}")
        self.conv_in_nchw(dy_nchw_f32, wt, None, dx)

    def end_wgrad_splitm(self, m, cw):
        """Default number of reduction slices of ``end_wgrad``: the output has only Cw/64 tiles (64 wide channels by all
        36 thin columns) and a reduction of M = B*H*W pixels behind each; split it until the launch has about 2 workgroups
        per CU, every slice keeping at least 64 pixels (the kernel itself takes slices down to one 32-pixel MFMA step,
        ``splitm <= ceil(M/32)``): ``max(1, min(ceil(2 * CUs / (Cw/64)), ceil(M/64)))``, the rule of ``wgrad_splitm``."""
        return self._splitm(m, max(1, cw // 64))

    def end_wgrad_partial_numel(self, splitm, ct, cw, mode):
        """fp32 elements of the ``partial`` scratch of an ``end_wgrad`` call (nothing for ``splitm == 1``): per slice dw
        in its final layout and the bias sums."""
        return self._scratch_numel(self.lib.dadd_end_wgrad_partial_floats, (int(mode), int(ct), int(cw), int(splitm)),
                                   "end_wgrad takes mode 0 or 1, Ct in 1..4 and Cw a multiple of 64 (got mode {}, Ct {}, Cw {})")

    def end_wgrad(self, thin, wide, dw, *, dbias=None, mode, splitm=None, partial=None):
        """Weight (and bias) gradient of a 4-channel end conv (3x3, stride 1, padding 1), fp32, overwritten.  ``thin`` is
        the fp32 NCHW tensor [B,Ct<=4,H,W], ``wide`` the fp16 or bf16 NHWC tensor [B,H,W,Cw] (possibly a channel slice of a
        wider one: the row stride travels); thin is rounded to wide's type before the product, as the forward kernels do.
        ``mode = lib.END_WGRAD_IN`` (conv_in: thin = latents, wide = dy): dw [Cw,9,8] in the ``pack_conv_cin8`` layout,
        channels >= Ct written as zero, dbias [Cw] = column sums of wide.
        ``mode = lib.END_WGRAD_OUT`` (conv_out: thin = dy, wide = x): dw [Ct,9,Cw] in the ``pack_conv_cout4`` layout,
        dbias [Ct] = sums of the rounded thin planes.
        ``splitm`` = number of slices of the pixel reduction; ``None`` takes ``end_wgrad_splitm``.  ``splitm > 1`` needs
        ``partial``, fp32 with ``end_wgrad_partial_numel`` elements; the slabs are added in slice order by a second launch
        of the same call, so the result is bit-reproducible."""
        if thin.dim() != 4 or wide.dim() != 4 or thin.dtype != torch.float32 or not thin.is_contiguous():
            raise ValueError(f"end_wgrad takes thin fp32 NCHW (contiguous) and wide NHWC, got {tuple(thin.shape)} {thin.dtype} "
                             f"and {tuple(wide.shape)}")
        b, ct, h, wd = thin.shape
        cw = wide.shape[-1]
        if wide.shape != (b, h, wd, cw):
            raise ValueError(f"end_wgrad: thin {tuple(thin.shape)} and wide {tuple(wide.shape)} are not one map")
        fn = getattr(self.lib, "dadd_conv_end_wgrad_" + _sfx(wide))
        nb = cw if mode == L.END_WGRAD_IN else ct
        want = (cw, 9, 8) if mode == L.END_WGRAD_IN else (ct, 9, cw)
        if dw.dtype != torch.float32 or not dw.is_contiguous() or (mode in (L.END_WGRAD_IN, L.END_WGRAD_OUT)
                                                                   and dw.numel() != want[0] * want[1] * want[2]):
            raise ValueError(f"end_wgrad: dw must be contiguous fp32 {want}, got {tuple(dw.shape)} {dw.dtype}")
        if dbias is not None and (dbias.dtype != torch.float32 or not dbias.is_contiguous() or dbias.numel() != nb):
            raise ValueError(f"end_wgrad: dbias must be contiguous fp32 [{nb}], got {tuple(dbias.shape)} {dbias.dtype}")
        if splitm is None:
            splitm = self.end_wgrad_splitm(b * h * wd, cw)
        if splitm > 1 and partial is not None:      # (a missing partial is the library's to refuse)
            need = self.end_wgrad_partial_numel(splitm, ct, cw, mode)
            if partial.dtype != torch.float32 or not partial.is_contiguous() or partial.numel() < need:
                raise ValueError(f"end_wgrad: partial must be contiguous fp32 with at least {need} elements, got "
                                 f"{tuple(partial.shape)} {partial.dtype}")
        d = self._edesc
        d.thin, d.wide, d.dw, d.dbias, d.partial = _p(thin), _p(wide), _p(dw), _p(dbias), _p(partial)
        d.B, d.H, d.W, d.Ct, d.Cw = b, h, wd, ct, cw
        d.ld_wide, d.mode, d.splitm = self._pixel_ld(wide), int(mode), int(splitm)
        L.check(fn(C.byref(d), self.s))

    def mse_rows_grad(self, pred, target, rowgrad, out):
        """Backward of ``mse_rows``: out[b] = rowgrad[b] * (2 / per_sample) * (pred[b] - target[b]), all fp32; ``rowgrad``
        [B] is the gradient of the B row means and is read on the device."""
        b = pred.shape[0]
        for t in (pred, target, rowgrad, out):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"mse_rows_grad takes contiguous fp32 tensors, got {tuple(t.shape)} {t.dtype}")
        if pred.shape != target.shape or out.shape != pred.shape or rowgrad.numel() != b:
            raise ValueError(f"mse_rows_grad: pred {tuple(pred.shape)}, target {tuple(target.shape)}, out {tuple(out.shape)} "
                             f"and rowgrad {tuple(rowgrad.shape)} do not belong together")
        L.check(self.lib.dadd_mse_rows_grad_f32(_p(pred), _p(target), _p(rowgrad), _p(out), b, pred.numel() // b, self.s))

    def dgrad_resample(self, dy, wt, dx, *, stride=1, ups=0):
        """Data gradient of the stride-2 (``stride=2``) or upsampled (``ups=1``) 3x3 ``igemm``, exactly one of the two:
        dy [B,Ho,Wo,N] and the re-laid weight wt (``grad_ops.dgrad_weight_stride2`` [C,9N] or ``dgrad_weight_ups``
        [C,16N]) -> dx [B,Hi,Wi,C], every pixel overwritten (csrc/dgrad.hip).  dy and dx are fp16 or bf16 and may be
        channel slices of wider tensors: the row strides travel.  One launch, bit-reproducible."""
        if (stride, int(ups)) not in ((2, 0), (1, 1)):
            raise ValueError(f"dgrad_resample takes exactly one of stride=2 or ups=1, got stride {stride}, ups {ups}")
        b, ho, wo, n = dy.shape
        bx, hi, wi, c = dx.shape
        t = 16 if ups else 9
        if bx != b or wt.dim() != 2 or wt.shape != (c, t * n) or not wt.is_contiguous():
            raise ValueError(f"dgrad_resample: dy {tuple(dy.shape)}, dx {tuple(dx.shape)} take a contiguous wt [{c}, {t}*{n}], "
                             f"got {tuple(wt.shape)}")
        fn = getattr(self.lib, "dadd_conv_dgrad_" + _sfx(dy, wt, dx))
        d = self._ddesc
        d.dy, d.wt, d.dx = _p(dy), _p(wt), _p(dx)
        d.B, d.Hi, d.Wi, d.C, d.Ho, d.Wo, d.N = b, hi, wi, c, ho, wo, n
        d.mode = L.DGRAD_UPS if ups else L.DGRAD_STRIDE2
        d.ld_dy, d.ld_dx = self._pixel_ld(dy), self._pixel_ld(dx)
        L.check(fn(C.byref(d), self.s))

    def groupnorm(self, x1, x2, gamma, beta, out, ws, groups, eps, silu, ws_chunks=0):
        """``ws_chunks`` > 0: ``ws`` holds the chunk partials written by the producing GEMM's epilogue."""
        b = x1.shape[0]
        hw = x1.shape[1] * x1.shape[2]
        c1 = x1.shape[-1]
        c2 = 0 if x2 is None else x2.shape[-1]
        need = (ws_chunks + (64 if ws_chunks > 128 else 0)) if ws_chunks else L.GN_MAX_CHUNKS
        assert out.shape[-1] == c1 + c2 and ws.numel() >= b * need * groups * 2
        fn = getattr(self.lib, "dadd_groupnorm_" + _sfx(x1, x2, out))
        L.check(fn(_p(x1), c1, _p(x2), c2, _p(gamma), _p(beta), _p(out), _p(ws), b, hw, groups, float(eps), int(silu),
                   int(ws_chunks), self.s))

    def layernorm(self, x, gamma, beta, out, eps=1e-5):
        c = x.shape[-1]
        m = x.numel() // c
        fn = getattr(self.lib, "dadd_layernorm_" + _sfx(x, out))
        L.check(fn(_p(x), _p(gamma), _p(beta), _p(out), m, c, float(eps), self.s))

    # -- training backward of the norms and GEGLU (csrc/norm_grad.hip)
    def groupnorm_grad_ws_numel(self, b, hw, c, groups):
        """fp32 elements of the ``ws`` scratch of a ``groupnorm_grad`` call: the chunk partials of the statistics, of
        s1 / s2 and of the channel sums (include/dadd_hip_norm_grad.h)."""
        return self._scratch_numel(self.lib.dadd_groupnorm_grad_ws_floats, (b, hw, c, groups),
                                   "groupnorm_grad takes C a multiple of 8 up to 4096 and groups <= 32 dividing C "
                                   "(got B {}, HW {}, C {}, groups {})")

    def groupnorm_grad(self, x1, x2, dy, gamma, beta, *, dx1=None, dx2=None, dgamma=None, dbeta=None, ws, groups, eps,
                       silu):
        """Backward of ``groupnorm``: from the forward's input x1 [B,H,W,C1] (+ x2 [B,H,W,C2], a skip-concat) and
        dy [B,H,W,C1+C2], all fp16 or all bf16, dx1 / dx2 in the same type and dgamma / dbeta [C] in fp32, overwritten.
        Mean and rstd are recomputed from x; with ``silu`` dy is first taken through the derivative of SiLU at the
        normalised value.  ``dx1`` None: parameter gradients only; ``dgamma`` and ``dbeta`` None: data gradient only.
        ``ws`` is fp32 scratch of ``groupnorm_grad_ws_numel`` elements.  Four launches (statistics, chunk partials,
        apply, column sums), every sum in a fixed order: the result is bit-reproducible."""
        if x1.dim() != 4 or dy.dim() != 4:
            raise ValueError(f"groupnorm_grad takes NHWC tensors, got {tuple(x1.shape)} and {tuple(dy.shape)}")
        b, hw, c1 = x1.shape[0], x1.shape[1] * x1.shape[2], x1.shape[-1]
        c2 = 0 if x2 is None else x2.shape[-1]
        c = c1 + c2
        fn = getattr(self.lib, "dadd_groupnorm_grad_" + _sfx(x1, x2, dy, dx1, dx2))
        need = self.groupnorm_grad_ws_numel(b, hw, c, groups)
        if c1 % 8 or c2 % 8:
            raise ValueError(f"groupnorm_grad: C1 = {c1} and C2 = {c2} must be multiples of 8")
        for t in (x1, x2, dy, dx1, dx2):
            assert t is None or (t.is_contiguous() and t.dtype in _SFX), "16-bit contiguous tensors expected"
        assert dy.shape == x1.shape[:-1] + (c,) and (x2 is None or x2.shape[:-1] == x1.shape[:-1])
        assert gamma.dtype == beta.dtype == torch.float32 and gamma.numel() == beta.numel() == c \
            and gamma.is_contiguous() and beta.is_contiguous()
        # (the asserts keep the parent's order - together / shaped / dx shapes / ws - so a call that breaks several rules
        # fails on the same one, with the same message, as before the checks were shared)
        together, shaped, ws_ok = self._param_grad_checks(dgamma, dbeta, c, ws, need)
        assert together and (dx1 is not None or dgamma is not None)
        assert shaped
        assert (dx1 is None or dx1.shape == x1.shape) and ((dx2 is not None) == (dx1 is not None and x2 is not None)) \
            and (dx2 is None or dx2.shape == x2.shape)
        assert ws_ok, (ws.shape, need)
        d = self._gdesc
        d.x1, d.x2, d.dy, d.gamma, d.beta = _p(x1), _p(x2), _p(dy), _p(gamma), _p(beta)
        d.dx1, d.dx2, d.dgamma, d.dbeta, d.ws = _p(dx1), _p(dx2), _p(dgamma), _p(dbeta), _p(ws)
        d.B, d.HW, d.C1, d.C2, d.groups, d.silu, d.eps = b, hw, c1, c2, int(groups), int(bool(silu)), float(eps)
        L.check(fn(C.byref(d), self.s))

    def layernorm_grad_ws_numel(self, m, c):
        """fp32 elements of the ``ws`` scratch of ``layernorm_grad``: per-workgroup column sums [nblk][C][2]."""
        return self._scratch_numel(self.lib.dadd_layernorm_grad_ws_floats, (m, c),
                                   "layernorm_grad takes C a multiple of 8 up to 2048 and at least one row (got M {}, C {})")

    def layernorm_grad(self, x, dy, gamma, *, dx=None, dgamma=None, dbeta=None, ws=None, eps=1e-5):
        """Backward of ``layernorm`` over the last axis: from the forward's input x [..., C] and dy of the same shape (fp16
        or bf16), dx in the same type and dgamma / dbeta [C] in fp32, overwritten.  Mean and rstd of every row are
        recomputed (two-pass).  ``dx`` None: parameter gradients only; ``dgamma`` and ``dbeta`` None: data gradient only.
        The parameter gradients need ``ws``, fp32 scratch of ``layernorm_grad_ws_numel`` elements.  One launch over the
        rows and one for the column sums, fixed summation order: bit-reproducible."""
        c = x.shape[-1]
        m = x.numel() // max(c, 1)
        fn = getattr(self.lib, "dadd_layernorm_grad_" + _sfx(x, dy, dx))
        need = self.layernorm_grad_ws_numel(m, c)
        for t in (x, dy, dx):
            assert t is None or (t.is_contiguous() and t.dtype in _SFX and t.shape == x.shape), "x, dy, dx: one 16-bit shape"
        assert gamma.dtype == torch.float32 and gamma.numel() == c and gamma.is_contiguous()
        # (same order as groupnorm_grad; ws is asked for only with the parameter gradients, and its message is ``need``)
        together, shaped, ws_ok = self._param_grad_checks(dgamma, dbeta, c, ws, need)
        assert together and (dx is not None or dgamma is not None)
        assert shaped
        assert dgamma is None or ws_ok, need
        L.check(fn(_p(x), _p(dy), _p(gamma), _p(dx), _p(dgamma), _p(dbeta), _p(ws), m, c, float(eps), self.s))

    def geglu(self, h, y):
        """GEGLU as a layer of its own: h [..., 2F] with the hidden half in [..., :F] and the gate in [..., F:] (chunk(2)
        order, not the interleaved weight rows of EPI_GEGLU) -> y [..., F] = hidden * gelu(gate), fp16 or bf16.  The
        training step keeps h for ``geglu_grad``; the inference plans keep the GEMM epilogue."""
        f = y.shape[-1]
        fn = getattr(self.lib, "dadd_geglu_" + _sfx(h, y))
        self._pointwise_width("geglu", f)
        assert h.shape == y.shape[:-1] + (2 * f,) and h.is_contiguous() and y.is_contiguous() and h.dtype in _SFX
        L.check(fn(_p(h), _p(y), h.numel() // (2 * f), f, self.s))

    def geglu_grad(self, h, dy, dh):
        """Backward of ``geglu``: dh[..., :F] = dy * gelu(gate) and dh[..., F:] = dy * hidden * gelu'(gate), gelu' from the
        same erf approximation as the forward.  h and dh [..., 2F], dy [..., F], all fp16 or all bf16."""
        f = dy.shape[-1]
        fn = getattr(self.lib, "dadd_geglu_grad_" + _sfx(h, dy, dh))
        self._pointwise_width("geglu_grad", f)
        assert h.shape == dy.shape[:-1] + (2 * f,) and dh.shape == h.shape and h.dtype in _SFX
        assert h.is_contiguous() and dy.is_contiguous() and dh.is_contiguous()
        L.check(fn(_p(h), _p(dy), _p(dh), h.numel() // (2 * f), f, self.s))

    # -- training kernels of the conditioning front-end (csrc/cond_grad.hip)
    def gelu(self, x, y):
        """Exact-form GELU as a layer of its own: y = gelu(x) over x [..., F], fp16 or bf16, the value the EPI_GELU
        epilogue stores for the same rounded input.  The training step keeps x for ``gelu_grad``; the inference modules
        keep the GEMM epilogue."""
        f = x.shape[-1]
        fn = getattr(self.lib, "dadd_gelu_" + _sfx(x, y))
        self._pointwise_width("gelu", f)
        assert y.shape == x.shape and x.is_contiguous() and y.is_contiguous() and x.dtype in _SFX
        L.check(fn(_p(x), _p(y), x.numel() // f, f, self.s))

    def gelu_grad(self, x, dy, dx):
        """Backward of ``gelu``: dx = dy * (Phi(x) + x * phi(x)), Phi from the same erf approximation as the forward.
        x, dy and dx [..., F], all fp16 or all bf16."""
        f = x.shape[-1]
        fn = getattr(self.lib, "dadd_gelu_grad_" + _sfx(x, dy, dx))
        self._pointwise_width("gelu_grad", f)
        assert dy.shape == x.shape and dx.shape == x.shape and x.dtype in _SFX
        assert x.is_contiguous() and dy.is_contiguous() and dx.is_contiguous()
        L.check(fn(_p(x), _p(dy), _p(dx), x.numel() // f, f, self.s))

    def purifier_gate_tail(self, img, dis, z, gamma, beta, out, eps=1e-5):
        """The FeaturePurifier's tail for training: out = LayerNorm(img - sigmoid(z) * dis) over the last axis.  img, dis
        and z [..., C] fp16 or bf16, z the gate's pre-activation (``purifier_tail`` takes the gate itself); gamma, beta
        fp32 [C]; out fp32 [..., C].  C a multiple of 8, at most 2048."""
        c = img.shape[-1]
        fn = getattr(self.lib, "dadd_purifier_gate_tail_" + _sfx(img, dis, z))
        for t in (img, dis, z):
            assert t.is_contiguous() and t.dtype in _SFX and t.shape == img.shape, "img, dis, z: one 16-bit shape"
        assert out.dtype == torch.float32 and out.shape == img.shape and out.is_contiguous()
        assert all(t.dtype == torch.float32 and t.numel() == c and t.is_contiguous() for t in (gamma, beta))
        L.check(fn(_p(img), _p(dis), _p(z), _p(gamma), _p(beta), _p(out), img.numel() // max(c, 1), c, float(eps), self.s))

    def purifier_gate_tail_grad_ws_numel(self, m, c):
        """fp32 elements of the ``ws`` scratch of ``purifier_gate_tail_grad``: per-workgroup column sums [nblk][C][2]."""
        return self._scratch_numel(self.lib.dadd_purifier_gate_tail_grad_ws_floats, (m, c),
                                   "purifier_gate_tail_grad takes C a multiple of 8 up to 2048 and at least one row (got M {}, C {})")

    def purifier_gate_tail_grad(self, img, dis, z, dout, gamma, *, dimg=None, ddis=None, dz=None, dgamma=None, dbeta=None,
                                ws=None, eps=1e-5):
        """Backward of ``purifier_gate_tail``: from the forward's inputs img, dis, z [..., C] (fp16 or bf16) and the fp32
        dout of the same shape, dimg / ddis / dz in the inputs' type and dgamma / dbeta [C] in fp32, overwritten.  The
        gate, the row statistics and xhat are recomputed.  Each of ``dimg`` / ``ddis`` / ``dz`` may be None; ``dgamma`` and
        ``dbeta`` are None together; at least one output.  The parameter gradients need ``ws``, fp32 scratch of
        ``purifier_gate_tail_grad_ws_numel`` elements.  One launch over the rows and one for the column sums, fixed
        summation order: bit-reproducible."""
        c = img.shape[-1]
        m = img.numel() // max(c, 1)
        fn = getattr(self.lib, "dadd_purifier_gate_tail_grad_" + _sfx(img, dis, z, dimg, ddis, dz))
        need = self.purifier_gate_tail_grad_ws_numel(m, c)
        for t in (img, dis, z, dimg, ddis, dz):
            assert t is None or (t.is_contiguous() and t.dtype in _SFX and t.shape == img.shape), "one 16-bit shape"
        assert dout.dtype == torch.float32 and dout.shape == img.shape and dout.is_contiguous()
        assert gamma.dtype == torch.float32 and gamma.numel() == c and gamma.is_contiguous()
        # (the two ValueErrors come before the asserts, as they always did: "come together" wins over "no output")
        together, shaped, ws_ok = self._param_grad_checks(dgamma, dbeta, c, ws, need)
        if not together:
            raise ValueError("purifier_gate_tail_grad: dgamma and dbeta come together")
        if dimg is None and ddis is None and dz is None and dgamma is None:
            raise ValueError("purifier_gate_tail_grad: no output")
        assert shaped
        assert dgamma is None or ws_ok, need
        L.check(fn(_p(img), _p(dis), _p(z), _p(dout), _p(gamma), _p(dimg), _p(ddis), _p(dz), _p(dgamma), _p(dbeta), _p(ws),
                   m, c, float(eps), self.s))

    # -- training backward of the fp32 row path (csrc/rows_grad.hip)
    def linear_rows_grad_ws_numel(self, m, k, n):
        """fp32 elements of the ``ws`` scratch of ``linear_rows_grad`` with ``dx``: the per-strip partial sums
        [strips][M][K]."""
        return self._scratch_numel(self.lib.dadd_linear_rows_grad_ws_floats, (m, k, n),
                                   "linear_rows_grad takes K a multiple of 8 up to 2048 and M, N >= 1 (got M {}, K {}, N {})")

    def linear_rows_grad(self, x, w, dy, *, dx=None, dw=None, db=None, ws=None, act_in=0):
        """Backward of ``linear_rows(x, w, bias, out, act_in, 0)``: from the forward's fp32 input x [M][K] (the
        pre-activation), w [N][K] (fp16 or fp32) and the fp32 dy [M][N]: dx [M][K], dw [N][K] (fp32 also for an fp16 w) and
        db [N], overwritten.  ``dx`` may be None; ``dw`` and ``db`` None together, or ``db`` alone; at least one output.
        ``dx`` needs ``ws``, fp32 scratch of ``linear_rows_grad_ws_numel`` elements (allocated here when None).  Fixed
        summation order: bit-reproducible."""
        m, k = x.shape
        n = w.shape[0]
        need = self.linear_rows_grad_ws_numel(m, k, n)
        if act_in not in (0, 1, 2):
            raise ValueError(f"linear_rows_grad: act_in must be 0, 1 (SiLU) or 2 (GELU), got {act_in}")
        if dx is None and dw is None:
            raise ValueError("linear_rows_grad: no output")
        if dw is None and db is not None:
            raise ValueError("linear_rows_grad: db comes with dw")
        assert w.shape == (n, k) and w.dtype in (torch.float16, torch.float32) and w.is_contiguous()
        assert x.dtype == torch.float32 and x.is_contiguous()
        assert dy.dtype == torch.float32 and dy.shape == (m, n) and dy.is_contiguous()
        for t, shape in ((dx, (m, k)), (dw, (n, k)), (db, (n,))):
            assert t is None or (t.dtype == torch.float32 and t.shape == shape and t.is_contiguous()), shape
        if dx is not None:
            if ws is None:
                ws = self.empty((need,), torch.float32)
            assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= need, need
        L.check(self.lib.dadd_linear_rows_grad_f32(_p(x), _p(w), _p(dy), _p(dx), _p(dw), _p(db), _p(ws), m, k, n, int(act_in),
                                                   int(w.dtype == torch.float32), self.s))

    def aoe_interp_grad(self, labels, dout, dbase, ddeltas):
        """Backward of ``aoe_interp``: labels fp32 [B], dout fp32 [B][D] -> dbase [D] and ddeltas [classes - 1][D],
        overwritten; classes <= 16.  The labels get no gradient."""
        b, d = dout.shape
        classes = ddeltas.shape[0] + 1
        if not 2 <= classes <= 16:
            raise ValueError(f"aoe_interp_grad takes 2..16 classes, got {classes}")
        assert labels.shape == (b,) and dbase.shape == (d,) and ddeltas.shape == (classes - 1, d)
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (labels, dout, dbase, ddeltas))
        L.check(self.lib.dadd_aoe_interp_grad_f32(_p(labels), _p(dout), _p(dbase), _p(ddeltas), b, d, classes, self.s))

    def rowvec_grad_ws_numel(self, b, hw, c):
        """fp32 elements of the ``ws`` scratch of ``rowvec_grad``: the column sums of every 64-pixel chunk."""
        return self._scratch_numel(self.lib.dadd_rowvec_grad_ws_floats, (b, hw, c),
                                   "rowvec_grad takes C a multiple of 8, B in 1..65535 and HW >= 1 (got B {}, HW {}, C {})")

    def rowvec_grad(self, dy, drow, ws=None):
        """Gradient of the row ``EPI_ROWVEC`` adds: drow[b][c] = sum over the pixels of dy [B, ..., C] (fp16 or bf16, NHWC)
        in fp32, overwritten.  ``ws``: fp32 scratch of ``rowvec_grad_ws_numel`` elements (allocated here when None)."""
        b, c = dy.shape[0], dy.shape[-1]
        hw = dy.numel() // max(b * c, 1)
        fn = getattr(self.lib, "dadd_rowvec_grad_" + _sfx(dy))
        need = self.rowvec_grad_ws_numel(b, hw, c)
        if ws is None:
            ws = self.empty((need,), torch.float32)
        assert dy.is_contiguous() and drow.dtype == torch.float32 and drow.shape == (b, c) and drow.is_contiguous()
        assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= need, need
        L.check(fn(_p(dy), _p(drow), _p(ws), b, hw, c, self.s))

    # -- training backward of attention (csrc/attn_grad.hip)
    def attn_grad_ws_numel(self, b, heads, nq):
        """fp32 elements of the ``ws`` scratch of an ``attn_grad`` call: (LSE, D) per (sample, head, query row)."""
        return self._scratch_numel(self.lib.dadd_attn_grad_ws_floats, (b, heads, nq),
                                   "attn_grad takes positive sizes (got B {}, heads {}, Nq {})")

    @staticmethod
    def _token_ld(t, what):
        """(row stride, sample stride) of a [B,N,C] view: a column block of wider rows and / or a token range of a
        longer sequence."""
        if t.dim() != 3 or t.stride(2) != 1:
            raise ValueError(f"attn_grad: {what} must be a [B,N,C] view with unit column stride, got shape "
                             f"{tuple(t.shape)} strides {t.stride()}")
        return t.stride(1), (t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.stride(1))

    def attn_grad(self, q, k, v, dout, *, dq=None, dk=None, dv=None, ws, heads, do_scale=1.0, do_scale_dev=None):
        """Backward of ``attention`` / ``self_attn``: from q, dout [B,Nq,C] and k, v [B,Nk,C] (fp16 or bf16, strided 3-D
        views: column blocks of wider rows are fine, k and v share one row stride) the gradients dq [B,Nq,C] and
        dk, dv [B,Nk,C] (one row stride) of softmax(q k^T / sqrt(d)) v, for dout * do_scale * do_scale_dev[0]
        (``do_scale_dev``: device fp32[1], read by the kernels).  Each output may be None; without dk and dv the dkv launch
        is skipped, without dq the dq launch.  ``ws`` is fp32 scratch of ``attn_grad_ws_numel`` elements.  Up to three
        launches (row statistics, dK / dV, dQ), fixed summation order: bit-reproducible.  d in {40, 80, 96, 160}; Nq a
        multiple of 16; Nk any positive count (257 CLIP tokens: the rows past Nk of a longer buffer are never touched)."""
        fn = getattr(self.lib, "dadd_attn_grad_" + _sfx(q, k, v, dout, dq, dk, dv))
        for t in (q, k, v, dout, dq, dk, dv):
            if t is not None and t.dtype not in _SFX:
                raise ValueError(f"attn_grad takes 16-bit tensors, got {t.dtype}")
        b, nq, c = q.shape
        nk = k.shape[1]
        if c % heads:
            raise ValueError(f"attn_grad: C = {c} is not a multiple of heads = {heads}")
        if dq is None and dk is None and dv is None:
            raise ValueError("attn_grad: no output")
        assert dout.shape == q.shape and k.shape == (b, nk, c) and v.shape == k.shape
        assert all(t is None or t.shape == q.shape for t in (dq,)) and all(t is None or t.shape == k.shape for t in (dk, dv))
        (ld_q, bs_q), (ld_kv, bs_kv), (ld_do, bs_do) = self._token_ld(q, "q"), self._token_ld(k, "k"), self._token_ld(dout, "dout")
        if self._token_ld(v, "v") != (ld_kv, bs_kv):
            raise ValueError("attn_grad: k and v must share their strides")
        ld_dq, bs_dq = self._token_ld(dq, "dq") if dq is not None else (0, 0)
        lds = {self._token_ld(t, "dk / dv") for t in (dk, dv) if t is not None}
        if len(lds) > 1:
            raise ValueError("attn_grad: dk and dv must share their strides")
        ld_dkv, bs_dkv = lds.pop() if lds else (0, 0)
        need = self.attn_grad_ws_numel(b, heads, nq)
        assert ws is not None and ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= need, need
        assert do_scale_dev is None or (do_scale_dev.dtype == torch.float32 and do_scale_dev.numel() >= 1)
        d = self._adesc
        d.q, d.k, d.v, d.dout = _p(q), _p(k), _p(v), _p(dout)
        d.dq, d.dk, d.dv, d.ws, d.do_scale_dev = _p(dq), _p(dk), _p(dv), _p(ws), _p(do_scale_dev)
        d.B, d.Nq, d.Nk, d.heads, d.d = b, nq, nk, heads, c // heads
        d.ld_q, d.ld_kv, d.ld_do, d.ld_dq, d.ld_dkv = ld_q, ld_kv, ld_do, ld_dq, ld_dkv
        d.bs_q, d.bs_kv, d.bs_do, d.bs_dq, d.bs_dkv = bs_q, bs_kv, bs_do, bs_dq, bs_dkv
        d.do_scale = float(do_scale)
        L.check(fn(C.byref(d), self.s))

    # -- the optimizer step (csrc/optim.hip); optim.FusedAdamW is the owner of these buffers
    @staticmethod
    def _optim_flat(t, what, n=None, dtype=torch.float32):
        if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or (n is not None and t.numel() != n):
            raise ValueError(f"optim: {what} must be a flat contiguous {dtype} tensor" + (f" of {n} elements" if n else "") +
                             f", got {tuple(t.shape)} {t.dtype}")

    def optim_grad_stats(self, g, partials, flags, *, max_blocks=0):
        """One pass over the flat fp32 gradient ``g`` (a multiple of ``lib.OPTIM_CHUNK`` elements): ``partials`` [chunks]
        fp32 = sum of g^2 per chunk, ``flags`` [chunks] int32 = 1 where a chunk holds an inf or NaN.  Fixed summation order,
        the result does not depend on ``max_blocks`` (the cap of the grid; 0 = the kernel's default)."""
        n = g.numel()
        if n == 0 or n % L.OPTIM_CHUNK:
            raise ValueError(f"optim_grad_stats: {n} elements is not a positive multiple of the chunk {L.OPTIM_CHUNK}")
        self._optim_flat(g, "g")
        self._optim_flat(partials, "partials", n // L.OPTIM_CHUNK)
        self._optim_flat(flags, "flags", n // L.OPTIM_CHUNK, torch.int32)
        L.check(self.lib.dadd_optim_grad_stats(_p(g), n, _p(partials), _p(flags), int(max_blocks), self.s))

    def optim_finalize(self, partials, flags, state):
        """One workgroup: from the chunk partials and flags to the norm, the clip coefficient, the step count, the
        per-group constants and the loss scale in ``state`` (int32 words of ``lib.OptimState``), all on the device."""
        self._optim_flat(partials, "partials")
        self._optim_flat(flags, "flags", partials.numel(), torch.int32)
        self._optim_flat(state, "state", C.sizeof(L.OptimState) // 4, torch.int32)
        L.check(self.lib.dadd_optim_finalize(_p(partials), _p(flags), partials.numel(), _p(state), self.s))

    def optim_adamw_step(self, p, g, m, v, state, group_chunks, *, ema=None, p16=None, ema_weight=0.0, flags=0, max_blocks=0):
        """The fused AdamW pass over the flat fp32 arrays ``p, g, m, v`` with the constants ``optim_finalize`` left in
        ``state``; ``group_chunks``: chunks per group (a sequence or a ctypes int array).  ``flags`` (``lib.OPTIM_*``)
        select the EMA update into ``ema`` (weight ``ema_weight`` = 1 - decay), the 16-bit copy into ``p16`` (its dtype
        must match the flag) and the zeroing of ``g``."""
        n = p.numel()
        for t, what in ((p, "p"), (g, "g"), (m, "m"), (v, "v")) + (((ema, "ema"),) if ema is not None else ()):
            self._optim_flat(t, what, n)
        self._optim_flat(state, "state", C.sizeof(L.OptimState) // 4, torch.int32)
        want16 = {L.OPTIM_P16_F16: torch.float16, L.OPTIM_P16_BF16: torch.bfloat16}.get(flags & (L.OPTIM_P16_F16 | L.OPTIM_P16_BF16))
        if (p16 is None) != (want16 is None) or (p16 is not None and flags & L.OPTIM_P16_F16 and flags & L.OPTIM_P16_BF16):
            raise ValueError("optim_adamw_step: p16 goes with exactly one of OPTIM_P16_F16 / OPTIM_P16_BF16")
        if p16 is not None:
            self._optim_flat(p16, "p16", n, want16)
        if bool(flags & L.OPTIM_EMA) != (ema is not None):
            raise ValueError("optim_adamw_step: ema goes with OPTIM_EMA")
        if not isinstance(group_chunks, C.Array):
            group_chunks = (C.c_int * len(group_chunks))(*group_chunks)
        L.check(self.lib.dadd_optim_adamw_step(_p(p), _p(g), _p(m), _p(v), _p(ema), _p(p16), n, group_chunks, len(group_chunks),
                                               _p(state), float(ema_weight), int(flags), int(max_blocks), self.s))

    def dgrad_relayout(self, src, dst, table, n_desc, n_tiles):
        """One launch (csrc/relayout.hip): from the flat 16-bit ``src`` (the arena's ``p16``) into the flat ``dst`` of the
        same type, for every descriptor of ``table`` what ``grad_ops.dgrad_weight`` / ``_stride2`` / ``_ups`` / ``_cout4``
        give for that tensor.  ``table``: the device copy (int32 words) of an array of ``lib.RelayoutDesc`` that
        ``dadd_dgrad_relayout_plan`` has checked against both lengths; ``n_tiles`` its return value.
        ``optim.DgradRelayout`` is the owner of table and buffer."""
        fn = getattr(self.lib, "dadd_dgrad_relayout_" + _sfx(src, dst))
        words = C.sizeof(L.RelayoutDesc) // 4
        if src.dim() != 1 or dst.dim() != 1 or not src.is_contiguous() or not dst.is_contiguous():
            raise ValueError(f"dgrad_relayout: src and dst must be flat contiguous 16-bit tensors, got {tuple(src.shape)} "
                             f"and {tuple(dst.shape)}")
        if table.dtype != torch.int32 or table.dim() != 1 or not table.is_contiguous() or table.numel() != n_desc * words \
                or n_desc < 1 or n_tiles < 1:
            raise ValueError(f"dgrad_relayout: table must be {n_desc} x {words} contiguous int32 words and n_tiles positive, "
                             f"got {tuple(table.shape)} {table.dtype}, n_tiles {n_tiles}")
        L.check(fn(_p(src), src.numel(), _p(dst), dst.numel(), _p(table), int(n_desc), int(n_tiles), self.s))

    def plan_refresh(self, src, table, n_desc, n_wgs, dtype=torch.float16):
        """One launch (csrc/plan_refresh.hip): from the flat fp32 ``src`` (the arena's ``p`` or ``ema``) into the
        destinations the descriptors of ``table`` point to, for each what its packer in ``engine`` gives.  ``table``: the
        device copy (int32 words) of an array of ``lib.PlanRefreshDesc`` that ``dadd_plan_refresh_plan`` has checked;
        ``n_wgs`` its return value; ``dtype`` the 16-bit type of the table's destinations.  ``optim.PlanRefresh`` is the
        owner of the tables."""
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"plan_refresh: destinations are fp16 or bf16, not {dtype}")
        fn = getattr(self.lib, "dadd_plan_refresh_" + ("bf16" if dtype == torch.bfloat16 else "f16"))
        words = C.sizeof(L.PlanRefreshDesc) // 4
        if src.dtype != torch.float32 or src.dim() != 1 or not src.is_contiguous():
            raise ValueError(f"plan_refresh: src must be a flat contiguous fp32 tensor, got {tuple(src.shape)} {src.dtype}")
        if table.dtype != torch.int32 or table.dim() != 1 or not table.is_contiguous() or table.numel() != n_desc * words \
                or n_desc < 1 or n_wgs < 1:
            raise ValueError(f"plan_refresh: table must be {n_desc} x {words} contiguous int32 words and n_wgs positive, "
                             f"got {tuple(table.shape)} {table.dtype}, n_wgs {n_wgs}")
        L.check(fn(_p(src), src.numel(), _p(table), int(n_desc), int(n_wgs), self.s))

    # ------------------------------------------------------------------ evaluation metrics (csrc/metrics.hip)
    def metrics_scratch_bytes(self, n, m=0, sigmas=0):
        """Bytes of scratch ``feat_prepare`` / ``rbf_mmd`` take for sets of ``n`` and ``m`` rows and ``sigmas`` bandwidths."""
        need = int(self.lib.dadd_metrics_scratch_bytes(int(n), int(m), int(sigmas)))
        if need < 0:
            raise ValueError(f"metrics: no scratch size for n = {n}, m = {m}, {sigmas} bandwidths")
        return need

    @staticmethod
    def _prepared(op, what, xc, sq, d):
        """A prepared set: fp32 contiguous [rows][ldc] with ldc >= d rounded up to ``lib.METRICS_KPAD`` and a multiple of 4,
        and its squared norms fp32 [rows]."""
        kp = -(-int(d) // L.METRICS_KPAD) * L.METRICS_KPAD
        ok = xc.dtype == torch.float32 and xc.dim() == 2 and xc.is_contiguous() and xc.shape[1] >= kp and xc.shape[1] % 4 == 0 \
            and sq.dtype == torch.float32 and sq.is_contiguous() and tuple(sq.shape) == (xc.shape[0],)
        if not ok:
            raise ValueError(f"{op}: {what} must be contiguous fp32 [rows][>= {kp}] with fp32 [rows] squared norms, got "
                             f"{tuple(xc.shape)} {xc.dtype} and {tuple(sq.shape)} {sq.dtype}")

    def clip_preprocess(self, frames, out, mean, std):
        """u8 NHWC ``frames`` [B,H,W,3] -> fp32 NCHW ``out`` [B,3,S,S]: shortest-edge bicubic resize to S, centre crop, /255
        and normalisation with ``mean`` / ``std`` (three floats each), as transformers' ``CLIPImageProcessor``."""
        b, h, w, c = frames.shape
        s = out.shape[-1]
        assert c == 3 and frames.dtype == torch.uint8 and frames.is_contiguous()
        assert out.dtype == torch.float32 and tuple(out.shape) == (b, 3, s, s) and out.is_contiguous()
        assert len(mean) == 3 and len(std) == 3
        L.check(self.lib.dadd_clip_preprocess_u8(_p(frames), _p(out), b, h, w, s, (L.f32 * 3)(*mean), (L.f32 * 3)(*std), self.s))

    def feat_prepare(self, x, y, xc, yc, sqx, sqy, center, scratch, normalize=False):
        """``x`` [n,D] and optionally ``y`` [m,D] (fp32 rows, unit column stride) -> the prepared sets ``xc`` / ``yc``
        [rows][ldc], their squared norms ``sqx`` / ``sqy`` and the common ``center`` [>= D rounded up to 32]; ``normalize``
        scales every row to unit length first.  ``scratch``: uint8, ``metrics_scratch_bytes(n, m)`` bytes."""
        n, d = x.shape
        assert x.dtype == torch.float32 and x.stride(1) == 1 and x.stride(0) >= d
        self._prepared("feat_prepare", "xc / sqx", xc, sqx, d)
        assert xc.shape[0] == n and center.dtype == torch.float32 and center.is_contiguous() and center.numel() >= xc.shape[1]
        m, ldy = 0, 0
        if y is not None:
            m, ldy = y.shape[0], y.stride(0)
            assert y.dtype == torch.float32 and y.shape[1] == d and y.stride(1) == 1 and ldy >= d
            self._prepared("feat_prepare", "yc / sqy", yc, sqy, d)
            assert yc.shape == (m, xc.shape[1])
        assert scratch.dtype == torch.uint8 and scratch.is_contiguous() and scratch.numel() >= self.metrics_scratch_bytes(n, m)
        L.check(self.lib.dadd_feat_prepare_f32(_p(x), n, x.stride(0), _p(y), m, ldy, d, int(bool(normalize)), _p(xc), _p(yc),
                                               xc.shape[1], _p(sqx), _p(sqy), _p(center), _p(scratch), scratch.numel(), self.s))

    def rbf_mmd(self, xc, sqx, yc, sqy, d, sigmas, out, scratch):
        """Prepared sets -> ``out`` (float64 [3 S + 1]): per bandwidth the means of u = 1 - k over the pairs of XX (i != j),
        of YY (i != j) and of XY, as ``out[:3 S].view(3, S)``, and the unbiased MMD^2 in ``out[3 S]``."""
        s = len(sigmas)
        self._prepared("rbf_mmd", "xc / sqx", xc, sqx, d)
        self._prepared("rbf_mmd", "yc / sqy", yc, sqy, d)
        assert xc.shape[1] == yc.shape[1] and 1 <= s <= L.METRICS_MAX_SIGMAS
        assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == 3 * s + 1
        assert scratch.dtype == torch.uint8 and scratch.is_contiguous() \
            and scratch.numel() >= self.metrics_scratch_bytes(xc.shape[0], yc.shape[0], s)
        L.check(self.lib.dadd_rbf_mmd_f32(_p(xc), _p(sqx), xc.shape[0], _p(yc), _p(sqy), yc.shape[0], int(d), xc.shape[1],
                                          (L.f32 * s)(*sigmas), s, _p(out), out.data_ptr() + 8 * 3 * s, _p(scratch),
                                          scratch.numel(), self.s))

    def knn_radius(self, xc, sqx, d, k, radius):
        """``radius`` [n] fp32: the distance from every row of the prepared set to its k-th nearest other row (the (k+1)-th
        smallest with itself counted), ``cdist(x, x).topk(k + 1, largest=False).values[:, -1]``."""
        self._prepared("knn_radius", "xc / sqx", xc, sqx, d)
        assert radius.dtype == torch.float32 and radius.is_contiguous() and tuple(radius.shape) == (xc.shape[0],)
        L.check(self.lib.dadd_knn_radius_f32(_p(xc), _p(sqx), xc.shape[0], int(d), xc.shape[1], int(k), _p(radius), self.s))

    def manifold_hits(self, qc, sqq, rc, sqr, radius, d, hit):
        """``hit`` [nq] int32: 1 where the query row lies within ``radius[j]`` of some reference row j (both sets prepared
        by one ``feat_prepare`` call, so centred on the same vector)."""
        self._prepared("manifold_hits", "qc / sqq", qc, sqq, d)
        self._prepared("manifold_hits", "rc / sqr", rc, sqr, d)
        assert qc.shape[1] == rc.shape[1]
        assert radius.dtype == torch.float32 and radius.is_contiguous() and tuple(radius.shape) == (rc.shape[0],)
        assert hit.dtype == torch.int32 and hit.is_contiguous() and tuple(hit.shape) == (qc.shape[0],)
        L.check(self.lib.dadd_manifold_hits_f32(_p(qc), _p(sqq), qc.shape[0], _p(rc), _p(sqr), _p(radius), rc.shape[0], int(d),
                                                qc.shape[1], _p(hit), self.s))

    def self_attn(self, qkv, out, heads):
        """qkv [B,N,3C] (q|k|v blocks of C columns); out [B,N,C]."""
        b, n, c3 = qkv.shape
        c = c3 // 3
        base = qkv.data_ptr()
        fn = getattr(self.lib, "dadd_self_attn_" + _sfx(qkv, out))
        L.check(fn(base, base + 2 * c, base + 4 * c, _p(out), b, n, heads, c // heads, c3, out.stride(-2), self.s))

    def tri_xattn(self, q, kv, out, gates, lam, mode, heads, lam_dev=None):
        """``lam_dev`` (device float32[1]) overrides ``lam``: lambda is then a device-side parameter."""
        b, n, c = q.shape
        fn = getattr(self.lib, "dadd_tri_xattn_" + _sfx(q, kv, out))
        L.check(fn(_p(q), _p(kv), _p(out), _p(gates), float(lam), _p(lam_dev), int(mode), b, n, heads, c // heads,
                   kv.shape[1], kv.stride(1), self.s))

    def attn2_fused(self, x, mcat, vw, bias, residual, out, ln_stats_out=None, ln_stats_in=None, ln_c1=None, ln_d=None,
                    ln_eps=1e-5):
        """x, residual, out [B,HW,C]; mcat [B,384,C]; vw [B,C,384] (include/dadd_hip.h); ``ln_stats_out`` [C/80][B*HW][2]
        fp32: LayerNorm row partials of ``out`` for the linear behind the next LayerNorm.  ``ln_stats_in`` [P][B*HW][2]
        with ``ln_c1`` / ``ln_d`` [B,384]: norm2 folded in (x un-normalised, mcat carrying gamma)."""
        b, hw, c = x.shape
        assert mcat.shape == (b, 384, c) and vw.shape == (b, c, 384) and out.shape == x.shape
        if _sfx(x, mcat, vw, residual, out) != "f16":
            raise ValueError("attn2_fused has no bf16 form: the bf16 plan takes the to_q + tri_xattn + to_out path")
        if ln_stats_out is not None:
            assert ln_stats_out.shape == (c // 80, b * hw, 2) and ln_stats_out.dtype == torch.float32 \
                and ln_stats_out.is_contiguous()
        parts = 0
        if ln_stats_in is not None:
            assert ln_stats_in.dim() == 3 and ln_stats_in.shape[1:] == (b * hw, 2) and ln_stats_in.dtype == torch.float32 \
                and ln_stats_in.is_contiguous() and ln_c1.shape == (b, 384) and ln_d.shape == (b, 384) \
                and ln_c1.dtype == ln_d.dtype == torch.float32 and ln_c1.is_contiguous() and ln_d.is_contiguous()
            parts = ln_stats_in.shape[0]
        L.check(self.lib.dadd_attn2_fused_f16(_p(x), _p(mcat), _p(vw), _p(bias), _p(residual), _p(out), _p(ln_stats_out),
                                              _p(ln_stats_in), parts, _p(ln_c1), _p(ln_d), float(ln_eps), b, hw, c, self.s))

    def ffn_block(self, x, stream, ln_g, ln_b, b1, b2, bp, xres, out, gn_ws=None, gn_nchunk=0, ln_eps=1e-5):
        """Transformer-block tail in one launch (csrc/ffn_block.hip): x, xres, out [B,HW,320] fp16; ``stream`` / ``b1``
        from ``engine.pack_ffn_stream``; ``gn_ws`` [B*gn_nchunk*64] fp32 receives GroupNorm partials of ``out``
        (chunks of 32 rows)."""
        b, hw, c = x.shape
        assert out.shape == x.shape == xres.shape and x.dtype == out.dtype == xres.dtype == torch.float16
        assert stream.dtype == torch.float16 and stream.numel() * 2 == self.lib.dadd_ffn_block_bytes()
        assert b1.numel() == 2560 and b2.numel() == c and bp.numel() == c and ln_g.numel() == c and ln_b.numel() == c
        assert all(t.dtype == torch.float32 for t in (ln_g, ln_b, b1, b2, bp))
        assert x.is_contiguous() and xres.is_contiguous() and out.is_contiguous()
        if gn_ws is not None:
            assert gn_ws.dtype == torch.float32 and gn_ws.numel() >= b * gn_nchunk * 64
        L.check(self.lib.dadd_ffn_block_f16(_p(x), _p(stream), _p(ln_g), _p(ln_b), float(ln_eps), _p(b1), _p(b2), _p(bp),
                                            _p(xres), _p(out), _p(gn_ws), int(gn_nchunk), b * hw, hw, c, self.s))

    def tf_head(self, x, stream, gn_ws, gn_nchunk, gn_g, gn_b, bp, ln_g, ln_b, hs, qkv, gn_eps=1e-6, ln_eps=1e-5):
        """Transformer-block head in one launch (csrc/tf_head.hip): x, hs [B,HW,320], qkv [B,HW,960] fp16; ``gn_ws`` the
        producer's GroupNorm chunk partials of x ([B*gn_nchunk*64] fp32); ``stream`` from ``engine.pack_head_stream``."""
        b, hw, c = x.shape
        assert hs.shape == x.shape and qkv.shape == (b, hw, 3 * c) and x.dtype == hs.dtype == qkv.dtype == torch.float16
        assert stream.dtype == torch.float16 and stream.numel() * 2 == self.lib.dadd_tf_head_bytes()
        assert gn_ws.dtype == torch.float32 and gn_ws.numel() >= b * gn_nchunk * 64
        assert all(t.dtype == torch.float32 and t.numel() == c for t in (gn_g, gn_b, bp, ln_g, ln_b))
        assert x.is_contiguous() and hs.is_contiguous() and qkv.is_contiguous()
        L.check(self.lib.dadd_tf_head_f16(_p(x), _p(stream), _p(gn_ws), int(gn_nchunk), _p(gn_g), _p(gn_b), float(gn_eps),
                                          _p(bp), _p(ln_g), _p(ln_b), float(ln_eps), _p(hs), _p(qkv), b * hw, hw, c, self.s))

    def timestep_features(self, t, out):
        assert t.dtype == torch.int64 and out.dtype == torch.float32
        L.check(self.lib.dadd_timestep_features_f32(_p(t), _p(out), out.shape[0], out.shape[1], self.s))

    def linear_rows(self, x, w, bias, out, act_in=0, act_out=0):
        """fp32 rows x (fp16 or fp32) weights; act 0 none, 1 SiLU, 2 GELU."""
        m, k = x.shape
        n = w.shape[0]
        assert w.shape[1] == k and out.shape == (m, n) and x.dtype == torch.float32
        assert w.dtype in (torch.float16, torch.float32)
        L.check(self.lib.dadd_linear_rows_f32(_p(x), _p(w), _p(bias), _p(out), m, k, n, act_in,
                                              act_out, int(w.dtype == torch.float32), self.s))

    def attention(self, q, k, v, out, heads):
        """softmax(q k^T / sqrt(d)) v with separate query / key-value lengths: q [B,Nq,*], k, v [B,Nk,*] (views
        into wider rows are fine: the row strides travel), out [B,Nq,C]."""
        b, nq, c = out.shape
        nk = k.shape[1]
        assert q.shape[:2] == (b, nq) and v.shape[:2] == (b, nk) and k.stride(1) == v.stride(1)
        fn = getattr(self.lib, "dadd_attn_" + _sfx(q, k, v, out))
        L.check(fn(_p(q), _p(k), _p(v), _p(out), b, nq, nk, heads, c // heads, q.stride(1), k.stride(1), out.stride(1),
                   self.s))

    def clip_patch_rows(self, pixels, out, patch):
        b, _, h, w = pixels.shape
        assert pixels.dtype == torch.float32 and out.dtype == torch.float16 and out.shape[0] == b
        L.check(self.lib.dadd_clip_patch_rows_f16(_p(pixels), _p(out), b, h, w, patch, out.shape[-1], self.s))

    def aoe_interp(self, labels, base, deltas, out):
        L.check(self.lib.dadd_aoe_interp_f32(_p(labels), _p(base), _p(deltas), _p(out), labels.shape[0],
                                             out.shape[1], deltas.shape[0] + 1, self.s))

    def purifier_tail(self, img, dis, gate, gamma, beta, out, eps=1e-5):
        c = img.shape[-1]
        L.check(self.lib.dadd_purifier_tail_f16(_p(img), _p(dis), _p(gate), _p(gamma), _p(beta), _p(out),
                                                img.numel() // c, c, float(eps), self.s))

    def begin_step(self, table, cur_rows, coef, cur_coef, step):
        assert step.numel() == 2 and step.dtype == torch.int32
        L.check(self.lib.dadd_begin_step(_p(table), _p(cur_rows), cur_rows.shape[0], table.shape[1],
                                         _p(coef), _p(cur_coef), _p(step), self.s))

    def ddim_update(self, x, eps_c, eps_u, guidance, coef, guidance_dev=None):
        L.check(self.lib.dadd_ddim_update_f32(_p(x), _p(eps_c), _p(eps_u), float(guidance), _p(guidance_dev),
                                              _p(coef), x.numel(), self.s))

    def prefetch(self, t: torch.Tensor):
        """Read ``t`` on the library's side stream (a parallel branch inside a graph capture): its lines are in the
        Infinity Cache when a later kernel streams them.  ``prefetch_join`` before the capture ends."""
        if self._prof_on:            # per-launch timing runs one kernel at a time: no side branch
            return
        L.check(self.lib.dadd_prefetch(_p(t), t.numel() * t.element_size(), self.s))

    def prefetch_join(self):
        L.check(self.lib.dadd_prefetch_join(self.s))

    # ------------------------------------------------------------------ graphs / profiling
    def graph_begin(self):
        L.check(self.lib.dadd_graph_begin(self.s))
        self._capturing = True

    def graph_end(self):
        self._capturing = False
        g = C.c_void_p()
        L.check(self.lib.dadd_graph_end(self.s, C.byref(g)))
        return g

    def graph_launch(self, g):
        L.check(self.lib.dadd_graph_launch(g, self.s))

    def graph_destroy(self, g):
        L.check(self.lib.dadd_graph_destroy(g))

    def prof_begin(self):
        """Start recording every kernel launch of the library (eager launches only)."""
        L.check(self.lib.dadd_prof_begin())
        self._prof_on = True

    def prof_end(self):
        """-> list of (kernel name, microseconds, algorithmic flop, algorithmic bytes) in issue order; the time
        is the dispatch's own begin/end timestamp pair (what rocprofv3's kernel trace reports)."""
        n = C.c_int(0)
        self._prof_on = False
        L.check(self.lib.dadd_prof_end(C.byref(n)))
        out, name, vals = [], C.c_char_p(), (C.c_double * 3)()
        for i in range(n.value):
            L.check(self.lib.dadd_prof_record(i, C.byref(name), vals))
            out.append((name.value.decode(), vals[0] * 1e3, vals[1], vals[2]))
        return out
