"""The differentiable operators of a training step: ``torch.autograd.Function``s whose forward and backward are launches
of the HIP kernels through a backend (``HipBackend``, or the reference backends of the test-suite).

Operands: ``x`` is a 16-bit (fp16 or bf16) NHWC / token-major tensor on the backend's device, ``w`` the **fp32 master**
weight in the library layout ``[N][taps*C]`` (``[Cout][ky][kx][Cin]`` flattened), ``bias`` / ``gamma`` / ``beta`` fp32.
The forward of a product rounds the master to ``x.dtype`` once and keeps the rounded copy for the backward; gradients of
``w``, ``bias``, ``gamma`` and ``beta`` come back in fp32, the gradient of ``x`` in ``x.dtype``.  Every backward recomputes
what it needs (statistics, softmax rows, gates) from the saved inputs, in a fixed summation order.

Every operator allocates and launches inside ``on_backend(be)``, the bracket that orders the backend's stream after
torch's current stream and back; what runs before the bracket (casts, re-layouts, ``contiguous()``) is torch work on the
current stream.

=========================================  ==================================  ==========================================
operator                                   forward                             backward
=========================================  ==================================  ==========================================
``linear``, ``conv3x3``                    ``igemm``                           ``dgrad`` (the forward kernel on dy with
                                                                               ``dgrad_weight``), ``wgrad``
``conv3x3(rowvec=)``                       ``igemm`` + ``EPI_ROWVEC``          the same, and ``rowvec_grad``
``downsample2d``, ``upsample2d``           ``igemm`` (stride 2 / upsampled)    ``dgrad_resample`` (``dgrad_weight_stride2``
                                                                               / ``dgrad_weight_ups``), ``wgrad``
``conv_in``, ``conv_out``                  ``conv_in_nchw``, ``conv_cout4``    ``end_wgrad``; ``dgrad_cout4``
                                                                               (``dgrad_weight_cout4``) for conv_out
``mse_rows``                               ``mse_rows``                        ``mse_rows_grad``
``linear_rows``, ``aoe_interp``            the fp32 row path                   ``linear_rows_grad``, ``aoe_interp_grad``
``group_norm``, ``layer_norm``             ``groupnorm``, ``layernorm``        ``groupnorm_grad``, ``layernorm_grad``
``geglu``, ``gelu``                        ``geglu``, ``gelu``                 ``geglu_grad``, ``gelu_grad``
``purifier_gate_tail``                     ``purifier_gate_tail``              ``purifier_gate_tail_grad``
``self_attention``, ``attention``          ``self_attn``, ``attention``        ``attn_grad``
``tri_cross_attention``                    ``tri_xattn``                       one ``attn_grad`` per pathway, the gate or
                                                                               lambda as the scale of dy
=========================================  ==================================  ==========================================

The matrix products take ``prepared=``: the 16-bit copy and the data-gradient layout of a weight that
``optim.DgradRelayout`` keeps, instead of a cast and a torch re-layout per call.  A master weight may be a view of an
``optim.ParamArena``, whose ``.grad`` then accumulates in the arena's flat gradient buffer for ``optim.FusedAdamW``.

These are operators, not the model: ``conditioning_grad`` builds the conditioning front-end and the time path from them,
``unet_grad`` the UNet, ``training.Trainer`` the step.  Not covered: attention with Nq not a multiple of 16 or a head dim
other than 40 / 80 / 96 / 160, and the data gradient of ``conv3x3(stride=2)`` / ``conv3x3(ups=True)`` under those names
(``downsample2d`` / ``upsample2d`` have it); DESIGN.md §7.1.
"""
from __future__ import annotations

import torch

from . import lib as L
from .backend import on_backend      # the stream bracket; ``grad_ops.on_backend`` stays importable


def dgrad_weight(w16: torch.Tensor, taps: int) -> torch.Tensor:
    """``[N][taps*C] -> [C][taps*N]`` with the taps flipped: wt[c][8-tap][n] = w[n][tap][c].  The forward kernel run on
    ``dy`` with this weight is the data gradient of a stride-1 convolution (include/dadd_hip.h); for ``taps == 1`` it is
    the plain transpose.  Applying it twice gives the weight back (with the channel roles swapped twice).
    Torch does the re-layout: one read and one write of the weight per call."""
    n = w16.shape[0]
    c = w16.shape[1] // taps
    assert w16.dim() == 2 and w16.shape[1] == taps * c
    return w16.reshape(n, taps, c).flip(1).permute(2, 1, 0).reshape(c, taps * n).contiguous()


# (ky, kx) of the 9 slabs of ``dgrad_weight_stride2``, in the class order of include/dadd_hip_dgrad.h: the slabs of the
# parity classes (py, px) = (0,0) | (0,1) | (1,0) | (1,1) of the input pixels, 1 + 2 + 2 + 4 taps.  The resolve table
# (``first_slab``, ``ntaps``) and the kernel (source pixel (jy + (ky == 0), jx + (kx == 0))) read this order.
STRIDE2_SLABS = ((1, 1), (1, 0), (1, 2), (0, 1), (2, 1), (0, 0), (0, 2), (2, 0), (2, 2))
# S(e) for e = -1, 0, 1, 2: the taps of a 3-tap axis that reach input pixel i from row 2i + e of the upsampled output
UPS_TAP_SETS = ((2,), (1, 2), (0, 1), (0,))


def dgrad_weight_stride2(w16: torch.Tensor) -> torch.Tensor:
    """``[N][9*C] -> [C][9*N]`` for the data gradient of the stride-2 conv (``HipBackend.dgrad_resample(stride=2)``):
    wt[c][s][n] = w[n][ky_s][kx_s][c] with the slabs s in ``STRIDE2_SLABS`` order, so that the taps of one parity class are
    one contiguous run of K.  A torch re-layout on the current stream, like ``dgrad_weight``."""
    n, c = w16.shape[0], w16.shape[1] // 9
    assert w16.dim() == 2 and w16.shape[1] == 9 * c
    order = [3 * ky + kx for ky, kx in STRIDE2_SLABS]
    return w16.reshape(n, 9, c)[:, order].permute(2, 1, 0).reshape(c, 9 * n).contiguous()


def dgrad_weight_ups(w16: torch.Tensor) -> torch.Tensor:
    """``[N][9*C] -> [C][16*N]`` for the data gradient of the upsampled conv (``HipBackend.dgrad_resample(ups=1)``):
    wt[c][4(e+1) + (f+1)][n] = W4[e][f] = sum of w[n][ky][kx][c] over ky in S(e), kx in S(f) (``UPS_TAP_SETS``), e, f in
    {-1, 0, 1, 2}: the 36 (tap, phase) products of an input pixel collapse onto 16 source pixels of dy.  A 16-bit weight is
    summed in fp32 and rounded once to its type (a float32 / float64 weight is summed as it is)."""
    n, c = w16.shape[0], w16.shape[1] // 9
    assert w16.dim() == 2 and w16.shape[1] == 9 * c
    w = w16.reshape(n, 3, 3, c)
    w = w.float() if w16.dtype in (torch.float16, torch.bfloat16) else w
    rows = torch.stack([w[:, list(s)].sum(1) for s in UPS_TAP_SETS], 1)          # [n][e][kx][c]
    w4 = torch.stack([rows[:, :, list(s)].sum(2) for s in UPS_TAP_SETS], 2)      # [n][e][f][c]
    return w4.permute(3, 1, 2, 0).reshape(c, 16 * n).to(w16.dtype).contiguous()


def dgrad_weight_cout4(w16: torch.Tensor) -> torch.Tensor:
    """``[Co<=4][9*C] -> [C][9][8]`` with the taps flipped and the columns ``>= Co`` zero: wt[c][8-tap][o] = w[o][tap][c],
    the ``pack_conv_cin8`` layout of the transposed conv.  ``HipBackend.conv_in_nchw`` run on the fp32 NCHW dy of
    ``conv_out`` with this weight is conv_out's data gradient (``HipBackend.dgrad_cout4``).  A torch re-layout, like
    ``dgrad_weight``."""
    co, c = w16.shape[0], w16.shape[1] // 9
    assert w16.dim() == 2 and w16.shape[1] == 9 * c and 1 <= co <= 4
    wt = w16.new_zeros((c, 9, 8))
    wt[:, :, :co] = w16.reshape(co, 9, c).flip(1).permute(2, 1, 0)
    return wt


def _wt_shape(n, c, taps, stride, ups):
    return (c, 16 * n) if ups else (c, taps * n)


def _check_prepared(prepared, x, w, wt_shape, what):
    """``prepared = (w16, wt)``: the 16-bit copy of the master ``w`` (its shape) and the weight of the data gradient
    (``wt_shape``), both contiguous, of x's type and on x's device.  Their VALUES are the caller's business
    (``optim.DgradRelayout``)."""
    if not isinstance(prepared, (tuple, list)) or len(prepared) != 2 or not all(isinstance(t, torch.Tensor) for t in prepared):
        raise TypeError(f"{what}: prepared is the pair (w16, wt) of tensors, got {type(prepared).__name__}")
    w16, wt = prepared
    for t, shape, name in ((w16, tuple(w.shape), "w16"), (wt, tuple(wt_shape), "wt")):
        if t.dtype != x.dtype:
            raise TypeError(f"{what}: prepared {name} must have x's type {x.dtype}, got {t.dtype}")
        if tuple(t.shape) != shape or not t.is_contiguous() or t.device != x.device or t.requires_grad:
            raise ValueError(f"{what}: prepared {name} must be a contiguous {shape} tensor on {x.device} without gradient, "
                             f"got {tuple(t.shape)} on {t.device}")
    return w16, wt


def _forward(be, x, w, bias, taps, stride, ups, rowvec=None, w16=None):
    n = w.shape[0]
    c = x.shape[-1]
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"x must be fp16 or bf16, got {x.dtype}")
    if w.dtype != torch.float32 or w.shape != (n, taps * c) or (bias is not None and bias.dtype != torch.float32):
        raise ValueError(f"w must be the fp32 master [N][{taps}*{c}] and bias fp32, got {tuple(w.shape)} {w.dtype}")
    x = x.contiguous()
    if w16 is None:
        w16 = w.to(x.dtype)                     # on torch's current stream, like every producer of the inputs
    if taps == 1:
        x4 = x.reshape(1, 1, -1, c)
        out_shape4, out_shape = (1, 1, x4.shape[2], n), x.shape[:-1] + (n,)
    else:
        b, h, wd, _ = x.shape
        ho, wo = (2 * h, 2 * wd) if ups else ((h - 1) // stride + 1, (wd - 1) // stride + 1)
        x4 = x
        out_shape4 = out_shape = (b, ho, wo, n)
    with on_backend(be):
        y = be.empty(out_shape4, x.dtype)
        if rowvec is None:
            be.igemm(x4, w16, y, bias=bias, taps=taps, stride=stride, ups=int(ups), pad=1 if taps == 9 else 0,
                     flags=L.EPI_BIAS if bias is not None else 0)
        else:
            be.igemm(x4, w16, y, bias=bias, rowvec=rowvec, taps=taps, stride=stride, ups=int(ups), pad=1 if taps == 9 else 0,
                     flags=(L.EPI_BIAS if bias is not None else 0) | L.EPI_ROWVEC)
    return x4, w16, y.view(out_shape)


def _backward(be, x4, w16, dy, taps, stride, ups, need_dx, need_dw, need_db, wt=None):
    n, c = w16.shape[0], x4.shape[-1]
    dy4 = dy.contiguous() if taps == 9 else dy.contiguous().reshape(1, 1, -1, n)
    resample = stride != 1 or ups
    if need_dx and wt is None:                             # torch plumbing, current stream
        wt = dgrad_weight(w16, taps) if not resample else dgrad_weight_ups(w16) if ups else dgrad_weight_stride2(w16)
    with on_backend(be):
        dx = dw = db = None
        if need_dx:
            dx = be.empty(tuple(x4.shape), x4.dtype)
            if resample:
                be.dgrad_resample(dy4, wt, dx, stride=stride, ups=int(ups))
            else:
                be.dgrad(dy4, wt, dx, taps=taps)
        if need_dw or need_db:
            m = dy4.shape[0] * dy4.shape[1] * dy4.shape[2]
            dw = be.empty((n, taps * c), torch.float32)
            db = be.empty((n,), torch.float32) if need_db else None
            splitm = be.wgrad_splitm(m, n, c, taps)
            partial = be.empty((be.wgrad_partial_numel(splitm, n, c, taps),), torch.float32) if splitm > 1 else None
            be.wgrad(dy4, x4, dw, dbias=db, taps=taps, stride=stride, ups=int(ups), pad=1 if taps == 9 else 0,
                     splitm=splitm, partial=partial)
    return dx, dw, db


class _Product(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, be, taps, stride, ups, prepared=None):
        w16 = wt = None
        if prepared is not None:
            w16, wt = _check_prepared(prepared, x, w, _wt_shape(w.shape[0], x.shape[-1], taps, stride, ups), "product")
        x4, w16, y = _forward(be, x, w, bias, taps, stride, ups, w16=w16)
        ctx.save_for_backward(x4, w16)
        ctx.be, ctx.cfg, ctx.x_shape, ctx.wt = be, (taps, stride, ups), x.shape, wt
        return y

    @staticmethod
    def backward(ctx, dy):
        x4, w16 = ctx.saved_tensors
        taps, stride, ups = ctx.cfg
        need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
        dx, dw, db = _backward(ctx.be, x4, w16, dy.to(x4.dtype), taps, stride, ups, need_dx, need_dw, need_db, wt=ctx.wt)
        return (dx.view(ctx.x_shape) if need_dx else None, dw if need_dw else None, db, None, None, None, None, None)


class _ProductRowvec(torch.autograd.Function):
    """The stride-1 3x3 conv with the per-sample fp32 row of ``EPI_ROWVEC`` added in the epilogue."""

    @staticmethod
    def forward(ctx, x, w, bias, rowvec, be, prepared=None):
        n = w.shape[0]
        if rowvec.dtype != torch.float32 or rowvec.dim() != 2 or rowvec.shape != (x.shape[0], n) or rowvec.stride(1) != 1 \
                or rowvec.stride(0) % 4 or rowvec.data_ptr() % 16:
            raise ValueError(f"rowvec must be fp32 [B][N] = [{x.shape[0]}][{n}] with unit column stride, a row stride that is a "
                             f"multiple of 4 and a 16-byte aligned start, got {tuple(rowvec.shape)} {rowvec.dtype} strides "
                             f"{tuple(rowvec.stride())}")
        w16 = wt = None
        if prepared is not None:
            w16, wt = _check_prepared(prepared, x, w, _wt_shape(n, x.shape[-1], 9, 1, False), "conv3x3")
        x4, w16, y = _forward(be, x, w, bias, 9, 1, False, rowvec=rowvec.detach(), w16=w16)
        ctx.save_for_backward(x4, w16)
        ctx.be, ctx.x_shape, ctx.wt = be, x.shape, wt
        return y

    @staticmethod
    def backward(ctx, dy):
        x4, w16 = ctx.saved_tensors
        be = ctx.be
        need_dx, need_dw, need_db, need_row = ctx.needs_input_grad[:4]
        dy = dy.to(x4.dtype).contiguous()
        dx = dw = db = drow = None
        if need_dx or need_dw or need_db:
            dx, dw, db = _backward(be, x4, w16, dy, 9, 1, False, need_dx, need_dw, need_db, wt=ctx.wt)
        if need_row:
            with on_backend(be):
                drow = be.empty((dy.shape[0], dy.shape[-1]), torch.float32)
                be.rowvec_grad(dy, drow)
        return (dx.view(ctx.x_shape) if need_dx else None, dw if need_dw else None, db, drow, None, None)


def linear(be, x, w, bias=None, prepared=None):
    """y = x w^T + bias over the last axis of ``x`` ([..., C] -> [..., N]); differentiable in x, w and bias.
    ``prepared``: the pair ``(w16, wt)`` of ``optim.DgradRelayout.prepared(name)`` - the 16-bit copy of ``w`` that the
    optimizer step already wrote and the weight of the data gradient that one re-layout launch wrote (here
    ``dgrad_weight(w16, 1)``).  The forward then reads ``w16`` instead of casting ``w``, the backward ``wt`` instead of
    re-laying; the gradients still go to the master ``w``.  The same keyword, with the layout of their own helper, is taken
    by ``conv3x3`` (stride 1), ``downsample2d``, ``upsample2d`` and ``conv_out``.  Without it nothing changes."""
    return _Product.apply(x, w, bias, be, 1, 1, False, prepared)


def conv3x3(be, x, w, bias=None, stride=1, ups=False, rowvec=None, prepared=None):
    """3x3 convolution, padding 1, of NHWC ``x`` with ``w`` [N][9*C]; ``stride`` 1 or 2, or ``ups``: through a nearest
    2x upsample.  Differentiable in w and bias for every form; in x for stride 1 without upsample only: the resampling
    forms with a data gradient are ``downsample2d`` and ``upsample2d``.
    ``rowvec``: fp32 [B][N], one row per sample added to every pixel in the conv's epilogue (``EPI_ROWVEC``: the resnet's
    time row, rounded once with the bias and the sum) - stride 1 without ``ups`` only.  It may be a strided slice of a
    wider rows tensor (``conditioning_grad.time_embedding``); its gradient is the fp32 sum of dy over the pixels
    (``HipBackend.rowvec_grad``).  Without ``rowvec`` nothing changes.
    ``prepared``: as in ``linear``, with ``wt = dgrad_weight(w16, 9)``; stride 1 without ``ups`` only."""
    if stride not in (1, 2) or (ups and stride != 1) or x.dim() != 4:
        raise ValueError(f"conv3x3 takes NHWC x, stride 1 or 2, or ups with stride 1 (got stride {stride}, ups {ups})")
    if rowvec is not None:
        if stride != 1 or ups:
            raise ValueError(f"conv3x3: rowvec goes with stride 1 and no upsample (got stride {stride}, ups {bool(ups)})")
        return _ProductRowvec.apply(x, w, bias, rowvec, be, prepared)
    if prepared is not None and (stride != 1 or ups):
        raise ValueError("conv3x3: prepared goes with stride 1 and no upsample; the resampling forms that take it are "
                         "downsample2d and upsample2d")
    if (stride != 1 or ups) and x.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(
            f"conv3x3(stride={stride}, ups={bool(ups)}) has no data gradient yet: the strided / upsampled dgrad kernel is "
            "missing; pass x.detach() to get the weight and bias gradients")
    return _Product.apply(x, w, bias, be, 9, stride, bool(ups), prepared)


def downsample2d(be, x, w, bias=None, prepared=None):
    """diffusers' ``Downsample2D`` conv: 3x3, stride 2, padding 1 of NHWC ``x`` [B,H,W,C] with ``w`` [N][9*C] ->
    [B,(H-1)//2+1,(W-1)//2+1,N]; odd maps are legal.  Differentiable in x, w and bias: forward and weight / bias gradient
    are those of ``conv3x3(stride=2)``, the data gradient is the parity-class gather-GEMM of csrc/dgrad.hip on the
    weight re-laid by ``dgrad_weight_stride2`` (9 tap products per input pixel, none on a zero of a dilated dy).
    ``prepared``: as in ``linear``, with ``wt = dgrad_weight_stride2(w16)``."""
    if x.dim() != 4:
        raise ValueError(f"downsample2d takes NHWC x, got {tuple(x.shape)}")
    return _Product.apply(x, w, bias, be, 9, 2, False, prepared)


def upsample2d(be, x, w, bias=None, prepared=None):
    """diffusers' ``Upsample2D``: nearest 2x upsample, then 3x3 conv, padding 1, of NHWC ``x`` [B,H,W,C] with ``w``
    [N][9*C] -> [B,2H,2W,N]; the upsampled tensor is never materialised.  Differentiable in x, w and bias: forward and
    weight / bias gradient are those of ``conv3x3(ups=True)``, the data gradient is csrc/dgrad.hip on the 16 pre-summed
    taps of ``dgrad_weight_ups`` (summed in fp32, rounded once: one rounding more than the forward has).
    ``prepared``: as in ``linear``, with ``wt = dgrad_weight_ups(w16)``."""
    if x.dim() != 4:
        raise ValueError(f"upsample2d takes NHWC x, got {tuple(x.shape)}")
    return _Product.apply(x, w, bias, be, 9, 1, True, prepared)


def _end_wgrad(be, thin, wide, dw_shape, nb, mode, need_db):
    """dw (in the kernel's layout) and dbias of an end conv on the backend stream, default split."""
    b, ct, h, wd = thin.shape
    cw = wide.shape[-1]
    dw = be.empty(dw_shape, torch.float32)
    db = be.empty((nb,), torch.float32) if need_db else None
    splitm = be.end_wgrad_splitm(b * h * wd, cw)
    partial = be.empty((be.end_wgrad_partial_numel(splitm, ct, cw, mode),), torch.float32) if splitm > 1 else None
    be.end_wgrad(thin, wide, dw, dbias=db, mode=mode, splitm=splitm, partial=partial)
    return dw, db


class _ConvIn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, be, dtype, data_grad=False):
        if x.dim() != 4 or x.dtype != torch.float32 or not 1 <= x.shape[1] <= 4:
            raise ValueError(f"conv_in takes fp32 NCHW x with 1..4 channels, got {tuple(x.shape)} {x.dtype}")
        b, ct, h, wd = x.shape
        n = w.shape[0]
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"conv_in writes fp16 or bf16, got {dtype}")
        if w.dtype != torch.float32 or w.shape != (n, 9 * ct) or n % 8 or (
                bias is not None and (bias.dtype != torch.float32 or bias.shape != (n,))):
            raise ValueError(f"w must be the fp32 master [N][9*{ct}] with N a multiple of 8 and bias fp32 [N], got "
                             f"{tuple(w.shape)} {w.dtype}")
        if (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]) and n % 64:
            raise ValueError(f"conv_in: the weight / bias gradient takes N a multiple of 64, got {n} (detach w and bias for a "
                             "forward alone)")
        x = x.contiguous()
        w8 = torch.zeros((n, 9, 8), dtype=dtype, device=w.device)     # pack_conv_cin8 of the rounded master
        w16 = w.detach().reshape(n, 9, ct).to(dtype)
        w8[:, :, :ct] = w16
        bias = None if bias is None else bias.detach().contiguous()
        with on_backend(be):
            y = be.empty((b, h, wd, n), dtype)
            be.conv_in_nchw(x, w8, bias, y)
        need_dx = bool(data_grad) and ctx.needs_input_grad[0]
        ctx.save_for_backward(x, w16 if need_dx else None)
        ctx.be, ctx.need_dx = be, need_dx
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w16 = ctx.saved_tensors
        be = ctx.be
        _, need_dw, need_db = ctx.needs_input_grad[:3]
        need_dx = ctx.need_dx
        if not (need_dx or need_dw or need_db):
            return (None,) * 6
        ct, n = x.shape[1], dy.shape[-1]
        dy = dy.contiguous()
        wt = w16.flip(1).permute(2, 1, 0).contiguous() if need_dx else None     # [Ct][8 - tap][N]: torch plumbing, tiny
        with on_backend(be):
            dx = dw = db = None
            if need_dx:                      # the conv_out kernel on dy with the flipped, transposed weight
                dx = be.empty(tuple(x.shape), torch.float32)
                be.conv_cout4(dy.to(w16.dtype), wt, None, dx, mode=0)
            if need_dw or need_db:
                dw8, db = _end_wgrad(be, x, dy, (n, 9, 8), n, L.END_WGRAD_IN, need_db)
                with be.ctx():
                    dw = dw8[:, :, :ct].reshape(n, 9 * ct)
        return dx, dw if need_dw else None, db, None, None, None


class _ConvOut(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, be, prepared=None):
        _check16(x, "x")
        if x.dim() != 4:
            raise ValueError(f"conv_out takes NHWC x, got {tuple(x.shape)}")
        b, h, wd, c = x.shape
        co = w.shape[0]
        if w.dtype != torch.float32 or w.shape != (co, 9 * c) or not 1 <= co <= 4 or (
                bias is not None and (bias.dtype != torch.float32 or bias.shape != (co,))):
            raise ValueError(f"w must be the fp32 master [Co <= 4][9*{c}] and bias fp32 [Co], got {tuple(w.shape)} {w.dtype}")
        if (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]) and c % 64:
            raise ValueError(f"conv_out: the weight / bias gradient takes C a multiple of 64, got {c} (detach w and bias for a "
                             "forward and a data gradient alone)")
        x = x.contiguous()
        wt = None
        if prepared is not None:
            w16, wt = _check_prepared(prepared, x, w, (c, 9, 8), "conv_out")
        else:
            w16 = w.detach().to(x.dtype).contiguous()   # [Co][9*C] is pack_conv_cout4's [Co][9][C]
        bias = None if bias is None else bias.detach().contiguous()
        with on_backend(be):
            y = be.empty((b, co, h, wd), torch.float32)
            be.conv_cout4(x, w16.view(co, 9, c), bias, y, mode=0)
        ctx.save_for_backward(x, w16)
        ctx.be, ctx.wt = be, wt
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w16 = ctx.saved_tensors
        be = ctx.be
        need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
        if not (need_dx or need_dw or need_db):
            return (None,) * 5
        co, c = w16.shape[0], x.shape[-1]
        dy = dy.float().contiguous()
        wt = ctx.wt
        if need_dx and wt is None:
            wt = dgrad_weight_cout4(w16)                       # torch plumbing, current stream
        with on_backend(be):
            dx = dw = db = None
            if need_dx:
                dx = be.empty(tuple(x.shape), x.dtype)
                be.dgrad_cout4(dy, wt, dx)
            if need_dw or need_db:
                dw, db = _end_wgrad(be, dy, x, (co, 9, c), co, L.END_WGRAD_OUT, need_db)
                dw = dw.view(co, 9 * c)
        return dx, dw if need_dw else None, db, None, None


class _MseRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, be):
        if pred.dtype != torch.float32 or target.dtype != torch.float32 or pred.shape != target.shape or pred.dim() < 2:
            raise ValueError(f"mse_rows takes fp32 pred and target of one shape [B, ...], got {tuple(pred.shape)} {pred.dtype} "
                             f"and {tuple(target.shape)} {target.dtype}")
        pred, target = pred.contiguous(), target.contiguous()
        with on_backend(be):
            out = be.empty((pred.shape[0],), torch.float32)
            be.mse_rows(pred, target, out)
        ctx.save_for_backward(pred, target)
        ctx.be = be
        return out

    @staticmethod
    def backward(ctx, drow):
        pred, target = ctx.saved_tensors
        be = ctx.be
        if not ctx.needs_input_grad[0]:
            return None, None, None
        drow = drow.float().contiguous()
        with on_backend(be):
            dpred = be.empty(tuple(pred.shape), torch.float32)
            be.mse_rows_grad(pred, target, drow, dpred)
        return dpred, None, None


class _LinearRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, be, act_in, weight_dtype):
        if x.dtype != torch.float32 or x.dim() != 2:
            raise ValueError(f"linear_rows takes fp32 rows x [M][K], got {tuple(x.shape)} {x.dtype}")
        m, k = x.shape
        n = w.shape[0]
        if w.dtype != torch.float32 or w.shape != (n, k) or (bias is not None and (bias.dtype != torch.float32 or bias.shape != (n,))):
            raise ValueError(f"w must be the fp32 master [N][{k}] and bias fp32 [N], got {tuple(w.shape)} {w.dtype}")
        if weight_dtype not in (torch.float32, torch.float16):
            raise ValueError(f"linear_rows multiplies with fp32 or fp16 weights, got {weight_dtype}")
        if act_in not in (0, 1, 2) or k % 8 or not 0 < k <= 2048 or m < 1 or n < 1:
            raise ValueError(f"linear_rows takes act_in 0, 1 (SiLU) or 2 (GELU) and K a multiple of 8 up to 2048 (got act_in "
                             f"{act_in}, M {m}, K {k}, N {n})")
        x = x.contiguous()
        wk = w.detach().to(weight_dtype).contiguous()     # rounded once (fp16) and kept for the backward
        bias = None if bias is None else bias.detach().contiguous()
        with on_backend(be):
            out = be.empty((m, n), torch.float32)
            be.linear_rows(x, wk, bias, out, act_in, 0)
        ctx.save_for_backward(x, wk)
        ctx.be, ctx.act_in = be, act_in
        return out

    @staticmethod
    def backward(ctx, dy):
        x, wk = ctx.saved_tensors
        be = ctx.be
        need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
        if not (need_dx or need_dw or need_db):
            return (None,) * 6
        (m, k), n = x.shape, wk.shape[0]
        dy = dy.float().contiguous()
        with on_backend(be):
            dx = be.empty((m, k), torch.float32) if need_dx else None
            dw = be.empty((n, k), torch.float32) if need_dw or need_db else None
            db = be.empty((n,), torch.float32) if need_db else None
            ws = be.empty((be.linear_rows_grad_ws_numel(m, k, n),), torch.float32) if need_dx else None
            be.linear_rows_grad(x, wk, dy, dx=dx, dw=dw, db=db, ws=ws, act_in=ctx.act_in)
        return dx, dw if need_dw else None, db, None, None, None


class _AoeInterp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, labels, base, deltas, be):
        if base.dtype != torch.float32 or deltas.dtype != torch.float32 or base.dim() != 1 or deltas.dim() != 2 \
                or deltas.shape[1] != base.shape[0] or not 1 <= deltas.shape[0] <= 15:
            raise ValueError(f"aoe_interp takes the fp32 masters base [D] and deltas [classes - 1 <= 15][D], got "
                             f"{tuple(base.shape)} {base.dtype} and {tuple(deltas.shape)} {deltas.dtype}")
        if labels.dim() != 1 or labels.shape[0] < 1:
            raise ValueError(f"aoe_interp takes labels [B], got {tuple(labels.shape)}")
        labels = labels.detach().float().contiguous()
        base, deltas = base.detach().contiguous(), deltas.detach().contiguous()
        with on_backend(be):
            out = be.empty((labels.shape[0], base.shape[0]), torch.float32)
            be.aoe_interp(labels, base, deltas, out)
        ctx.save_for_backward(labels)
        ctx.be, ctx.classes = be, deltas.shape[0] + 1
        return out

    @staticmethod
    def backward(ctx, dout):
        (labels,) = ctx.saved_tensors
        be = ctx.be
        _, need_b, need_d = ctx.needs_input_grad[:3]
        if not (need_b or need_d):
            return (None,) * 4
        dout = dout.float().contiguous()
        d = dout.shape[1]
        with on_backend(be):
            dbase, ddeltas = be.empty((d,), torch.float32), be.empty((ctx.classes - 1, d), torch.float32)
            be.aoe_interp_grad(labels, dout, dbase, ddeltas)
        return None, dbase if need_b else None, ddeltas if need_d else None, None


def linear_rows(be, x, w, bias=None, act_in=0, weight_dtype=torch.float32):
    """out = act_in(x) w^T + bias on the fp32 row path (``HipBackend.linear_rows``): x fp32 [M][K], ``w`` the fp32 master
    [N][K], bias fp32 [N]; ``act_in`` 0 none, 1 SiLU, 2 exact GELU.  With ``weight_dtype=torch.float16`` (the time
    embedding) the master is rounded once and the rounded copy kept for the backward; its gradient comes back in fp32.
    Differentiable in x, w and bias (``HipBackend.linear_rows_grad``, csrc/rows_grad.hip).
    The operator has no ``act_out`` on purpose: a layer's activation is applied as the NEXT layer's ``act_in``, which
    the forward kernel supports.  The values are bit-identical to the inference path's ``act_out`` followed by ``act_in =
    0`` (both evaluate the same fp32 function of the same fp32 sum), and the pre-activation the backward needs is then
    simply the saved input."""
    return _LinearRows.apply(x, w, bias, be, int(act_in), weight_dtype)


def aoe_interp(be, labels, base, deltas):
    """The AdditiveOrdinalEmbedder's class interpolation (``HipBackend.aoe_interp``): labels [B] (clamped to [0, classes -
    1]), the fp32 masters ``base`` [D] and ``deltas`` [classes - 1][D] -> fp32 [B][D], the lerp between the neighbouring
    rows of the table base + cumsum(deltas).  Differentiable in base and deltas (``HipBackend.aoe_interp_grad``); the
    labels get no gradient."""
    return _AoeInterp.apply(labels, base, deltas, be)


def conv_in(be, x_nchw, w, bias=None, dtype=torch.float16, data_grad=False):
    """The UNet's conv_in: 3x3, padding 1, of the fp32 NCHW latents ``x_nchw`` [B, Ct <= 4, H, W] with the fp32 master
    ``w`` [N][9*Ct] -> ``dtype`` (fp16 or bf16) NHWC [B,H,W,N]; the latents are rounded to ``dtype`` in registers
    (``HipBackend.conv_in_nchw``).  Differentiable in w and bias (``HipBackend.end_wgrad``, IN mode; N a multiple of
    64: with a trainable w or bias any other N is refused by the forward, N a multiple of 8 suffices without).  The latents are data: there is no gradient of ``x_nchw``.
    ``data_grad=True`` lifts that for a caller that asks (a gradient check of the whole UNet): the fp32 NCHW gradient of
    ``x_nchw`` is then ``HipBackend.conv_cout4`` (the conv_out kernel) on dy with the flipped, transposed weight."""
    if x_nchw.requires_grad and torch.is_grad_enabled() and not data_grad:
        raise NotImplementedError("conv_in has no data gradient: the latents are data; pass x_nchw.detach() to get the "
                                  "weight and bias gradients")
    return _ConvIn.apply(x_nchw, w, bias, be, dtype, bool(data_grad))


def conv_out(be, x, w, bias=None, prepared=None):
    """The UNet's conv_out: 3x3, padding 1, of 16-bit NHWC ``x`` [B,H,W,C] with the fp32 master ``w`` [Co <= 4][9*C] ->
    fp32 NCHW [B,Co,H,W] (``HipBackend.conv_cout4``, mode 0).  Differentiable in x, w and bias: the incoming fp32
    gradient is rounded to ``x.dtype`` in registers by both backward kernels (``HipBackend.dgrad_cout4`` on the weight of
    ``dgrad_weight_cout4``; ``HipBackend.end_wgrad``, OUT mode; C a multiple of 64: with a trainable w or bias any other C is refused by the
    forward).  ``prepared``: as in ``linear``, with ``wt = dgrad_weight_cout4(w16)``."""
    return _ConvOut.apply(x, w, bias, be, prepared)


def mse_rows(be, pred, target):
    """mean((pred - target)^2) over every axis but the first: fp32 [B, ...] -> fp32 [B] (``HipBackend.mse_rows``);
    differentiable in pred (``HipBackend.mse_rows_grad``): whatever weights the rows afterwards - a Min-SNR weight, the
    mean over the batch, a loss scale - reaches the kernel as the upstream gradient of the B rows, on the device."""
    return _MseRows.apply(pred, target, be)


def _check16(x, what):
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"{what} must be fp16 or bf16, got {x.dtype}")


def _check_affine(gamma, beta, c):
    if gamma.dtype != torch.float32 or beta.dtype != torch.float32 or gamma.shape != (c,) or beta.shape != (c,):
        raise ValueError(f"gamma and beta must be the fp32 masters [{c}], got {tuple(gamma.shape)} {gamma.dtype} and "
                         f"{tuple(beta.shape)} {beta.dtype}")


class _GroupNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x2, gamma, beta, be, groups, eps, silu):
        _check16(x, "x")
        if x.dim() != 4 or (x2 is not None and (x2.dtype != x.dtype or x2.shape[:-1] != x.shape[:-1])):
            raise ValueError("group_norm takes NHWC x (and x2 of the same type and map)")
        c = x.shape[-1] + (0 if x2 is None else x2.shape[-1])
        _check_affine(gamma, beta, c)
        x = x.contiguous()
        x2 = None if x2 is None else x2.contiguous()
        gamma, beta = gamma.contiguous(), beta.contiguous()
        with on_backend(be):
            y = be.empty(x.shape[:-1] + (c,), x.dtype)
            ws = be.empty((x.shape[0] * L.GN_MAX_CHUNKS * groups * 2,), torch.float32)
            be.groupnorm(x, x2, gamma, beta, y, ws, groups, eps, silu)
        ctx.save_for_backward(x, x2, gamma, beta)
        ctx.be, ctx.cfg = be, (groups, eps, silu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, x2, gamma, beta = ctx.saved_tensors
        be, (groups, eps, silu) = ctx.be, ctx.cfg
        need_x, need_x2, need_g, need_b = ctx.needs_input_grad[:4]
        need_dx, need_dp = need_x or need_x2, need_g or need_b
        if not (need_dx or need_dp):
            return (None,) * 8
        dy = dy.to(x.dtype).contiguous()
        b, hw, c = x.shape[0], x.shape[1] * x.shape[2], dy.shape[-1]
        with on_backend(be):
            dx1 = be.empty(tuple(x.shape), x.dtype) if need_dx else None
            dx2 = be.empty(tuple(x2.shape), x.dtype) if need_dx and x2 is not None else None
            dg = be.empty((c,), torch.float32) if need_dp else None
            db = be.empty((c,), torch.float32) if need_dp else None
            ws = be.empty((be.groupnorm_grad_ws_numel(b, hw, c, groups),), torch.float32)
            be.groupnorm_grad(x, x2, dy, gamma, beta, dx1=dx1, dx2=dx2, dgamma=dg, dbeta=db, ws=ws, groups=groups, eps=eps,
                              silu=silu)
        return (dx1 if need_x else None, dx2 if need_x2 else None, dg if need_g else None, db if need_b else None,
                None, None, None, None)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, be, eps):
        _check16(x, "x")
        _check_affine(gamma, beta, x.shape[-1])
        x, gamma, beta = x.contiguous(), gamma.contiguous(), beta.contiguous()
        with on_backend(be):
            y = be.empty(tuple(x.shape), x.dtype)
            be.layernorm(x, gamma, beta, y, eps)
        ctx.save_for_backward(x, gamma)
        ctx.be, ctx.eps = be, eps
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma = ctx.saved_tensors
        be = ctx.be
        need_x, need_g, need_b = ctx.needs_input_grad[:3]
        need_dp = need_g or need_b
        if not (need_x or need_dp):
            return (None,) * 5
        dy = dy.to(x.dtype).contiguous()
        c = x.shape[-1]
        with on_backend(be):
            dx = be.empty(tuple(x.shape), x.dtype) if need_x else None
            dg = be.empty((c,), torch.float32) if need_dp else None
            db = be.empty((c,), torch.float32) if need_dp else None
            ws = be.empty((be.layernorm_grad_ws_numel(x.numel() // c, c),), torch.float32) if need_dp else None
            be.layernorm_grad(x, dy, gamma, dx=dx, dgamma=dg, dbeta=db, ws=ws, eps=ctx.eps)
        return dx, dg if need_g else None, db if need_b else None, None, None


class _Pointwise(torch.autograd.Function):
    """``op`` = "gelu": x [..., F] -> [..., F]; "geglu": h [..., 2F] -> [..., F].  Forward ``be.<op>(x, y)``, backward
    ``be.<op>_grad(x, dy, dx)`` on the saved input."""

    @staticmethod
    def forward(ctx, x, be, op):
        ratio, what = (2, "h [..., 2F]") if op == "geglu" else (1, "x [..., F]")
        _check16(x, what[0])
        if x.shape[-1] % (8 * ratio):
            raise ValueError(f"{op} takes {what} with F a multiple of 8, got {tuple(x.shape)}")
        x = x.contiguous()
        with on_backend(be):
            y = be.empty(x.shape[:-1] + (x.shape[-1] // ratio,), x.dtype)
            getattr(be, op)(x, y)
        ctx.save_for_backward(x)
        ctx.be, ctx.op = be, op
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        be = ctx.be
        if not ctx.needs_input_grad[0]:
            return None, None, None
        dy = dy.to(x.dtype).contiguous()
        with on_backend(be):
            dx = be.empty(tuple(x.shape), x.dtype)
            getattr(be, ctx.op + "_grad")(x, dy, dx)
        return dx, None, None


class _PurifierGateTail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, dis, z, gamma, beta, be, eps):
        for t, what in ((img, "img"), (dis, "dis"), (z, "z")):
            _check16(t, what)
        if not (img.shape == dis.shape == z.shape and img.dtype == dis.dtype == z.dtype):
            raise ValueError(f"purifier_gate_tail takes img, dis and z of one shape and 16-bit type, got {tuple(img.shape)} "
                             f"{img.dtype}, {tuple(dis.shape)} {dis.dtype}, {tuple(z.shape)} {z.dtype}")
        _check_affine(gamma, beta, img.shape[-1])
        img, dis, z, gamma, beta = (t.contiguous() for t in (img, dis, z, gamma, beta))
        with on_backend(be):
            out = be.empty(tuple(img.shape), torch.float32)
            be.purifier_gate_tail(img, dis, z, gamma, beta, out, eps)
        ctx.save_for_backward(img, dis, z, gamma)
        ctx.be, ctx.eps = be, eps
        return out

    @staticmethod
    def backward(ctx, dout):
        img, dis, z, gamma = ctx.saved_tensors
        be = ctx.be
        need_i, need_d, need_z, need_g, need_b = ctx.needs_input_grad[:5]
        need_dp = need_g or need_b
        if not (need_i or need_d or need_z or need_dp):
            return (None,) * 7
        dout = dout.float().contiguous()
        c = img.shape[-1]
        with on_backend(be):
            dimg, ddis, dz = (be.empty(tuple(img.shape), img.dtype) if need else None for need in (need_i, need_d, need_z))
            dg = be.empty((c,), torch.float32) if need_dp else None
            db = be.empty((c,), torch.float32) if need_dp else None
            ws = be.empty((be.purifier_gate_tail_grad_ws_numel(img.numel() // c, c),), torch.float32) if need_dp else None
            be.purifier_gate_tail_grad(img, dis, z, dout, gamma, dimg=dimg, ddis=ddis, dz=dz, dgamma=dg, dbeta=db, ws=ws,
                                       eps=ctx.eps)
        return dimg, ddis, dz, dg if need_g else None, db if need_b else None, None, None


def _attn_ws(be, q, heads):
    return be.empty((be.attn_grad_ws_numel(q.shape[0], heads, q.shape[1]),), torch.float32)


class _SelfAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, be, heads):
        _check16(qkv, "qkv")
        if qkv.dim() != 3 or qkv.shape[-1] % (3 * heads):
            raise ValueError(f"self_attention takes qkv [B,N,3C] with C a multiple of heads = {heads}, got {tuple(qkv.shape)}")
        qkv = qkv.contiguous()
        b, n, c3 = qkv.shape
        with on_backend(be):
            out = be.empty((b, n, c3 // 3), qkv.dtype)
            be.self_attn(qkv, out, heads)
        ctx.save_for_backward(qkv)
        ctx.be, ctx.heads = be, heads
        return out

    @staticmethod
    def backward(ctx, dy):
        (qkv,) = ctx.saved_tensors
        be, heads = ctx.be, ctx.heads
        if not ctx.needs_input_grad[0]:
            return None, None, None
        c = qkv.shape[-1] // 3
        dy = dy.to(qkv.dtype).contiguous()
        with on_backend(be):
            dqkv = be.empty(tuple(qkv.shape), qkv.dtype)
            q, k, v = (qkv[..., i * c:(i + 1) * c] for i in range(3))
            be.attn_grad(q, k, v, dy, dq=dqkv[..., :c], dk=dqkv[..., c:2 * c], dv=dqkv[..., 2 * c:], ws=_attn_ws(be, q, heads),
                         heads=heads)
        return dqkv, None, None


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, be, heads):
        for t, what in ((q, "q"), (k, "k"), (v, "v")):
            _check16(t, what)
        if not (q.dim() == k.dim() == v.dim() == 3 and k.shape == v.shape and q.shape[0] == k.shape[0]
                and q.shape[2] == k.shape[2] and q.dtype == k.dtype == v.dtype) or q.shape[2] % heads:
            raise ValueError(f"attention takes q [B,Nq,C] and k, v [B,Nk,C] of one 16-bit type, got {tuple(q.shape)} "
                             f"{tuple(k.shape)} {tuple(v.shape)}")
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        with on_backend(be):
            out = be.empty(tuple(q.shape), q.dtype)
            be.attention(q, k, v, out, heads)
        ctx.save_for_backward(q, k, v)
        ctx.be, ctx.heads = be, heads
        return out

    @staticmethod
    def backward(ctx, dy):
        q, k, v = ctx.saved_tensors
        be, heads = ctx.be, ctx.heads
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        if not (need_q or need_k or need_v):
            return (None,) * 5
        dy = dy.to(q.dtype).contiguous()
        with on_backend(be):
            dq = be.empty(tuple(q.shape), q.dtype) if need_q else None
            dk = be.empty(tuple(k.shape), q.dtype) if need_k else None
            dv = be.empty(tuple(v.shape), q.dtype) if need_v else None
            be.attn_grad(q, k, v, dy, dq=dq, dk=dk, dv=dv, ws=_attn_ws(be, q, heads), heads=heads)
        return dq, dk, dv, None, None


class _TriCrossAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, kv, gates, be, lam, heads, mode):
        _check16(q, "q")
        c = q.shape[-1]
        want = (48, 4 * c) if mode == L.XATTN_SPLIT else (32, 2 * c)
        if mode not in (L.XATTN_SPLIT, L.XATTN_BASELINE) or q.dim() != 3 or kv.dtype != q.dtype \
                or kv.shape != (q.shape[0],) + want or c % heads:
            raise ValueError(f"tri_cross_attention takes q [B,N,C] and kv [B,{want[0]},{want[1] // c}C] of q's type in mode "
                             f"{mode}, got {tuple(q.shape)} and {tuple(kv.shape)} {kv.dtype}")
        if mode == L.XATTN_SPLIT and (gates is None or gates.dtype != torch.float32 or gates.numel() != 2):
            raise ValueError("tri_cross_attention: split mode takes gates, a device fp32[2] buffer")
        q, kv = q.contiguous(), kv.contiguous()
        gates = None if gates is None else gates.contiguous()
        with on_backend(be):
            out = be.empty(tuple(q.shape), q.dtype)
            be.tri_xattn(q, kv, out, gates, lam, mode, heads)
        ctx.save_for_backward(q, kv, gates)
        ctx.be, ctx.cfg = be, (lam, heads, mode)
        return out

    @staticmethod
    def backward(ctx, dy):
        q, kv, gates = ctx.saved_tensors
        be, (lam, heads, mode) = ctx.be, ctx.cfg
        need_q, need_kv = ctx.needs_input_grad[:2]
        if not (need_q or need_kv):
            return (None,) * 7
        c = q.shape[-1]
        dy = dy.to(q.dtype).contiguous()
        # (first token, tokens, first column of K; V follows K) and the scale of dy of every pathway
        if mode == L.XATTN_SPLIT:
            paths = [(16, 16, 0, 1.0, gates[0:1]), (0, 16, 2 * c, 1.0, gates[1:2])]     # anatomy, disease
            if lam != 0.0:
                paths.append((32, 16, 2 * c, float(lam), None))                          # delta, skipped as in the forward
        else:
            paths = [(0, 32, 0, 1.0, None)]
        with on_backend(be):
            dkv = be.zeros(tuple(kv.shape), kv.dtype) if need_kv else None
            ws = _attn_ws(be, q, heads)
            dqs = []
            for t0, nt, kc, scale, scale_dev in paths:
                k, v = kv[:, t0:t0 + nt, kc:kc + c], kv[:, t0:t0 + nt, kc + c:kc + 2 * c]
                dq = be.empty(tuple(q.shape), q.dtype) if need_q else None
                dk = dkv[:, t0:t0 + nt, kc:kc + c] if need_kv else None
                dv = dkv[:, t0:t0 + nt, kc + c:kc + 2 * c] if need_kv else None
                be.attn_grad(q, k, v, dy, dq=dq, dk=dk, dv=dv, ws=ws, heads=heads, do_scale=scale, do_scale_dev=scale_dev)
                dqs.append(dq)
            dq = None
            if need_q:
                dq = dqs[0]
                if len(dqs) > 1:
                    with be.ctx():      # fp32 sum of the pathways' dq, rounded once
                        acc = dqs[0].float()
                        for t in dqs[1:]:
                            acc += t.float()
                        dq = acc.to(q.dtype)
        return dq, dkv, None, None, None, None, None


def self_attention(be, qkv, heads):
    """qkv [B,N,3C] (q | k | v blocks of C columns) -> softmax(q k^T / sqrt(d)) v [B,N,C] per head; differentiable in qkv:
    the backward is one ``attn_grad`` call that writes dq, dk and dv into the column blocks of one [B,N,3C] tensor.
    The backward takes d = C / heads in {40, 80, 96, 160} and N a multiple of 16."""
    return _SelfAttention.apply(qkv, be, int(heads))


def attention(be, q, k, v, heads):
    """softmax(q k^T / sqrt(d)) v with separate lengths: q [B,Nq,C], k, v [B,Nk,C] -> [B,Nq,C]; differentiable in q, k and
    v (only the gradients that are needed are computed).  Backward: d in {40, 80, 96, 160}, Nq a multiple of 16, Nk any
    positive count."""
    return _Attention.apply(q, k, v, be, int(heads))


def tri_cross_attention(be, q, kv, gates, lam, heads, mode=L.XATTN_SPLIT):
    """The triple-pathway cross-attention of ``HipBackend.tri_xattn``: q [B,N,C] against kv [B,48,4C] (split mode: anatomy,
    disease and delta pathways of 16 tokens with independent softmaxes, weighted by ``gates`` (device fp32[2]) and the
    python float ``lam``) or kv [B,32,2C] (baseline mode: one softmax over 32 tokens).  Differentiable in q and kv; the
    gates and lambda are not learnable in the reference model and get no gradient.  The backward is one ``attn_grad``
    call per pathway on the pathway's slice of kv (the delta pathway is skipped when ``lam == 0``, as in the forward) with
    the gate (read on the device) or lambda as the scale of dy; dq is the fp32 sum of the pathways' dq, dkv is zero
    outside the slices the pathways read."""
    return _TriCrossAttention.apply(q, kv, gates, be, float(lam), int(heads), int(mode))


def group_norm(be, x, gamma, beta, groups=32, eps=1e-5, silu=False, x2=None):
    """GroupNorm (+ SiLU with ``silu``) of NHWC ``x`` [B,H,W,C1], or of the channel concatenation [x | x2] (the decoder's
    skip-concat, never materialised); ``gamma`` / ``beta`` are the fp32 masters [C1+C2].  Differentiable in x, x2, gamma
    and beta; the backward recomputes the statistics from x."""
    return _GroupNorm.apply(x, x2, gamma, beta, be, int(groups), float(eps), bool(silu))


def layer_norm(be, x, gamma, beta, eps=1e-5):
    """LayerNorm over the last axis of ``x`` [..., C] (C a multiple of 8, at most 2048); differentiable in x, gamma and
    beta."""
    return _LayerNorm.apply(x, gamma, beta, be, float(eps))


def geglu(be, h):
    """h [..., 2F] -> h[..., :F] * gelu(h[..., F:]) (the chunk(2) order of the reference model); differentiable in h."""
    return _Pointwise.apply(h, be, "geglu")


def gelu(be, x):
    """Exact-form GELU of x [..., F] (F a multiple of 8), the activation of the conditioning front-end's MLPs;
    differentiable in x (``HipBackend.gelu`` / ``gelu_grad``, csrc/cond_grad.hip)."""
    return _Pointwise.apply(x, be, "gelu")


def purifier_gate_tail(be, img, dis, z, gamma, beta, eps=1e-5):
    """The FeaturePurifier's tail LayerNorm(img - sigmoid(z) * dis): img, dis and z [..., C] in one 16-bit type, z the
    gate's pre-activation, ``gamma`` / ``beta`` the fp32 masters [C] -> fp32 [..., C].  Differentiable in all five: the
    incoming gradient is taken in fp32, the gradients of img, dis and z come back in their 16-bit type."""
    return _PurifierGateTail.apply(img, dis, z, gamma, beta, be, float(eps))
