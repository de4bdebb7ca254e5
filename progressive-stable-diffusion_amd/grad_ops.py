"""Differentiable Linear / conv3x3 on the HIP kernels: the matrix products of a training step and their gradients.

Forward is ``HipBackend.igemm``; the data gradient is the same kernel on ``dy`` with the weight re-laid by
``dgrad_weight``; the weight and bias gradients are the M-reduction GEMM of ``HipBackend.wgrad`` (csrc/wgrad.hip).
These are operators, not the training loop: norms, GEGLU and attention have no backward yet, and neither do the
strided / upsampled data gradient and the 4-channel end convolutions.

Operands: ``x`` is a 16-bit (fp16 or bf16) NHWC / token-major tensor on the backend's device, ``w`` the **fp32 master**
weight in the library layout ``[N][taps*C]`` (``[Cout][ky][kx][Cin]`` flattened), ``bias`` fp32.  The forward rounds the
master to ``x.dtype`` once and keeps the rounded copy for the backward; gradients of ``w`` and ``bias`` come back in fp32,
the gradient of ``x`` in ``x.dtype``.
"""
from __future__ import annotations

import torch

from . import lib as L


def dgrad_weight(w16: torch.Tensor, taps: int) -> torch.Tensor:
    """``[N][taps*C] -> [C][taps*N]`` with the taps flipped: wt[c][8-tap][n] = w[n][tap][c].  The forward kernel run on
    ``dy`` with this weight is the data gradient of a stride-1 convolution (include/dadd_hip.h); for ``taps == 1`` it is
    the plain transpose.  Applying it twice gives the weight back (with the channel roles swapped twice).
    Torch does the re-layout: one read and one write of the weight per call."""
    n = w16.shape[0]
    c = w16.shape[1] // taps
    assert w16.dim() == 2 and w16.shape[1] == taps * c
    return w16.reshape(n, taps, c).flip(1).permute(2, 1, 0).reshape(c, taps * n).contiguous()


def _forward(be, x, w, bias, taps, stride, ups):
    n = w.shape[0]
    c = x.shape[-1]
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"x must be fp16 or bf16, got {x.dtype}")
    if w.dtype != torch.float32 or w.shape != (n, taps * c) or (bias is not None and bias.dtype != torch.float32):
        raise ValueError(f"w must be the fp32 master [N][{taps}*{c}] and bias fp32, got {tuple(w.shape)} {w.dtype}")
    x = x.contiguous()
    w16 = w.to(x.dtype)                         # on torch's current stream, like every producer of the inputs
    if taps == 1:
        x4 = x.reshape(1, 1, -1, c)
        out_shape4, out_shape = (1, 1, x4.shape[2], n), x.shape[:-1] + (n,)
    else:
        b, h, wd, _ = x.shape
        ho, wo = (2 * h, 2 * wd) if ups else ((h - 1) // stride + 1, (wd - 1) // stride + 1)
        x4 = x
        out_shape4 = out_shape = (b, ho, wo, n)
    be.wait_current()
    y = be.empty(out_shape4, x.dtype)
    be.igemm(x4, w16, y, bias=bias, taps=taps, stride=stride, ups=int(ups), pad=1 if taps == 9 else 0,
             flags=L.EPI_BIAS if bias is not None else 0)
    be.release_to_current()
    return x4, w16, y.view(out_shape)


def _backward(be, x4, w16, dy, taps, stride, ups, need_dx, need_dw, need_db):
    n, c = w16.shape[0], x4.shape[-1]
    dy4 = dy.contiguous() if taps == 9 else dy.contiguous().reshape(1, 1, -1, n)
    wt = dgrad_weight(w16, taps) if need_dx else None      # torch plumbing, current stream
    be.wait_current()
    dx = dw = db = None
    if need_dx:
        dx = be.empty(tuple(x4.shape), x4.dtype)
        be.dgrad(dy4, wt, dx, taps=taps)
    if need_dw or need_db:
        m = dy4.shape[0] * dy4.shape[1] * dy4.shape[2]
        dw = be.empty((n, taps * c), torch.float32)
        db = be.empty((n,), torch.float32) if need_db else None
        splitm = be.wgrad_splitm(m, n, c, taps)
        partial = be.empty((be.wgrad_partial_numel(splitm, n, c, taps),), torch.float32) if splitm > 1 else None
        be.wgrad(dy4, x4, dw, dbias=db, taps=taps, stride=stride, ups=int(ups), pad=1 if taps == 9 else 0,
                 splitm=splitm, partial=partial)
    be.release_to_current()
    return dx, dw, db


class _Product(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, be, taps, stride, ups):
        x4, w16, y = _forward(be, x, w, bias, taps, stride, ups)
        ctx.save_for_backward(x4, w16)
        ctx.be, ctx.cfg, ctx.x_shape = be, (taps, stride, ups), x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        x4, w16 = ctx.saved_tensors
        taps, stride, ups = ctx.cfg
        need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
        dx, dw, db = _backward(ctx.be, x4, w16, dy.to(x4.dtype), taps, stride, ups, need_dx, need_dw, need_db)
        return (dx.view(ctx.x_shape) if need_dx else None, dw if need_dw else None, db, None, None, None, None)


def linear(be, x, w, bias=None):
    """y = x w^T + bias over the last axis of ``x`` ([..., C] -> [..., N]); differentiable in x, w and bias."""
    return _Product.apply(x, w, bias, be, 1, 1, False)


def conv3x3(be, x, w, bias=None, stride=1, ups=False):
    """3x3 convolution, padding 1, of NHWC ``x`` with ``w`` [N][9*C]; ``stride`` 1 or 2, or ``ups``: through a nearest
    2x upsample.  Differentiable in w and bias for every form; in x for stride 1 without upsample only."""
    if stride not in (1, 2) or (ups and stride != 1) or x.dim() != 4:
        raise ValueError(f"conv3x3 takes NHWC x, stride 1 or 2, or ups with stride 1 (got stride {stride}, ups {ups})")
    if (stride != 1 or ups) and x.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(
            f"conv3x3(stride={stride}, ups={bool(ups)}) has no data gradient yet: the strided / upsampled dgrad kernel is "
            "missing; pass x.detach() to get the weight and bias gradients")
    return _Product.apply(x, w, bias, be, 9, stride, bool(ups))
