"""Differentiable Linear / conv3x3, GroupNorm(+SiLU), LayerNorm and GEGLU on the HIP kernels: the operators of a training
step and their gradients.

Matrix products: forward is ``HipBackend.igemm``; the data gradient is the same kernel on ``dy`` with the weight re-laid
by ``dgrad_weight``; the weight and bias gradients are the M-reduction GEMM of ``HipBackend.wgrad`` (csrc/wgrad.hip).
Norms and gating: forward is ``HipBackend.groupnorm`` / ``layernorm`` / ``geglu``, backward the reduction kernels of
csrc/norm_grad.hip (``groupnorm_grad`` / ``layernorm_grad`` / ``geglu_grad``), which recompute the statistics from the
saved input.  With these a ResnetBlock2D and a transformer feed-forward are differentiable end to end.
These are operators, not the training loop: attention has no backward yet, and neither do the strided / upsampled data
gradient and the 4-channel end convolutions.

Operands: ``x`` is a 16-bit (fp16 or bf16) NHWC / token-major tensor on the backend's device, ``w`` the **fp32 master**
weight in the library layout ``[N][taps*C]`` (``[Cout][ky][kx][Cin]`` flattened), ``bias`` / ``gamma`` / ``beta`` fp32.
The forward of a product rounds the master to ``x.dtype`` once and keeps the rounded copy for the backward; gradients of
``w``, ``bias``, ``gamma`` and ``beta`` come back in fp32, the gradient of ``x`` in ``x.dtype``.
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
        be.wait_current()
        y = be.empty(x.shape[:-1] + (c,), x.dtype)
        ws = be.empty((x.shape[0] * L.GN_MAX_CHUNKS * groups * 2,), torch.float32)
        be.groupnorm(x, x2, gamma, beta, y, ws, groups, eps, silu)
        be.release_to_current()
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
        be.wait_current()
        dx1 = be.empty(tuple(x.shape), x.dtype) if need_dx else None
        dx2 = be.empty(tuple(x2.shape), x.dtype) if need_dx and x2 is not None else None
        dg = be.empty((c,), torch.float32) if need_dp else None
        db = be.empty((c,), torch.float32) if need_dp else None
        ws = be.empty((be.groupnorm_grad_ws_numel(b, hw, c, groups),), torch.float32)
        be.groupnorm_grad(x, x2, dy, gamma, beta, dx1=dx1, dx2=dx2, dgamma=dg, dbeta=db, ws=ws, groups=groups, eps=eps,
                          silu=silu)
        be.release_to_current()
        return (dx1 if need_x else None, dx2 if need_x2 else None, dg if need_g else None, db if need_b else None,
                None, None, None, None)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, be, eps):
        _check16(x, "x")
        _check_affine(gamma, beta, x.shape[-1])
        x, gamma, beta = x.contiguous(), gamma.contiguous(), beta.contiguous()
        be.wait_current()
        y = be.empty(tuple(x.shape), x.dtype)
        be.layernorm(x, gamma, beta, y, eps)
        be.release_to_current()
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
        be.wait_current()
        dx = be.empty(tuple(x.shape), x.dtype) if need_x else None
        dg = be.empty((c,), torch.float32) if need_dp else None
        db = be.empty((c,), torch.float32) if need_dp else None
        ws = be.empty((be.layernorm_grad_ws_numel(x.numel() // c, c),), torch.float32) if need_dp else None
        be.layernorm_grad(x, dy, gamma, dx=dx, dgamma=dg, dbeta=db, ws=ws, eps=ctx.eps)
        be.release_to_current()
        return dx, dg if need_g else None, db if need_b else None, None, None


class _Geglu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, be):
        _check16(h, "h")
        if h.shape[-1] % 16:
            raise ValueError(f"geglu takes h [..., 2F] with F a multiple of 8, got {tuple(h.shape)}")
        h = h.contiguous()
        be.wait_current()
        y = be.empty(h.shape[:-1] + (h.shape[-1] // 2,), h.dtype)
        be.geglu(h, y)
        be.release_to_current()
        ctx.save_for_backward(h)
        ctx.be = be
        return y

    @staticmethod
    def backward(ctx, dy):
        (h,) = ctx.saved_tensors
        be = ctx.be
        if not ctx.needs_input_grad[0]:
            return None, None
        dy = dy.to(h.dtype).contiguous()
        be.wait_current()
        dh = be.empty(tuple(h.shape), h.dtype)
        be.geglu_grad(h, dy, dh)
        be.release_to_current()
        return dh, None


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
    return _Geglu.apply(h, be)
