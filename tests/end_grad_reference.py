"""float64 references for the gradients of the UNet's 4-channel end convolutions and of the loss
(include/dadd_hip_end_grad.h, csrc/end_grad.hip).

Index-level models: every function here is written from the index formulas of the header - shifted slices of zero-padded
maps, explicit tap loops - and NOT from ``F.conv2d``, so that comparing them with autograd of ``F.conv2d`` checks the
algebra (tap flip, transposition, pad channels) the kernels implement.

Layouts are the library's: ``thin`` fp32 NCHW [B,Ct,H,W], ``wide`` NHWC [B,H,W,Cw]; IN mode dw [Cw][9][8] (the
``pack_conv_cin8`` layout, channels >= Ct zero), OUT mode dw [Ct][9][Cw] (``pack_conv_cout4``).
"""
import functools

import torch
import torch.nn.functional as F

from tests import dgrad_reference as D
from tests import grad_reference as R

IN, OUT = 0, 1
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64


def shifted(t_nchw, dy, dx):
    """s[b,c,y,x] = t[b,c,y+dy,x+dx], zero outside the map."""
    h, w = t_nchw.shape[2:]
    p = F.pad(t_nchw, (1, 1, 1, 1))
    return p[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def conv_in_nchw_model(x_nchw, w8, bias=None):
    """``dadd_conv_in_nchw_*`` in float64: out[b,y,x,n] = bias[n] + sum_{tap,c<Ct} x[b,c,y+ky-1,x+kx-1] * w8[n][tap][c]
    with w8 [N][9][8]; -> NHWC [B,H,W,N]."""
    b, ct, h, w = x_nchw.shape
    n = w8.shape[0]
    out = torch.zeros(b, h, w, n, dtype=F64)
    for tap in range(9):
        s = shifted(x_nchw.double(), tap // 3 - 1, tap % 3 - 1)                 # [B,Ct,H,W]
        out += torch.einsum("bchw,nc->bhwn", s, w8[:, tap, :ct].double())
    return out if bias is None else out + bias.double()


def end_wgrad_model(thin, wide, mode):
    """Both modes of ``dadd_conv_end_wgrad_*`` in float64 from the kernel's one formula
    G[tap][t][n] = sum_p wide[p][n] * thin[t][p + off(tap)], stored as dw[n][tap][t] (IN) or dw[t][8 - tap][n] (OUT).
    ``thin`` is taken as given (round it first to model the kernel's r()).  -> (dw, dbias) in the kernel's layouts."""
    b, ct, h, w = thin.shape
    cw = wide.shape[-1]
    g = torch.stack([torch.einsum("bthw,bhwn->tn", shifted(thin.double(), tap // 3 - 1, tap % 3 - 1), wide.double())
                     for tap in range(9)])                                       # [tap][t][n]
    if mode == IN:
        dw = torch.zeros(cw, 9, 8, dtype=F64)
        dw[:, :, :ct] = g.permute(2, 0, 1)
        return dw, wide.double().sum((0, 1, 2))
    dw = g.flip(0).permute(1, 0, 2).contiguous()                                 # [t][8 - tap][n]
    return dw, thin.double().sum((0, 2, 3))


def conv2d_grads(x_nchw, w_oihw, dy_nchw):
    """float64 autograd of F.conv2d(padding=1) -> (dx NCHW, dw [O,I,3,3], dbias [O])."""
    x = x_nchw.double().clone().requires_grad_(True)
    w = w_oihw.double().clone().requires_grad_(True)
    bias = torch.zeros(w.shape[0], dtype=F64, requires_grad=True)
    F.conv2d(x, w, bias, padding=1).backward(dy_nchw.double())
    return x.grad, w.grad, bias.grad


def nchw(t_nhwc):
    return t_nhwc.permute(0, 3, 1, 2).contiguous()


def nhwc(t_nchw):
    return t_nchw.permute(0, 2, 3, 1).contiguous()


# ---- the operands of the GPU cases, computed once and shared (never modified by a test) -------------------------------------
@functools.lru_cache(maxsize=None)
def wgrad_case(b, h, w, ct, cw, mode, dtype=F16, integer=False):
    """-> (thin fp32 NCHW, wide 16-bit NHWC, WgradRef from r(thin) and wide).  ``integer``: small integer operands, every
    partial sum below 2^24, so fp32 accumulation in any order is exact."""
    g = torch.Generator().manual_seed(1000 + 97 * b + 13 * h + 7 * w + 3 * ct + cw + mode)
    if integer:
        thin = torch.randint(-3, 4, (b, ct, h, w), generator=g).float()
        wide = torch.randint(-4, 5, (b, h, w, cw), generator=g).to(dtype)
    else:
        thin = torch.randn((b, ct, h, w), generator=g)
        wide = torch.randn((b, h, w, cw), generator=g).to(dtype)
    thin16 = nhwc(thin.to(dtype))
    ref = R.WgradRef(thin16, wide, 9) if mode == IN else R.WgradRef(wide, thin16, 9)
    return thin, wide, ref


# ---- the UNet's shell: conv_in -> GN+SiLU -> conv3x3 -> GN+SiLU -> conv_out -> Min-SNR MSE ------------------------------------
def shell_stage64(lat, target, wrow, q):
    """float64: latents NCHW [B,4,H,W] -> the scalar (wrow * mse_rows).mean(); ``q`` holds the parameters in the library
    layouts (w* [N][9*C], c* biases, g* / b* GroupNorm affine)."""
    h = D.conv64(nhwc(lat), q["w_in"], q["c_in"])
    h = D.conv64(D.gn_silu64(h, q["g1"], q["b1"]), q["w_mid"], q["c_mid"])
    pred = nchw(D.conv64(D.gn_silu64(h, q["g2"], q["b2"]), q["w_out"], q["c_out"]))
    base = ((pred - target) ** 2).mean((1, 2, 3))
    return (wrow * base).mean()
