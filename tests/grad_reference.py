"""float64 references for the gradients of Linear / conv3x3, computed by autograd FROM THE SAME 16-BIT OPERANDS the
kernels get, and the error bound of the weight gradient.

Layouts are the library's: activations NHWC, weights ``[N][taps*C]`` = ``[Cout][ky][kx][Cin]``.

Bound of ``dW`` / ``dbias``: a product of two fp16 (or two bf16) values is exact in fp32, so only the fp32 accumulation
of the M terms errs, in whatever order it runs: |got - ref| <= (M + 2) * 2^-24 * E elementwise, with
E = (|dy|^T |x|)[n, tap, c] for dW and E = sum_m |dy[m][n]| for dbias - the same float64 reference on the absolute values.
"""
import functools

import torch
import torch.nn.functional as F

CONV_ATOL, CONV_RTOL = 3e-3, 2e-3      # the project's conv tolerance (tests/test_gpu_kernels.py)


def rnd(shape, seed, scale=1.0, dtype=torch.float16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def conv_autograd(x16, w16, dy16, taps=1, stride=1, ups=False, bias=None):
    """-> (y, dx, dw, db) in float64: y NHWC, dx NHWC, dw [N, taps*C], db [N].  x16 [B,H,W,C], w16 [N, taps*C],
    dy16 [B,Ho,Wo,N]."""
    n = w16.shape[0]
    c = x16.shape[-1]
    k = 3 if taps == 9 else 1
    x = x16.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    w = w16.double().reshape(n, k, k, c).permute(0, 3, 1, 2).clone().requires_grad_(True)
    b = (torch.zeros(n, dtype=torch.float64) if bias is None else bias.double().clone()).requires_grad_(True)
    xi = F.interpolate(x, scale_factor=2.0, mode="nearest") if ups else x
    y = F.conv2d(xi, w, b, stride=stride, padding=k // 2)
    assert y.shape[2:] == dy16.shape[1:3], (y.shape, dy16.shape)
    y.backward(dy16.double().permute(0, 3, 1, 2))
    return (y.detach().permute(0, 2, 3, 1), x.grad.permute(0, 2, 3, 1),
            w.grad.permute(0, 2, 3, 1).reshape(n, taps * c), b.grad)


def _as4(t):
    return t.reshape(1, 1, *t.shape) if t.dim() == 2 else t


class WgradRef:
    """dW [N, taps, C] and dbias [N] in float64 with their elementwise bounds (module docstring)."""

    def __init__(self, x16, dy16, taps=1, stride=1, ups=False):
        x16, dy16 = _as4(x16), _as4(dy16)
        n, c = dy16.shape[-1], x16.shape[-1]
        self.m = dy16.shape[0] * dy16.shape[1] * dy16.shape[2]
        zero_w = torch.zeros(n, taps * c, dtype=x16.dtype)
        _, _, dw, db = conv_autograd(x16, zero_w, dy16, taps, stride, ups)
        _, _, ew, eb = conv_autograd(x16.abs(), zero_w, dy16.abs(), taps, stride, ups)
        u = (self.m + 2) * 2.0 ** -24
        self.dw, self.db = dw.reshape(n, taps, c), db
        self.dw_bound, self.db_bound = u * ew.reshape(n, taps, c), u * eb

    def check(self, dw=None, db=None, what="", cols=None):
        """``cols`` = slice of the c axis that ``dw`` [N, taps, len(cols)] holds (one source of a skip-concat)."""
        for name, got, ref, bound in (("dW", dw, self.dw, self.dw_bound), ("dbias", db, self.db, self.db_bound)):
            if got is None:
                continue
            assert got.dtype == torch.float32, (name, got.dtype)
            got = got.detach().double().cpu().reshape((ref.shape[0], ref.shape[1], -1) if name == "dW" else (-1,))
            if cols is not None and name == "dW":
                ref, bound = ref[..., cols], bound[..., cols]
            assert bool(torch.isfinite(got).all()), f"{what} {name}: non-finite values"
            err = (got - ref).abs()
            worst = (err / bound.clamp_min(1e-300)).max().item()
            print(f"{what} {name}: max err {err.max().item():.3e}, worst err/bound {worst:.3f} (M = {self.m})")
            assert bool((err <= bound).all()), f"{what} {name}: {int((err > bound).sum())}/{err.numel()} over the bound, worst ratio {worst:.2f}"


def close(got, ref, what="", atol=CONV_ATOL, rtol=CONV_RTOL):
    got, ref = got.detach().double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    print(f"{what}: max err {err.max().item():.3e}")
    assert not bool(bad.any()), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {err.max().item():.4e}"


# ---- the operands of the cases, computed once and shared (never modified by a test) ----------------------------------
@functools.lru_cache(maxsize=None)
def linear_case(m, n, c, dtype=torch.float16):
    x, dy = rnd((m, c), 100 + m, dtype=dtype), rnd((m, n), 200 + n, dtype=dtype)
    return x, dy, WgradRef(x, dy)


@functools.lru_cache(maxsize=None)
def conv_case(b, h, c, n, stride=1, ups=False, dtype=torch.float16):
    ho = 2 * h if ups else (h - 1) // stride + 1
    x, dy = rnd((b, h, h, c), 300 + c + h, dtype=dtype), rnd((b, ho, ho, n), 400 + n + h, dtype=dtype)
    return x, dy, WgradRef(x, dy, 9, stride, ups)


@functools.lru_cache(maxsize=None)
def op_case(kind):
    """Operands of the operator / dgrad tests -> (x16, w32, bias32, dy16, taps, (y, dx, dw, db) in float64 from the
    16-bit operands)."""
    if kind == "conv":
        b, h, c, n, taps = 2, 12, 64, 128, 9
        x, dy = rnd((b, h, h, c), 501), rnd((b, h, h, n), 502)
    elif kind == "conv_s2":
        b, h, c, n, taps = 2, 16, 64, 72, 9
        x, dy = rnd((b, h, h, c), 503), rnd((b, h // 2, h // 2, n), 504)
    elif kind == "two_source":
        b, h, c, n, taps = 2, 8, 192, 64, 9
        x, dy = rnd((b, h, h, c), 505), rnd((b, h, h, n), 506)
    else:
        m, n, c, taps = 200, 192, 128, 1
        x, dy = rnd((1, 1, m, c), 507), rnd((1, 1, m, n), 508)
    w = rnd((n, taps * c), 509, (taps * c) ** -0.5, torch.float32)
    bias = rnd((n,), 510, 0.1, torch.float32)
    ref = conv_autograd(x, w.half(), dy, taps, 2 if kind == "conv_s2" else 1, False, bias)
    return x, w, bias, dy, taps, ref
