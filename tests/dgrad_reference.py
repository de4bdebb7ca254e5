"""The data gradient of the stride-2 and the upsampled 3x3 conv (csrc/dgrad.hip): the tap tables of
include/dadd_hip_dgrad.h restated, a plain-torch model of the kernel on the re-laid weights of ``grad_ops``
(``dgrad_weight_stride2`` / ``dgrad_weight_ups``), the cases of the CPU and GPU suites and their float64 references from
``grad_reference.conv_autograd`` on the same 16-bit operands.

Tolerances.  dx is a 16-bit output: fp16 takes the project's conv tolerance 3e-3 + 2e-3 |ref| (``grad_reference.close``),
bf16 takes 2e-2 + 1.6e-2 |ref| (``norm_grad_reference.TOL16``).  The stride-2 gradient has the rounding points of the
stride-1 one (16-bit operands, fp32 sums, dx rounded once).  The upsample has one more: the 16 weights W4 are sums of 1,
2 or 4 taps, formed in fp32 and rounded to the operand type.  The model below carries exactly these rounding points; its
worst err/bound over the cases below is printed by tests/test_dgrad_cpu.py: stride 2 at most 0.15 for either type, which
is the rounding of the float64 dx alone; upsample at most 0.66 (fp16) and 0.71 (bf16), of which rounding dx alone is 0.20.
"""
import collections
import functools

import torch

from progressive_stable_diffusion_amd import grad_ops
from tests import grad_reference as R

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64

# ---- tap tables (include/dadd_hip_dgrad.h) ---------------------------------------------------------------------------
# stride 2: parity class (py, px) of input pixel (2 jy + py, 2 jx + px) -> (first slab, taps); slab -> (ky, kx) of the
# forward weight and the source output pixel (jy + ey, jx + ex)
STRIDE2_CLASSES = {(0, 0): (0, 1), (0, 1): (1, 2), (1, 0): (3, 2), (1, 1): (5, 4)}
STRIDE2_KYX = ((1, 1), (1, 0), (1, 2), (0, 1), (2, 1), (0, 0), (0, 2), (2, 0), (2, 2))
STRIDE2_SRC = tuple((int(ky == 0), int(kx == 0)) for ky, kx in STRIDE2_KYX)
# upsample: one class; slab 4 (e + 1) + (f + 1) reads output pixel (2 iy + e, 2 ix + f), e, f in {-1, 0, 1, 2}
UPS_SRC = tuple((e, f) for e in (-1, 0, 1, 2) for f in (-1, 0, 1, 2))

Case = collections.namedtuple("Case", "mode b h w c n")
CASES = (Case("stride2", 2, 16, 16, 64, 72),     # ragged K; whole tiles
         Case("stride2", 2, 7, 9, 64, 64),       # four unequal classes below one tile; oy + 1 == Ho; batch edge in a tile
         Case("stride2", 1, 6, 10, 128, 64),     # H and W swapped; two c tiles
         Case("stride2", 3, 10, 10, 64, 128),    # 75 rows per class: a ragged second tile
         Case("ups", 2, 8, 8, 64, 72),
         Case("ups", 1, 3, 5, 128, 64),          # M = 15
         Case("ups", 3, 5, 5, 64, 128),
         Case("stride2", 4, 16, 16, 128, 64),    # 16 x 2 workgroups, renumbered across the XCDs (xcd_by_c)
         Case("ups", 8, 8, 8, 192, 64))          # 8 x 3 workgroups, renumbered
BF16_CASES = (CASES[1], CASES[4])
EXACT_CASES = (Case("stride2", 2, 7, 9, 64, 200), Case("ups", 2, 5, 6, 64, 136))


def out_hw(case):
    return (2 * case.h, 2 * case.w) if case.mode == "ups" else ((case.h - 1) // 2 + 1, (case.w - 1) // 2 + 1)


def relaid(w, mode):
    return grad_ops.dgrad_weight_ups(w) if mode == "ups" else grad_ops.dgrad_weight_stride2(w)


def classes(mode):
    """-> (so, sd, [(py, px, first_slab, ntaps)], slab -> (ey, ex))."""
    if mode == "ups":
        return 1, 2, [(0, 0, 0, 16)], UPS_SRC
    return 2, 1, [(py, px, s0, nt) for (py, px), (s0, nt) in STRIDE2_CLASSES.items()], STRIDE2_SRC


def model(dy, wt, mode, hi, wi, acc=F32, out_dtype=None):
    """The kernel in plain torch: per class, per tap, the gathered rows of dy (zero outside the map) times the tap's slab
    of ``wt`` [C][T*N], summed in ``acc``; dx [B,hi,wi,C] rounded once to ``out_dtype`` (default: dy's type).  Every
    pixel of dx belongs to exactly one class: what no class writes stays NaN."""
    b, ho, wo, n = dy.shape
    c = wt.shape[0]
    so, sd, cls, src = classes(mode)
    dya, wta = dy.to(acc), wt.to(acc).reshape(c, len(src), n)
    dx = torch.full((b, hi, wi, c), float("nan"), dtype=acc)
    for py, px, s0, nt in cls:
        hc, wc = len(range(py, hi, so)), len(range(px, wi, so))
        if hc == 0 or wc == 0:
            continue
        total = torch.zeros((b, hc, wc, c), dtype=acc)
        for s in range(s0, s0 + nt):
            y, x = torch.arange(hc) * sd + src[s][0], torch.arange(wc) * sd + src[s][1]
            inside = ((y >= 0) & (y < ho))[:, None] & ((x >= 0) & (x < wo))[None, :]
            rows = dya[:, y.clamp(0, ho - 1)][:, :, x.clamp(0, wo - 1)] * inside[None, :, :, None].to(acc)
            total += rows @ wta[:, s].t()
        dx[:, py::so, px::so] = total
    return dx.to(out_dtype or dy.dtype)


def bound_ratio(got, ref, atol, rtol):
    """Worst elementwise |got - ref| / (atol + rtol |ref|)."""
    got, ref = got.detach().double().cpu(), ref.double()
    return ((got - ref).abs() / (atol + rtol * ref.abs())).max().item()


# ---- operands and float64 references, computed once and shared (never modified by a test) -----------------------------
@functools.lru_cache(maxsize=None)
def case_operands(case, dtype=F16):
    """-> (dy 16-bit [B,Ho,Wo,N], w 16-bit [N][9*C], dx float64 [B,H,W,C] from autograd on those operands)."""
    ho, wo = out_hw(case)
    seed = 7000 + 13 * CASES.index(case) if case in CASES else 7900
    dy = R.rnd((case.b, ho, wo, case.n), seed, dtype=dtype)
    w = R.rnd((case.n, 9 * case.c), seed + 1, (9 * case.c) ** -0.5, dtype)
    x0 = torch.zeros((case.b, case.h, case.w, case.c), dtype=dtype)
    _, dx, _, _ = R.conv_autograd(x0, w, dy, 9, 2 if case.mode == "stride2" else 1, case.mode == "ups")
    return dy, w, dx


@functools.lru_cache(maxsize=None)
def exact_operands(case):
    """Integer operands: dy in {-2..2}, w in {-1, 0, 1}, asymmetric in (ky, kx) and in (n, c); every partial sum and every
    W4 is an integer that fp16 and fp32 hold exactly, so dx must equal the float64 result bit for bit."""
    ho, wo = out_hw(case)
    g = torch.Generator().manual_seed(8100 + len(case.mode))
    dy = torch.randint(-2, 3, (case.b, ho, wo, case.n), generator=g).to(F16)
    w = torch.randint(-1, 2, (case.n, 3, 3, case.c), generator=g)
    assert not torch.equal(w, w.transpose(1, 2)) and not torch.equal(w[:64, ..., :64], w[:64, ..., :64].transpose(0, 3))
    w = w.reshape(case.n, 9 * case.c).to(F16)
    x0 = torch.zeros((case.b, case.h, case.w, case.c), dtype=F16)
    _, dx, _, _ = R.conv_autograd(x0, w, dy, 9, 2 if case.mode == "stride2" else 1, case.mode == "ups")
    assert dx.abs().max().item() < 2048 and bool((dx == dx.round()).all())
    return dy, w, dx


# ---- the two composed stages of tests/test_gpu_dgrad.py in float64 --------------------------------------------------------
def conv64(x, w, bias, stride=1, ups=False):
    """NHWC float64 conv3x3 with the library's weight layout [N][9*C]."""
    import torch.nn.functional as F
    n, c = w.shape[0], x.shape[-1]
    xi = x.permute(0, 3, 1, 2)
    if ups:
        xi = F.interpolate(xi, scale_factor=2.0, mode="nearest")
    y = F.conv2d(xi, w.reshape(n, 3, 3, c).permute(0, 3, 1, 2), bias, stride=stride, padding=1)
    return y.permute(0, 2, 3, 1)


def gn_silu64(x, gamma, beta, groups=32, eps=1e-5):
    import torch.nn.functional as F
    return F.silu(F.group_norm(x.permute(0, 3, 1, 2), groups, gamma, beta, eps)).permute(0, 2, 3, 1)


def down_stage64(x, q):
    """GroupNorm+SiLU -> conv3x3 -> Downsample2D conv -> conv3x3."""
    h = conv64(gn_silu64(x, q["g"], q["b"]), q["w1"], q["c1"])
    return conv64(conv64(h, q["wd"], q["cd"], stride=2), q["w2"], q["c2"])


def up_stage64(x, skip, q):
    """Upsample2D(x) -> GroupNorm+SiLU of [h | skip] -> conv3x3."""
    h = conv64(x, q["wu"], q["cu"], ups=True)
    return conv64(gn_silu64(torch.cat([h, skip], -1), q["g"], q["b"]), q["w1"], q["c1"])
