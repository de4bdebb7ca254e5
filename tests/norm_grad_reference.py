"""float64 references for the backward of GroupNorm(+SiLU), LayerNorm and GEGLU, computed by autograd (``F.group_norm``,
``F.silu``, ``F.layer_norm``, exact ``F.gelu``) FROM THE SAME 16-BIT ``x`` / ``dy`` AND fp32 ``gamma`` / ``beta`` the
kernels get; the error bounds; and a plain-torch fp32 restatement of the kernels' formulas (csrc/norm_grad.hip) with the
chunk partials combined in the kernels' order, so that the algebra is checked without a GPU.

Operands are non-centred, as in the forward tests: x = 1.5 randn + 0.3, gamma = 1 + 0.2 randn, beta = 0.2 randn.

Bounds.
16-bit outputs (dx, dh, y of GEGLU): fp16 takes the project's 3e-3 + 2e-3 |ref| (``grad_reference.close``); bf16 takes
2e-2 + 1.6e-2 |ref|, the bound of test_groupnorm_bf16 (rounding the float64 reference to fp16 uses at most 0.21 of the
fp16 bound on the cases of the suite; rounding it to bf16 alone exceeds the fp16 bound, 1.33 of it on the GroupNorm case).
fp32 outputs (dgamma, dbeta), elementwise: |got - ref| <= (M + 16) * 2^-24 * E, with M the number of summed terms per
channel (B*HW for GroupNorm, rows for LayerNorm) and E the float64 sum of the absolute values of the same terms,
sum |dz * xhat| and sum |dz|.  M * 2^-24 * E bounds the fp32 accumulation of M terms in any order (the derivation of
``grad_reference.WgradRef``: every partial sum is at most E and every addition rounds once).  The + 16 covers the fp32
evaluation of each term (xhat, the sigmoid, their products): torch's fp32 evaluation of the same formulas against float64
came to at most 3.2 * 2^-24 * E over all cases of the suite; four times that, rounded up, leaves room for the hardware
exp and rcp.  A dropped or doubled row is about E / M, at least 25 times the bound at every M used here.
"""
import functools

import torch
import torch.nn.functional as F

from tests import grad_reference as R

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
TOL16 = {F16: (R.CONV_ATOL, R.CONV_RTOL), BF16: (2e-2, 1.6e-2)}
GROUPS = 32


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def operands(shape, c, seed, dtype=F16):
    """-> x, dy in ``dtype`` of ``shape`` (x non-centred) and fp32 gamma, beta [c]."""
    x = (1.5 * _randn(shape, seed) + 0.3).to(dtype)
    dy = _randn(shape, seed + 1).to(dtype)
    return x, dy, 1.0 + 0.2 * _randn((c,), seed + 2), 0.2 * _randn((c,), seed + 3)


def close16(got, ref, what):
    """A 16-bit output against the float64 reference, with the tolerance of its type (module docstring)."""
    assert got.dtype in TOL16, (what, got.dtype)
    atol, rtol = TOL16[got.dtype]
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite values"
    R.close(got, ref, what, atol=atol, rtol=rtol)


def sum_bound(m, e):
    return (m + 16) * 2.0 ** -24 * e


def check_sums(got, ref, e, m, what):
    """An fp32 column sum (dgamma or dbeta) against float64: elementwise (M + 16) * 2^-24 * E."""
    assert got.dtype == F32, (what, got.dtype)
    got = got.detach().double().cpu().reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    err, bound = (got - ref).abs(), sum_bound(m, e)
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, worst err/bound {worst:.3f} (M = {m})")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())}/{err.numel()} over the bound, worst ratio {worst:.2f}"


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.double().reshape(-1)
    return ((got - ref).norm() / ref.norm().clamp_min(1e-300)).item()


class NormRef:
    """dx, dgamma, dbeta in float64 and E of the two column sums; ``m`` = summed terms per channel."""

    def check(self, dx=None, dgamma=None, dbeta=None, what=""):
        if dx is not None:
            close16(dx, self.dx.reshape(dx.shape), f"{what} dx")
        if dgamma is not None:
            check_sums(dgamma, self.dgamma, self.e_gamma, self.m, f"{what} dgamma")
        if dbeta is not None:
            check_sums(dbeta, self.dbeta, self.e_beta, self.m, f"{what} dbeta")


def _silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1.0 + z * (1.0 - s))


def gn_ref(x16, dy16, gamma, beta, eps, silu, groups=GROUPS):
    """x16, dy16 NHWC [B,H,W,C] -> NormRef (dx NHWC)."""
    b, h, w, c = x16.shape
    x = x16.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    g, bt = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    y = F.group_norm(x, groups, g, bt, eps)
    (F.silu(y) if silu else y).backward(dy16.double().permute(0, 3, 1, 2))
    r = NormRef()
    r.dx, r.dgamma, r.dbeta, r.m = x.grad.permute(0, 2, 3, 1), g.grad, bt.grad, b * h * w
    with torch.no_grad():           # the summed terms themselves, for E
        xg = x16.double().reshape(b, h * w, groups, c // groups)
        mu = xg.mean(dim=(1, 3), keepdim=True)
        var = ((xg - mu) ** 2).mean(dim=(1, 3), keepdim=True)
        xhat = ((xg - mu) / torch.sqrt(var + eps)).reshape(b, h * w, c)
        dz = dy16.double().reshape(b, h * w, c)
        if silu:
            dz = dz * _silu_grad(xhat * gamma.double() + beta.double())
        r.e_gamma, r.e_beta = (dz * xhat).abs().sum(dim=(0, 1)), dz.abs().sum(dim=(0, 1))
    return r


def ln_ref(x16, dy16, gamma, beta, eps):
    c = x16.shape[-1]
    x = x16.double().reshape(-1, c).clone().requires_grad_(True)
    g, bt = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    F.layer_norm(x, (c,), g, bt, eps).backward(dy16.double().reshape(-1, c))
    r = NormRef()
    r.dx, r.dgamma, r.dbeta, r.m = x.grad.reshape(x16.shape), g.grad, bt.grad, x.shape[0]
    with torch.no_grad():
        xd = x.detach()
        mu = xd.mean(dim=1, keepdim=True)
        xhat = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(dim=1, keepdim=True) + eps)
        dy = dy16.double().reshape(-1, c)
        r.e_gamma, r.e_beta = (dy * xhat).abs().sum(dim=0), dy.abs().sum(dim=0)
    return r


def geglu_ref(h16, dy16):
    """-> (y, dh) in float64: y = h[:, :F] * gelu(h[:, F:]) with the exact gelu."""
    h = h16.double().clone().requires_grad_(True)
    a, g = h.chunk(2, dim=-1)
    y = a * F.gelu(g)
    y.backward(dy16.double())
    return y.detach(), h.grad


# ---- the cases, computed once and shared (never modified by a test) --------------------------------------------------
@functools.lru_cache(maxsize=None)
def gn_case(b, c1, c2, h, w, silu, eps, dtype=F16, constant_group=False):
    """-> (x [B,H,W,C1+C2], dy, gamma, beta, NormRef).  ``constant_group``: (sample 1, group 3) of x is the constant 0.5."""
    c = c1 + c2
    x, dy, gamma, beta = operands((b, h, w, c), c, 1000 + c + h * w, dtype)
    if constant_group:
        cg = c // GROUPS
        x[b - 1, :, :, 3 * cg:4 * cg] = 0.5
    return x, dy, gamma, beta, gn_ref(x, dy, gamma, beta, eps, bool(silu))


@functools.lru_cache(maxsize=None)
def ln_case(m, c, dtype=F16, eps=1e-5):
    x, dy, gamma, beta = operands((m, c), c, 2000 + m + c, dtype)
    return x, dy, gamma, beta, ln_ref(x, dy, gamma, beta, eps)


@functools.lru_cache(maxsize=None)
def geglu_case(m, f, dtype=F16):
    h, dy = (1.5 * _randn((m, 2 * f), 3000 + m + f) + 0.3).to(dtype), _randn((m, f), 3001 + m + f).to(dtype)
    return h, dy, geglu_ref(h, dy)


GN_CASES = [(2, 320, 0, 8, 8, 1, 1e-5), (2, 64, 0, 12, 12, 1, 1e-5), (2, 640, 320, 10, 10, 0, 1e-6),
            (2, 1280, 1280, 4, 4, 1, 1e-5), (1, 320, 0, 64, 64, 1, 1e-5)]
LN_CASES = [(3, 8), (130, 320), (37, 1280), (65, 2048), (1030, 320)]
GEGLU_CASES = [(5, 8), (130, 1280)]


# ---- the kernels' formulas in plain torch, fp32, chunk partials combined in the kernels' order -----------------------
def gn_geometry(b, hw, c):
    """Row chunks of the statistics / partials passes (gng_geom of csrc/norm_grad.hip) -> (nchunk, rows per chunk)."""
    nvec = c // 8
    tv = min(nvec, 256)
    rp = 256 // tv
    nchunk = hw // max(2 * rp, 16)
    if b * nchunk < 256:
        nchunk = hw // (4 * rp)
    nchunk = max(1, min(64, nchunk))
    rows = -(-hw // nchunk)
    return -(-hw // rows), rows


def gn_model(x16, dy16, gamma, beta, eps, silu, groups=GROUPS):
    """-> dx (x16.dtype), dgamma, dbeta (fp32) by the passes of the kernels: fp32 chunk sums of x - p and (x - p)^2 about
    the slab's first element p, combined in double with max(var, 0); per-chunk channel sums of dz and dz*xhat, their gamma-weighted group sums combined in double into
    s1/n and s2/n; dx = rstd * (dz*gamma - (s1/n + xhat * s2/n)); the channel sums added over (sample, chunk) in double."""
    b, h, w, c = x16.shape
    hw, cg = h * w, c // groups
    nchunk, rows = gn_geometry(b, hw, c)
    x, dy = x16.float().reshape(b, hw, c), dy16.float().reshape(b, hw, c)
    chunks = [slice(k * rows, min(hw, (k + 1) * rows)) for k in range(nchunk)]
    n = float(hw * cg)
    piv = x[:, 0].reshape(b, groups, cg)[:, :, 0]                    # [B][G]: the first element of every slab
    xp = x - piv.repeat_interleave(cg, dim=1)[:, None, :]
    st = torch.stack([torch.stack([xp[:, s].reshape(b, -1, groups, cg).sum(dim=(1, 3)),
                                   (xp[:, s] ** 2).reshape(b, -1, groups, cg).sum(dim=(1, 3))], -1) for s in chunks], 1)
    tot = st.double().sum(dim=1)                                     # [B][G][2]
    d = tot[..., 0] / n
    var = (tot[..., 1] / n - d * d).clamp_min(0.0)
    mu = piv.double() + d
    mean = mu.float().repeat_interleave(cg, dim=1)[:, None, :]       # [B][1][C]
    rstd = (1.0 / torch.sqrt(var + eps)).float().repeat_interleave(cg, dim=1)[:, None, :]
    xhat = (x - mean) * rstd
    dz = dy * _silu_grad(xhat * gamma + beta) if silu else dy
    cp = torch.stack([torch.stack([dz[:, s].sum(dim=1), (dz[:, s] * xhat[:, s]).sum(dim=1)], -1) for s in chunks], 1)
    gp = (cp * gamma[None, None, :, None]).reshape(b, nchunk, groups, cg, 2).sum(dim=3)
    sn = (gp.double().sum(dim=1) / n).float().repeat_interleave(cg, dim=1)[:, None]      # [B][1][C][2]
    dx = rstd * (dz * gamma - (sn[..., 0] + xhat * sn[..., 1]))
    col = cp.double().sum(dim=(0, 1)).float()                        # [C][2]
    return dx.to(x16.dtype).reshape(x16.shape), col[:, 1].contiguous(), col[:, 0].contiguous()


def ln_model(x16, dy16, gamma, eps):
    """Rows in fp32 with the two-pass variance; the column sums per workgroup (rows 4k .. 4k+3 of every nblk-th quad),
    the workgroups added in double."""
    c = x16.shape[-1]
    x, dy = x16.float().reshape(-1, c), dy16.float().reshape(-1, c)
    m = x.shape[0]
    mean = x.mean(dim=1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(dim=1, keepdim=True) + eps)
    xhat = (x - mean) * rstd
    a = dy * gamma
    dx = rstd * (a - (a.mean(dim=1, keepdim=True) + xhat * (a * xhat).mean(dim=1, keepdim=True)))
    nblk = min(256, -(-m // 8))
    blk = (torch.arange(m) // 4) % nblk
    part = torch.zeros(nblk, c, 2)
    part.index_add_(0, blk, torch.stack([dy, dy * xhat], -1))
    col = part.double().sum(dim=0).float()
    return dx.to(x16.dtype).reshape(x16.shape), col[:, 1].contiguous(), col[:, 0].contiguous()


def _phi(g):
    """Phi and phi of the kernels: erf of Abramowitz & Stegun 7.1.26 in fp32 (dadd_gelu)."""
    z = g.abs() * 0.70710678118654752440
    t = 1.0 / (0.3275911 * z + 1.0)
    p = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592)
    e = torch.exp(-z * z)
    erf_abs = 1.0 - p * t * e
    return 0.5 * (1.0 + torch.copysign(erf_abs, g)), 0.39894228040143267794 * e


def geglu_model(h16, dy16):
    f = h16.shape[-1] // 2
    a, g, dy = h16[..., :f].float(), h16[..., f:].float(), dy16.float()
    big, small = _phi(g)
    y = a * (g * big)
    dh = torch.cat([dy * g * big, dy * a * (big + g * small)], -1)
    return y.to(h16.dtype), dh.to(h16.dtype)


# ---- the two composed blocks of the GPU suite, in float64 --------------------------------------------------------------
def conv3x3_nhwc(x, w, bias):
    """x [B,H,W,C] float64, w [N][9*C] in the library layout."""
    n, c = w.shape[0], x.shape[-1]
    return F.conv2d(x.permute(0, 3, 1, 2), w.reshape(n, 3, 3, c).permute(0, 3, 1, 2), bias, padding=1).permute(0, 2, 3, 1)


def gn_nhwc(x, gamma, beta, eps, silu):
    y = F.group_norm(x.permute(0, 3, 1, 2), GROUPS, gamma, beta, eps).permute(0, 2, 3, 1)
    return F.silu(y) if silu else y


def resnet_block64(x, temb, p):
    """norm -> SiLU -> conv3x3 -> + time row -> norm -> SiLU -> conv3x3 -> + 1x1 shortcut, float64, NHWC."""
    hdn = conv3x3_nhwc(gn_nhwc(x, p["g1"], p["b1"], 1e-5, True), p["w1"], p["c1"])
    hdn = hdn + temb[:, None, None, :]
    hdn = conv3x3_nhwc(gn_nhwc(hdn, p["g2"], p["b2"], 1e-5, True), p["w2"], p["c2"])
    return hdn + (x @ p["ws"].t() + p["cs"])


def feed_forward64(x, p):
    """LayerNorm -> Linear -> GEGLU -> Linear -> + x, float64."""
    c = x.shape[-1]
    hdn = F.layer_norm(x, (c,), p["g"], p["b"], 1e-5) @ p["w1"].t() + p["c1"]
    a, g = hdn.chunk(2, dim=-1)
    return (a * F.gelu(g)) @ p["w2"].t() + p["c2"] + x
