"""Float64 models, the fp32 yardstick and the inputs of the evaluation-metric tests (csrc/metrics.hip, evaluation.py).

Nothing here touches the GPU or the library: the CPU test checks these models against the reference's formulas and
against ``CLIPImageProcessor``; the GPU test checks the kernels against these models.
"""
import torch

F64 = torch.float64
DEFAULT_SIGMAS = (0.1, 1.0, 10.0, 100.0)
SIGMAS_8 = (0.05, 0.1, 0.5, 1.0, 2.0, 10.0, 50.0, 100.0)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

# (n, m, D, shift) of the input recipe: MMD^2 of -4.1e-3, -4.3e-3, +1.9e-3, +3.1e-3 with all four default bandwidths
# contributing, precision / recall 0.88 .. 1.0 at k = 3 ...
RECIPE_CASES = ((70, 45, 768, 0.0), (70, 45, 768, 0.5), (300, 257, 768, 0.2), (33, 17, 40, 0.3))
# ... and one with the sets pulled apart: precision 0.689, recall 0.129 at k = 3 (float64, chosen on the CPU)
FAR_CASE = (70, 45, 768, 4.0)
# further shapes of the rbf_mmd test: D no multiple of the K chunk (32), n and m just over a tile (64), a long K
EDGE_CASES = ((2, 2, 8, 0.3), (130, 129, 100, 0.3), (257, 64, 1024, 0.3))
SEED_PAIRS = ((1, 2), (3, 4), (5, 6))


def recipe_set(n, d, seed, shift=0.0):
    """One feature set (float64, unit rows): a common component, a 16-dimensional structured part, a little noise, and
    ``shift`` along the first structured direction."""
    g = torch.Generator().manual_seed(99)
    base = torch.randn(1, d, generator=g, dtype=F64)
    mix = 0.25 * torch.randn(16, d, generator=g, dtype=F64)
    gs = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 16, generator=gs, dtype=F64) @ mix + base + 0.05 * torch.randn(n, d, generator=gs, dtype=F64) + shift * mix[0]
    return x / x.norm(dim=1, keepdim=True)


def recipe(n, m, d, shift, seeds=(1, 2)):
    """X (seed ``seeds[0]``, no shift) and Y (seed ``seeds[1]``, ``shift``)."""
    return recipe_set(n, d, seeds[0]), recipe_set(m, d, seeds[1], shift)


# ------------------------------------------------------------------------------------------------ MMD
def sqdist64(a, b):
    """Squared distances from the differences themselves, float64."""
    return torch.cdist(a.to(F64), b.to(F64), p=2, compute_mode="donot_use_mm_for_euclid_dist").pow(2)


def mmd_model(x, y, sigmas=DEFAULT_SIGMAS):
    """The arithmetic the kernel is specified to do, in float64: u = -expm1(-d2 / (2 sigma^2)); per bandwidth the mean of u
    over i != j of XX, over i != j of YY, over all of XY -> (means [3, S], mmd2 = -sum_s (xx + yy - 2 xy))."""
    n, m = x.shape[0], y.shape[0]
    xx, yy, xy = sqdist64(x, x), sqdist64(y, y), sqdist64(x, y)
    off_x, off_y = ~torch.eye(n, dtype=torch.bool), ~torch.eye(m, dtype=torch.bool)
    means = torch.zeros(3, len(sigmas), dtype=F64)
    for s, sigma in enumerate(sigmas):
        gamma = 1.0 / (2.0 * sigma ** 2)
        means[0, s] = (-torch.expm1(-gamma * xx))[off_x].sum() / (n * (n - 1))
        means[1, s] = (-torch.expm1(-gamma * yy))[off_y].sum() / (m * (m - 1))
        means[2, s] = (-torch.expm1(-gamma * xy)).sum() / (n * m)
    return means, float(-(means[0] + means[1] - 2 * means[2]).sum())


def mmd_reference_formula(x, y, sigmas=DEFAULT_SIGMAS, dtype=F64):
    """The reference's ``_mmd_rbf`` restated (evaluation_pipeline.py:630-666) in ``dtype`` on the CPU: cdist(...).pow(2),
    exp, sum, diagonal subtracted, k_xx + k_yy - 2 k_xy accumulated as a Python float.  With ``dtype=torch.float32`` this
    is ``ref32``, the yardstick of the accuracy criterion."""
    x, y = x.to(dtype), y.to(dtype)
    n, m = x.shape[0], y.shape[0]
    if n < 2 or m < 2:
        return -1.0
    xx, yy, xy = torch.cdist(x, x, p=2).pow(2), torch.cdist(y, y, p=2).pow(2), torch.cdist(x, y, p=2).pow(2)
    mmd2 = 0.0
    for sigma in sigmas:
        gamma = 1.0 / (2.0 * sigma ** 2)
        kxx, kyy, kxy = torch.exp(-gamma * xx), torch.exp(-gamma * yy), torch.exp(-gamma * xy)
        kxx_sum = (kxx.sum() - kxx.diagonal().sum()) / (n * (n - 1))
        kyy_sum = (kyy.sum() - kyy.diagonal().sum()) / (m * (m - 1))
        kxy_sum = kxy.sum() / (n * m)
        mmd2 += float(kxx_sum + kyy_sum - 2 * kxy_sum)
    return mmd2


def ref32(x, y, sigmas=DEFAULT_SIGMAS):
    return mmd_reference_formula(x.to(torch.float32), y.to(torch.float32), sigmas, torch.float32)


# ------------------------------------------------------------------------------------------------ precision / recall
def knn_radius_model(x, k):
    """Distance to the (k+1)-th smallest of each row's distances to its own set, itself included; float64."""
    return sqdist64(x, x).sqrt().topk(k + 1, largest=False).values[:, -1]


def hits_model(q, r, radius):
    """-> (hit [nq] bool, near [nq] bool): whether some j has d(q_i, r_j) <= radius_j, and whether a row has NO clear hit
    (d < radius_j (1 - 1e-5)) but some pair within the band |d - radius_j| <= 1e-5 radius_j - the rows whose decision a
    rounding may turn."""
    d = sqdist64(q, r).sqrt()
    rad = radius.to(F64)[None, :]
    hit = (d <= rad).any(1)
    clear = (d < rad * (1 - 1e-5)).any(1)
    band = ((d - rad).abs() <= 1e-5 * rad).any(1)
    return hit, band & ~clear


def ipr_model(real, fake, k=3):
    """The reference's ``_compute_ipr_from_features`` (evaluation_pipeline.py:744-791) in float64."""
    n, m = real.shape[0], fake.shape[0]
    if n < k + 1 or m < k + 1:
        return -1.0, -1.0
    in_real, _ = hits_model(fake, real, knn_radius_model(real, k))
    in_fake, _ = hits_model(real, fake, knn_radius_model(fake, k))
    return float(in_real.to(F64).mean()), float(in_fake.to(F64).mean())


def ipr_reference_formula(real, fake, k=3):
    """The same through torch.cdist / topk as the reference writes it, in the dtype of the inputs."""
    n, m = real.shape[0], fake.shape[0]
    if n < k + 1 or m < k + 1:
        return -1.0, -1.0
    real_r = torch.cdist(real, real, p=2).topk(k + 1, largest=False).values[:, -1]
    fake_r = torch.cdist(fake, fake, p=2).topk(k + 1, largest=False).values[:, -1]
    cross = torch.cdist(fake, real, p=2)
    return (float((cross <= real_r.unsqueeze(0)).any(dim=1).float().mean().item()),
            float((cross.T <= fake_r.unsqueeze(0)).any(dim=1).float().mean().item()))


# ------------------------------------------------------------------------------------------------ feature preparation
def prepare_model(x, y=None, normalize=False):
    """Float64 model of ``dadd_feat_prepare_f32`` on fp32 inputs -> (xc, yc or None, sqx, sqy or None, center)."""
    def norm(t):
        t = t.to(F64)
        return t / t.norm(dim=1, keepdim=True) if normalize else t
    xn = norm(x)
    c = xn.mean(0)
    xc = xn - c
    if y is None:
        return xc, None, (xc ** 2).sum(1), None, c
    yc = norm(y) - c
    return xc, yc, (xc ** 2).sum(1), (yc ** 2).sum(1), c


# ------------------------------------------------------------------------------------------------ CLIP preprocessing
PREPROCESS_SHAPES = ((512, 512), (256, 256), (224, 224), (300, 260), (128, 128))     # (H, W), all to S = 224


def _cubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def resize_coeffs(in_size, out_size):
    """Index-level model of the antialiased bicubic coefficient table: per output pixel (first tap, float64 weights that
    sum to 1).  scale = in / out; the support 2 is widened by the scale on downscale only; taps are the integers of
    [centre - support + 0.5, centre + support + 0.5) truncated and clipped to the image."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support, rows = 2.0 * fs, []
    for o in range(out_size):
        centre = (o + 0.5) * scale
        lo = max(int(centre - support + 0.5), 0)
        hi = min(int(centre + support + 0.5), in_size)
        w = [_cubic((t - centre + 0.5) / fs) for t in range(lo, hi)]
        total = sum(w)
        rows.append((lo, torch.tensor([v / total for v in w], dtype=F64)))
    return rows


def resized_shape(h, w, s):
    """{"shortest_edge": s}: the short edge becomes s, the long one int(s * long / short)."""
    return (s, int(s * w / h)) if h <= w else (int(s * h / w), s)


def max_abs_row_sum(h, w, s):
    oh, ow = resized_shape(h, w, s)
    return max(float(r[1].abs().sum()) for r in resize_coeffs(h, oh) + resize_coeffs(w, ow))


def clip_preprocess_model(frames_u8, s=224, mean=CLIP_MEAN, std=CLIP_STD):
    """u8 NHWC [B, H, W, 3] -> float64 NCHW [B, 3, s, s]: separable resize with ``resize_coeffs`` (no rounding between the
    passes), centre crop, / 255, (v - mean) / std."""
    b, h, w, _ = frames_u8.shape
    oh, ow = resized_shape(h, w, s)
    top, left = (oh - s) // 2, (ow - s) // 2

    def matrix(in_size, out_size, first, count):
        mat = torch.zeros(count, in_size, dtype=F64)
        rows = resize_coeffs(in_size, out_size)
        for o in range(count):
            lo, wts = rows[first + o]
            mat[o, lo:lo + len(wts)] = wts
        return mat
    my, mx = matrix(h, oh, top, s), matrix(w, ow, left, s)
    x = frames_u8.to(F64).permute(0, 3, 1, 2)                    # [B, 3, H, W]
    x = torch.einsum("oh,bchw->bcow", my, torch.einsum("pw,bchw->bchp", mx, x))
    mean_t, std_t = torch.tensor(mean, dtype=F64).view(1, 3, 1, 1), torch.tensor(std, dtype=F64).view(1, 3, 1, 1)
    return (x / 255.0 - mean_t) / std_t


def test_frames(b, h, w, seed=0):
    """u8 NHWC frames with structure at every scale: a smooth field plus pixel noise."""
    g = torch.Generator().manual_seed(1000 * h + w + seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=F64), torch.arange(w, dtype=F64), indexing="ij")
    out = torch.empty(b, h, w, 3, dtype=torch.uint8)
    for i in range(b):
        for c in range(3):
            f = 0.5 + 0.3 * torch.sin(xx * (0.05 + 0.02 * c) + i) * torch.cos(yy * (0.04 + 0.01 * i) + c) \
                + 0.2 * (torch.rand(h, w, generator=g, dtype=F64) - 0.5)
            out[i, :, :, c] = (f.clamp(0, 1) * 255).to(torch.uint8)
    return out


test_frames.__test__ = False     # a helper, not a test
