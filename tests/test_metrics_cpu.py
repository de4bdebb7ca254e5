"""CPU checks of the evaluation metrics: the float64 models of tests/metrics_reference.py against the reference's formulas
and against ``CLIPImageProcessor``, the return conventions, the contracts the library checks before it launches, and the
wiring of ``evaluation`` on a CPU stand-in of the five backend calls."""
import contextlib
import ctypes

import pytest
import torch

from progressive_stable_diffusion_amd import evaluation as EV
from progressive_stable_diffusion_amd import lib as L
from tests import metrics_reference as R

F32, F64 = torch.float32, torch.float64
ALL_CASES = R.RECIPE_CASES + (R.FAR_CASE,)


# ------------------------------------------------------------------------------------------------ models vs the reference
@pytest.mark.parametrize("case", ALL_CASES + R.EDGE_CASES, ids=str)
def test_mmd_model_equals_reference_formula_in_float64(case):
    n, m, d, shift = case
    x, y = R.recipe(n, m, d, shift)
    for sigmas in (R.DEFAULT_SIGMAS, (1.0,), R.SIGMAS_8):
        means, mmd2 = R.mmd_model(x, y, sigmas)
        assert abs(mmd2 - R.mmd_reference_formula(x, y, sigmas)) <= 1e-12
        assert means.shape == (3, len(sigmas)) and bool((means >= 0).all()) and bool((means <= 1).all())


def test_recipe_gives_the_recorded_figures():
    got = [R.mmd_model(*R.recipe(*c))[1] for c in R.RECIPE_CASES]
    assert [round(v, 4) for v in got] == [-0.0041, -0.0043, 0.0019, 0.0031]
    for c in R.RECIPE_CASES:
        p, r = R.ipr_model(*R.recipe(*c))
        assert 0.88 <= p <= 1.0 and 0.88 <= r <= 1.0
    p, r = R.ipr_model(*R.recipe(*R.FAR_CASE))
    assert 0.2 < p < 0.8 and (round(p, 3), round(r, 3)) == (0.689, 0.129)


def test_ref32_is_the_yardstick_it_is_said_to_be():
    """The fp32 restatement of the reference loses 3e-8 .. 5e-7 absolute on the recipe: the figures the accuracy criterion
    of the GPU test rests on."""
    for c in R.RECIPE_CASES:
        errs = [abs(R.ref32(*R.recipe(*c, seeds=sp)) - R.mmd_model(*R.recipe(*c, seeds=sp))[1]) for sp in R.SEED_PAIRS]
        assert 1e-8 < max(errs) < 1e-6, errs


@pytest.mark.parametrize("case", ALL_CASES, ids=str)
@pytest.mark.parametrize("k", (1, 3, 7))
def test_ipr_model_equals_reference_formula_in_float64(case, k):
    x, y = R.recipe(*case)
    assert R.ipr_model(x, y, k) == pytest.approx(R.ipr_reference_formula(x, y, k), abs=1e-6)     # the reference averages in fp32


def test_return_conventions_for_small_sets():
    x, y = R.recipe(5, 5, 16, 0.1)
    assert EV._mmd_rbf(x[:1], y) == -1.0 and EV._mmd_rbf(x, y[:1]) == -1.0
    assert R.mmd_reference_formula(x[:1], y) == -1.0
    for k in (3, 4):
        assert EV._compute_ipr_from_features(x[:k], y, k=k) == (-1.0, -1.0)
        assert EV._compute_ipr_from_features(x, y[:k], k=k) == (-1.0, -1.0)
        assert R.ipr_model(x[:k], y, k) == (-1.0, -1.0)


# ------------------------------------------------------------------------------------------------ preprocessing model
@pytest.mark.parametrize("hw", R.PREPROCESS_SHAPES, ids=str)
def test_preprocess_model_against_clip_image_processor(hw):
    """The coefficient-table model, applied in float64, against the processor the reference's call resolves to (with
    transformers 5 and no torchvision that is the PIL one), called as ``_extract_clip_features`` calls it.  PIL rounds to
    8 bits after each pass: half a level each, and the second pass spreads the first rounding by at most the largest
    sum of |w| of a coefficient row; 0.01 for its fixed-point coefficients.  Measured: 0.99, 1.08, 1e-5, 1.08, 1.10 levels
    against bounds of 1.09, 1.14, 1.01, 1.14, 1.14."""
    transformers = pytest.importorskip("transformers")
    image = pytest.importorskip("PIL.Image")
    proc = transformers.CLIPImageProcessor(
        do_resize=True, size={"shortest_edge": 224}, resample=3, do_center_crop=True, crop_size={"height": 224, "width": 224},
        do_rescale=True, rescale_factor=1 / 255, do_normalize=True, image_mean=list(R.CLIP_MEAN), image_std=list(R.CLIP_STD),
        do_convert_rgb=True)
    h, w = hw
    frames = R.test_frames(2, h, w)
    pil = [image.fromarray(f.numpy()) for f in frames]
    got = proc(images=pil, return_tensors="pt", do_rescale=True).pixel_values.to(F64)
    model = R.clip_preprocess_model(frames)
    assert got.shape == model.shape == (2, 3, 224, 224)
    row_sum = R.max_abs_row_sum(h, w, 224)
    assert 1.0 <= row_sum < 1.3
    std = torch.tensor(R.CLIP_STD, dtype=F64).view(1, 3, 1, 1)
    bound = (0.5 * row_sum + 0.5 + 0.01) / 255 / std
    diff = (got - model).abs()
    print(f"{hw}: max |processor - model| = {float((diff * std * 255).max()):.4f} levels, bound {0.5 * row_sum + 0.51:.4f}")
    assert bool((diff <= bound).all())


def test_coefficient_rows():
    for n_in, n_out in ((512, 224), (256, 224), (224, 224), (300, 258), (260, 224), (128, 224)):
        rows = R.resize_coeffs(n_in, n_out)
        assert len(rows) == n_out
        for lo, wts in rows:
            assert 0 <= lo and lo + len(wts) <= n_in and len(wts) <= 32      # DADD_CLIP_MAX_TAPS
            assert abs(float(wts.sum()) - 1.0) < 1e-12
    assert all(len(w) == 1 or float(w.abs().max()) == 1.0 for _, w in R.resize_coeffs(224, 224))     # identity
    assert max(len(w) for _, w in R.resize_coeffs(128, 224)) <= 5                                     # upscale: support 2
    assert max(len(w) for _, w in R.resize_coeffs(512, 224)) >= 9                                     # widened by 16 / 7
    assert R.resized_shape(300, 260, 224) == (258, 224) and R.resized_shape(260, 300, 224) == (224, 258)


# ------------------------------------------------------------------------------------------------ the library, host side
def test_scratch_bytes_and_contracts_without_a_gpu():
    """``dadd_metrics_scratch_bytes`` is host only, and every contract is checked before anything is launched."""
    lib = L.load()
    assert set(L.METRICS_PROTOTYPES) <= set(L.ALL_PROTOTYPES) and L.HEADER_PROTOTYPES["dadd_hip_metrics.h"] is L.METRICS_PROTOTYPES
    sb = lib.dadd_metrics_scratch_bytes
    assert sb(0, 0, 0) == -1 and sb(4, -1, 0) == -1 and sb(4, 4, 9) == -1
    assert sb(70, 45, 0) == 512 and sb(70, 0, 4) == 512 and sb(70, 45, 4) == 512     # 115 (70) floats, in 256-byte steps
    assert sb(300, 257, 8) == 3584                       # 15 + 15 + 25 tiles, 8 doubles each = 3520 bytes
    tiles = 157 * 158 // 2 * 2 + 157 * 157
    assert sb(10000, 10000, 8) == -(-tiles * 64 // 256) * 256
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    sig = (L.f32 * 4)(*R.DEFAULT_SIGMAS)
    assert lib.dadd_rbf_mmd_f32(p, p, 1, p, p, 5, 8, 32, sig, 4, p, p, p, 1 << 20, None) == L.DADD_EINVAL
    assert b"two rows" in lib.dadd_last_error()
    assert lib.dadd_rbf_mmd_f32(p, p, 5, p, p, 5, 8, 32, sig, 9, p, p, p, 1 << 20, None) == L.DADD_EINVAL
    assert lib.dadd_rbf_mmd_f32(p, p, 5, p, p, 5, 40, 32, sig, 4, p, p, p, 1 << 20, None) == L.DADD_EINVAL     # ldc < kp
    assert lib.dadd_rbf_mmd_f32(p, p, 5, p, p, 5, 8, 32, sig, 4, p, p, p, 8, None) == L.DADD_EINVAL            # scratch
    assert lib.dadd_knn_radius_f32(p, p, 3, 8, 32, 3, p, None) == L.DADD_EINVAL                                  # n < k + 1
    assert lib.dadd_knn_radius_f32(p, p, 30, 8, 32, 8, p, None) == L.DADD_EINVAL                                 # k > 7
    assert lib.dadd_manifold_hits_f32(p, p, 0, p, p, p, 4, 8, 32, p, None) == L.DADD_EINVAL
    assert lib.dadd_feat_prepare_f32(p, 4, 8, None, 0, 0, 8, 0, p, None, 30, p, None, p, p, 1 << 20, None) == L.DADD_EINVAL
    m3, s3 = (L.f32 * 3)(*R.CLIP_MEAN), (L.f32 * 3)(*R.CLIP_STD)
    assert lib.dadd_clip_preprocess_u8(p, p, 1, 2048, 2048, 224, m3, s3, None) == L.DADD_EINVAL                  # shrinks > 7
    assert lib.dadd_clip_preprocess_u8(p, p, 0, 64, 64, 224, m3, s3, None) == L.DADD_EINVAL


# ------------------------------------------------------------------------------------------------ wiring on a stand-in
class StandInBackend:
    """The five metric calls of ``HipBackend`` from the float64 models, on the CPU; records the calls."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def ctx(self):
        return contextlib.nullcontext()

    def wait_current(self):
        self.calls.append("wait")

    def release_to_current(self):
        self.calls.append("release")

    def empty(self, shape, dtype):
        return torch.full(shape, float("nan"), dtype=dtype) if dtype.is_floating_point else torch.zeros(shape, dtype=dtype)

    def to_device(self, t, dtype=None):
        return t.to(dtype or t.dtype).contiguous()

    def copy_(self, dst, src):
        dst.copy_(src.reshape(dst.shape))

    def metrics_scratch_bytes(self, n, m=0, sigmas=0):
        return int(L.load().dadd_metrics_scratch_bytes(n, m, sigmas))

    def clip_preprocess(self, frames, out, mean, std):
        assert frames.dtype == torch.uint8 and frames.shape[-1] == 3 and out.shape[1] == 3
        self.calls.append("clip_preprocess")
        out.copy_(R.clip_preprocess_model(frames, out.shape[-1], mean, std))

    def feat_prepare(self, x, y, xc, yc, sqx, sqy, center, scratch, normalize=False):
        assert scratch.numel() >= self.metrics_scratch_bytes(x.shape[0], 0 if y is None else y.shape[0])
        self.calls.append(("feat_prepare", bool(normalize)))
        d = x.shape[1]
        a, b, sa, sb, c = R.prepare_model(x, y, normalize)
        for dst, src in ((xc, a), (yc, b)):
            if src is not None:
                dst.zero_()
                dst[:, :d] = src
        sqx.copy_(sa)
        if y is not None:
            sqy.copy_(sb)
        center.zero_()
        center[:d] = c

    def rbf_mmd(self, xc, sqx, yc, sqy, d, sigmas, out, scratch):
        assert scratch.numel() >= self.metrics_scratch_bytes(xc.shape[0], yc.shape[0], len(sigmas))
        self.calls.append(("rbf_mmd", tuple(sigmas)))
        means, mmd2 = R.mmd_model(xc[:, :d], yc[:, :d], sigmas)
        out[:-1] = means.reshape(-1)
        out[-1] = mmd2

    def knn_radius(self, xc, sqx, d, k, radius):
        self.calls.append(("knn_radius", k))
        radius.copy_(R.knn_radius_model(xc[:, :d], k))

    def manifold_hits(self, qc, sqq, rc, sqr, radius, d, hit):
        self.calls.append("manifold_hits")
        hit.copy_(R.hits_model(qc[:, :d], rc[:, :d], radius)[0].to(torch.int32))


class StandInEncoder:
    """An ``ImageEncoder`` as far as ``evaluation`` looks at one: a fixed random projection of the pixel values."""
    patch, projection_dim = 14, 24

    def __init__(self, be):
        self.be = be
        self.tok_rows = torch.zeros(1 + 16 * 16, 8)           # 224 / 14 = 16 patches per edge
        self.w = torch.randn(3 * 8 * 8, self.projection_dim, generator=torch.Generator().manual_seed(5))
        self.batches = []

    def __call__(self, px):
        assert px.dtype == F32 and tuple(px.shape[1:]) == (3, 224, 224)
        self.batches.append(px.shape[0])
        return torch.nn.functional.adaptive_avg_pool2d(px, 8).reshape(px.shape[0], -1) @ self.w + 3.0


def test_feature_functions_on_the_stand_in():
    be = StandInBackend()
    x, y = R.recipe(33, 17, 40, 0.3)
    x32, y32 = x.to(F32) * 3.0, y.to(F32) * 2.0          # not unit rows: normalize must matter
    got = EV._mmd_rbf(x32, y32, be=be)
    assert isinstance(got, float) and abs(got - R.mmd_model(x32, y32)[1]) < 1e-6
    got_n = EV._mmd_rbf(x32, y32, normalize=True, be=be)
    assert abs(got_n - R.mmd_model(x, y)[1]) < 1e-6 and abs(got_n - got) > 1e-4
    assert EV._mmd_rbf(x32, y32, sigmas=[0.5], be=be) == pytest.approx(R.mmd_model(x32, y32, (0.5,))[1], abs=1e-6)
    assert be.calls.count("wait") == be.calls.count("release") == 3
    assert ("feat_prepare", True) in be.calls and ("rbf_mmd", R.DEFAULT_SIGMAS) in be.calls and ("rbf_mmd", (0.5,)) in be.calls
    pr = EV._compute_ipr_from_features(x32, y32, k=3, be=be)
    assert pr == R.ipr_model(x32, y32, 3) and all(isinstance(v, float) for v in pr)
    assert be.calls.count(("knn_radius", 3)) == 2 and be.calls.count("manifold_hits") == 2
    assert ("feat_prepare", False) in be.calls            # the reference does not normalise the manifold features
    with pytest.raises(ValueError):
        EV._mmd_rbf(x32, y32[:, :8], be=be)


def test_clip_features_and_evaluate_sets_on_the_stand_in(monkeypatch):
    be = StandInBackend()
    enc = StandInEncoder(be)
    g = torch.Generator().manual_seed(3)
    real = {0: torch.rand(6, 3, 32, 32, generator=g), 1: torch.rand(3, 3, 32, 32, generator=g), 2: torch.rand(5, 3, 32, 32, generator=g)}
    fake = {0: torch.rand(5, 3, 32, 32, generator=g) * 0.7, 1: torch.rand(4, 3, 32, 32, generator=g), 3: torch.rand(4, 3, 32, 32, generator=g)}
    # float frames are truncated to 8 bits as the reference does, u8 NHWC frames are taken as they are: same features
    f_float = EV.clip_features(enc, real[0], batch_size=4)
    u8 = real[0].permute(0, 2, 3, 1).mul(255).to(torch.uint8)
    assert enc.batches == [4, 2] and f_float.shape == (6, 24) and f_float.dtype == F32
    assert torch.equal(f_float, EV.clip_features(enc, u8))
    assert torch.equal(f_float, EV.clip_features(enc, u8.permute(0, 3, 1, 2).float().add(0.6).div(255)))     # k + 0.6 -> k
    cm = EV.compute_cmmd(real[0], fake[0], enc)
    assert cm == pytest.approx(R.mmd_model(*(t / t.norm(dim=1, keepdim=True) for t in
                                             (f_float.to(F64), EV.clip_features(enc, fake[0]).to(F64))))[1], abs=1e-6)
    res = EV.evaluate_sets(enc, real, fake, k=3)
    assert set(res) == {0, 1, "overall"}                 # classes both dicts hold
    for v in res.values():
        assert set(v) == {"cmmd", "precision", "recall", "n_real", "n_fake"}
    assert res[0]["cmmd"] == pytest.approx(cm, abs=1e-9) and 0.0 <= res[0]["precision"] <= 1.0
    assert (res[1]["precision"], res[1]["recall"]) == (-1.0, -1.0) and res[1]["cmmd"] != -1.0     # 3 images at k = 3
    assert (res["overall"]["n_real"], res["overall"]["n_fake"]) == (9, 9)
    # precision / recall on features of the caller's
    mine = {c: (torch.randn(len(real[c]), 10, generator=g), torch.randn(len(fake[c]), 10, generator=g)) for c in (0, 1)}
    res2 = EV.evaluate_sets(enc, real, fake, k=2, features=mine)
    assert res2[0]["cmmd"] == res[0]["cmmd"]
    assert (res2[0]["precision"], res2[0]["recall"]) == R.ipr_model(*mine[0], 2)
    assert (res2[1]["precision"], res2[1]["recall"]) == R.ipr_model(*mine[1], 2)

    # cmmd_preview: generate_all on the trainer's module, real features computed once
    from progressive_stable_diffusion_amd import generation
    seen = []

    def fake_generate_all(module, jobs, cfg, device, **kw):
        seen.append((jobs, cfg, kw))
        return fake

    monkeypatch.setattr(generation, "generate_all", fake_generate_all)

    class Module:
        image_encoder, device = enc, torch.device("cpu")

    class Trainer:
        module = Module()

    cb = EV.cmmd_preview(real, ["job"], "cfg", sampling_steps=2)
    first = cb(Trainer(), 0)
    n_batches = len(enc.batches)
    second = cb(Trainer(), 1)
    assert len(enc.batches) - n_batches == 2              # only the two generated classes are encoded again
    assert first["epoch"] == 0 and second["epoch"] == 1 and cb.results == [first, second]
    assert first[0]["cmmd"] == pytest.approx(res[0]["cmmd"], abs=1e-9) and seen[0] == (["job"], "cfg", {"sampling_steps": 2})


def test_reference_path_alias():
    import src.pipelines.evaluation.evaluation_pipeline as alias
    assert alias._mmd_rbf is EV._mmd_rbf and alias._compute_ipr_from_features is EV._compute_ipr_from_features
    assert alias.compute_cmmd is EV.compute_cmmd and alias.evaluate_sets is EV.evaluate_sets
