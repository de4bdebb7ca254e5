"""-m gpu: the evaluation-metric kernels (csrc/metrics.hip) through ``HipBackend`` and ``evaluation``, against the float64
models of tests/metrics_reference.py.  Every kernel call follows the project's habit: outputs and scratch are NaN-filled
beforehand, sentinels before and behind every output stay intact, and a repeated call and two replays of a graph captured
on the backend's stream are bit-equal (``run_checked``).

The accuracy criterion of ``rbf_mmd``: per case and input seed pair, |kernel - float64| must not exceed the largest
|ref32 - float64| of that case's three seed pairs, ref32 being the reference's own arithmetic in fp32 on the CPU.

Measured on an MI355X: rbf_mmd largest error 8.5e-10 .. 9.2e-9 against ref32's 1.5e-7 .. 4.2e-7 on the shapes
with more than two rows (26x .. 280x), 7.0e-8 against 2.1e-7 at n = m = 2; means of u within 1 % of their tolerance;
feat_prepare 0.64 / 1.2 x 2^-24 (bound 8); knn_radius 5.6e-8 .. 1.0e-7 against torch's 2.5e-7 .. 1.0e-6 (6.9e-4 with twin
rows); manifold_hits equal to float64 on every row, no row excused; clip_preprocess 3.0e-7 .. 9.1e-7 (bound 1e-5);
clip_features against processor + transformers 9.2e-4 (bound 1e-2)."""
import functools

import pytest
import torch

from progressive_stable_diffusion_amd import evaluation as EV
from progressive_stable_diffusion_amd import lib as L
from progressive_stable_diffusion_amd.backend import on_backend
from tests import metrics_reference as R

pytestmark = pytest.mark.gpu

F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8
DEV = torch.device("cuda:0")
EPS = 2.0 ** -24
TINY_CLIP = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1,
                 image_size=224, patch_size=14, projection_dim=32)


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(DEV)


class Guarded:
    """An output (or scratch) tensor with 64 sentinel elements before and behind it, NaN-filled (all bits set for
    integers) before every launch."""
    PAD = 64

    def __init__(self, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        self.full = torch.empty(n + 2 * self.PAD, dtype=dtype, device=DEV)
        self.t = self.full[self.PAD:self.PAD + n].view(shape)
        self.sentinel = 1234.5 if dtype.is_floating_point else 0x5A
        self.reset()

    def reset(self):
        self.full.fill_(self.sentinel)
        self.t.fill_(float("nan") if self.t.dtype.is_floating_point else (255 if self.t.dtype == U8 else -1))

    def bits(self):
        g = torch.cat([self.full[:self.PAD], self.full[-self.PAD:]]).cpu()
        assert bool((g == self.sentinel).all()), "a sentinel next to an output was overwritten"
        t = self.t.cpu()
        return t.view({F32: I32, F64: torch.int64}.get(t.dtype, t.dtype)).clone()


def run_checked(hip, launch, outs, scratch=()):
    """``launch()`` on NaN-filled outputs and scratch: once, once more (bit-equal), and two replays of its captured graph
    (bit-equal to the eager result); sentinels checked every time."""
    def once(fn):
        for o in tuple(outs) + tuple(scratch):
            o.reset()
        with on_backend(hip):
            fn()
        return [o.bits() for o in outs]
    first = once(launch)
    again = once(launch)
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "a repeated call differs"
    torch.cuda.synchronize()
    hip.graph_begin()
    launch()
    g = hip.graph_end()
    try:
        for _ in range(2):
            replay = once(lambda: hip.graph_launch(g))
            assert all(torch.equal(a, b) for a, b in zip(first, replay)), "a graph replay differs"
    finally:
        hip.graph_destroy(g)
    for o in scratch:
        o.bits()
    return [o.t for o in outs]


def kpad(d):
    return -(-d // L.METRICS_KPAD) * L.METRICS_KPAD


class Prepared:
    """Guarded outputs of one ``feat_prepare`` call on device copies of ``x`` / ``y`` (fp32)."""

    def __init__(self, hip, x, y=None, normalize=False, sigmas=0, checked=False, x_dev=None):
        self.x, self.y = (x.to(DEV) if x_dev is None else x_dev), (None if y is None else y.to(DEV))
        (n, d), m = x.shape, (0 if y is None else y.shape[0])
        self.n, self.m, self.d, ldc = n, m, d, kpad(d)
        self.xc, self.sqx, self.center = Guarded((n, ldc), F32), Guarded((n,), F32), Guarded((ldc,), F32)
        self.yc, self.sqy = (Guarded((m, ldc), F32), Guarded((m,), F32)) if m else (None, None)
        self.scratch = Guarded((max(hip.metrics_scratch_bytes(n, m), hip.metrics_scratch_bytes(n, m, sigmas) if m else 0),), U8)
        outs = [o for o in (self.xc, self.sqx, self.center, self.yc, self.sqy) if o is not None]

        def launch():
            hip.feat_prepare(self.x, self.y, self.xc.t, self.yc.t if m else None, self.sqx.t, self.sqy.t if m else None,
                             self.center.t, self.scratch.t, normalize=normalize)
        if checked:
            run_checked(hip, launch, outs, [self.scratch])
        else:
            with on_backend(hip):
                launch()
            for o in outs:
                o.bits()


def inputs32(case, seeds=(1, 2)):
    n, m, d, shift = case
    x, y = R.recipe(n, m, d, shift, seeds)
    return x.to(F32), y.to(F32)


# ------------------------------------------------------------------------------------------------ clip_preprocess
@functools.lru_cache(maxsize=None)
def preprocess_case(hw):
    frames = R.test_frames(3, *hw)
    return frames, R.clip_preprocess_model(frames)


@pytest.mark.parametrize("b", (1, 3))
@pytest.mark.parametrize("hw", R.PREPROCESS_SHAPES, ids=str)
def test_clip_preprocess_matches_the_table_model(hip, hw, b):
    """<= 1e-5 absolute in normalised units: about 100 fp32 taps of values <= 255."""
    frames, model = preprocess_case(hw)
    dev = frames[:b].to(DEV)
    out = Guarded((b, 3, 224, 224), F32)
    got, = run_checked(hip, lambda: hip.clip_preprocess(dev, out.t, R.CLIP_MEAN, R.CLIP_STD), [out])
    err = float((got.cpu().to(F64) - model[:b]).abs().max())
    print(f"clip_preprocess {hw} B={b}: max |kernel - float64 model| = {err:.3e}")
    assert err <= 1e-5


def test_clip_preprocess_other_edge_and_contract(hip):
    """A landscape frame (crop along x), an output edge that is no multiple of the 16-pixel tile, and the contract."""
    frames = R.test_frames(2, 90, 141)
    dev = frames.to(DEV)
    for s in (224, 50):
        out = Guarded((2, 3, s, s), F32)
        got, = run_checked(hip, lambda: hip.clip_preprocess(dev, out.t, R.CLIP_MEAN, R.CLIP_STD), [out])
        assert float((got.cpu().to(F64) - R.clip_preprocess_model(frames, s)).abs().max()) <= 1e-5
    with pytest.raises(ValueError):
        hip.clip_preprocess(torch.zeros(1, 400, 400, 3, dtype=U8, device=DEV), torch.empty(1, 3, 50, 50, device=DEV), R.CLIP_MEAN, R.CLIP_STD)


# ------------------------------------------------------------------------------------------------ feat_prepare
@pytest.mark.parametrize("normalize", (False, True))
@pytest.mark.parametrize("case", ((70, 45, 768, 0.5), (33, 17, 40, 0.3), (130, 129, 100, 0.3), (2, 2, 8, 0.3), (300, 0, 1000, 0.0)), ids=str)
def test_feat_prepare(hip, case, normalize):
    """Centred copies within 8 * 2^-24 of the norm of the (normalised) input row, squared norms within 8 * 2^-24 of its
    square; pad columns exactly zero; pairwise distances of the centred copies equal to those of the inputs to 1e-6."""
    n, m, d, shift = case
    x, y = inputs32((n, max(m, 1), d, shift))
    if normalize:
        x, y = x * 3.0, y * 0.5                                 # rows far from unit length: normalisation must act
    x_dev = None
    if m == 0:
        wide = torch.randn(n, d + 24, generator=torch.Generator().manual_seed(2)).to(F32)     # a strided input, no Y
        wide[:, :d] = x
        x, y, x_dev = wide[:, :d], None, wide.to(DEV)[:, :d]
    p = Prepared(hip, x, y, normalize, checked=True, x_dev=x_dev)
    xc64, yc64, sqx64, sqy64, c64 = R.prepare_model(x, y, normalize)
    for got, sq, want, want_sq, src in ((p.xc, p.sqx, xc64, sqx64, x), (p.yc, p.sqy, yc64, sqy64, y)):
        if src is None:
            continue
        row = torch.ones(src.shape[0], dtype=F64) if normalize else src.to(F64).norm(dim=1)
        g = got.t.cpu().to(F64)
        assert bool((g[:, d:] == 0).all())
        e_copy = ((g[:, :d] - want).abs().amax(1) / row).max()
        e_sq = ((sq.t.cpu().to(F64) - want_sq).abs() / row ** 2).max()
        print(f"feat_prepare {case} normalize={normalize}: copy {float(e_copy) / EPS:.2f}, sq {float(e_sq) / EPS:.2f} (x 2^-24, bound 8)")
        assert e_copy <= 8 * EPS and e_sq <= 8 * EPS
    c = p.center.t.cpu().to(F64)
    assert bool((c[d:] == 0).all()) and float((c[:d] - c64).abs().max()) <= 8 * EPS * float(c64.abs().max() + 1e-30)
    if m:
        xin, yin = (t.to(F64) / (t.to(F64).norm(dim=1, keepdim=True) if normalize else 1.0) for t in (x, y))
        got_d = R.sqdist64(p.xc.t.cpu()[:, :d], p.yc.t.cpu()[:, :d]).sqrt()
        assert float((got_d - R.sqdist64(xin, yin).sqrt()).abs().max()) <= 1e-6


# ------------------------------------------------------------------------------------------------ rbf_mmd
def mmd_on_device(hip, x, y, sigmas, checked=False, normalize=False):
    p = Prepared(hip, x, y, normalize, sigmas=len(sigmas))
    out = Guarded((3 * len(sigmas) + 1,), F64)

    def launch():
        hip.rbf_mmd(p.xc.t, p.sqx.t, p.yc.t, p.sqy.t, p.d, sigmas, out.t, p.scratch.t)
    if checked:
        run_checked(hip, launch, [out], [p.scratch])
    else:
        with on_backend(hip):
            launch()
        out.bits()
    res = out.t.cpu()
    return res[:-1].view(3, len(sigmas)), float(res[-1])


def assert_means(means, want, what):
    err = (means - want).abs()
    tol = 64 * EPS * want.abs() + 2.0 ** -40
    print(f"{what}: means of u, worst error / tolerance {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all()), (what, err / tol)


MMD_CASES = [(c, R.DEFAULT_SIGMAS) for c in R.RECIPE_CASES + R.EDGE_CASES] + \
    [(c, s) for c in (R.RECIPE_CASES[1], R.EDGE_CASES[1]) for s in ((1.0,), R.SIGMAS_8)]


@pytest.mark.parametrize("case,sigmas", MMD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_rbf_mmd_is_never_worse_than_the_reference_in_fp32(hip, case, sigmas):
    errs, refs = [], []
    for sp in R.SEED_PAIRS:
        x, y = inputs32(case, sp)
        want_means, want = R.mmd_model(x, y, sigmas)
        means, got = mmd_on_device(hip, x, y, sigmas, checked=(sp == R.SEED_PAIRS[0]))
        errs.append(abs(got - want))
        refs.append(abs(R.ref32(x, y, sigmas) - want))
        assert_means(means, want_means, f"rbf_mmd {case} S={len(sigmas)} seeds {sp}")
        assert abs(got - float(-(means[0] + means[1] - 2 * means[2]).sum())) <= 1e-14
    print(f"rbf_mmd {case} S={len(sigmas)}: |kernel - f64| {['%.2e' % e for e in errs]}, |ref32 - f64| {['%.2e' % e for e in refs]}, "
          f"ratio max ref32 / max kernel {max(refs) / max(max(errs), 1e-300):.1f}")
    assert max(errs) <= max(refs)


def test_rbf_mmd_xx_consistency_and_duplicate_rows(hip):
    """X against itself: the XY sum (whose diagonal has u = 0) equals the XX sum.  Duplicate rows: d2 clamps at 0, u = 0,
    nothing is NaN."""
    x, y = inputs32(R.RECIPE_CASES[0])
    n = x.shape[0]
    means, mmd2 = mmd_on_device(hip, x, x.clone(), R.DEFAULT_SIGMAS)
    xx, xy = means[0] * n * (n - 1), means[2] * n * n
    assert bool(((xx - xy).abs() <= 64 * EPS * xx.abs() + 2.0 ** -40).all()) and torch.equal(means[0], means[1])
    x[1], x[6], x[7] = x[0], x[5], x[5]
    y[3] = y[2]
    means, mmd2 = mmd_on_device(hip, x, y, R.DEFAULT_SIGMAS, checked=True)
    want_means, want = R.mmd_model(x, y)
    assert bool(torch.isfinite(means).all()) and mmd2 == mmd2
    assert_means(means, want_means, "rbf_mmd with duplicate rows")
    with pytest.raises(ValueError):
        mmd_on_device(hip, x[:1], y, R.DEFAULT_SIGMAS)


# ------------------------------------------------------------------------------------------------ knn_radius
KNN_D = {33: 40, 70: 768, 300: 768}


@pytest.mark.parametrize("k", (1, 3, 7))
@pytest.mark.parametrize("n", ("k+1", 33, 70, 300, "twins"))
def test_knn_radius_against_torch_fp32(hip, n, k):
    """Max abs error against the float64 radii no larger than that of torch's fp32 cdist + topk on the same inputs."""
    twins = n == "twins"
    n = k + 1 if n == "k+1" else 33 if twins else n
    x = R.recipe_set(n, KNN_D.get(n, 100), seed=7).to(F32) * 2.0
    if twins:
        x[4] = x[3]
    p = Prepared(hip, x)
    rad = Guarded((n,), F32)
    got, = run_checked(hip, lambda: hip.knn_radius(p.xc.t, p.sqx.t, p.d, k, rad.t), [rad])
    want = R.knn_radius_model(x, k)
    e_kernel = float((got.cpu().to(F64) - want).abs().max())
    e_torch = float((torch.cdist(x, x, p=2).topk(k + 1, largest=False).values[:, -1].to(F64) - want).abs().max())
    print(f"knn_radius n={n} k={k} twins={twins}: |kernel - f64| {e_kernel:.2e}, |torch fp32 - f64| {e_torch:.2e}")
    assert e_kernel <= e_torch
    if twins and k == 1:
        assert float(got[3]) == 0.0 and float(got[4]) == 0.0
    if n == k + 1:
        with pytest.raises(ValueError):
            hip.knn_radius(p.xc.t[:k], p.sqx.t[:k], p.d, k, rad.t[:k])


# ------------------------------------------------------------------------------------------------ manifold_hits
@pytest.mark.parametrize("case", R.RECIPE_CASES + (R.FAR_CASE,), ids=str)
def test_manifold_hits_and_precision_recall(hip, case):
    """The float64 decision for every row, except rows with no clear hit and some pair within 1e-5 of the radius; at most
    max(1, 2 %) of the rows may be excused, asserted from the float64 distances.  Then precision / recall as counts."""
    x, y = inputs32(case)
    n, m = x.shape[0], y.shape[0]
    p = Prepared(hip, x, y)
    total_excused = {}
    for name, q, qc, sqq, r, rc, sqr in (("precision", y, p.yc, p.sqy, x, p.xc, p.sqx), ("recall", x, p.xc, p.sqx, y, p.yc, p.sqy)):
        radius = R.knn_radius_model(r, 3).to(F32)
        want, near = R.hits_model(q, r, radius)
        assert int(near.sum()) <= max(1, q.shape[0] // 50), "the case itself has too many ties"
        hit = Guarded((q.shape[0],), I32)
        rdev = radius.to(DEV)
        got, = run_checked(hip, lambda: hip.manifold_hits(qc.t, sqq.t, rc.t, sqr.t, rdev, p.d, hit.t), [hit])
        got = got.cpu()
        assert bool(((got == 0) | (got == 1)).all())
        wrong = (got.bool() != want) & ~near
        print(f"manifold_hits {case} {name}: {int(got.sum())} of {q.shape[0]} hit, {int(near.sum())} rows excused")
        assert not bool(wrong.any()), wrong.nonzero().flatten().tolist()
        total_excused[name] = int(near.sum())
    precision, recall = EV._compute_ipr_from_features(x, y, k=3, be=hip)
    want_p, want_r = R.ipr_model(x, y, 3)
    assert abs(round(precision * m) - round(want_p * m)) <= total_excused["precision"]
    assert abs(round(recall * n) - round(want_r * n)) <= total_excused["recall"]
    if case == R.FAR_CASE:
        assert 0.2 < precision < 0.8


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def tower(hip):
    from progressive_stable_diffusion_amd import conditioning as PC
    from progressive_stable_diffusion_amd import weights as W
    sd = W.init_state_dict(W.clip_shapes(dict(TINY_CLIP)), 5)
    g = torch.Generator().manual_seed(11)
    real = torch.rand(6, 3, 64, 64, generator=g)
    fake = (torch.rand(5, 3, 64, 64, generator=g) * 0.8 + 0.1 * torch.rand(5, 3, 1, 1, generator=g)).clamp(0, 1)
    return sd, PC.ImageEncoder(sd, DEV, be=hip), real, fake


def test_clip_features_match_transformers_fed_by_the_processor(hip, tower):
    """Frames -> device preprocessing -> HIP tower against CLIPImageProcessor -> ``CLIPVisionModelWithProjection`` in fp32 on
    the CPU with the same seeded weights, at the tolerance of ``test_clip_tower_matches_transformers`` (1e-2 of the largest
    value)."""
    transformers = pytest.importorskip("transformers")
    image = pytest.importorskip("PIL.Image")
    sd, enc, real, fake = tower
    hf = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(**TINY_CLIP)).eval()
    pref = "image_encoder.image_encoder."
    hf.load_state_dict({k[len(pref):]: v for k, v in sd.items()}, strict=False)
    proc = transformers.CLIPImageProcessor(
        do_resize=True, size={"shortest_edge": 224}, resample=3, do_center_crop=True, crop_size={"height": 224, "width": 224},
        do_rescale=True, rescale_factor=1 / 255, do_normalize=True, image_mean=list(R.CLIP_MEAN), image_std=list(R.CLIP_STD))
    frames = torch.cat([real, fake])
    pil = [image.fromarray(f.permute(1, 2, 0).mul(255).to(U8).numpy()) for f in frames]
    with torch.no_grad():
        want = hf(pixel_values=proc(images=pil, return_tensors="pt", do_rescale=True).pixel_values).image_embeds
    got = EV.clip_features(enc, frames.to(DEV), batch_size=4)
    assert got.shape == (11, 32) and got.dtype == F32 and got.device.type == "cuda"
    err = float((got.cpu() - want).abs().max() / want.abs().max())
    print(f"clip_features vs processor + transformers: rel {err:.3e}")
    assert err < 1e-2
    assert torch.equal(got, EV.clip_features(enc, frames.permute(0, 2, 3, 1).mul(255).to(U8), batch_size=4))     # u8 NHWC from the host


def test_compute_cmmd_and_evaluate_sets(hip, tower):
    """``compute_cmmd`` against the float64 MMD of the device's own (normalised) features under the ``rbf_mmd`` criterion,
    over three pairings of the 6 + 5 frames; the keys of ``evaluate_sets`` and its (-1, -1) for a class of 3 at k = 3."""
    sd, enc, real, fake = tower
    errs, refs = [], []
    for a, b in ((real, fake), (real[:5], fake[:4]), (real[1:], fake[1:])):
        fa, fb = (EV.clip_features(enc, t).cpu().to(F64) for t in (a, b))
        fa, fb = fa / fa.norm(dim=1, keepdim=True), fb / fb.norm(dim=1, keepdim=True)
        want = R.mmd_model(fa, fb)[1]
        errs.append(abs(EV.compute_cmmd(a, b, enc) - want))
        refs.append(abs(R.ref32(fa, fb) - want))
    print(f"compute_cmmd: |device - f64| {['%.2e' % e for e in errs]}, |ref32 - f64| {['%.2e' % e for e in refs]}")
    assert max(errs) <= max(refs)
    res = EV.evaluate_sets(enc, {0: real, 1: real[:3], 2: real}, {0: fake, 1: fake[:4]}, k=3)
    assert set(res) == {0, 1, "overall"}
    assert all(set(v) == {"cmmd", "precision", "recall", "n_real", "n_fake"} for v in res.values())
    assert (res[1]["precision"], res[1]["recall"]) == (-1.0, -1.0) and res[1]["cmmd"] != -1.0
    assert res[0]["cmmd"] == EV.compute_cmmd(real, fake, enc)
    fa, fb = (EV.clip_features(enc, t).cpu() for t in (real, fake))
    assert (res[0]["precision"], res[0]["recall"]) == pytest.approx(R.ipr_model(fa, fb, 3), abs=1e-12)
    assert (res["overall"]["n_real"], res["overall"]["n_fake"]) == (9, 9)


def test_cmmd_preview_on_a_module(hip, tmp_path):
    """The callable ``cmmd_preview`` returns, called directly on a module (building a ``Trainer`` and running an epoch takes
    far longer than a few seconds; ``Trainer.fit`` only calls ``preview(trainer, epoch)`` after ``sync_module``): one source
    image, three targets, one DDIM step at 8 x 8 latents."""
    np = pytest.importorskip("numpy")
    image = pytest.importorskip("PIL.Image")
    from progressive_stable_diffusion_amd import generation as G
    from progressive_stable_diffusion_amd.config import default_config
    from progressive_stable_diffusion_amd.diffusion_module_ip import DiffusionModuleWithIP
    (tmp_path / "0").mkdir()
    image.fromarray((np.random.RandomState(0).rand(40, 48, 3) * 255).astype("uint8")).save(tmp_path / "0" / "a.bmp")
    jobs = G._collect_jobs([tmp_path])
    assert len(jobs) == 3
    cfg = default_config(**{"dataset.image_size": 64})
    mod = DiffusionModuleWithIP(cfg, device=DEV, seed=0, batch_size=3, clip_config=TINY_CLIP, warm_start_dis=False, backend=hip)
    g = torch.Generator().manual_seed(4)
    real = {c: torch.rand(2, 3, 64, 64, generator=g) for c in (1, 2, 3)}

    class Holder:
        module = mod

    cb = EV.cmmd_preview(real, jobs, cfg, batch_images=1, sampling_steps=1, seed=3)
    res = cb(Holder(), 4)
    assert res["epoch"] == 4 and cb.results == [res] and set(res) == {1, 2, 3, "overall", "epoch"}
    assert res[1]["cmmd"] == -1.0 and res[1]["n_fake"] == 1                     # one generated frame per class: no estimator
    assert res["overall"]["n_real"] == 6 and res["overall"]["n_fake"] == 3 and res["overall"]["cmmd"] > -1.0
    assert (res["overall"]["precision"], res["overall"]["recall"]) == (-1.0, -1.0)      # 3 generated frames at k = 3
