"""Evaluation on the device: CMMD and improved precision / recall (evaluation_pipeline.py:602-701, :744-791).

The reference copies every frame to the host, runs it through PIL and ``CLIPImageProcessor`` into a second copy of CLIP,
and builds three N x N fp32 matrices per metric.  Here frames stay on the GPU: ``dadd_clip_preprocess_u8`` does what the
processor does, ``conditioning.ImageEncoder`` (the module's own CLIP tower) gives ``image_embeds``, and the pair kernels
of ``csrc/metrics.hip`` reduce 64 x 64 Gram tiles without storing them (include/dadd_hip_metrics.h).

Names, defaults and return conventions of ``_mmd_rbf``, ``_compute_ipr_from_features`` and ``compute_cmmd`` are the
reference's: Python floats, -1.0 and (-1.0, -1.0) for sets that are too small.  FID is not built: it needs an Inception
network and its weights, which the project does not have.  A command line and report files are not part of this module.
"""
from __future__ import annotations

import logging
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import lib as L
from .backend import on_backend

log = logging.getLogger(__name__)

# CLIPImageProcessor's normalisation for the OpenAI towers
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
DEFAULT_SIGMAS = (0.1, 1.0, 10.0, 100.0)

_backends: Dict[torch.device, object] = {}


def _default_backend(t: Tensor):
    """The backend the feature-level functions run on when none is given: one ``HipBackend`` per device, made on first use
    (a missing library or device raises there: there is no CPU path)."""
    from .backend import HipBackend
    dev = t.device if t.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
    if dev not in _backends:
        _backends[dev] = HipBackend(dev)
    return _backends[dev]


def _kpad(d: int) -> int:
    return -(-d // L.METRICS_KPAD) * L.METRICS_KPAD


class _Prepared:
    """Two feature sets prepared by one ``feat_prepare`` call: centred on the column mean of ``x`` and zero-padded."""

    def __init__(self, be, x: Tensor, y: Tensor, normalize: bool, sigmas: int = 0):
        if x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1]:
            raise ValueError(f"feature sets must be [N, D] and [M, D], got {tuple(x.shape)} and {tuple(y.shape)}")
        self.be, self.d = be, x.shape[1]
        (n, d), m, f32 = x.shape, y.shape[0], torch.float32
        x, y = be.to_device(x.detach(), f32), be.to_device(y.detach(), f32)
        ldc = _kpad(d)
        self.xc, self.yc = be.empty((n, ldc), f32), be.empty((m, ldc), f32)
        self.sqx, self.sqy, self.center = be.empty((n,), f32), be.empty((m,), f32), be.empty((ldc,), f32)
        self.scratch = be.empty((max(be.metrics_scratch_bytes(n, m), be.metrics_scratch_bytes(n, m, sigmas)),), torch.uint8)
        be.feat_prepare(x, y, self.xc, self.yc, self.sqx, self.sqy, self.center, self.scratch, normalize=normalize)


def _frames_u8(be, frames: Tensor) -> Tensor:
    """One batch of frames as contiguous u8 NHWC on the device.  Float NCHW frames in [0, 1] are converted as the reference
    converts them for PIL, ``mul(255).to(uint8)`` - a truncation, not the rounding ``frames_to_u8`` applies for files."""
    if frames.dtype == torch.uint8:
        if frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError(f"u8 frames must be NHWC [N, H, W, 3], got {tuple(frames.shape)}")
        return be.to_device(frames)
    if frames.dim() != 4 or frames.shape[1] != 3 or not frames.dtype.is_floating_point:
        raise ValueError(f"frames must be float NCHW [N, 3, H, W] in [0, 1] or u8 NHWC, got {tuple(frames.shape)} {frames.dtype}")
    dev = be.to_device(frames.detach().float())
    with be.ctx():
        return dev.permute(0, 2, 3, 1).mul(255).to(torch.uint8).contiguous()


@torch.no_grad()
def clip_features(module_or_encoder, frames: Tensor, batch_size: int = 64) -> Tensor:
    """Raw CLIP ``image_embeds`` [N, projection_dim] (fp32, on the device) of ``frames``: fp32 NCHW in [0, 1] or u8 NHWC, on
    the device or the host.  ``module_or_encoder``: a ``DiffusionModuleWithIP`` (its ``image_encoder`` is used) or a
    ``conditioning.ImageEncoder``.  The features are NOT normalised (``_extract_clip_features`` divides by the norm;
    ``compute_cmmd`` does that inside the preparation kernel)."""
    enc = getattr(module_or_encoder, "image_encoder", module_or_encoder)
    be = enc.be
    side = int(round((enc.tok_rows.shape[0] - 1) ** 0.5)) * enc.patch      # the tower's input edge, from its position embeddings
    n = frames.shape[0]
    with on_backend(be):
        out = be.empty((n, enc.projection_dim), torch.float32)
        for i in range(0, n, batch_size):
            u8 = _frames_u8(be, frames[i:i + batch_size])
            px = be.empty((u8.shape[0], 3, side, side), torch.float32)
            be.clip_preprocess(u8, px, CLIP_MEAN, CLIP_STD)
            be.copy_(out[i:i + batch_size], enc(px))
    return out


def _mmd_rbf(x: Tensor, y: Tensor, sigmas: Optional[Sequence[float]] = None, normalize: bool = False, be=None) -> float:
    """MMD^2 with a sum of RBF kernels, unbiased estimator (evaluation_pipeline.py:630-666); -1.0 when either set has fewer
    than two rows.  ``normalize``: rows are scaled to unit length first.  At most ``lib.METRICS_MAX_SIGMAS`` bandwidths."""
    sigmas = list(DEFAULT_SIGMAS if sigmas is None else sigmas)
    if x.shape[0] < 2 or y.shape[0] < 2:
        return -1.0
    be = be or _default_backend(x)
    with on_backend(be):
        p = _Prepared(be, x, y, normalize, len(sigmas))
        out = be.empty((3 * len(sigmas) + 1,), torch.float64)
        be.rbf_mmd(p.xc, p.sqx, p.yc, p.sqy, p.d, sigmas, out, p.scratch)
    return float(out[-1].item())


def _compute_ipr_from_features(real_feats: Tensor, fake_feats: Tensor, k: int = 3, be=None) -> Tuple[float, float]:
    """Improved precision and recall (Kynkaanniemi et al. 2019; evaluation_pipeline.py:744-791) of two feature sets;
    (-1.0, -1.0) when either has fewer than k + 1 rows.  k <= ``lib.METRICS_MAX_K``."""
    n, m = real_feats.shape[0], fake_feats.shape[0]
    if n < k + 1 or m < k + 1:
        return -1.0, -1.0
    be = be or _default_backend(real_feats)
    with on_backend(be):
        p = _Prepared(be, real_feats, fake_feats, False)
        r_real, r_fake = be.empty((n,), torch.float32), be.empty((m,), torch.float32)
        in_real, in_fake = be.empty((m,), torch.int32), be.empty((n,), torch.int32)
        be.knn_radius(p.xc, p.sqx, p.d, k, r_real)
        be.knn_radius(p.yc, p.sqy, p.d, k, r_fake)
        be.manifold_hits(p.yc, p.sqy, p.xc, p.sqx, r_real, p.d, in_real)      # generated samples inside the real manifold
        be.manifold_hits(p.xc, p.sqx, p.yc, p.sqy, r_fake, p.d, in_fake)      # real samples inside the generated manifold
    return float(in_real.sum().item()) / m, float(in_fake.sum().item()) / n


def compute_cmmd(real: Tensor, fake: Tensor, module) -> float:
    """CMMD between real and generated frames: CLIP features of the module's own tower, normalised, RBF-kernel MMD^2."""
    enc = getattr(module, "image_encoder", module)
    return _mmd_rbf(clip_features(enc, real), clip_features(enc, fake), normalize=True, be=enc.be)


def _as_features(enc, v: Tensor) -> Tensor:
    return v if v.dim() == 2 else clip_features(enc, v)


def evaluate_sets(module, real_by_class: Dict[int, Tensor], fake_by_class: Dict[int, Tensor], k: int = 3,
                  features: Optional[Dict[int, Tuple[Tensor, Tensor]]] = None) -> Dict[object, Dict[str, float]]:
    """``{class: {"cmmd", "precision", "recall", "n_real", "n_fake"}, ..., "overall": {...}}`` for the classes both dicts
    hold; "overall" pools all of them.  A value is a set of frames (4-D, as ``clip_features`` takes them) or a 2-D matrix
    of CLIP features computed earlier.  CMMD always uses the CLIP features.  Precision and recall are computed on
    ``features[class] = (real, fake)`` when given, else on the CLIP features: the reference uses VGG16 fc7 features there,
    and that extractor (torchvision weights) is the caller's - this library has no VGG."""
    enc = getattr(module, "image_encoder", module)
    classes = sorted(c for c in real_by_class if c in fake_by_class and len(real_by_class[c]) and len(fake_by_class[c]))
    clip = {c: (_as_features(enc, real_by_class[c]), _as_features(enc, fake_by_class[c])) for c in classes}
    ipr = features if features is not None else clip

    def one(cf, pf):
        precision, recall = _compute_ipr_from_features(pf[0], pf[1], k=k, be=enc.be)
        return {"cmmd": _mmd_rbf(cf[0], cf[1], normalize=True, be=enc.be), "precision": precision, "recall": recall,
                "n_real": int(cf[0].shape[0]), "n_fake": int(cf[1].shape[0])}

    out: Dict[object, Dict[str, float]] = {c: one(clip[c], ipr[c]) for c in classes}
    if classes:
        def pool(src):
            dev = enc.be.device
            return tuple(torch.cat([src[c][i].to(dev) for c in classes], dim=0) for i in (0, 1))
        out["overall"] = one(pool(clip), pool(ipr))
    return out


def cmmd_preview(real_by_class: Dict[int, Tensor], jobs, cfg, **generation_kw) -> Callable:
    """A callable ``(trainer, epoch)`` for ``Trainer.fit(preview=)``: samples ``jobs`` with ``generation.generate_all`` on
    the trainer's module (which ``fit`` has just synced with the averaged weights), scores the frames against
    ``real_by_class`` with ``evaluate_sets``, logs the dict, appends it (with ``"epoch"``) to the callable's ``results``
    and returns it.  The CLIP features of the real sets are computed once, at the first call."""
    from . import generation
    real_feats: Dict[int, Tensor] = {}
    k = generation_kw.pop("k", 3)

    def preview(trainer, epoch):
        module = trainer.module
        for c, v in real_by_class.items():
            if c not in real_feats and len(v):
                real_feats[c] = _as_features(module.image_encoder, v)
        fake = generation.generate_all(module, jobs, cfg, module.device, **generation_kw)
        res = evaluate_sets(module, real_feats, fake, k=k)
        res["epoch"] = epoch
        log.info("epoch %d: %s", epoch, res)
        preview.results.append(res)
        return res

    preview.results = []
    return preview
