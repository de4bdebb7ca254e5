"""Alias of progressive_stable_diffusion_amd.evaluation under the reference's path (the metrics half of
evaluation_pipeline.py; the generation half is progressive_stable_diffusion_amd.generation)."""
from progressive_stable_diffusion_amd.evaluation import *  # noqa: F401,F403
from progressive_stable_diffusion_amd.evaluation import (  # noqa: F401
    _compute_ipr_from_features, _mmd_rbf, clip_features, cmmd_preview, compute_cmmd, evaluate_sets)
from progressive_stable_diffusion_amd.generation import generate_all  # noqa: F401
