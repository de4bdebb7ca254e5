"""-m gpu: every launch of the benchmarked plans against a float64 restatement of the same op (tests/launch_audit.py).

``UNetPlan(4, 64)`` followed by the VAE decode is what bench.py times; ``engine.plan_tiling`` picks its kernels from tables
keyed on M = B*H*W of exactly that step, so at any smaller batch or map the launches under test do not exist (census:
tests/test_launch_audit_cpu.py).  Each launch is recomputed from the tensors the kernel read - nothing accumulates - and
held to the elementwise bound of its op and to rms(o - r) <= 1.5 rms(r32 - r).  The per-signature table is printed; a
failure names the launch index, op, signature, worst element and both ratios.
"""
import gc
import time

import pytest
import torch

from tests import golden_inputs as GI
from tests import launch_audit as LA

pytestmark = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(DEV)


@pytest.fixture(scope="module")
def unet_sd():
    from progressive_stable_diffusion_amd import weights as W
    return W.init_state_dict(dict(W.unet_shapes()), 0, gates=GI.GATES, warm_start_dis=False)


@pytest.fixture(autouse=True)
def _free_plans():
    """A plan and its backend refer to each other: only the cycle collector frees its buffers.  Collect after each test."""
    yield
    gc.collect()


def _finish(title, be, plan, expected, t0, fp=None):
    wall = time.perf_counter() - t0
    print(LA.report(title, be, wall))
    print(f"{title}: {wall:.1f} s")
    be.assert_clean()
    assert be.launches == expected, (be.launches, expected)
    if fp is not None:
        assert LA.fingerprint(plan) == LA.FINGERPRINTS[fp], LA.fingerprint(plan)


def test_audit_benchmark_plan(hip, unet_sd):
    """UNetPlan(4, 64), fp16, default policy, lambda = 3: 157 igemm (76 chosen by the tiling tables), 5 tf_head, 5
    attn2_fused, 5 ffn_block, 16 self_attn, 11 _xattn."""
    t0 = time.perf_counter()
    be, plan, expected = LA.audit_unet(hip, unet_sd, 4, 64, 3.0, device=DEV)
    _finish("UNetPlan(4, 64) fp16", be, plan, expected, t0, "bench")


def test_audit_benchmark_plan_unfused(hip, unet_sd, monkeypatch):
    """The A/B path ``bench.py --set`` reaches: the row-block fusions off.  Selects the remaining 3 tiling-table keys."""
    from progressive_stable_diffusion_amd import engine as E
    for sw in ("FUSED_FFN", "FUSED_HEAD", "FUSED_ATTN2"):
        monkeypatch.setattr(E, sw, False)
    t0 = time.perf_counter()
    be, plan, expected = LA.audit_unet(hip, unet_sd, 4, 64, 3.0, device=DEV)
    _finish("UNetPlan(4, 64) fp16, FUSED_FFN / HEAD / ATTN2 off", be, plan, expected, t0, "bench_unfused")


def test_audit_benchmark_plan_bf16(hip, unet_sd):
    t0 = time.perf_counter()
    be, plan, expected = LA.audit_unet(hip, unet_sd, 4, 64, 3.0, dtype=BF16, device=DEV)
    _finish("UNetPlan(4, 64) bf16", be, plan, expected, t0, "bench_bf16")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_audit_ragged_plan(hip, unet_sd, dtype):
    """UNetPlan(2, 24), lambda = 0: ragged 576 / 144 / 36 / 9-key attention, rule-chosen tiles, the delta pathway skipped."""
    t0 = time.perf_counter()
    be, plan, expected = LA.audit_unet(hip, unet_sd, 2, 24, 0.0, dtype=dtype, device=DEV)
    _finish(f"UNetPlan(2, 24) {dtype}", be, plan, expected, t0, "s24")


def test_audit_vae_decoder(hip):
    """VaeDecoderPlan(4, 64): the decode behind the benchmark's sampler, 512x512 maps."""
    from progressive_stable_diffusion_amd import weights as W
    sd = W.init_state_dict(W.vae_shapes(encoder=False), 0)
    t0 = time.perf_counter()
    be, plan, expected = LA.audit_vae_decoder(hip, sd, 4, 64, device=DEV)
    _finish("VaeDecoderPlan(4, 64)", be, plan, expected, t0)


@pytest.mark.parametrize("image,batch", [(128, 2), (256, 1)])
def test_audit_vae_encoder(hip, image, batch):
    """VaeEncoderPlan at the geometry of test_gpu_parity.py::test_vae_encode_matches_oracle, and the sample behind it."""
    from progressive_stable_diffusion_amd import weights as W
    sd = W.init_state_dict(W.vae_shapes(decoder=False), 0)
    t0 = time.perf_counter()
    be, plan, expected = LA.audit_vae_encoder(hip, sd, batch, image // 8, device=DEV)
    _finish(f"VaeEncoderPlan({batch}, {image // 8})", be, plan, expected, t0)
