"""Not-GPU: the stream hand-off of the entry points.  Every kernel runs on the backend's own stream, so an entry point
owes ``be.wait_current()`` before its first backend call and ``be.release_to_current()`` after its last, also when the
body raises: ``backend.on_backend``.  A counting subclass of the TEST-ONLY torch backend records waits, releases and op
calls in order; each site is run once as it is and once with one of its ops made to raise."""
import pytest
import torch

from progressive_stable_diffusion_amd import grad_ops
from progressive_stable_diffusion_amd import weights as W
from progressive_stable_diffusion_amd.backend import on_backend
from progressive_stable_diffusion_amd.config import default_config
from progressive_stable_diffusion_amd.diffusion_module_ip import DiffusionModuleWithIP
from tests.torch_backend import TorchRefBackend

TINY_CLIP = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1,
                 image_size=224, patch_size=14, projection_dim=32)
SIDE = 16               # latent side: the smallest of tests/plan_cases.py
# what the backend offers besides ops: the two hand-off calls themselves and host-side helpers that touch no stream
NOT_OPS = ("wait_current", "release_to_current", "synchronize", "ctx", "c", "conv2d")


class Boom(RuntimeError):
    pass


class CountingBackend(TorchRefBackend):
    """Records ``"wait"``, ``"release"`` and the name of every op (launches, ``empty``, ``copy_``, ``clone``, ...) in call
    order; ``fail_on`` names an op that raises ``Boom`` instead of running."""

    def __init__(self):
        super().__init__()
        self.log, self.fail_on = [], None

    def wait_current(self):
        self.log.append("wait")

    def release_to_current(self):
        self.log.append("release")

    def __getattribute__(self, name):
        attr = object.__getattribute__(self, name)
        if name.startswith("_") or name in NOT_OPS or not callable(attr):
            return attr
        log, fail_on = object.__getattribute__(self, "log"), object.__getattribute__(self, "fail_on")

        def op(*a, **k):
            log.append(name)
            if name == fail_on:
                raise Boom(name)
            return attr(*a, **k)
        return op


def check_log(log):
    """Waits equal releases, and every op lies between a wait and its release."""
    ops, depth = 0, 0
    for i, entry in enumerate(log):
        if entry == "wait":
            depth += 1
        elif entry == "release":
            depth -= 1
            assert depth >= 0, f"entry {i}: a release without a wait"
        else:
            ops += 1
            assert depth > 0, f"entry {i}: {entry} outside the bracket"
    assert depth == 0 and log.count("wait") == log.count("release") > 0, (log.count("wait"), log.count("release"))
    return ops


def check_site(be, call, fail_on):
    be.log.clear()
    call()
    assert check_log(be.log) > 0 and fail_on in be.log
    be.log.clear()
    be.fail_on = fail_on
    try:
        with pytest.raises(Boom):
            call()
    finally:
        be.fail_on = None
    assert be.log[-2:] == [fail_on, "release"]        # nothing ran after the failing op but the release
    check_log(be.log)


def test_on_backend_itself():
    assert grad_ops.on_backend is on_backend
    be = CountingBackend()
    with on_backend(be):
        be.empty((2,), torch.float32)
    assert be.log == ["wait", "empty", "release"]
    check_site(be, lambda: _bracketed_empty(be), "empty")


def _bracketed_empty(be):
    with on_backend(be):
        return be.empty((2,), torch.float32)


@pytest.fixture(scope="module")
def mod():
    shapes = dict(W.unet_shapes())
    shapes.update(W.vae_shapes(encoder=False))
    shapes.update(W.conditioning_shapes(clip_hidden=TINY_CLIP["hidden_size"], clip_proj=TINY_CLIP["projection_dim"]))
    shapes.update(W.clip_shapes(TINY_CLIP))
    cfg = default_config(**{"dataset.image_size": 8 * SIDE})
    return DiffusionModuleWithIP(cfg, state_dict=W.init_state_dict(shapes, 0), device="cpu", batch_size=1,
                                 clip_config=TINY_CLIP, backend=CountingBackend())


@pytest.fixture(scope="module")
def inputs(mod):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 4, SIDE, SIDE, generator=g)
    cond = torch.randn(1, mod._unets[(1, SIDE)]._plan.T, 768, generator=g)
    return x, torch.tensor([7]), cond


def test_module_call(mod, inputs):
    x, t, cond = inputs
    with torch.no_grad():
        check_site(mod.be, lambda: mod(x, t, cond), "clone")


def test_inner_unet_call_takes_the_same_path(mod, inputs):
    """``module.unet.unet(...)``: both hand-offs, and a Python scalar timestep as diffusers accepts it."""
    x, t, cond = inputs
    with torch.no_grad():
        check_site(mod.be, lambda: mod.unet.unet(x, 7, encoder_hidden_states=cond).sample, "clone")
        assert torch.equal(mod.unet.unet(x, 7, encoder_hidden_states=cond).sample, mod.unet(x, t, cond))
        assert torch.equal(mod.unet.unet(x, 7.0, encoder_hidden_states=cond).sample, mod(x, t[0], cond))


def test_vae_decode(mod, inputs):
    check_site(mod.be, lambda: mod.vae.decode(inputs[0]).sample, "clone")


def test_conditioning_module(mod):
    labels = torch.tensor([2.0])
    check_site(mod.be, lambda: mod.ordinal_embedder(labels), "aoe_interp")


def test_ddim_loop_sample(mod, inputs):
    x, t, cond = inputs
    loop = mod.ddim_loop(1, SIDE)
    steps = torch.linspace(mod.diff_cfg.num_train_timesteps - 1, 0, steps=2, dtype=torch.long)
    with torch.no_grad():
        mod(x, t, cond)                                 # the conditioning of the plan; sample() reuses it
        check_site(mod.be, lambda: loop.sample(x, steps, mod.alphas_cumprod, 0.0, use_graph=False), "begin_step")
