"""-m gpu: the differentiable UNet (``unet_grad``) and a complete training step (``training.Trainer``) on the HIP kernels.

UNet gradients: the full UNet, seeded weights, B = 2, 32x32 latents, 48 conditioning tokens, split mode, fp16, loss scale
2^12.  Reference: float64 autograd of ``oracle.sd_unet.unet_forward`` on the device with the weight matrices rounded to
fp16 (as in the block tests).  Per tensor (every UNet parameter, dx of the latents, d cond) the relative L2 error must
stay within max(4e-3, 2 * e16): 4e-3 is the project's block bound, e16 the error of torch's own fp16 run (autocast) of the
same oracle function, inputs and loss scale against the same reference, the factor 2 what the attention tests give a
kernel whose rounding points differ from the model's.  The oracle's sinusoid is fp32 by construction; the test casts its
OUTPUT to the run's type and changes nothing else.

Measured on MI355X: eps within 1.9e-3 of the fp32 oracle (bound 1.4e-2); worst relative L2 per class 1.8e-3 .. 3.8e-3
against e16 of 3.2e-3 .. 6.9e-3, i.e. 0.25 .. 0.35 of the bound max(4e-3, 2 * e16).  Most of the test's
twelve seconds are torch's float64 convolutions of the reference.

Training step: tiny CLIP config, 256x256 image (32x32 latents), B = 2, one sample dropped, every draw injected; the
bounds are those of the existing forward test (2e-2 * max(1, |ref|))."""
import pytest
import torch

from oracle import sampler as OS
from oracle import sd_unet as OU
from oracle import training as OT
from progressive_stable_diffusion_amd import training as TR
from progressive_stable_diffusion_amd import unet_grad as UG
from progressive_stable_diffusion_amd import weights as W
from tests import golden_inputs as GI
from tests.test_train_cpu import _helper

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
DEV = torch.device("cuda:0")
BLOCK_BOUND = 4e-3
SCALE = 4096.0
TINY_CLIP = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, image_size=224,
                 patch_size=14, projection_dim=32)


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(DEV)


@pytest.fixture(scope="module")
def unet_sd():
    return W.init_state_dict(W.unet_shapes(), 0, gates=GI.GATES, warm_start_dis=False)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _oracle_grads(sd, x, t, cond, g, dtype, monkeypatch):
    """Gradients of SCALE * sum(eps * g) by torch autograd of the oracle on the device, divided by SCALE, in float64."""
    orig = OU.timestep_embedding
    monkeypatch.setattr(OU, "timestep_embedding", lambda tt, dim=320: orig(tt, dim).to(dtype))
    leaves = {k: v.to(DEV).to(dtype).requires_grad_(v.dim() > 0) for k, v in sd.items()}
    xl, cl = x.to(DEV).to(dtype).requires_grad_(True), cond.to(DEV).to(dtype).requires_grad_(True)
    with torch.device(DEV), torch.autocast("cuda", dtype=F16, enabled=dtype == F16):
        eps = OU.unet_forward(leaves, xl, t.to(DEV), cl)
    (SCALE * (eps.to(dtype) * g.to(DEV).to(dtype)).sum()).backward()
    monkeypatch.setattr(OU, "timestep_embedding", orig)
    out = {k: v.grad.double() / SCALE for k, v in leaves.items() if v.requires_grad}
    return eps.detach().double(), out, xl.grad.double() / SCALE, cl.grad.double() / SCALE


def _class_of(k):
    if k.endswith(".bias") or ".norm" in k or "conv_norm_out" in k:
        return "norm affine" if ("norm" in k) else "bias"
    for tag, name in ((".attn1.", "attn1 weights"), (".attn2.", "attn2 weights"), (".ff.", "ff weights"), ("time_emb", "time path"),
                      (".conv_shortcut.", "1x1 weights"), (".proj_", "1x1 weights"), ("samplers.", "resampling convs"),
                      ("conv_in", "end convs"), ("conv_out", "end convs")):
        if tag in k:
            return name
    return "3x3 convs"


def test_unet_forward_and_every_gradient_against_float64_autograd(hip, unet_sd, monkeypatch):
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(2, 4, 32, 32, generator=gen)
    t = torch.tensor([650, 40])
    cond = torch.randn(2, 48, 768, generator=gen) * 0.5
    g = torch.randn(2, 4, 32, 32, generator=gen) / SCALE
    sd16 = {k: (v.half().float() if v.dim() >= 2 else v) for k, v in unet_sd.items()}     # matrices rounded to fp16

    eps64, ref, dx64, dc64 = _oracle_grads(sd16, x, t, cond.half().float(), g, F64, monkeypatch)
    _, g16, dx16, dc16 = _oracle_grads(sd16, x, t, cond.half().float(), g, F16, monkeypatch)

    masters = {k: v.to(DEV).requires_grad_(v.dim() > 0) for k, v in UG.masters_from_state_dict(sd16).items()}
    xd, cd = x.to(DEV).requires_grad_(True), cond.half().float().to(DEV).requires_grad_(True)
    eps = UG.unet_forward(hip, masters, xd, t.to(DEV), cd)
    (SCALE * (eps * g.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    with torch.no_grad(), torch.device(DEV):                       # the fp32 oracle, full-precision weights, on the device
        eps_ref = OU.unet_forward({k: v.to(DEV) for k, v in unet_sd.items()}, x.to(DEV), t.to(DEV), cond.half().float().to(DEV))
    tol = 1e-2 * max(1.0, eps_ref.abs().max().item())
    err = (eps.detach() - eps_ref).abs().max().item()
    print(f"unet_grad forward: max|eps - fp32 oracle| = {err:.3e} (bound {tol:.3e}); vs float64 on fp16 weights "
          f"{(eps.detach().double() - eps64).abs().max().item():.3e}")

    got = UG.state_dict_from_masters({k: (v.grad if v.requires_grad else v).detach() / (SCALE if v.requires_grad else 1.0)
                                      for k, v in masters.items()})
    rows, worst = [], {}
    for k, r in ref.items():
        e, e16 = _rel(got[k], r), _rel(g16[k], r)
        rows.append((k, e, e16, max(BLOCK_BOUND, 2 * e16)))
    rows.append(("dx (latents)", _rel(xd.grad / SCALE, dx64), _rel(dx16, dx64), max(BLOCK_BOUND, 2 * _rel(dx16, dx64))))
    rows.append(("d cond", _rel(cd.grad / SCALE, dc64), _rel(dc16, dc64), max(BLOCK_BOUND, 2 * _rel(dc16, dc64))))
    for k, e, e16, bound in rows:
        cls = k if k.startswith("d") and " " in k else _class_of(k)
        w = worst.get(cls)
        if w is None or e / bound > w[1] / w[3]:
            worst[cls] = (k, e, e16, bound)
    for cls, (k, e, e16, bound) in sorted(worst.items()):
        print(f"unet_grad {cls}: worst ratio {e / bound:.3f}: {k} rel L2 {e:.3e}, e16 {e16:.3e}, bound {bound:.3e}")
    assert len(ref) == sum(1 for v in unet_sd.values() if v.dim() > 0)
    assert err <= tol, (err, tol)
    bad = [(k, e, bound) for k, e, e16, bound in rows if not e <= bound]
    assert not bad, (len(bad), bad[:8])
    gates = [k for k, v in masters.items() if not v.requires_grad]
    assert len(gates) == 32 and all(masters[k].grad is None for k in gates)


# ---- the training step ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trainer_setup(unet_sd):
    from progressive_stable_diffusion_amd.config import default_config
    from progressive_stable_diffusion_amd.diffusion_module_ip import DiffusionModuleWithIP
    shapes = dict(W.vae_shapes())
    shapes.update(W.conditioning_shapes(clip_hidden=TINY_CLIP["hidden_size"], clip_proj=TINY_CLIP["projection_dim"]))
    shapes.update(W.clip_shapes(TINY_CLIP))
    sd = dict(unet_sd)
    sd.update(W.init_state_dict(shapes, 0, warm_start_dis=False))
    # weight decay 0: a master that moves has received a gradient
    cfg = default_config(**{"dataset.image_size": 256, "optimizer": {"weight_decay": 0.0, "betas": [0.9, 0.999]}})
    mod = DiffusionModuleWithIP(cfg, state_dict=sd, device=DEV, seed=0, batch_size=2, clip_config=TINY_CLIP)
    g = torch.Generator().manual_seed(31)
    batch = (torch.rand(2, 3, 256, 256, generator=g) * 2 - 1, torch.tensor([1.0, 3.0]), torch.randn(2, 3, 224, 224, generator=g))
    draws = dict(t=torch.tensor([700, 35]), noise=torch.randn(2, 4, 32, 32, generator=g),
                 latent_noise=torch.randn(2, 4, 32, 32, generator=g), drop_mask=torch.tensor([False, True]))
    return cfg, sd, mod, batch, draws


def test_trainer_loss_step_and_export(trainer_setup):
    from progressive_stable_diffusion_amd.diffusion_module_ip import DiffusionModuleWithIP
    cfg, sd, mod, batch, draws = trainer_setup
    dbatch = tuple(v.to(DEV) for v in batch)
    tr = TR.Trainer(mod, 1e-4, init_scale=SCALE)
    arena = tr.arena
    assert [g["name"] for g in tr.groups] == ["unet", "ordinal_embedder", "image_projection", "feature_purifier"]
    assert not any(k.endswith(("anat_gate", "dis_gate")) for k in arena.names) and len(tr.gates) == 32

    loss = tr.loss(dbatch, is_training=False, **draws)
    with torch.no_grad():
        feats = mod.image_encoder.get_hidden_states(dbatch[2]).cpu()
        ocfg = OS.OracleCfg(image_size=256, use_routing_gates=True)
        ref, _ = OT.training_loss(sd, ocfg, batch[0], batch[1], feats, draws["t"], draws["noise"], draws["latent_noise"],
                                  draws["drop_mask"])
    print(f"trainer loss {loss.item():.6f} vs oracle {ref.item():.6f}")
    assert loss.requires_grad and loss.grad_fn is not None
    assert abs(loss.item() - ref.item()) < 2e-2 * max(1.0, abs(ref.item())), (loss.item(), ref.item())
    del loss

    before, gates_before = arena.p.clone(), {k: v.clone() for k, v in tr.gates.items()}
    l1 = tr.step(dbatch, is_training=False, **draws)
    st = tr.optimizer.stats()
    assert st["step"] == 1 and not st["found_inf"] and st["scale"] == SCALE, st
    unused = ("ordinal_embedder.norm.weight", "ordinal_embedder.norm.bias")
    still = [k for k in arena.names if k not in unused and torch.equal(arena.param(k), before[arena.offsets[k]:arena.offsets[k]
                                                                     + arena.shapes[k].numel()].view(arena.shapes[k]))]
    # the null embedding is read by the unconditional path only: no gradient
    assert still == ["ordinal_embedder.null_embedding"], still[:8]
    assert all(torch.equal(tr.gates[k], v) for k, v in gates_before.items())
    assert not bool(arena.g.any())                                       # zeroed by the step
    assert torch.equal(arena.p16, arena.p.half())
    for name, (kind, taps) in tr.relayout.kinds.items():
        assert torch.equal(tr.relayout.wt(name), _helper(kind, taps, arena.param16(name))), name

    l2 = tr.step(dbatch, is_training=False, **draws)
    print(f"trainer: loss of step 1 {l1.item():.6f}, of step 2 {l2.item():.6f}")
    assert torch.isfinite(l1) and torch.isfinite(l2)

    nxt = tr.loss(dbatch, is_training=False, **draws).item()
    exported = tr.export_state_dict()
    assert set(exported) == set(sd) and all(exported[k].shape == sd[k].shape and exported[k].dtype == F32 for k in sd)
    assert set(tr.export_state_dict(ema=True)) == set(sd)
    mod2 = DiffusionModuleWithIP(cfg, state_dict=exported, device=DEV, seed=0, batch_size=2, clip_config=TINY_CLIP)
    with torch.no_grad():
        again = mod2.training_step(dbatch, 0, is_training=False, **draws).item()
    print(f"trainer: next loss {nxt:.6f}, the exported module's training_step {again:.6f}")
    assert abs(again - nxt) < 2e-2 * max(1.0, abs(nxt)), (again, nxt)
