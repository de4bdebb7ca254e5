"""-m gpu: trained weights handed to LIVE inference plans - ``optim.PlanRefresh`` over the recipes of a full ``UNetPlan``,
``Trainer.sync_module``, a ``DdimLoop`` graph captured before the sync, plans built after it, and ``fit(preview=...)``.

``weights.unet_shapes()`` has one size, so plans and arenas are the full ones; what is small is the work: B = 1 or 2,
32x32 latents (8x8 for the sampler), two optimizer steps.  The module, its trainer and the two modules rebuilt from
``export_state_dict()`` are built once and shared.

Bounds.  Packed weights: bit-equal to a plan built from the same weights, c1 / bias of a folded LayerNorm within
2^-23 |ref| + (K + 2) 2^-52 sum|term| (tests/test_gpu_plan_refresh.py).  Epsilon and conditioning tokens: the module
parity tolerance of the suite, 2e-3 max|ref|.  Sampled latents: 5e-2, what ``smoke()`` allows."""
from collections import OrderedDict

import pytest
import torch

from progressive_stable_diffusion_amd import engine as E
from progressive_stable_diffusion_amd import inference_pipeline_ip as PIPE
from progressive_stable_diffusion_amd import optim as O
from progressive_stable_diffusion_amd import training as TR
from progressive_stable_diffusion_amd import unet_grad as UG
from progressive_stable_diffusion_amd import weights as W
from tests import golden_inputs as GI
from tests import plan_refresh_reference as REF

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DEV = torch.device("cuda:0")
SCALE, LR = 4096.0, 1e-3
TINY_CLIP = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, image_size=224,
                 patch_size=14, projection_dim=32)
ARRAYS = ("p", "m", "v", "ema", "p16")
_GATES = ("processor.anat_gate", "processor.dis_gate")


def _r(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(DEV)


def _eps(plan, lat, t, cond, lam=3.0):
    out = plan.forward(lat.to(DEV), t.to(DEV), cond.to(DEV), lam=lam)
    plan.be.synchronize()
    return out.float().cpu()


# ----------------------------------------------------------------------------------------------- plan parity
@pytest.fixture(scope="module")
def two_state_dicts():
    return tuple(W.init_state_dict(W.unet_shapes(), seed, gates=GI.GATES, warm_start_dis=False) for seed in (0, 1))


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16-fused", "bf16"])
def test_a_refreshed_plan_is_the_plan_built_from_the_same_weights(hip, two_state_dicts, dtype, monkeypatch):
    """Plan from state dict A, refreshed from an arena that holds B's masters, against a plan built from B: every recipe
    destination tensor by tensor, then epsilon on the same inputs.  tf_head, ffn_block and fused attn2 are on at this size
    for fp16 (thresholds lowered here only)."""
    monkeypatch.setattr(E, "A2_MIN_TILES", 1)
    monkeypatch.setattr(E, "FFN_MIN_BLOCKS", 1)
    sd_a, sd_b = two_state_dicts
    plan_a, plan_b = E.UNetPlan(hip, sd_a, 1, 32, dtype=dtype), E.UNetPlan(hip, sd_b, 1, 32, dtype=dtype)
    names = [getattr(fn, "__name__", "") for fn, _, _ in plan_a.ops]
    if dtype == F16:
        assert names.count("tf_head") == 5 and names.count("ffn_block") == 5 and names.count("attn2_fused") >= 5
    assert plan_a.unrefreshable == [] and len(plan_a.recipes) == len(plan_b.recipes) > 500
    masters = OrderedDict((k, v) for k, v in UG.masters_from_state_dict(sd_b).items() if not k.endswith(_GATES))
    arena = O.ParamArena(masters, {k: 0 for k in masters}, device=DEV)
    pr = O.PlanRefresh(hip, arena, plan_a.recipes)
    assert pr.n_launches == (1 if dtype == F16 else 2)
    x, t, cond = _r((1, 4, 32, 32), 3), torch.tensor([500]), _r((1, 48, 768), 4, 0.5)
    stale = _eps(plan_a, x, t, cond)
    pr.refresh("raw")
    plan_a._a2_dirty = True
    hip.synchronize()
    torch.cuda.synchronize()
    worst, n_cmp = 0.0, 0
    for ra, rb in zip(plan_a.recipes, plan_b.recipes):
        assert ra.kind == rb.kind and ra.src == rb.src
        bounds = REF.lnfold_bounds(rb, arena, rb.dst) if ra.kind == "lnfold" else None
        for i, (da, db) in enumerate(zip(ra.dst, rb.dst)):
            n_cmp += 1
            if bounds is not None and i > 0:
                share = ((da.double() - db.double()).abs() / bounds[i - 1]).max().item()
                worst = max(worst, share)
                assert share <= 1.0, (ra.kind, ra.src, i, share)
            else:
                assert torch.equal(da, db), (ra.kind, ra.src, i, tuple(da.shape))
    want = _eps(plan_b, x, t, cond)
    got = _eps(plan_a, x, t, cond)
    tol = 2e-3 * want.abs().max().item()
    err = (got - want).abs().max().item()
    print(f"plan parity {dtype}: {n_cmp} tensors, worst share of the c1 / bias bound {worst:.3g}; max|eps - eps_ref| = {err:.3e} "
          f"(tolerance {tol:.3e}, stale plan {(stale - want).abs().max().item():.3e})")
    assert (stale - want).abs().max().item() > tol          # the comparison can fail
    assert err <= tol


# ----------------------------------------------------------------------------------------------- trainer
def _batch(seed, labels, t, drop):
    g = torch.Generator().manual_seed(seed)
    batch = (torch.rand(2, 3, 256, 256, generator=g) * 2 - 1, torch.tensor(labels), torch.randn(2, 3, 224, 224, generator=g))
    draws = dict(t=torch.tensor(t), noise=torch.randn(2, 4, 32, 32, generator=g),
                 latent_noise=torch.randn(2, 4, 32, 32, generator=g), drop_mask=torch.tensor(drop))
    return batch, draws


def _sample(mod, lat):
    target, source = torch.tensor([3.0, 1.0], device=DEV), torch.tensor([0.0, 2.0], device=DEV)
    pix = _r((1, 3, 224, 224), 1).to(DEV)
    with torch.no_grad():
        z = PIPE._ddim_sample_ip(mod, target, source, pix, 3, DEV, steer_scale=3.0, latents=lat)
    torch.cuda.synchronize()
    return z.float().cpu()


def _cond(mod):
    labels, pix = torch.tensor([1.0, 2.5], device=DEV), _r((2, 3, 224, 224), 5).to(DEV)
    with torch.no_grad():
        parts = mod._prepare_conditioning(labels, pix, is_training=False)
    torch.cuda.synchronize()
    return [p.float().cpu() for p in parts[:2]]


@pytest.fixture(scope="module")
def world():
    from progressive_stable_diffusion_amd.config import default_config
    from progressive_stable_diffusion_amd.diffusion_module_ip import DiffusionModuleWithIP
    shapes = dict(W.unet_shapes())
    shapes.update(W.vae_shapes())
    shapes.update(W.conditioning_shapes(clip_hidden=TINY_CLIP["hidden_size"], clip_proj=TINY_CLIP["projection_dim"]))
    shapes.update(W.clip_shapes(TINY_CLIP))
    sd = W.init_state_dict(shapes, 0, gates=GI.GATES, warm_start_dis=False)
    cfg = default_config(**{"dataset.image_size": 256, "model.cfg_drop_prob": 0.5,
                            "optimizer": {"weight_decay": 0.01, "betas": [0.9, 0.999]},
                            "scheduler": {"warmup_epochs": 0, "min_lr": 0.0},
                            "training": {"precision": "16-mixed", "use_min_snr_weighting": True, "max_epochs": 10,
                                         "ema_decay": 0.5, "update_starting_at_step": 0, "update_every_n_steps": 1,
                                         "log_every_n_steps": 1}})

    def module(state_dict):
        return DiffusionModuleWithIP(cfg, state_dict=state_dict, device=DEV, seed=0, batch_size=2, clip_config=TINY_CLIP)
    mod = module(sd)
    tr = TR.Trainer(mod, LR, init_scale=SCALE)
    fresh = tr.state(device=DEV)
    lat8 = _r((2, 4, 8, 8), 2)
    z_before = _sample(mod, lat8)                       # captures the (2, 8) DdimLoop graph on the untrained weights
    loop = mod._loops[(2, 8)]
    graphs = dict(loop.graphs)
    a, da = _batch(31, [1.0, 3.0], [700, 35], [False, True])
    b, db = _batch(32, [0.0, 2.0], [410, 900], [False, False])
    A, B = (tuple(v.to(DEV) for v in a), da), (tuple(v.to(DEV) for v in b), db)
    for batch, draws in (A, B):
        tr.step(batch, is_training=False, **draws)
    st = tr.optimizer.stats()
    assert st["step"] == 2 and not st["found_inf"] and tr.ema_latest_step == 2
    x, t, cond = _r((2, 4, 32, 32), 3), torch.tensor([500, 20]), _r((2, 48, 768), 4, 0.5)
    x16, t16, cond16 = _r((1, 4, 16, 16), 6), torch.tensor([300]), _r((1, 48, 768), 7, 0.5)
    before = dict(eps=_eps(mod.unet._plan, x, t, cond), cond=_cond(mod))
    ref = {}
    for which in ("ema", "raw"):
        m = module(tr.export_state_dict(ema=which == "ema"))
        ref[which] = dict(eps=_eps(m.unet._plan, x, t, cond), cond=_cond(m))
        if which == "ema":
            ref[which]["z"] = _sample(m, lat8)
            ref[which]["eps16"] = _eps(m._unet_for(1, 16)._plan, x16, t16, cond16)
        del m
        torch.cuda.empty_cache()
    return dict(mod=mod, tr=tr, fresh=fresh, A=A, B=B, host=(a, b), inputs=(x, t, cond), inputs16=(x16, t16, cond16),
                before=before, ref=ref, lat8=lat8, z_before=z_before, loop=loop, graphs=graphs)


def _close(got, want):
    """(max|got - want|, 2e-3 max|want|)"""
    return (got - want).abs().max().item(), 2e-3 * want.abs().max().item()


@pytest.mark.parametrize("which", ["ema", "raw"])
def test_sync_module_gives_the_module_the_trained_weights(world, which):
    mod, tr, ref = world["mod"], world["tr"], world["ref"][which]
    e0, tol = _close(world["before"]["eps"], ref["eps"])
    assert e0 > tol, (e0, tol)                           # the untrained module is told apart: the test can fail
    c0 = [_close(g, w) for g, w in zip(world["before"]["cond"], ref["cond"])]
    assert any(e > t_ for e, t_ in c0), c0
    gens = [(p.cond_gen, p.weights_gen) for p in (u._plan for u in mod._unets.values())]
    ptrs = [t.data_ptr() for t in mod.unet._plan.keep]
    tr.sync_module(which)
    plans = [u._plan for u in mod._unets.values()]
    assert all(p._a2_dirty for p in plans) and mod._synced == which
    assert [(p.cond_gen, p.weights_gen) for p in plans] == [(c + 1, w + 1) for c, w in gens]
    assert [t.data_ptr() for t in mod.unet._plan.keep] == ptrs          # weight buffers keep their addresses
    err, tol = _close(_eps(mod.unet._plan, *world["inputs"]), ref["eps"])
    cerr = [_close(g, w) for g, w in zip(_cond(mod), ref["cond"])]
    print(f"sync_module({which!r}): max|eps - eps_ref| = {err:.3e} (tolerance {tol:.3e}, before the sync {e0:.3e}); "
          f"conditioning tokens {[f'{e:.2e}/{t_:.2e}' for e, t_ in cerr]} (before {[f'{e:.2e}' for e, _ in c0]})")
    assert err <= tol
    assert all(e <= t_ for e, t_ in cerr), cerr


def test_a_graph_captured_before_the_sync_samples_with_the_new_weights(world):
    mod, tr, ref = world["mod"], world["tr"], world["ref"]["ema"]
    tr.sync_module("ema")
    z = _sample(mod, world["lat8"])
    assert mod._loops[(2, 8)] is world["loop"] and dict(world["loop"].graphs) == world["graphs"]      # no re-capture
    err, moved = (z - ref["z"]).abs().max().item(), (world["z_before"] - ref["z"]).abs().max().item()
    print(f"captured DdimLoop after sync: max|z - z_ref| = {err:.3e} (untrained weights: {moved:.3e})")
    assert err < 5e-2


def test_a_plan_built_after_a_sync_carries_the_synced_weights(world):
    mod, tr, ref = world["mod"], world["tr"], world["ref"]["ema"]
    tr.sync_module("ema")
    mod._unets.pop((1, 16), None)
    plan = mod._unet_for(1, 16)._plan
    assert plan.weights_gen == 1
    err, tol = _close(_eps(plan, *world["inputs16"]), ref["eps16"])
    print(f"late plan (1, 16): max|eps - eps_ref| = {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol
    del mod._unets[(1, 16)]


def test_sync_module_refuses_pending_micro_batches_and_unknown_sources(world):
    tr = world["tr"]
    with pytest.raises(ValueError):
        tr.sync_module("p16")
    batch, draws = world["A"]
    tr.backward(batch, is_training=False, **draws)
    assert tr.pending == 1
    with pytest.raises(RuntimeError, match="1 micro-batch"):
        tr.sync_module("ema")
    tr.arena.g.zero_()
    tr.pending = 0


def test_fit_previews_after_a_sync_and_is_the_parents_loop_without_one(world):
    mod, x = world["mod"], world["tr"]
    y = TR.Trainer(mod, LR, init_scale=SCALE)
    batches = list(world["host"])

    def arrays(t):
        torch.cuda.synchronize()
        return {n: getattr(t.arena, n).clone() for n in ARRAYS}
    # the parent's loop, written out
    y.load_state(world["fresh"])
    torch.manual_seed(7)
    for e in range(y.next_epoch, 2):
        y.set_epoch(e)
        for batch in batches:
            y.step(tuple(v.to(DEV, non_blocking=True) for v in batch))
        y.flush()
        y.next_epoch = e + 1
    want = arrays(y)
    del y
    x.load_state(world["fresh"])
    torch.manual_seed(7)
    x.fit(batches, epochs=2)
    got = arrays(x)
    assert [n for n in ARRAYS if not torch.equal(got[n], want[n])] == []
    assert not torch.equal(want["p"], want["ema"]) and x.steps == 4
    # with a preview: called after every epoch, each time on freshly synced plans; training itself is untouched
    x.load_state(world["fresh"])
    torch.manual_seed(7)
    calls = []
    key = "unet.unet.time_embedding.linear_1.weight"

    def preview(trainer, epoch):
        assert trainer is x and trainer.pending == 0
        torch.cuda.synchronize()
        calls.append((epoch, torch.equal(mod.unet._plan.w_t1, trainer.arena.ema_param(key).half()), trainer.steps))
    x.fit(batches, epochs=2, preview=preview)
    assert calls == [(0, True, 2), (1, True, 4)], calls
    got = arrays(x)
    assert [n for n in ARRAYS if not torch.equal(got[n], want[n])] == []
    calls.clear()
    x.load_state(world["fresh"])
    x.fit(batches, epochs=2, preview=preview, preview_every=2)
    assert [c[0] for c in calls] == [1]
