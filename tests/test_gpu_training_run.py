"""-m gpu: a training RUN on ``training.Trainer`` - gradient accumulation, the run's numbers, state / exact resume and
``fit`` - at the smallest case the UNet takes: B = 2, 256x256 images (32x32 latents), the tiny CLIP config of
tests/test_gpu_train_step.py, seeded weights, loss scale 4096, EMA from the first optimizer step on and at every one.

``weights.unet_shapes()`` has one size, so the arena is the full one: the module and two trainers are built once, a
state of the untouched trainer (on the device) sets either back where a test wants a fresh one, and no test writes a
checkpoint file of that size (the file layer is tests/test_training_run_cpu.py's).

Equalities are ``torch.equal``: the step is deterministic, an accumulated gradient is one fp32 add per element onto the
first micro-batch's, and a restored run has the same bits to continue from.  The one bound is the forward bound of the
existing training test, 2e-2 * max(1, |ref|), for the mean micro loss against the oracle loss of the joined batch."""
import math

import pytest
import torch

from oracle import sampler as OS
from oracle import training as OT
from progressive_stable_diffusion_amd import training as TR
from progressive_stable_diffusion_amd import training_io as IO
from progressive_stable_diffusion_amd import weights as W
from progressive_stable_diffusion_amd.lr_scheduler import warmup_cosine_lr
from tests import golden_inputs as GI

pytestmark = pytest.mark.gpu

F32 = torch.float32
DEV = torch.device("cuda:0")
SCALE = 4096.0
LR = 1e-4
TINY_CLIP = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, image_size=224,
                 patch_size=14, projection_dim=32)
ARRAYS = ("p", "m", "v", "ema", "p16")


def _batch(seed, labels, t, drop):
    g = torch.Generator().manual_seed(seed)
    batch = (torch.rand(2, 3, 256, 256, generator=g) * 2 - 1, torch.tensor(labels), torch.randn(2, 3, 224, 224, generator=g))
    draws = dict(t=torch.tensor(t), noise=torch.randn(2, 4, 32, 32, generator=g),
                 latent_noise=torch.randn(2, 4, 32, 32, generator=g), drop_mask=torch.tensor(drop))
    return batch, draws


@pytest.fixture(scope="module")
def run():
    from progressive_stable_diffusion_amd.config import default_config
    from progressive_stable_diffusion_amd.diffusion_module_ip import DiffusionModuleWithIP
    shapes = dict(W.unet_shapes())
    shapes.update(W.vae_shapes())
    shapes.update(W.conditioning_shapes(clip_hidden=TINY_CLIP["hidden_size"], clip_proj=TINY_CLIP["projection_dim"]))
    shapes.update(W.clip_shapes(TINY_CLIP))
    sd = W.init_state_dict(shapes, 0, gates=GI.GATES, warm_start_dis=False)
    cfg = default_config(**{"dataset.image_size": 256, "model.cfg_drop_prob": 0.5,
                            "optimizer": {"weight_decay": 0.01, "betas": [0.9, 0.999]},
                            "scheduler": {"warmup_epochs": 2, "min_lr": 0.0},
                            "training": {"precision": "16-mixed", "use_min_snr_weighting": True, "max_epochs": 10,
                                         "update_starting_at_step": 1, "update_every_n_steps": 1, "log_every_n_steps": 1}})
    mod = DiffusionModuleWithIP(cfg, state_dict=sd, device=DEV, seed=0, batch_size=2, clip_config=TINY_CLIP)
    a, da = _batch(31, [1.0, 3.0], [700, 35], [False, True])
    b, db = _batch(32, [0.0, 2.0], [410, 900], [False, False])
    x, y = TR.Trainer(mod, LR, init_scale=SCALE), TR.Trainer(mod, LR, init_scale=SCALE)
    assert x.accumulate == 1 and x.log_every == 1 and (x.ema_start, x.ema_every) == (1, 1)
    fresh = x.state(device=DEV)
    return dict(cfg=cfg, sd=sd, mod=mod, x=x, y=y, fresh=fresh, A=(tuple(v.to(DEV) for v in a), da), B=(tuple(v.to(DEV) for v in b), db),
                host=(a, b))


def _fresh(run, tr, accumulate=1):
    tr.load_state(run["fresh"])
    tr.accumulate = accumulate
    assert tr.steps == 0 and tr.pending == 0 and tr.next_epoch == 0
    return tr


def _same_arrays(t1, t2):
    torch.cuda.synchronize()
    bad = [n for n in ARRAYS if not torch.equal(getattr(t1.arena, n), getattr(t2.arena, n))]
    if t1.relayout is not None and not torch.equal(t1.relayout.buf, t2.relayout.buf):
        bad.append("relayout.buf")
    return bad


def test_step_is_the_parents_sequence_bit_for_bit(run):
    """X runs ``step()``; Y runs what ``step()`` was before accumulation existed, by hand; same injected draws."""
    x, y = _fresh(run, run["x"]), _fresh(run, run["y"])
    for n, (batch, draws) in enumerate((run["A"], run["B"], run["A"]), start=1):
        lx = x.step(batch, is_training=False, **draws)
        loss = y.loss(batch, is_training=False, **draws)
        (loss * y.optimizer.scale()).backward()
        y.optimizer.step(update_ema=n >= y.ema_start and n % y.ema_every == 0, zero_grad=True)
        y.relayout.refresh()
        assert torch.equal(lx, loss.detach()), n
        assert _same_arrays(x, y) == [], n
    assert not torch.equal(x.arena.ema, x.arena.p)                              # the EMA lags the weights
    sx, sy = x.optimizer.stats(), y.optimizer.stats()
    assert sx == sy and sx["step"] == 3 and not sx["found_inf"], (sx, sy)
    assert x.steps == 3 and x.pending == 0 and not bool(x.arena.g.any())


def test_accumulated_gradient_is_the_sum_of_the_micro_gradients(run):
    tr = _fresh(run, run["x"])
    (a, da), (b, db), g = run["A"], run["B"], run["x"].arena.g
    assert not bool(g.any())
    la = tr.backward(a, weight=0.5, is_training=False, **da)
    ga = g.clone()
    g.zero_()
    lb = tr.backward(b, weight=0.5, is_training=False, **db)
    gb = g.clone()
    g.zero_()
    assert tr.pending == 2 and bool(ga.any()) and bool(gb.any()) and not torch.equal(ga, gb)
    tr.backward(a, weight=0.5, is_training=False, **da)
    tr.backward(b, weight=0.5, is_training=False, **db)
    want = ga + gb
    diff = (g != want)
    assert not bool(diff.any()), (int(diff.sum()), float((g - want).abs().max()), diff.nonzero()[:8].flatten().tolist())
    with pytest.raises(RuntimeError, match="4 micro-batch"):
        tr.state(device=DEV)
    g.zero_()
    tr.pending = 0

    # the mean of the two micro losses against the oracle loss of the joined batch of four
    ha, hb = run["host"]
    with torch.no_grad():
        feats = torch.cat([run["mod"].image_encoder.get_hidden_states(v[2]).cpu() for v in (a, b)])
        ref, _ = OT.training_loss(run["sd"], OS.OracleCfg(image_size=256, use_routing_gates=True), torch.cat([ha[0], hb[0]]),
                                  torch.cat([ha[1], hb[1]]), feats, *(torch.cat([da[k], db[k]]) for k in
                                                                     ("t", "noise", "latent_noise", "drop_mask")))
    got, ref = 0.5 * (la.item() + lb.item()), ref.item()
    print(f"micro losses {la.item():.6f}, {lb.item():.6f}: mean {got:.6f} vs oracle loss of the joined batch {ref:.6f}")
    assert abs(got - ref) < 2e-2 * max(1.0, abs(ref)), (got, ref)


def test_two_micro_batches_per_optimizer_step(run):
    tr = _fresh(run, run["x"], accumulate=2)
    emas, p0 = [tr.arena.ema.clone()], tr.arena.p.clone()
    for i, (batch, draws) in enumerate((run["A"], run["B"], run["B"], run["A"]), start=1):
        tr.step(batch, is_training=False, **draws)
        assert tr.pending == i % 2 and tr.steps == i // 2
        if i == 1:
            assert torch.equal(tr.arena.p, p0) and bool(tr.arena.g.any())        # no optimizer step yet
        if i % 2 == 0:
            emas.append(tr.arena.ema.clone())
    st = tr.optimizer.stats()
    assert st["step"] == 2 and tr.steps == 2 and not st["found_inf"], st
    assert not torch.equal(emas[1], emas[0]) and not torch.equal(emas[2], emas[1])      # the EMA moved at both steps
    assert tr.ema_latest_step == 2 and not bool(tr.arena.g.any())
    m = tr.pop_metrics()
    assert m["micro_batches"] == 4 and m["global_step"] == 2 and m["skipped_steps"] == 0 and m["cfg_drop_rate"] == 0.25
    assert tr.flush() is False
    tr.step(run["A"][0], is_training=False, **run["A"][1])                                  # a short last group
    assert tr.pending == 1 and tr.flush() is True and tr.steps == 3 and tr.pending == 0
    assert tr.pop_metrics()["micro_batches"] == 1 and tr.pop_metrics()["micro_batches"] == 0


def test_resume_is_exact(run):
    t1, t2 = _fresh(run, run["x"]), run["y"]
    batch = run["A"][0]
    torch.manual_seed(2024)
    t1.step(batch)
    t1.step(batch)
    saved = t1.state(device=DEV)
    l3 = t1.step(batch)
    st1 = t1.optimizer.stats()
    assert st1["step"] == 3 and saved["global_step"] == 2 and saved["callbacks"]["EMAWeightAveraging"]["latest_update_step"] == 2

    torch.manual_seed(7)                        # another generator state and another history: both must go
    torch.randn(11, device=DEV)
    t2.step(run["B"][0])
    t2.load_state(saved)
    assert t2.steps == 2 and t2.epoch == t1.epoch and t2.next_epoch == 1 and t2.ema_latest_step == 2
    l3b = t2.step(batch)
    assert torch.equal(l3b, l3), (l3b.item(), l3.item())
    assert _same_arrays(t1, t2) == []
    assert t2.optimizer.stats() == st1
    assert all(torch.equal(t2.gates[k], v) for k, v in t1.gates.items())


def test_state_holds_the_two_exports(run):
    tr = _fresh(run, run["x"])
    tr.step(run["A"][0], is_training=False, **run["A"][1])                       # moments, and an EMA that is not the weights
    state = tr.state(device=DEV)
    assert set(state) == {"epoch", "global_step", "state_dict", "current_model_state", "optimizer_states", "lr_schedulers",
                          "callbacks", "rng", "dadd"}
    assert state["dadd"] == {"format": 1, "operand_dtype": "torch.float16", "accumulate": tr.accumulate,
                             "parts": ["ema", "raw", "optimizer"]}
    assert set(state["rng"]) == {"cpu", "cuda"} and torch.equal(state["rng"]["cuda"], torch.cuda.get_rng_state(DEV))
    for key, ema in (("state_dict", True), ("current_model_state", False)):
        want = tr.export_state_dict(ema=ema)
        assert list(state[key]) == list(want) == list(run["sd"])
        bad = [k for k, v in want.items() if state[key][k].dtype != v.dtype or not torch.equal(state[key][k].cpu(), v)]
        assert bad == [], (key, bad[:8])
    names = [k for gi in range(tr.arena.n_groups) for k in tr.arena.group_names[gi]]
    osd = state["optimizer_states"][0]
    # copies, not views: a 1x1 conv's OIHW form is contiguous as it lies in the arena, and a state that aliased it would
    # follow the next step
    live = {getattr(tr.arena, n).untyped_storage().data_ptr() for n in ("p", "ema", "m", "v")}
    held = list(state["state_dict"].items()) + list(state["current_model_state"].items()) + \
        [(f"{i}.{n}", st[n]) for i, st in osd["state"].items() for n in ("exp_avg", "exp_avg_sq")]
    assert [k for k, t in held if t.untyped_storage().data_ptr() in live] == []
    assert osd["format"] == IO.OPTIMIZER_FORMAT and [i for g in osd["param_groups"] for i in g["params"]] == list(range(len(names)))
    assert all(torch.equal(osd["state"][i]["exp_avg"], tr.arena.exp_avg(k)) for i, k in enumerate(names))
    with pytest.raises(ValueError, match="format"):
        tr.load_state({**state, "dadd": {**state["dadd"], "format": 2}})


def test_fit_two_epochs(run):
    tr = _fresh(run, run["x"])
    torch.manual_seed(5)
    seen = []
    logged = tr.fit([run["host"][0], run["A"][0]], epochs=2, on_log=seen.append, log_every=1)
    assert logged == seen and len(logged) == 4
    base = [g["lr"] for g in tr.groups]
    for i, m in enumerate(logged):
        assert set(m) == set(TR.Trainer.METRIC_KEYS), sorted(m)
        assert math.isfinite(m["loss"]) and m["loss"] > 0 and 0.0 <= m["cfg_drop_rate"] <= 1.0
        assert (m["global_step"], m["step"], m["epoch"], m["micro_batches"], m["skipped_steps"]) == (i + 1, i + 1, i // 2, 1, 0), m
        assert not m["found_inf"] and m["scale"] == SCALE and m["grad_norm"] > 0
        want = warmup_cosine_lr(i // 2, base, 2, 10, LR * 0.01, 0.0)
        assert list(m["lr"]) == ["unet", "ordinal_embedder", "image_projection", "feature_purifier"]
        assert list(m["lr"].values()) == [torch.tensor(v, dtype=F32).item() for v in want], (m["lr"], want)
    assert logged[0]["lr"]["unet"] < logged[2]["lr"]["unet"]                    # the warm-up: epoch 1 is above epoch 0
    assert tr.steps == 4 and tr.next_epoch == 2 and tr.pending == 0
    assert tr.fit([run["A"][0]], epochs=2) == []                                 # nothing left below epoch 2
