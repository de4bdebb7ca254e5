"""Not-GPU: the host side of the optimizer (progressive-stable-diffusion_amd/optim.py) and the binding of its entry points
(include/dadd_hip_optim.h, ``lib.OPTIM_PROTOTYPES``, ``lib.OptimState``): the arena's layout, in-place gradient
accumulation, the state dict against ``torch.optim.AdamW``, the reference's parameter groups - and the check that the
bounds of tests/optim_reference.py admit a correct implementation: the fp32 model of the kernel stays inside every one of
them on a sweep of gradient scales, step counts and learning rates."""
import ctypes
import os
import re
import subprocess
from collections import OrderedDict

import pytest
import torch

from progressive_stable_diffusion_amd import lib as L
from progressive_stable_diffusion_amd import optim as O
from progressive_stable_diffusion_amd import weights as W
from progressive_stable_diffusion_amd.lr_scheduler import warmup_cosine_lr
from tests import optim_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "dadd_hip_optim.h"
F32 = torch.float32


# ---- binding -----------------------------------------------------------------------------------------------------------
def test_header_and_prototype_table_declare_the_same_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    names = set(re.findall(r"\b(dadd_[a-z0-9_]+)\s*\(", text))
    assert names == set(L.OPTIM_PROTOTYPES) == {"dadd_optim_grad_stats", "dadd_optim_finalize", "dadd_optim_adamw_step"}
    assert not names & (set(L.PROTOTYPES) | set(L.GRAD_PROTOTYPES) | set(L.HOST_PROTOTYPES) | set(L.NORM_GRAD_PROTOTYPES)
                        | set(L.ATTN_GRAD_PROTOTYPES))


def test_every_entry_point_is_exported_by_the_built_library():
    assert "optim.hip" in L.SOURCES and "optim_bf16.hip" not in L.SOURCES        # one source, the 16-bit type is a flag
    handle = ctypes.CDLL(L.build())
    missing = [n for n in L.OPTIM_PROTOTYPES if not hasattr(handle, n)]
    assert not missing, missing


def test_state_block_layout_and_constants_match_header(tmp_path):
    top = [f[0] for f in L.OptimState._fields_]
    grp = [f[0] for f in L.OptimGroup._fields_]
    consts = ["DADD_OPTIM_CHUNK", "DADD_OPTIM_MAX_GROUPS", "DADD_OPTIM_EMA", "DADD_OPTIM_P16_F16", "DADD_OPTIM_P16_BF16",
              "DADD_OPTIM_ZERO_GRAD"]
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void) {{\n'
                   '  printf("%zu %zu\\n", sizeof(dadd_optim_state), sizeof(dadd_optim_group));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(dadd_optim_state, {f}));\n' for f in top)
                   + "".join(f'  printf("%zu\\n", offsetof(dadd_optim_group, {f}));\n' for f in grp)
                   + "".join(f'  printf("%d\\n", {c});\n' for c in consts) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert [ctypes.sizeof(L.OptimState), ctypes.sizeof(L.OptimGroup)] == out[:2]
    assert [getattr(L.OptimState, f).offset for f in top] == out[2:2 + len(top)]
    assert [getattr(L.OptimGroup, f).offset for f in grp] == out[2 + len(top):2 + len(top) + len(grp)]
    assert [L.OPTIM_CHUNK, L.OPTIM_MAX_GROUPS, L.OPTIM_EMA, L.OPTIM_P16_F16, L.OPTIM_P16_BF16, L.OPTIM_ZERO_GRAD] == out[-6:]
    assert R.CHUNK == O.CHUNK == L.OPTIM_CHUNK


# ---- arena -------------------------------------------------------------------------------------------------------------
def test_arena_layout_alignment_groups_and_aliasing():
    tensors, group_of = R.layout_tensors()
    a = O.ParamArena(tensors, group_of, working_dtype=torch.bfloat16, ema=True)
    assert a.n_groups == 4 and a.numel % O.CHUNK == 0 and a.numel == O.CHUNK * sum(a.group_chunks) == O.CHUNK * a.n_chunks
    assert sorted(t.numel() for t in tensors.values()) == sorted(R.SIZES * 2)
    covered = torch.zeros(a.numel, dtype=torch.bool)
    end_of_previous = 0
    for gi in range(4):
        assert a.group_start[gi] % O.CHUNK == 0 and a.group_start[gi] >= end_of_previous
        lo, hi = a.group_start[gi], a.group_start[gi] + a.group_chunks[gi] * O.CHUNK
        for k in a.group_names[gi]:
            assert group_of[k] == gi and lo <= a.offsets[k] and a.offsets[k] + tensors[k].numel() <= hi
        end_of_previous = hi
    assert a.names == [k for gi in range(4) for k in tensors if group_of[k] == gi]
    for k, t in tensors.items():
        off, n = a.offsets[k], t.numel()
        assert off % 8 == 0 and not covered[off:off + n].any()
        covered[off:off + n] = True
        for view, flat in ((a.param(k), a.p), (a.grad(k), a.g), (a.exp_avg(k), a.m), (a.exp_avg_sq(k), a.v),
                           (a.ema_param(k), a.ema), (a.param16(k), a.p16)):
            assert view.shape == t.shape and view.data_ptr() % 16 == 0
            assert view.data_ptr() == flat.data_ptr() + off * flat.element_size()          # a view, not a copy
        assert torch.equal(a.param(k), t) and torch.equal(a.ema_param(k), t) and torch.equal(a.param16(k), t.to(torch.bfloat16))
        a.param(k).add_(1.0)
        assert torch.equal(a.p[off:off + n], (t + 1.0).reshape(-1))
    for flat in (a.p, a.g, a.m, a.v, a.ema):
        pad = flat[~covered]
        assert pad.numel() == a.numel - sum(R.SIZES) * 2 and not (pad != 0).any()
    assert not (a.g != 0).any() and not (a.m != 0).any() and not (a.v != 0).any()
    with pytest.raises(ValueError):
        a.ensure_p16(torch.float16)
    with pytest.raises(ValueError):
        O.ParamArena({"x": torch.zeros(3, dtype=torch.float16)}, {"x": 0})


def test_attach_accumulates_in_place_over_two_backwards():
    tensors, group_of = R.layout_tensors()
    a = O.ParamArena(tensors, group_of)
    params = {k: torch.nn.Parameter(torch.empty_like(t)) for k, t in tensors.items()}
    a.attach(params)
    ptrs = {k: q.grad.data_ptr() for k, q in params.items()}
    for k, q in params.items():
        assert q.data_ptr() == a.param(k).data_ptr() and torch.equal(q.detach(), tensors[k])
        assert q.grad.data_ptr() == a.grad(k).data_ptr()
    coef = {k: torch.randn(t.shape, generator=torch.Generator().manual_seed(i)) for i, (k, t) in enumerate(tensors.items())}
    for weight in (1.0, 0.5):
        loss = sum((q * coef[k]).sum() for k, q in params.items()) * weight
        loss.backward()
    for k, q in params.items():
        assert q.grad.data_ptr() == ptrs[k], k                                  # torch added into the preset view
        assert torch.equal(a.grad(k), coef[k] + 0.5 * coef[k]), k               # and the arena's g holds the sum
    used = sum(t.numel() for t in tensors.values())
    assert int((a.g != 0).sum()) <= used


# ---- the bounds admit a correct implementation ----------------------------------------------------------------------------
def test_model_stays_inside_every_bound_on_the_sweep():
    """400 000 elements, gradient scales 1e-6 .. 1e3, t in {1, 2, 9, 1000, 100000}, lr in {1e-4, 2e-4, 1e-6}, zero p, zero
    g and m = -g rows; clip active except at scale 1e-3."""
    n, worst = 400_000, {}
    for si, sg in enumerate((1e-6, 1e-3, 1.0, 1e3)):
        for t in (1, 2, 9, 1000, 100000):
            for lr in (1e-4, 2e-4, 1e-6):
                p, g, m, v, ema = R.sweep_case(n, sg, t, seed=si)
                h = R.Hyper(lr, 1e-3)
                c = R.f32r(R.coef64(R.norm64(g), 1.0)) if sg != 1e-3 else 1.0
                got = R.model_step32(p, g, m, v, ema, c, R.kernel_consts(h, t), 1.0 - R.EMA_DECAY)
                ref = R.ref_step64(p, g, m, v, ema, c, R.true_consts(h, t), 1.0 - R.EMA_DECAY)
                for k, x in R.worst_ratios(got, ref).items():
                    worst[k] = max(worst.get(k, 0.0), x)
    print("model against the bounds, worst error / bound:", {k: round(x, 3) for k, x in worst.items()})
    assert set(worst) == {"p", "m", "v", "ema"}
    for k, x in worst.items():
        assert x <= 1.0, (k, x)
    assert worst["p"] > 0.05 and worst["v"] > 0.05           # the bounds are within a small factor of what fp32 does


def test_bounds_reject_a_wrong_step():
    """Not vacuous: a step that ignores the bias correction, skips the weight decay, or takes 1 - beta2 from beta2 rounded
    to fp32 (relative error 3e-5 on 0.001) is far outside."""
    p, g, m, v, ema = R.sweep_case(20_000, 1.0, 9, seed=5)
    h = R.Hyper(1e-4, 0.1)            # (at wd = 1e-3 one step's decay, 1e-7, is below the resolution of fp32 itself)
    ref = R.ref_step64(p, g, m, v, ema, 1.0, R.true_consts(h, 9), 1e-3)
    K = R.kernel_consts(h, 9)
    for wrong in (dict(K, rsqrt_bc2=1.0), dict(K, decay=1.0), dict(K, omb2=R.f32r(1 - R.f32r(0.999)))):
        r = R.worst_ratios(R.model_step32(p, g, m, v, ema, 1.0, wrong, 1e-3), ref)
        assert max(r.values()) > 3.0, r


def test_norm_model_inside_its_bound_and_padding_stays_zero():
    tensors, group_of = R.layout_tensors()
    a = O.ParamArena(tensors, group_of, ema=True)
    gen = torch.Generator().manual_seed(3)
    for k in a.names:
        a.grad(k).copy_(torch.randn(a.shapes[k], generator=gen) * 0.3)
    covered = a.g != 0
    part = R.model_partials(a.g)
    assert part.shape == (a.n_chunks,)
    norm = float(part.double().sum().sqrt())
    ref = R.norm64(a.g)
    print(f"norm model: relative error {abs(norm - ref) / ref:.3e}, bound {R.NORM_REL:.3e}")
    assert abs(norm - ref) <= R.NORM_REL * ref
    sizes = [c * O.CHUNK for c in a.group_chunks]
    for t in (1, 7):
        K = R.expand([R.kernel_consts(h, t) for h in R.HYPERS4], sizes, F32)
        out = R.model_step32(a.p, a.g, a.m, a.v, a.ema, R.f32r(R.coef64(ref, 1.0)), K, 1e-3)
        for k in ("p", "m", "v", "ema"):
            assert not (out[k][~covered] != 0).any(), k                 # 0 * decay - step_size * (0 / (0 + eps)) = 0
        a.p, a.m, a.v, a.ema = out["p"], out["m"], out["v"], out["ema"]


# ---- state dict -----------------------------------------------------------------------------------------------------------
def _torch_adamw(arena, hypers):
    params = [[torch.nn.Parameter(arena.param(k)) for k in names] for names in arena.group_names]
    opt = torch.optim.AdamW([{"params": ps, "lr": h.lr, "weight_decay": h.wd, "betas": (h.b1, h.b2), "eps": h.eps}
                             for ps, h in zip(params, hypers)])
    return opt, [q for ps in params for q in ps]


def test_state_dict_round_trips_through_torch_adamw():
    tensors, group_of = R.layout_tensors()
    arena = O.ParamArena(tensors, group_of)
    fused = O.FusedAdamW(None, arena, R.as_groups(R.HYPERS4), max_grad_norm=1.0, init_scale=1024.0, growth_interval=7)
    sd0 = fused.state_dict()                                      # never stepped: no per-parameter state, as torch
    assert sd0["state"] == {} and [len(g["params"]) for g in sd0["param_groups"]] == [len(n) for n in arena.group_names]
    assert sd0["scaler"] == {"scale": 1024.0, "growth_tracker": 0}
    with pytest.raises(RuntimeError):
        fused.step()

    opt, flat = _torch_adamw(arena, R.HYPERS4)
    opt.load_state_dict(sd0)                                      # the layout loads into the real thing
    gen = torch.Generator().manual_seed(1)
    for _ in range(3):
        for q in flat:
            q.grad = torch.randn(q.shape, generator=gen)
        opt.step()
    sd = opt.state_dict()
    fused.load_state_dict(sd)
    assert fused.stats()["step"] == 3 and fused.stats()["scale"] == 1024.0
    for i, k in enumerate(arena.names):
        assert torch.equal(arena.exp_avg(k), sd["state"][i]["exp_avg"]) and arena.exp_avg(k).abs().sum() > 0
        assert torch.equal(arena.exp_avg_sq(k), sd["state"][i]["exp_avg_sq"])
    back = fused.state_dict()
    opt2, _ = _torch_adamw(arena, [R.Hyper(9.0, 9.0, 0.5, 0.5, 1.0)] * 4)
    opt2.load_state_dict(back)
    sd2 = opt2.state_dict()
    assert sorted(sd2["state"]) == sorted(sd["state"]) == list(range(len(arena.names)))
    for i in sd["state"]:
        assert float(sd2["state"][i]["step"]) == float(sd["state"][i]["step"]) == 3.0
        assert torch.equal(sd2["state"][i]["exp_avg"], sd["state"][i]["exp_avg"])
        assert torch.equal(sd2["state"][i]["exp_avg_sq"], sd["state"][i]["exp_avg_sq"])
    for g2, g1, h in zip(sd2["param_groups"], sd["param_groups"], R.HYPERS4):
        assert g2["params"] == g1["params"] and tuple(g2["betas"]) == (h.b1, h.b2)
        assert g2["lr"] == R.f32r(h.lr) and g2["weight_decay"] == R.f32r(h.wd) and g2["eps"] == R.f32r(h.eps)
    fused.load_state_dict(dict(back, scaler={"scale": 512.0, "growth_tracker": 4}))
    assert fused.stats()["scale"] == 512.0 and fused.stats()["growth_tracker"] == 4 and fused.stats()["step"] == 3
    uneven = {"state": dict(sd["state"]), "param_groups": sd["param_groups"]}
    uneven["state"][0] = dict(sd["state"][0], step=torch.tensor(5.0))
    with pytest.raises(ValueError):
        fused.load_state_dict(uneven)


def test_set_lrs_takes_the_scheduler_list_and_ema_state_names_the_views():
    tensors, group_of = R.layout_tensors()
    arena = O.ParamArena(tensors, group_of)
    fused = O.FusedAdamW(None, arena, R.as_groups(R.HYPERS4), ema_decay=0.999, working_dtype=torch.float16)
    lrs = warmup_cosine_lr(3, [h.lr for h in R.HYPERS4], 10, 100, 1e-7, 1e-6)
    fused.set_lrs(lrs)
    assert [g["lr"] for g in fused.state_dict()["param_groups"]] == [R.f32r(x) for x in lrs]
    with pytest.raises(ValueError):
        fused.set_lrs(lrs[:3])
    ema = fused.ema_state()
    assert list(ema) == arena.names and arena.p16.dtype == torch.float16
    for k, e in ema.items():
        assert e.data_ptr() == arena.ema_param(k).data_ptr() and torch.equal(e, tensors[k])


# ---- parameter groups -------------------------------------------------------------------------------------------------------
def test_reference_param_groups_on_the_full_model():
    keys = list(W.unet_shapes()) + list(W.conditioning_shapes()) + list(W.vae_shapes()) + list(W.clip_shapes())
    groups = O.reference_param_groups(keys, 1e-4, weight_decay=1e-3)
    assert [g["name"] for g in groups] == ["unet", "ordinal_embedder", "image_projection", "feature_purifier"]
    assert [g["lr"] for g in groups] == [1e-4, 1e-4, 2e-4, 2e-4] and all(g["weight_decay"] == 1e-3 for g in groups)
    placed = [k for g in groups for k in g["params"]]
    trainable = [k for k in keys if not k.startswith(("vae.", "image_encoder."))]
    assert sorted(placed) == sorted(trainable) and len(set(placed)) == len(placed)
    assert len(trainable) < len(keys) and not any(k.startswith(("vae.", "image_encoder.")) for k in placed)
    for g in groups:
        assert g["params"] and all(k.startswith(g["name"] + ".") for k in g["params"])
    no_purifier = O.reference_param_groups(list(W.unet_shapes()) + list(W.conditioning_shapes(purifier=False)), 1e-4)
    assert [g["name"] for g in no_purifier] == ["unet", "ordinal_embedder", "image_projection"]
    with pytest.raises(ValueError):
        O.reference_param_groups(["mystery.weight"], 1e-4)
    small = OrderedDict((k, torch.zeros(3)) for k in ("unet.a", "ordinal_embedder.b", "image_projection.c", "feature_purifier.d"))
    arena = O.arena_from_groups(small, O.reference_param_groups(list(small), 1e-4))
    assert arena.n_groups == 4 and arena.group_chunks == [1, 1, 1, 1] and arena.names == list(small)
