"""-m gpu: the optimizer step on the HIP kernels (csrc/optim.hip) through ``HipBackend.optim_*`` and ``optim.FusedAdamW``,
against the float64 restatement and within the bounds of tests/optim_reference.py (where they are derived).  Outputs and
scratch are NaN-filled before every call.  Arenas are the smallest that reach each hazard: tensors of 1, 7, 8, 9, 4095,
4096 and 4097 elements over four groups with different lr / wd (10 chunks: every chunk edge and group edge), and 40
chunks under ``max_blocks = 8`` (every workgroup strides five times).

Measured on an MI355X (error / bound): one warm step p 0.59-0.71, m 0.05-0.24, v 0.27-0.55, ema 0.25; norm 3e-9 .. 2.5e-8
relative (bound 1.9e-6), coef 5e-8 (bound 2.4e-6); trajectory, relative L2 of the displacement per tensor: p 2.6-4.5e-5, ema
2.3-4.6e-3, equal to the CPU model's to three digits (bound: twice the model's).  DESIGN.md §7.1."""
import math

import pytest
import torch

from progressive_stable_diffusion_amd import grad_ops
from progressive_stable_diffusion_amd import lib as L
from progressive_stable_diffusion_amd import optim as O
from progressive_stable_diffusion_amd.lr_scheduler import warmup_cosine_lr
from tests import optim_reference as R

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(DEV)


def nan_fill(*ts):
    for t in ts:
        if t is not None:
            (t.view(F32) if t.dtype == torch.int32 else t).fill_(NAN)


def covered_mask(arena):
    m = torch.zeros(arena.numel, dtype=torch.bool)
    for k in arena.names:
        m[arena.offsets[k]:arena.offsets[k] + arena.shapes[k].numel()] = True
    return m


def set_step(fused, t_done):
    """Pre-set the step count in the state block (the moments of a warm state go straight into the arena)."""
    h = fused._download()
    h.step = t_done
    fused._upload(h)


def make(hip, hypers=R.HYPERS4, tensors=None, group_of=None, dtype=None, ema=True, **kw):
    if tensors is None:
        tensors, group_of = R.layout_tensors()
    arena = O.ParamArena(tensors, group_of, device=DEV, working_dtype=dtype, ema=ema)
    fused = O.FusedAdamW(hip, arena, R.as_groups(hypers), ema_decay=R.EMA_DECAY if ema else None, **kw)
    nan_fill(fused.partials, fused.flags)
    return arena, fused


def load_flat(arena, **arrays):
    """Write flat CPU arrays (arena length) into the arena's buffers, keeping the padding zero."""
    mask = covered_mask(arena)
    for name, x in arrays.items():
        getattr(arena, name).copy_(torch.where(mask, x, torch.zeros_like(x)))


def sizes_of(arena):
    return [c * O.CHUNK for c in arena.group_chunks]


def snapshot(arena):
    torch.cuda.synchronize()
    return {k: (None if getattr(arena, k) is None else getattr(arena, k).detach().cpu().clone())
            for k in ("p", "g", "m", "v", "ema", "p16")}


def step_and_check(hip, arena, fused, hypers, t, what, *, update_ema, zero_grad, scale=0.0):
    """One ``step()`` from the arena's current state, every array against the float64 reference fed the kernel's own coef."""
    before = snapshot(arena)
    nan_fill(fused.partials, fused.flags, arena.p16)
    if not update_ema and arena.ema is not None:
        nan_fill(arena.ema)
    fused.step(update_ema=update_ema, zero_grad=zero_grad)
    after, st = snapshot(arena), fused.stats()
    assert st["step"] == t and not st["found_inf"], st
    ema_w = 1.0 - R.EMA_DECAY
    ref = R.ref_step64(before["p"], before["g"], before["m"], before["v"], before["ema"] if update_ema else None,
                       st["coef"], R.expand([R.true_consts(h, t) for h in hypers], sizes_of(arena), F64), ema_w)
    ratios = R.check_step(after, ref, what)
    if arena.p16 is not None:
        assert torch.equal(after["p16"].view(torch.int16), after["p"].to(arena.p16.dtype).view(torch.int16)), what
    if zero_grad:
        assert not (after["g"].view(torch.int32) != 0).any(), what                       # +0.0 everywhere
    else:
        assert torch.equal(after["g"].view(torch.int32), before["g"].view(torch.int32)), what
    if not update_ema and arena.ema is not None:
        assert bool(torch.isnan(after["ema"]).all()), what
    pad = ~covered_mask(arena)
    for k in ("p", "m", "v") + (("ema",) if update_ema else ()):
        assert not (after[k][pad] != 0).any(), (what, k)
    return ratios, st, before, after


# ---- norm and coefficient -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target_norm,max_norm", [(0.1, 1.0), (30.0, 1.0), (30.0, 0.0)])
def test_norm_and_coefficient(hip, target_norm, max_norm):
    arena, fused = make(hip, max_grad_norm=max_norm, ema=False)
    g = torch.where(covered_mask(arena), torch.randn(arena.numel, generator=torch.Generator().manual_seed(7)), torch.zeros(()))
    load_flat(arena, g=g * (target_norm / float(g.double().norm())))
    g = arena.g.cpu()
    hip.wait_current()
    words = []
    for rep in range(2):
        nan_fill(fused.partials, fused.flags)
        hip.wait_current()
        hip.optim_grad_stats(arena.g, fused.partials, fused.flags)
        hip.optim_finalize(fused.partials, fused.flags, fused.state)
        hip.release_to_current()
        st = fused.stats()
        words.append((fused.partials.cpu().view(torch.int32), fused.flags.cpu(), st["grad_norm"], st["coef"]))
        assert st["step"] == rep + 1 and not st["found_inf"]
    part, flags, norm, coef = words[0]
    assert not flags.any() and torch.equal(part, words[1][0]) and torch.equal(flags, words[1][1])
    assert (norm, coef) == words[1][2:]                                                  # same bits on a repeated call
    assert torch.equal(part, R.model_partials(g).view(torch.int32))                      # the documented summation order
    ref_norm = R.norm64(g)
    ref_coef = R.coef64(ref_norm, max_norm)
    print(f"norm {target_norm} max_norm {max_norm}: grad_norm rel err {abs(norm - ref_norm) / ref_norm:.3e} (bound {R.NORM_REL:.3e}), "
          f"coef {coef:.6g} rel err {abs(coef - ref_coef) / ref_coef:.3e} (bound {R.COEF_REL:.3e})")
    assert abs(norm - ref_norm) <= R.NORM_REL * ref_norm
    assert abs(coef - ref_coef) <= R.COEF_REL * ref_coef
    assert (coef < 0.04) == (max_norm > 0 and target_norm > 1) and (coef == 1.0) == (max_norm == 0 or target_norm < 1)


# ---- one step from a warm state -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 1000])
@pytest.mark.parametrize("dtype", [None, F16, BF16])
@pytest.mark.parametrize("update_ema,zero_grad", [(True, True), (False, False), (True, False), (False, True)])
def test_one_step_from_a_warm_state(hip, t, dtype, update_ema, zero_grad):
    arena, fused = make(hip, dtype=dtype, max_grad_norm=1.0)
    p, g, m, v, ema = R.sweep_case(arena.numel, 1.0, t, seed=t)
    load_flat(arena, p=p, g=g, m=m, v=v, ema=ema)
    set_step(fused, t - 1)
    what = f"warm step t {t} {dtype} ema {update_ema} zero {zero_grad}"
    _, st, before, _ = step_and_check(hip, arena, fused, R.HYPERS4, t, what, update_ema=update_ema, zero_grad=zero_grad)
    assert st["coef"] < 0.5                                                              # clipping is active here
    k = max(1, arena.numel // 400)
    assert not before["g"][2 * k:3 * k].any() and (t == 1 or torch.equal(before["m"][3 * k:4 * k], -before["g"][3 * k:4 * k]))


# ---- the bounded grid ------------------------------------------------------------------------------------------------------
def test_grid_stride_gives_the_same_bits(hip):
    gen = torch.Generator().manual_seed(11)
    tensors = {"a.w": torch.randn(17 * O.CHUNK - 5, generator=gen) * 0.05, "b.w": torch.randn(23 * O.CHUNK - 4095, generator=gen)}
    group_of = {"a.w": 0, "b.w": 1}
    hypers = R.HYPERS4[1:3]
    runs = []
    for max_blocks in (0, 8):
        arena, fused = make(hip, hypers, tensors, group_of, dtype=BF16, max_grad_norm=1.0, max_blocks=max_blocks)
        assert arena.n_chunks == 40
        p, g, m, v, ema = R.sweep_case(arena.numel, 1.0, 5, seed=2)
        load_flat(arena, g=g, m=m, v=v, ema=ema)
        set_step(fused, 4)
        if max_blocks == 0:
            step_and_check(hip, arena, fused, hypers, 5, "40 chunks, default grid", update_ema=True, zero_grad=True)
        else:
            nan_fill(arena.p16)
            fused.step(update_ema=True, zero_grad=True)
        snap = snapshot(arena)
        snap.update(partials=fused.partials.cpu(), flags=fused.flags.cpu(), state=fused.state.cpu())
        runs.append(snap)
    for k, x in runs[0].items():
        assert torch.equal(x.view(torch.int16 if x.element_size() == 2 else torch.int32),
                           runs[1][k].view(torch.int16 if x.element_size() == 2 else torch.int32)), k


# ---- overflow and the loss scale ------------------------------------------------------------------------------------------
def test_overflow_skips_halves_and_regrows(hip):
    arena, fused = make(hip, dtype=F16, max_grad_norm=1.0, init_scale=1024.0, growth_interval=3)
    gen = torch.Generator().manual_seed(5)
    _, g0, m, v, ema = R.sweep_case(arena.numel, 1.0, 9, seed=9)
    load_flat(arena, m=m, v=v, ema=ema)
    set_step(fused, 8)
    bad = (g0 * 1024.0).clone()
    bad[arena.offsets["g0.t4"] + 100] = float("inf")                                   # two different chunks
    bad[arena.offsets["g3.t7"] + 4000] = NAN
    load_flat(arena, g=bad)
    before = snapshot(arena)
    nan_fill(fused.partials, fused.flags, arena.p16)
    fused.step(update_ema=True, zero_grad=True)
    after, st = snapshot(arena), fused.stats()
    assert st["found_inf"] and st["step"] == 8 and st["coef"] == 0.0 and st["scale"] == 512.0 and st["growth_tracker"] == 0
    assert int(fused.flags.sum()) == 2
    for k in ("p", "m", "v"):
        assert torch.equal(after[k].view(torch.int32), before[k].view(torch.int32)), k   # bit-identical
    assert not (after["g"].view(torch.int32) != 0).any()                                 # zero_grad runs on a skipped step
    assert torch.equal(after["p16"].view(torch.int16), before["p"].to(F16).view(torch.int16))
    e64 = before["ema"].double() + (before["p"].double() - before["ema"].double()) * (1.0 - R.EMA_DECAY)
    e_bound = 2 * R.ulp32(e64) + 2 * R.U * (before["p"].double() - before["ema"].double()).abs()
    assert bool(((after["ema"].double() - e64).abs() <= e_bound).all())                  # the EMA does not know about skips
    for i in range(3):
        scale = fused.stats()["scale"]
        assert scale == 512.0
        g = torch.randn(arena.numel, generator=gen) * (0.002 if i == 1 else 1.0)         # step 1 unclipped
        load_flat(arena, g=g * scale)
        true_g = arena.g.cpu().double() / scale
        _, st, _, _ = step_and_check(hip, arena, fused, R.HYPERS4, 9 + i, f"clean step {i} under scale {scale}",
                                     update_ema=False, zero_grad=True)
        ref_norm = R.norm64(true_g)
        ref_coef = R.coef64(ref_norm, 1.0, scale)
        assert abs(st["grad_norm"] - ref_norm) <= R.NORM_REL * ref_norm                  # the norm of the unscaled gradient
        assert abs(st["coef"] - ref_coef) <= R.COEF_REL * ref_coef                       # clip and unscale in one factor
        assert (st["coef"] * scale == 1.0) == (i == 1)
    st = fused.stats()
    assert st["scale"] == 1024.0 and st["growth_tracker"] == 0 and st["step"] == 11


# ---- trajectory --------------------------------------------------------------------------------------------------------------
def test_twelve_step_trajectory_against_torch_adamw_in_float64(hip):
    gen = torch.Generator().manual_seed(21)
    shapes = {"unet.w": (67, 61), "unet.b": (4097,), "ordinal_embedder.w": (5000,), "image_projection.w": (40, 103),
              "image_projection.b": (3001,), "feature_purifier.w": (4095,)}
    tensors = {k: torch.randn(s, generator=gen) * 0.05 for k, s in shapes.items()}
    groups = O.reference_param_groups(list(tensors), 1e-4, weight_decay=1e-3)
    hypers = [R.Hyper(g["lr"], g["weight_decay"]) for g in groups]
    arena = O.arena_from_groups(tensors, groups, device=DEV, working_dtype=BF16)
    fused = O.FusedAdamW(hip, arena, groups, max_grad_norm=1.0, ema_decay=R.EMA_DECAY)
    mask, sizes = covered_mask(arena), sizes_of(arena)
    steps, ema_every = 12, 4
    grads = [torch.where(mask, torch.randn(arena.numel, generator=gen) * (0.002 if i % 3 == 1 else 0.05 * (1 + i)), torch.zeros(()))
             for i in range(steps)]
    lrs = [warmup_cosine_lr(i, [h.lr for h in hypers], 4, steps, 1e-6, 1e-6) for i in range(steps)]
    p0 = arena.p.cpu().clone()
    clipped = 0
    for i in range(steps):
        arena.g.copy_(grads[i])
        fused.set_lrs(lrs[i])
        fused.step(update_ema=(i + 1) % ema_every == 0, zero_grad=True)
        clipped += fused.stats()["coef"] < 1.0
    assert 0 < clipped < steps and fused.stats()["step"] == steps                       # clipping active on some steps only
    p, ema = arena.p.cpu(), arena.ema.cpu()
    ref_p, ref_ema = R.torch_trajectory(p0, grads, lrs, sizes, hypers, 1.0, R.EMA_DECAY, ema_every)
    mod_p, mod_ema = R.model_trajectory(p0, grads, lrs, sizes, hypers, 1.0, R.EMA_DECAY, ema_every)
    slices = [slice(arena.offsets[k], arena.offsets[k] + arena.shapes[k].numel()) for k in arena.names]
    for what, x, ref, mod in (("p", p, ref_p, mod_p), ("ema", ema, ref_ema, mod_ema)):
        err, e_model = R.displacement_error(x, p0, ref, slices), R.displacement_error(mod, p0, ref, slices)
        for k, e, em in zip(arena.names, err, e_model):
            bound = max(2 * em, 2.0 ** -20)
            print(f"trajectory {what}_12 - {what}_0 {k:22s} rel L2 {e:.3e}  (model {em:.3e}, bound {bound:.3e})")
        for k, e, em in zip(arena.names, err, e_model):
            assert e <= max(2 * em, 2.0 ** -20), (what, k, e, em)
    disp = (ref_p - p0.double())[mask].abs().mean()
    assert disp > 1e-4                                                                    # the weights did move
    assert torch.equal(arena.p16.cpu().view(torch.int16), p.to(BF16).view(torch.int16))


# ---- the working copy is what the forward kernels read ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16])
def test_second_forward_on_the_working_copy_through_grad_ops(hip, dtype):
    gen = torch.Generator().manual_seed(31)
    M, C, F, N2 = 128, 64, 64, 64
    tensors = {"unet.ff1.weight": torch.randn(2 * F, C, generator=gen) * 0.1, "unet.ff1.bias": torch.randn(2 * F, generator=gen) * 0.1,
               "unet.ff2.weight": torch.randn(N2, F, generator=gen) * 0.1, "unet.ff2.bias": torch.randn(N2, generator=gen) * 0.1}
    groups = O.reference_param_groups(list(tensors), 1e-2, weight_decay=1e-3)[:1]
    arena = O.arena_from_groups(tensors, groups, device=DEV, working_dtype=dtype)
    fused = O.FusedAdamW(hip, arena, groups, max_grad_norm=1.0)
    params = {k: torch.nn.Parameter(torch.empty(t.shape, device=DEV)) for k, t in tensors.items()}
    arena.attach(params)
    x = torch.randn(M, C, generator=gen).to(dtype).to(DEV)
    r = torch.randn(M, N2, generator=gen).to(DEV)

    def forward(w1, b1, w2, b2):
        return grad_ops.linear(hip, grad_ops.geglu(hip, grad_ops.linear(hip, x, w1, b1)), w2, b2)

    def loss_of(out):
        return (out.float() * r).sum()

    names = list(tensors)
    first = loss_of(forward(*(params[k] for k in names)))
    first.backward()
    assert all(float(arena.grad(k).abs().sum()) > 0 for k in names)                      # autograd wrote into the arena
    p_before = arena.p.clone()
    fused.step()
    assert not torch.equal(arena.p, p_before) and not arena.g.any()
    with torch.no_grad():
        cast = loss_of(forward(*(arena.param(k) for k in names)))                        # casts the masters with .to(dtype)
        hip.wait_current()
        h = hip.empty((1, 1, M, 2 * F), dtype)
        hip.igemm(x.view(1, 1, M, C), arena.param16(names[0]), h, bias=arena.param(names[1]), flags=L.EPI_BIAS)
        y = hip.empty((M, F), dtype)
        hip.geglu(h.view(M, 2 * F), y)
        out = hip.empty((1, 1, M, N2), dtype)
        hip.igemm(y.view(1, 1, M, F), arena.param16(names[2]), out, bias=arena.param(names[3]), flags=L.EPI_BIAS)
        hip.release_to_current()
        copy = loss_of(out.view(M, N2))
    print(f"{dtype}: loss {float(first.detach()):.6f} -> {float(cast):.6f} (masters cast) / {float(copy):.6f} (working copy)")
    assert torch.equal(cast.view(torch.int32), copy.view(torch.int32))                  # bitwise
    assert float(cast) != float(first.detach()) and math.isfinite(float(cast))


# ---- graph replay ------------------------------------------------------------------------------------------------------------
def test_captured_step_replays_across_a_schedule(hip):
    gen = torch.Generator().manual_seed(41)
    eager_arena, eager = make(hip, dtype=F16, max_grad_norm=1.0, init_scale=256.0, growth_interval=2)
    graph_arena, graphed = make(hip, dtype=F16, max_grad_norm=1.0, init_scale=256.0, growth_interval=2)
    grads = [torch.randn(eager_arena.numel, generator=gen) * s for s in (300.0, 2.0, 700.0)]
    lrs = [warmup_cosine_lr(i, [h.lr for h in R.HYPERS4], 2, 3, 1e-6, 1e-6) for i in range(3)]
    torch.cuda.synchronize()
    hip.graph_begin()
    graphed.step(update_ema=True, zero_grad=True)
    g = hip.graph_end()
    try:
        for i in range(3):
            for arena, fused in ((eager_arena, eager), (graph_arena, graphed)):
                load_flat(arena, g=grads[i])
                fused.set_lrs(lrs[i])
            eager.step(update_ema=True, zero_grad=True)
            hip.wait_current()
            hip.graph_launch(g)
            hip.release_to_current()
            a, b = snapshot(eager_arena), snapshot(graph_arena)
            for k in a:
                assert torch.equal(a[k].view(torch.int16 if a[k].element_size() == 2 else torch.int32),
                                   b[k].view(torch.int16 if a[k].element_size() == 2 else torch.int32)), (i, k)
            assert torch.equal(eager.state.cpu(), graphed.state.cpu()), i
            assert eager.stats()["step"] == i + 1
    finally:
        hip.graph_destroy(g)
    assert eager.stats()["scale"] == 512.0                                                # grew once in three clean steps
