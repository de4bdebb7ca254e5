"""Host-side checks of the plan refresh (csrc/plan_refresh.hip, optim.PlanRefresh, engine.Recipe): the CPU executor of
the descriptor items against the real packers, the rounding sequence torch uses from float64 to a 16-bit type, the
host-only table check of the library through ctypes, and the completeness of the recipes a ``UNetPlan`` and the
conditioning modules record.  No kernel runs here.
"""
import ctypes as C
from collections import OrderedDict

import pytest
import torch

from progressive_stable_diffusion_amd import engine as E
from progressive_stable_diffusion_amd import lib as L
from progressive_stable_diffusion_amd import optim as O
from progressive_stable_diffusion_amd import unet_grad as UG
from progressive_stable_diffusion_amd import weights as W
from tests import plan_refresh_reference as REF
from tests.torch_backend import TorchRefBackend

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
GATES = {"anatomy": (0.1, 0.9), "disease": (0.9, 0.1), "both": (0.5, 0.5)}


def test_sources_header_and_registry():
    assert {"plan_refresh.hip", "plan_refresh_bf16.hip"} <= set(L.SOURCES)
    assert set(L.HEADER_PROTOTYPES["dadd_hip_plan_refresh.h"]) == {
        "dadd_plan_refresh_wgs", "dadd_plan_refresh_plan", "dadd_plan_refresh_f16", "dadd_plan_refresh_bf16"}
    assert C.sizeof(L.PlanRefreshDesc) == 112 and L.PlanRefreshDesc.dst.offset == 32 and L.PlanRefreshDesc.kind.offset == 80


# ----------------------------------------------------------------------------------------------- executor vs packers
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_executor_reproduces_every_packer(dtype):
    """Every kind at the shapes of the kernel test: bit-equal to the packer of ``engine`` for COPY32, CAST, GEGLU, UPSFOLD,
    the streams and LNFOLD's w16; c1 / bias (summed in the kernel's order, not torch's) inside the bound."""
    cases = REF.Cases(dtype)
    pr = O.PlanRefresh(None, cases.arena, cases.recipes)
    assert pr.n_launches == 1 and set(pr.items) == {dtype}
    REF.execute(pr, cases.arena.p)
    bad, worst, name = cases.compare()
    print(f"{dtype}: worst share of the c1 / bias bound {worst:.3g} ({name})")
    assert bad == [] and worst <= 1.0
    assert len(cases.expect) >= (30 if dtype == F16 else 27)


def test_executor_is_sensitive():
    """The comparison can fail: a single-rounded LNFOLD weight or a swapped UPSFOLD tap set is seen."""
    cases = REF.Cases(F16)
    pr = O.PlanRefresh(None, cases.arena, cases.recipes)
    REF.execute(pr, cases.arena.p)
    cases.dst["ups.8.8"][0, 0, 0] += 1.0
    cases.dst["ln.24.c1"][3] *= 1.0 + 2.0 ** -20
    bad, worst, _ = cases.compare()
    assert bad == ["ups.8.8"] and worst > 1.0


# ----------------------------------------------------------------------------------------------- the rounding pin
@pytest.mark.parametrize("dtype,half_ulp", [(F16, 2.0 ** -11), (BF16, 2.0 ** -8)], ids=["fp16", "bf16"])
def test_float64_goes_to_16_bits_through_fp32(dtype, half_ulp):
    """``fold_layernorm`` and ``fold_ups_weight`` end in ``float64_tensor.to(16-bit type)``.  torch converts through fp32
    (two roundings), and the kernel restates exactly that.  On values a hair above a tie of the 16-bit grid the two
    candidate sequences differ: direct rounding goes up; rounding to fp32 first loses the hair (2^-30, below half an fp32
    spacing) and the tie then goes to the even neighbour.  A torch that changes this must change the kernel with it."""
    spacing = 2.0 * half_ulp                                         # of the 16-bit grid in [1, 2)
    m = 1.0 + 2.0 * torch.arange(8, dtype=F64) * spacing             # even last bit: a tie above m goes back to m
    x = m + half_ulp + 2.0 ** -30
    x, m = torch.cat([x, -x]), torch.cat([m, -m])
    through_fp32, direct = m.to(dtype), (m + torch.sign(m) * spacing).to(dtype)
    assert torch.equal(through_fp32.double(), m) and torch.equal(direct.double(), m + torch.sign(m) * spacing)
    got = x.to(dtype)
    assert torch.equal(got, x.to(F32).to(dtype)) and torch.equal(got, through_fp32)
    assert not bool((got == direct).any())
    # the two spot values
    assert torch.tensor(1 + 2.0 ** -11 + 2.0 ** -30, dtype=F64).to(F16).item() == 1.0
    assert torch.tensor(1 + 2.0 ** -8 + 2.0 ** -30, dtype=F64).to(BF16).item() == 1.0


@pytest.mark.parametrize("dtype,half_ulp", [(F16, 2.0 ** -11), (BF16, 2.0 ** -8)], ids=["fp16", "bf16"])
def test_packers_and_executor_round_twice(dtype, half_ulp):
    """... and the two packers inherit it, on fp32 masters.  W * gamma = (1 + h + 2^-23)(1 - 2^-24) lies above the 16-bit
    tie 1 + h and a hair below the fp32 midpoint 1 + h + 2^-24: fp32 takes it to 1 + h, the 16-bit tie then goes to 1.0,
    where one rounding gives 1 + 2 h.  The taps 1, h, 2^-24 sum to 1 + h + 2^-24: an fp32 tie (to even: 1 + h), then the
    16-bit tie.  The executor, which restates the kernel, lands on the same bits."""
    h = half_ulp
    w = torch.zeros(8, 72)
    w[:, 0] = 1.0 + h + 2.0 ** -23
    gamma, beta = torch.full((72,), 1.0 - 2.0 ** -24), torch.zeros(72)
    w16, c1, bias = E.fold_layernorm(w, None, gamma, beta, dtype)
    assert w16[0, 0].item() == 1.0 and (w.double() * gamma.double())[0, 0].item() > 1.0 + h
    ups = torch.zeros(8, 9 * 8)
    taps = ups.view(8, 3, 3, 8)
    taps[:, 1, 1], taps[:, 1, 2], taps[:, 2, 1] = 1.0, h, 2.0 ** -24
    w4 = E.fold_ups_weight(ups.to(dtype))
    assert w4[0, 0, 3 * 8].item() == 1.0 and w4[0, 0, 3 * 8].item() != 1.0 + 2 * h
    T = OrderedDict(w=w, gamma=gamma, beta=beta, ups=ups)
    arena = O.ParamArena(T, {k: 0 for k in T})
    nan = lambda *shape, dt=dtype: torch.full(shape, float("nan"), dtype=dt)            # noqa: E731
    recipes = [E.Recipe("lnfold", (["w"], None, "gamma", "beta"), (nan(8, 72), nan(8, dt=F32), nan(8, dt=F32))),
               E.Recipe("upsfold", ("ups",), (nan(4, 8, 32),))]
    REF.execute(O.PlanRefresh(None, arena, recipes), arena.p)
    assert torch.equal(recipes[0].dst[0], w16) and torch.equal(recipes[0].dst[1], c1) and torch.equal(recipes[0].dst[2], bias)
    assert torch.equal(recipes[1].dst[0], w4)


# ----------------------------------------------------------------------------------------------- the table check
def _desc(kind, n, k=0, cs=0, flags=0, src=(0,), dst=((0x10000, 1 << 30),)):
    return dict(kind=kind, N=n, K=k, Cs=cs, flags=flags, src=list(src), dst=list(dst))


def test_table_check_accepts_and_rejects():
    numel = 1 << 22
    good = [_desc("CAST", 16, 72, 72, src=[0], dst=[(0x10000, 16 * 72)]),
            _desc("COPY32", 5, src=[3], dst=[(0x20004, 5)]),
            _desc("LNFOLD", 24, 72, src=[4096, 8, 80, -1], dst=[(0x30000, 24 * 72), (0x40000, 24), (0x40060, 24)]),
            _desc("LNFOLD", 256, 72, flags=1, src=[4096, 8, 80, 160], dst=[(0x50000, 256 * 72), (0x60000, 256), (0x60400, 256)]),
            _desc("CAST", 72, 8, 4, src=[1], dst=[(0x70000, 72 * 8)]),
            _desc("GEGLU_W", 256, 8, src=[0], dst=[(0x80000, 2048)]),
            _desc("UPSFOLD", 8, 8, src=[0], dst=[(0x90000, 16 * 64)]),
            _desc("HEAD_STREAM", 320, 320, src=[0, 102400, 204800, 307200], dst=[(0x100000, 409600)]),
            _desc("FFN_STREAM", 2560, 320, src=[0, 819200, 1228800], dst=[(0x200000, 1331200)]),
            _desc("FFN_BIAS", 2560, 320, src=[0], dst=[(0x500000, 2560)])]
    table, n_wgs = O.plan_refresh_table(good, numel)
    wgs = [1, 1, 6, 64, 1, 1, 1, 50, 163, 2]
    assert n_wgs == sum(wgs) and [d.wg0 for d in table] == [sum(wgs[:i]) for i in range(len(wgs))]
    lib = L.load()
    assert lib.dadd_plan_refresh_wgs(L.PLAN_REFRESH_LNFOLD, 24, 72, 0, 0) == 6
    for kind, n, k, cs, flags in ((L.PLAN_REFRESH_CAST, 3, 7, 7, 0),            # N * K no multiple of 8
                                  (L.PLAN_REFRESH_CAST, 8, 16, 4, 0),           # padding only to 8
                                  (L.PLAN_REFRESH_GEGLU_W, 64, 8, 0, 0),        # GEGLU rows in whole 128-row tiles
                                  (L.PLAN_REFRESH_GEGLU_B, 100, 0, 0, 0),
                                  (L.PLAN_REFRESH_LNFOLD, 24, 72, 0, 1),        # GEGLU order: N a multiple of 128
                                  (L.PLAN_REFRESH_LNFOLD, 24, 12, 0, 0),        # K a multiple of 8
                                  (L.PLAN_REFRESH_UPSFOLD, 8, 12, 0, 0),
                                  (L.PLAN_REFRESH_HEAD_STREAM, 320, 640, 0, 0),  # the streams exist for C = 320 only
                                  (L.PLAN_REFRESH_FFN_STREAM, 2560, 1280, 0, 0),
                                  (L.PLAN_REFRESH_FFN_BIAS, 2560, 0, 0, 0),
                                  (L.PLAN_REFRESH_COPY32, 0, 0, 0, 0), (9, 8, 8, 8, 0), (L.PLAN_REFRESH_CAST, 8, 8, 8, 1)):
        assert lib.dadd_plan_refresh_wgs(kind, n, k, cs, flags) == -1, (kind, n, k, cs, flags)

    def rejected(items, word):
        with pytest.raises(ValueError) as e:
            O.plan_refresh_table(items, numel)
        assert word in str(e.value), str(e.value)
    cast = good[0]
    rejected([cast, _desc("CAST", 8, 8, 8, dst=[(0x10000 + 16 * 72 * 2 - 16, 64)])], "overlap")          # one vector into the first
    rejected([good[2], _desc("COPY32", 4, dst=[(0x40000 + 23 * 4, 4)])], "overlap")                          # into LNFOLD's c1
    rejected([_desc("CAST", 16, 72, 72, dst=[(0x10008, 16 * 72)])], "misaligned")                            # 16-bit destination
    rejected([_desc("CAST", 16, 72, 72, src=[2], dst=[(0x10000, 16 * 72)])], "misaligned")                   # source, 4 elements
    rejected([_desc("COPY32", 4, dst=[(0x10002, 4)])], "misaligned")
    rejected([_desc("CAST", 16, 72, 72, src=[numel - 16 * 72 + 4], dst=[(0x10000, 16 * 72)])], "leaves")     # source range
    rejected([_desc("CAST", 16, 72, 72, src=[-4], dst=[(0x10000, 16 * 72)])], "leaves")
    rejected([_desc("CAST", 16, 72, 72, dst=[(0x10000, 16 * 72 - 1)])], "room")                              # destination range
    rejected([_desc("LNFOLD", 24, 72, src=[4096, 8, 80, -1], dst=[(0x30000, 24 * 72), (0x40000, 23), (0x40060, 24)])], "room")
    rejected([_desc("LNFOLD", 24, 72, src=[4096, 8, 80, -1], dst=[(0x30000, 24 * 72), (0, 24), (0x40060, 24)])], "null")
    rejected([_desc("HEAD_STREAM", 320, 640, src=[0, 0, 0, 0], dst=[(0x100000, 409600)])], "contract")
    rejected([_desc("GEGLU_W", 200, 8, dst=[(0x80000, 1600)])], "contract")
    with pytest.raises(ValueError):
        O.plan_refresh_table([], numel)
    with pytest.raises(ValueError):
        O.plan_refresh_table([_desc("TRANSPOSE", 8)], numel)


# ----------------------------------------------------------------------------------------------- recipes of a plan
@pytest.fixture(scope="module")
def full_sd():
    shapes = dict(W.unet_shapes())
    shapes.update(W.conditioning_shapes(clip_hidden=64, clip_proj=32))
    return W.init_state_dict(shapes, 0, gates=GATES, warm_start_dis=False)


def _trained_unet_keys():
    return [k for k in W.unet_shapes() if not k.endswith(("processor.anat_gate", "processor.dis_gate"))]


@pytest.mark.parametrize("fusions", [False, True], ids=["generic", "rowblock"])
@pytest.mark.parametrize("gates", [True, False], ids=["gates", "baseline"])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_every_weight_upload_has_a_recipe(full_sd, dtype, gates, fusions, monkeypatch):
    """``unrefreshable`` is empty and every trained key feeds at least one recipe; recording leaves the op list alone."""
    if fusions:
        monkeypatch.setattr(E, "FFN_MIN_BLOCKS", 1)
        monkeypatch.setattr(E, "A2_MIN_TILES", 1)
        monkeypatch.setattr(E, "GN_FUSED_MAX_BYTES", 0)
    plan = E.UNetPlan(TorchRefBackend(), full_sd, 1, 16 if fusions else 8, use_routing_gates=gates, dtype=dtype)
    assert plan.unrefreshable == []
    used = {k for r in plan.recipes for k in r.keys()}
    trained = [k for k in _trained_unet_keys() if gates or ".processor." not in k]
    assert [k for k in trained if k not in used] == []
    assert not [k for k in used if k.endswith(("anat_gate", "dis_gate"))]
    kinds = {r.kind for r in plan.recipes}
    assert {"copy32", "cast", "cast_cin8"} <= kinds
    if fusions and dtype == F16:
        assert {"head_stream", "ffn_stream"} <= kinds and (not gates or plan.a2)
    # every destination is one of the plan's persistent tensors (or a slice of one)
    spans = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in plan.keep)
    for r in plan.recipes:
        for d in r.dst:
            assert any(lo <= d.data_ptr() and d.data_ptr() + d.numel() * d.element_size() <= hi for lo, hi in spans), r.kind


def test_vae_plans_record_nothing(full_sd):
    sd = dict(full_sd)
    sd.update(W.init_state_dict(W.vae_shapes(encoder=False), 0))
    plan = E.VaeDecoderPlan(TorchRefBackend(), sd, 1, 8)
    assert plan.frozen and plan.recipes == [] and plan.unrefreshable == []


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_refreshing_a_plan_from_its_own_masters_restores_it(full_sd, dtype, monkeypatch):
    """The whole chain on the CPU: recipes -> ``PlanRefresh`` items -> the executor.  Every destination of a plan (row-block
    fusions and fused attn2 on for fp16) is overwritten with NaN and written again from an arena that holds the state
    dict's masters in the library layout; the packed tensors come back bit-equal, c1 / bias inside the bound of the kernel
    test (``REF.lnfold_bounds``)."""
    monkeypatch.setattr(E, "FFN_MIN_BLOCKS", 1)
    monkeypatch.setattr(E, "A2_MIN_TILES", 1)
    monkeypatch.setattr(E, "GN_FUSED_MAX_BYTES", 0)
    plan = E.UNetPlan(TorchRefBackend(), full_sd, 1, 16, dtype=dtype)
    masters = OrderedDict((k, v) for k, v in UG.masters_from_state_dict(full_sd).items()
                          if not k.endswith(("anat_gate", "dis_gate")))
    arena = O.ParamArena(masters, {k: 0 for k in masters})
    pr = O.PlanRefresh(None, arena, plan.recipes)
    assert pr.n_launches == (1 if dtype == F16 else 2)          # the time path of a bf16 plan is fp16
    assert F16 in pr.items and any(it["kind"] == "CAST" for it in pr.items[F16])
    n, worst = REF.restore_check(plan.recipes, arena, lambda: REF.execute(pr, arena.p))
    print(f"{dtype}: {n} destinations, worst share of the c1 / bias bound {worst:.3g}")
    assert n > 500


def test_conditioning_modules_record_a_recipe_for_every_packed_tensor(full_sd):
    """The three trained conditioning modules on the stand-in backend, after one forward each (packing is lazy): nothing
    unrefreshable, every entry of ``_packed`` and every master is the destination of a recipe (or a view of a master),
    and the executor writes them all back from an arena of the masters.  The CLIP tower is frozen and records nothing."""
    from progressive_stable_diffusion_amd import conditioning as PC
    be, cpu = TorchRefBackend(), torch.device("cpu")
    clip = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, image_size=224,
                patch_size=14, projection_dim=32)
    sd = dict(full_sd)
    sd.update(W.init_state_dict(W.clip_shapes(clip), 0))
    aoe, plus, pur = PC.AdditiveOrdinalEmbedder(sd, cpu, be=be), PC.ImageProjectionPlus(sd, cpu, be=be), PC.FeaturePurifier(sd, cpu, be=be)
    enc = PC.ImageEncoder(sd, cpu, clip_config=clip, be=be)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        tokens = aoe(torch.tensor([1.0, 2.5]))
        img = plus(enc.get_hidden_states(torch.randn(2, 3, 224, 224, generator=g)))
        pur(img, tokens)
    assert enc.frozen and enc.recipes == [] and enc.unrefreshable == [] and enc._packed
    owners = [aoe, plus, pur]
    assert plus._packed and pur._packed and [o.unrefreshable for o in owners] == [[], [], []]
    masters = OrderedDict((f"{o.prefix}.{k}", t) for o in owners for k, t in o.p.items())
    for o in owners:
        dsts = {d.data_ptr() for r in o.recipes for d in r.dst}
        spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in o.p.values()]
        assert all(t.data_ptr() in dsts for t in o.p.values())
        for key, val in o._packed.items():
            for t in (val if isinstance(val, tuple) else (val,)):
                if t is not None:
                    assert t.data_ptr() in dsts or any(lo <= t.data_ptr() < hi for lo, hi in spans), key
        assert {k for r in o.recipes for k in r.keys()} == {f"{o.prefix}.{k}" for k in o.p}
    kinds = {r.kind for o in owners for r in o.recipes}
    assert kinds == {"copy32", "cast", "lnfold"}
    arena = O.ParamArena(OrderedDict((k, t.clone()) for k, t in masters.items()), {k: 0 for k in masters})
    recipes = [r for o in owners for r in o.recipes]
    pr = O.PlanRefresh(None, arena, recipes)
    assert pr.n_launches == 1
    n, worst = REF.restore_check(recipes, arena, lambda: REF.execute(pr, arena.p))
    print(f"conditioning: {n} destinations, worst share of the c1 / bias bound {worst:.3g}")
