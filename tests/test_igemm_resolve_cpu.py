"""CPU check of the planner / launcher contract of ``igemm``: every launch the engine's plans record, and the K/V
projections of ``set_cond``, is put through ``dadd_conv_igemm_resolve_*`` — the validation and the dispatch decisions of
``dadd_conv_igemm_*`` without the launch (csrc/igemm.hip) — with the descriptor ``HipBackend.igemm`` would fill.  Resolve
reads no buffer, so the CPU addresses of the reference backend's tensors stand in for device pointers.  A disagreement
between what ``engine.py`` predicts and what the library decides fails here instead of on a GPU machine."""
import collections
import ctypes as C
import gc
import re

import pytest
import torch

from progressive_stable_diffusion_amd import engine as E
from progressive_stable_diffusion_amd import lib as L
from progressive_stable_diffusion_amd.backend import _sfx, fill_igemm_desc
from tests import plan_cases
from tests.torch_backend import TorchRefBackend

F16, F32 = torch.float16, torch.float32


class Recording(TorchRefBackend):
    """The reference backend, keeping the arguments of every eager ``igemm`` (``set_cond`` calls the backend directly)."""

    def __init__(self):
        super().__init__()
        self.eager = []

    def igemm(self, x, w, out, **kw):
        self.eager.append((x, w, out, kw))
        super().igemm(x, w, out, **kw)


@pytest.fixture(scope="module")
def lib():
    L.build()
    return L.load()


@pytest.fixture(scope="module")
def sds():
    return plan_cases.state_dicts()


def _ptr(t):
    return None if t is None else t.data_ptr()


FIELDS = [f for f, _ in L.IgemmChoice._fields_]


def resolve(lib, sfx, x, w, out, num_cu=E.N_CU, **kw):
    """The ``IgemmChoice`` of one ``igemm`` call as a dict; raises what the launch would raise."""
    d, c = L.IgemmDesc(), L.IgemmChoice()
    fill_igemm_desc(d, _ptr, x, w, out, **kw)
    L.check(getattr(lib, "dadd_conv_igemm_resolve_" + sfx)(C.byref(d), num_cu, C.byref(c)))
    return {f: (v.decode() if isinstance(v := getattr(c, f), bytes) else v) for f in FIELDS}


def check_launch(lib, x, w, out, kw, census):
    g = kw.get("gn_apply")
    sfx = _sfx(x, kw.get("x2"), w, out, kw.get("residual"), None if g is None else g[0])
    c = resolve(lib, sfx, x, w, out, **kw)                     # DADD_OK, or check() raises
    twin = resolve(lib, "bf16" if sfx == "f16" else "f16", x, w, out, **kw)
    for f in FIELDS:                                           # the two builds decide alike; only the names carry the suffix
        a, b = c[f], twin[f]
        if f in ("kernel", "finish") and a is not None:
            a, b = a.replace("_bf16", ""), (b or "").replace("_bf16", "")
            assert ("_bf16" in c[f]) == (sfx == "bf16") and ("_bf16" in twin[f]) == (sfx == "f16"), (c[f], twin[f])
        assert a == b, (f, c, twin)
    what = (tuple(x.shape), tuple(w.shape), {k: v for k, v in kw.items() if not isinstance(v, (torch.Tensor, tuple))}, c)
    # a tile size the planner names is the tile that runs (0 leaves the choice to the library)
    assert kw.get("tile_m", 0) in (0, c["tile_m"]) and kw.get("tile_n", 0) in (0, c["tile_n"]), what
    m, n = out.shape[0] * out.shape[1] * out.shape[2], w.shape[0]
    if c["nsplit"] > 1:
        assert kw.get("partial") is not None and kw["partial"].dtype == F32 and kw["partial"].numel() >= c["nsplit"] * m * n, what
    assert (c["finish"] is not None) == (c["nsplit"] > 1 and kw.get("counters") is None), what
    if c["persistent"]:
        assert (c["grid_x"], c["grid_y"], c["nsplit"]) == (E.N_CU, 1, 1), what
    else:
        assert c["grid_y"] == c["nsplit"], what
    if kw.get("gn_in") is not None:
        assert re.fullmatch(r"conv3x3_halo_kernel(_bf16)?<\d+, false, true>", c["kernel"]), what
    if kw.get("flags", 0) & L.EPI_LNFOLD and kw.get("ln_stats_in") is None:
        assert re.fullmatch(r"igemm_dma_kernel(_bf16)?<\d+, \d+, false, (true|false), 1>", c["kernel"]), what
    census[c["kernel"]] += 1
    if c["finish"]:
        census[c["finish"]] += 1


CASES = [name for name, _, _ in plan_cases.cases(None, None, None, None)]


@pytest.fixture(autouse=True)
def _drop_dead_plans():
    """A plan is a reference cycle (its recorded ops hold its own bound methods) of several GB: collect it right away
    instead of whenever the allocation counters next trigger the collector."""
    yield
    gc.collect()


@pytest.mark.parametrize("case", CASES)
def test_every_planned_igemm_resolves(lib, sds, case):
    (pol, build), = [(p, b) for name, p, b in plan_cases.cases(E, Recording, *sds) if name == case]
    with plan_cases.policy(E, pol):
        plans = build()
    for i, plan in enumerate(plans):
        groups = {"plan.ops": [(a[0], a[1], a[2], k) for fn, a, k in plan.ops if getattr(fn, "__name__", "") == "igemm"]}
        assert groups["plan.ops"]
        if hasattr(plan, "set_cond"):
            plan.be.eager.clear()
            plan.set_cond(torch.zeros(plan.B, plan.T, 768))
            assert len(plan.be.eager) == 16                    # the K/V projections of the 16 cross-attention sites
            groups["set_cond"] = list(plan.be.eager)
        for what, launches in groups.items():                  # the census: kernel name -> launches, per case
            census = collections.Counter()
            for x, w, out, kw in launches:
                check_launch(lib, x, w, out, kw, census)
            print(f"\n{case}[{i}] {what}: {len(launches)} igemm calls")
            for name in sorted(census):
                print(f"  {census[name]:4d}  {name}")


def _t(shape, dtype=F16):
    return torch.zeros(shape, dtype=dtype)


def test_resolve_refuses_what_the_launch_refuses(lib):
    """The requests tests/test_gpu_kernels.py provokes a ValueError with, refused without a GPU."""
    x, w, o = _t((1, 256, 1, 320)), _t((320, 320)), _t((1, 256, 1, 320))
    c1 = _t((320,), F32)
    r = lambda *a, **k: resolve(lib, "f16", *a, **k)           # noqa: E731
    r(x, w, o)                                                 # (the plain request is fine)
    with pytest.raises(ValueError):                            # C % 64 != 0
        r(_t((1, 8, 1, 96)), _t((64, 96)), _t((1, 8, 1, 64)))
    with pytest.raises(ValueError):                            # a folded LayerNorm needs whole rows of A: no split-K
        r(x, w, o, flags=L.EPI_LNFOLD, splitk=2, partial=_t((2 * 256 * 320,), F32), ln_c1=c1)
    with pytest.raises(ValueError):                            # no activation on split-K slabs
        r(x, w, o, flags=L.EPI_GELU, splitk=2, partial=_t((2 * 256 * 320,), F32))
    with pytest.raises(ValueError):                            # the part count must be N / (tile_n / 2)
        r(x, w, o, flags=L.EPI_LNSTAT, tile_m=128, tile_n=160, ln_stats_out=_t((5, 256, 2), F32))
    r(x, w, o, flags=L.EPI_LNSTAT, tile_m=128, tile_n=160, ln_stats_out=_t((4, 256, 2), F32))
    with pytest.raises(ValueError):                            # no row partials of a GEGLU output
        r(x, _t((1024, 320)), _t((1, 256, 1, 512)), flags=L.EPI_LNSTAT | L.EPI_GEGLU, tile_m=128, tile_n=128,
          ln_stats_out=_t((16, 256, 2), F32))
    # GroupNorm on the way in: the 3x3 halo kernel only
    xc, wc, oc = _t((2, 16, 16, 320)), _t((320, 9 * 320)), _t((2, 16, 16, 320))
    gn = (_t((2 * 4 * 64,), F32), 4, _t((320,), F32), _t((320,), F32), 1e-5)
    assert r(xc, wc, oc, taps=9, pad=1, flags=L.PRE_GN, tile_m=128, tile_n=160, gn_in=gn)["kernel"] == "conv3x3_halo_kernel<16, false, true>"
    with pytest.raises(ValueError):                            # not a halo conv: a 1x1
        r(xc, _t((320, 320)), oc, flags=L.PRE_GN, gn_in=gn)
    with pytest.raises(ValueError):                            # two sources need the partials of both
        r(xc, _t((320, 18 * 320)), oc, x2=xc, taps=9, pad=1, flags=L.PRE_GN, tile_m=128, tile_n=160,
          gn_in=(gn[0], 4, _t((640,), F32), _t((640,), F32), 1e-5))
    with pytest.raises(ValueError):                            # ... and group widths that nest: (320 + 192) / 32 = 16 against 10 and 6
        r(xc, _t((320, 9 * 512)), oc, x2=_t((2, 16, 16, 192)), taps=9, pad=1, flags=L.PRE_GN, tile_m=128, tile_n=160,
          gn_in=(gn[0], 4, _t((512,), F32), _t((512,), F32), 1e-5, gn[0], 4))
    # GroupNorm statistics of the output
    ws = _t((2 * 5 * 64,), F32)
    assert r(xc, wc, oc, taps=9, pad=1, flags=L.EPI_GNSTAT, tile_m=128, tile_n=160, gn_ws=ws, gn_nchunk=4)["finish"] is None
    with pytest.raises(ValueError):                            # the chunk count must match the path that writes the partials
        r(xc, wc, oc, taps=9, pad=1, flags=L.EPI_GNSTAT, tile_m=128, tile_n=160, gn_ws=ws, gn_nchunk=5)
    with pytest.raises(ValueError):                            # a ragged tile: M = 2 * 12 * 12 is no multiple of 128
        r(_t((2, 12, 12, 320)), wc, _t((2, 12, 12, 320)), taps=9, pad=1, flags=L.EPI_GNSTAT, tile_m=128, tile_n=160,
          gn_ws=_t((2 * 3 * 64,), F32), gn_nchunk=2)
    # GroupNorm of the output in the finish kernel
    x8, w8, o8, y8 = _t((2, 8, 8, 320)), _t((320, 9 * 320)), _t((2, 8, 8, 320)), _t((2, 8, 8, 320))
    ga = (y8, _t((320,), F32), _t((320,), F32), 1e-5)
    c = r(x8, w8, o8, taps=9, pad=1, flags=L.EPI_GNAPPLY, splitk=4, partial=_t((4 * 128 * 320,), F32), gn_apply=ga)
    assert c["finish"] == "splitk_finish_gnapply_kernel" and c["nsplit"] == 4
    with pytest.raises(ValueError):                            # one K pass: there is no finish kernel to do it
        r(x8, w8, o8, taps=9, pad=1, flags=L.EPI_GNAPPLY, splitk=1, gn_apply=ga)
    with pytest.raises(ValueError):                            # split-K needs its slabs
        d, ch = L.IgemmDesc(), L.IgemmChoice()
        fill_igemm_desc(d, _ptr, x8, w8, o8, taps=9, pad=1, splitk=4)
        L.check(lib.dadd_conv_igemm_resolve_f16(C.byref(d), E.N_CU, C.byref(ch)))


def test_resolve_depends_on_the_cu_count_only_through_the_persistent_ring(lib):
    x, w, o = _t((1, 128 * 33, 1, 320)), _t((320, 320)), _t((1, 128 * 33, 1, 320))       # 33 row tiles x 2 column tiles
    small = resolve(lib, "f16", x, w, o, num_cu=64, flags=L.TUNE_PERSIST, tile_m=128, tile_n=160)
    big = resolve(lib, "f16", x, w, o, num_cu=256, flags=L.TUNE_PERSIST, tile_m=128, tile_n=160)
    assert small["kernel"] == "igemm_dma_kernel<128, 160, false, true, 0>" and (small["persistent"], small["grid_x"]) == (1, 64)
    assert big["kernel"] == "igemm_dma_kernel<128, 160, false, false, 0>" and (big["persistent"], big["grid_x"]) == (0, 66)
