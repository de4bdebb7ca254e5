"""-m gpu: the one-launch refresh of packed plan weights (csrc/plan_refresh.hip) through ``HipBackend.plan_refresh`` and
``optim.PlanRefresh``, against the packers of ``engine`` run on the CPU on the same fp32 sources.

ONE table per 16-bit type holds every case of tests/plan_refresh_reference.py (``Cases``): CAST (8, 1, 8), (16, 9, 72),
(136, 1, 200), three sources into one destination, ``conv_in`` 4 -> 8 channels, ``conv_out`` with 1 to 4 rows; COPY32 of 1,
8 and 200 elements at destination offsets 0, 1, 9; GEGLU (256, 8), (384, 72); LNFOLD (8, 8) without b, (24, 72),
(136, 200), (256, 72) in GEGLU order, two concatenated sources; UPSFOLD (8, 8), (16, 72); the two row-block streams
(fp16 only).  Every permutation kind, UPSFOLD and LNFOLD's w16 must be bit-equal; c1 / bias within
2^-23 |ref| + (K + 2) 2^-52 sum|term|.  Destinations live in one buffer filled with a NaN pattern, 32 guard bytes before,
between and behind them."""
import pytest
import torch

from progressive_stable_diffusion_amd import optim as O
from tests import plan_refresh_reference as REF

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DEV = torch.device("cuda:0")
GAP = 32                   # bytes
SENTINEL = 0x7FC1          # NaN in fp16 and bf16; two of them are an fp32 NaN


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(DEV)


class Guarded:
    """Destinations carved out of one sentinel-filled device buffer, 16-byte aligned, ``GAP`` bytes apart."""

    def __init__(self, nbytes=8 << 20):
        self.buf = torch.full((nbytes // 2,), SENTINEL, dtype=torch.int16, device=DEV)
        self.at, self.spans = GAP, {}

    def __call__(self, name, shape, dtype):
        numel = 1
        for v in shape:
            numel *= v
        size = numel * (4 if dtype == F32 else 2)
        lo = self.at
        self.at = -(-(lo + size + GAP) // 16) * 16
        assert self.at <= self.buf.numel() * 2
        self.spans[name] = (lo, lo + size)
        return self.buf[lo // 2:(lo + size) // 2].view(dtype).view(shape)

    def reset(self):
        self.buf.fill_(SENTINEL)

    def outside_intact(self):
        covered = torch.zeros(self.buf.numel(), dtype=torch.bool)
        for lo, hi in self.spans.values():
            covered[lo // 2:hi // 2] = True
        got = self.buf.cpu()
        return int((~covered).sum()) >= GAP // 2 * (len(self.spans) + 1) and bool((got[~covered] == SENTINEL).all())


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
def test_all_kinds_in_one_launch_against_the_packers(hip, dtype):
    mem = Guarded()
    cases = REF.Cases(dtype, alloc=mem, device=DEV)
    pr = O.PlanRefresh(hip, cases.arena, cases.recipes)
    assert pr.n_launches == 1 and set(pr.tables) == {dtype}
    torch.cuda.synchronize()
    pr.refresh("raw")
    torch.cuda.synchronize()
    bad, worst, name = cases.compare()
    print(f"plan_refresh {dtype}: {len(cases.expect)} destinations, worst share of the c1 / bias bound {worst:.3g} ({name})")
    assert bad == [], bad
    assert worst <= 1.0, (worst, name)
    assert mem.outside_intact(), "a sentinel outside the destinations changed"
    first = mem.buf.cpu()
    # a repeated call and two replays of a captured graph give the same bits
    pr.refresh("raw")
    torch.cuda.synchronize()
    assert torch.equal(mem.buf.cpu(), first)
    hip.graph_begin()
    try:
        pr.launch("raw")
    finally:
        g = hip.graph_end()
    try:
        for _ in range(2):
            mem.reset()
            hip.wait_current()
            hip.graph_launch(g)
            hip.release_to_current()
            torch.cuda.synchronize()
            assert torch.equal(mem.buf.cpu(), first)
    finally:
        hip.graph_destroy(g)
    # a workgroup whose descriptor does not fit the source length writes nothing: the same table over a source cut in
    # the middle leaves every destination either as the full launch wrote it or untouched
    table, n_desc, n_wgs = pr.tables[dtype]
    names = list(cases.tensors)
    cut = cases.arena.offsets[names[len(names) // 2]]
    mem.reset()
    hip.wait_current()
    hip.plan_refresh(cases.arena.p[:cut], table, n_desc, n_wgs, dtype)
    hip.release_to_current()
    torch.cuda.synchronize()
    after = mem.buf.cpu()
    written = untouched = 0
    for it in pr.items[dtype]:
        behind = any(o >= cut for o in it["src"])          # a source that starts behind the cut: the descriptor cannot fit
        for (t, off), n in zip(it["out"], it["writes"]):
            lo = (t.data_ptr() - mem.buf.data_ptr()) // 2 + off * t.element_size() // 2
            hi = lo + n * t.element_size() // 2
            same, blank = torch.equal(after[lo:hi], first[lo:hi]), bool((after[lo:hi] == SENTINEL).all())
            assert same or blank, (it["kind"], it["N"], it["K"])
            if behind:
                assert blank, (it["kind"], it["N"], it["K"], "written although a source lies behind the cut")
            written, untouched = written + same, untouched + blank
    assert written >= 5 and untouched >= 5 and mem.outside_intact()
    assert cases.arena.ema is None
    with pytest.raises(RuntimeError):
        pr.refresh("ema")
    with pytest.raises(ValueError):
        pr.refresh("p16")


def test_recipes_over_one_destination_are_written_once(hip):
    mem = Guarded(1 << 20)
    cases = REF.Cases(BF16, alloc=mem, device=DEV, streams=False)
    pr = O.PlanRefresh(hip, cases.arena, cases.recipes + cases.recipes[:5])      # (overlapping destinations would be refused)
    assert sum(len(v) for v in pr.items.values()) == sum(len(v) for v in O.PlanRefresh(None, cases.arena, cases.recipes).items.values())


def test_backend_refuses_a_malformed_call(hip):
    mem = Guarded(1 << 20)
    cases = REF.Cases(F16, alloc=mem, device=DEV, streams=False)
    pr = O.PlanRefresh(hip, cases.arena, cases.recipes)
    table, n_desc, n_wgs = pr.tables[F16]
    src = cases.arena.p
    for args in ((src.half(), table, n_desc, n_wgs), (src, table[:-1], n_desc, n_wgs), (src, table, n_desc, 0),
                 (src.view(2, -1), table, n_desc, n_wgs), (src, table, n_desc, n_wgs, F32)):
        with pytest.raises(ValueError):
            hip.plan_refresh(*args)
    with pytest.raises(ValueError):
        hip.plan_refresh(src.cpu(), table, n_desc, n_wgs)
    torch.cuda.synchronize()
    assert bool((mem.buf == SENTINEL).all())
