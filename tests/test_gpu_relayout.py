"""-m gpu: the one-launch re-layout of the data-gradient weights (csrc/relayout.hip) through ``HipBackend.dgrad_relayout``
and ``optim.DgradRelayout``, bit for bit against the torch helpers of ``grad_ops`` (the UPS kind's fp32 sums included), and
the ``prepared=`` keyword of the ``grad_ops`` products against the same calls without it.

The re-layout cases are those of tests/test_train_cpu.py - (N, C) = (8, 8), (16, 72), (72, 16), (136, 200) in every kind,
COUT4 with 1 to 4 rows - plus one 1280 x 1280 T tensor and one 320-channel UPS tensor, all kinds in ONE launch, fp16 and
bf16.  The destination is NaN-filled; 24 sentinel elements stand before, between and behind the destinations."""
import numpy as np
import pytest
import torch

from progressive_stable_diffusion_amd import grad_ops as G
from progressive_stable_diffusion_amd import optim as O
from tests import relayout_reference as RR
from tests.test_train_cpu import _cases, _helper, _weights

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DEV = torch.device("cuda:0")
GAP = 24
SENTINEL = 0x7E5A          # a NaN pattern in both 16-bit types that no rounding of a sum produces


@pytest.fixture(scope="module")
def hip():
    from progressive_stable_diffusion_amd.backend import HipBackend
    return HipBackend(DEV)


def _batch(dtype):
    cases = _cases() + [("T", 1, 1280, 1280), ("UPS", 9, 320, 320)]
    ws = _weights(cases, dtype, seed=13)
    items, soff, doff = [], 0, GAP
    for (kind, taps, n, c), w in zip(cases, ws):
        items.append((soff, doff, n, c, kind, taps))
        soff += -(-w.numel() // 8) * 8
        doff += -(-RR.dst_numel(RR.KIND[kind], taps, n, c) // 8) * 8 + GAP
    src = torch.zeros(soff, dtype=dtype)
    for it, w in zip(items, ws):
        src[it[0]:it[0] + w.numel()] = w.reshape(-1)
    return cases, ws, items, src, doff


def _table(table):
    import ctypes
    words = torch.frombuffer(bytearray(bytes(table)), dtype=torch.int32)
    assert words.numel() == len(table) * ctypes.sizeof(table[0]) // 4
    return words.to(DEV)


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_all_kinds_in_one_launch_bit_equal_to_the_torch_helpers(hip, dtype):
    cases, ws, items, src, dst_numel = _batch(dtype)
    table, n_tiles = O.relayout_plan(items, src.numel(), dst_numel)
    model, model_tiles = RR.plan(items)
    assert n_tiles == model_tiles
    src_d, table_d = src.to(DEV), _table(table)
    dst = torch.full((dst_numel,), SENTINEL, dtype=torch.int16, device=DEV).view(dtype)
    torch.cuda.synchronize()

    def launch():
        hip.wait_current()
        hip.dgrad_relayout(src_d, dst, table_d, len(items), n_tiles)
        hip.release_to_current()

    launch()
    torch.cuda.synchronize()
    got = dst.cpu().view(torch.int16)
    covered = torch.zeros(dst_numel, dtype=torch.bool)
    for (kind, taps, n, c), it, w in zip(cases, items, ws):
        want = _helper(kind, taps, w.to(DEV)).cpu().reshape(-1).view(torch.int16)      # the helper as the step runs it
        assert torch.equal(_helper(kind, taps, w).reshape(-1).view(torch.int16), want), ("helper, host vs device", kind, n, c)
        bad = (got[it[1]:it[1] + want.numel()] != want).nonzero()
        assert bad.numel() == 0, (kind, taps, n, c, bad[:4].flatten().tolist(), bad.numel())
        covered[it[1]:it[1] + want.numel()] = True
    assert (~covered).sum() >= GAP * (len(items) + 1)
    assert bool((got[~covered] == torch.tensor(SENTINEL, dtype=torch.int16)).all()), "a sentinel outside the destinations changed"
    # a repeated call and two replays of a captured graph give the same bits
    first = got.clone()
    launch()
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu().view(torch.int16), first)
    hip.graph_begin()
    hip.dgrad_relayout(src_d, dst, table_d, len(items), n_tiles)
    g = hip.graph_end()
    try:
        for _ in range(2):
            with torch.cuda.stream(torch.cuda.current_stream()):
                dst.view(torch.int16).fill_(SENTINEL)
            hip.wait_current()
            hip.graph_launch(g)
            hip.release_to_current()
            torch.cuda.synchronize()
            assert torch.equal(dst.cpu().view(torch.int16), first)
    finally:
        hip.graph_destroy(g)


def test_backend_refuses_a_malformed_call(hip):
    src, dst = torch.zeros(64, dtype=F16, device=DEV), torch.zeros(64, dtype=F16, device=DEV)
    table, n_tiles = O.relayout_plan([(0, 0, 8, 8, "T", 1)], 64, 64)
    t = _table(table)
    with pytest.raises(ValueError):
        hip.dgrad_relayout(src, dst.to(BF16), t, 1, n_tiles)
    with pytest.raises(ValueError):
        hip.dgrad_relayout(src, dst, t[:-1], 1, n_tiles)
    with pytest.raises(ValueError):
        hip.dgrad_relayout(src, dst, t, 1, 0)
    with pytest.raises(ValueError):
        hip.dgrad_relayout(src, src, t, 1, n_tiles)
    with pytest.raises(ValueError):
        hip.dgrad_relayout(src.cpu(), dst, t, 1, n_tiles)


# ---- prepared weights ----------------------------------------------------------------------------------------------------
def _r(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _ops():
    """name -> (kind, taps, master, bias, x, call(be, x, w, b, prepared)).  The smallest shapes the products take: C a
    multiple of 64 (and N too where the data gradient is the forward kernel on dy), N = 72 for the resampling convs, odd
    maps, more than one workgroup of every kernel."""
    row = _r((2, 128), 7)
    return {
        "linear": ("T", 1, _r((128, 64), 1, 64 ** -0.5), _r((128,), 2, 0.1), _r((2, 50, 64), 3).half(),
                   lambda be, x, w, b, p: G.linear(be, x, w, b, prepared=p)),
        "conv3x3": ("T", 9, _r((128, 9 * 64), 4, 576 ** -0.5), _r((128,), 5, 0.1), _r((2, 9, 11, 64), 6).half(),
                    lambda be, x, w, b, p: G.conv3x3(be, x, w, b, prepared=p)),
        "conv3x3 rowvec": ("T", 9, _r((128, 9 * 64), 4, 576 ** -0.5), _r((128,), 5, 0.1), _r((2, 9, 11, 64), 6).half(),
                           lambda be, x, w, b, p: G.conv3x3(be, x, w, b, rowvec=row.to(x.device), prepared=p)),
        "downsample2d": ("S2", 9, _r((72, 9 * 64), 8, 576 ** -0.5), _r((72,), 9, 0.1), _r((2, 9, 11, 64), 10).half(),
                         lambda be, x, w, b, p: G.downsample2d(be, x, w, b, prepared=p)),
        "upsample2d": ("UPS", 9, _r((72, 9 * 64), 11, 576 ** -0.5), _r((72,), 12, 0.1), _r((2, 5, 7, 64), 13).half(),
                       lambda be, x, w, b, p: G.upsample2d(be, x, w, b, prepared=p)),
        "conv_out": ("COUT4", 9, _r((4, 9 * 64), 14, 576 ** -0.5), _r((4,), 15, 0.1), _r((2, 9, 11, 64), 16).half(),
                     lambda be, x, w, b, p: G.conv_out(be, x, w, b, prepared=p)),
    }


def _run(be, call, x, w, b, prepared, seed):
    xd, wd, bd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = call(be, xd, wd, bd, prepared)
    dy = _r(tuple(y.shape), seed).to(DEV).to(y.dtype)
    y.backward(dy)
    torch.cuda.synchronize()
    return [t.detach().cpu() for t in (y, xd.grad, wd.grad, bd.grad)]


@pytest.fixture(scope="module")
def prepared_arena(hip):
    ops = _ops()
    tensors = {}
    for name, (kind, taps, w, b, x, call) in ops.items():
        tensors[name + ".weight"], tensors[name + ".bias"] = w, b
    arena = O.ParamArena(tensors, {k: 0 for k in tensors}, device=DEV, working_dtype=F16)
    owner = O.DgradRelayout(hip, arena, [(name + ".weight", kind, taps) for name, (kind, taps, *_r_) in ops.items()])
    owner.refresh()
    torch.cuda.synchronize()
    return ops, arena, owner


@pytest.mark.parametrize("name", list(_ops()))
def test_outputs_and_gradients_are_bit_equal_with_and_without_prepared(hip, prepared_arena, name):
    ops, arena, owner = prepared_arena
    kind, taps, w, b, x, call = ops[name]
    w16, wt = owner.prepared(name + ".weight")
    assert torch.equal(w16.cpu(), w.half()) and torch.equal(wt.cpu(), _helper(kind, taps, w.half()))
    plain = _run(hip, call, x, w, b, None, 21)
    prep = _run(hip, call, x, w, b, (w16, wt), 21)
    for what, a, p in zip(("y", "dx", "dw", "db"), plain, prep):
        assert a.dtype == p.dtype and a.shape == p.shape and torch.isfinite(a.float()).all(), (name, what)
        assert torch.equal(a, p), (name, what, (a.float() - p.float()).abs().max().item())


def test_gradients_reach_the_arena_and_a_refresh_follows_the_optimizer_step(hip, prepared_arena):
    """Masters attached to the arena accumulate in place; after ``FusedAdamW.step`` and ``refresh()`` the next forward on
    the prepared weights equals, bit for bit, a forward that casts the updated masters."""
    ops, arena, owner = prepared_arena
    fused = O.FusedAdamW(hip, arena, [{"lr": 1e-2, "weight_decay": 0.01}])
    leaves = {k: torch.empty(0, device=DEV).requires_grad_(True) for k in arena.names}
    for k, t in leaves.items():
        t.data = arena.param(k)
    arena.attach(leaves)
    before = arena.p.clone()
    for name, (kind, taps, w, b, x, call) in ops.items():
        y = call(hip, x.to(DEV), leaves[name + ".weight"], leaves[name + ".bias"], owner.prepared(name + ".weight"))
        y.float().square().mean().backward()
    torch.cuda.synchronize()
    for k in arena.names:
        assert leaves[k].grad.data_ptr() == arena.grad(k).data_ptr() and bool(arena.grad(k).any()), k
    fused.step()
    owner.refresh()
    torch.cuda.synchronize()
    assert bool((arena.p != before).any())
    assert torch.equal(arena.p16, arena.p.half())
    for name, (kind, taps, w, b, x, call) in ops.items():
        k = name + ".weight"
        assert bool((arena.param(k) != before[arena.offsets[k]:arena.offsets[k] + w.numel()].view_as(w)).any()), k
        assert torch.equal(owner.wt(k), _helper(kind, taps, arena.param(k).half())), k
        with torch.no_grad():
            got = call(hip, x.to(DEV), arena.param(k), arena.param(name + ".bias"), owner.prepared(k))
            want = call(hip, x.to(DEV), arena.param(k).clone(), arena.param(name + ".bias").clone(), None)
        torch.cuda.synchronize()
        assert torch.equal(got, want), name
