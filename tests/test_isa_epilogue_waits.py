"""Not-GPU: compile the three kernels that end in csrc/igemm_epilogue.h to gfx950 assembly and count, per kernel function,
the vector loads whose next instruction is `s_waitcnt vmcnt(0)` (scripts/epilogue_waits.py).

A load taken where it is used, under a run-time flag test inside the unrolled (row fragment, column block) loops, gets
such a wait of its own; on gfx9 that wait also covers the previous store's acknowledgement, so MI x J of them in a row are
MI x J dependent round trips at the end of every tile.  The epilogue issues its operand loads in batches instead, each
kind under one wave-uniform test, and one wait serves a whole batch.  A small source change (a flag test moved back into
the loop, a bounds test around a load) silently brings the chain back, and nothing else in the suite would notice.

PARENT: the count before the loads were batched (profiles/r12_a_epilogue_waits.txt, same script; it is summed over all
run-time paths of a function).  BOUND: what the batched epilogue measured, plus one.  The condition of the change: no
function keeps more than a quarter of its earlier count - every path is left with O(1), O(MI) or O(J) waits instead of
O(MI J)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("epilogue_waits", os.path.join(ROOT, "scripts", "epilogue_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# kernel<template arguments> -> (PARENT, measured now).  igemm_dma_kernel<BM, BN, UPS, PERS, LNK>, conv3x3_halo_kernel<W, DUO,
# GNIN>, igemm_kernel<BM, BN, DEEP>
COUNTS = {
    "igemm_dma_kernel<128, 128, false, false, 0>": (82, 1), "igemm_dma_kernel<128, 128, false, false, 1>": (50, 1),
    "igemm_dma_kernel<128, 128, false, false, 2>": (45, 1), "igemm_dma_kernel<128, 128, false, true, 0>": (81, 1),
    "igemm_dma_kernel<128, 128, false, true, 1>": (49, 1), "igemm_dma_kernel<128, 128, false, true, 2>": (97, 1),
    "igemm_dma_kernel<128, 128, true, false, 0>": (82, 1), "igemm_dma_kernel<128, 160, false, false, 0>": (102, 1),
    "igemm_dma_kernel<128, 160, false, false, 1>": (62, 1), "igemm_dma_kernel<128, 160, false, false, 2>": (110, 1),
    "igemm_dma_kernel<128, 160, false, true, 0>": (101, 1), "igemm_dma_kernel<128, 160, false, true, 1>": (61, 1),
    "igemm_dma_kernel<128, 160, false, true, 2>": (121, 1), "igemm_dma_kernel<128, 160, true, false, 0>": (102, 1),
    "igemm_dma_kernel<64, 128, false, false, 0>": (42, 1), "igemm_dma_kernel<64, 128, false, false, 1>": (26, 1),
    "igemm_dma_kernel<64, 160, false, false, 0>": (52, 1), "igemm_dma_kernel<64, 160, false, false, 1>": (32, 1),
    "igemm_dma_kernel<64, 64, false, false, 0>": (22, 1), "igemm_dma_kernel<64, 64, false, false, 1>": (14, 1),
    "conv3x3_halo_kernel<16, false, false>": (106, 1), "conv3x3_halo_kernel<16, false, true>": (106, 1),
    "conv3x3_halo_kernel<16, true, false>": (101, 1), "conv3x3_halo_kernel<32, false, false>": (106, 1),
    "conv3x3_halo_kernel<32, false, true>": (106, 1), "conv3x3_halo_kernel<32, true, false>": (101, 1),
    "conv3x3_halo_kernel<64, false, false>": (106, 1), "conv3x3_halo_kernel<64, false, true>": (106, 1),
    "conv3x3_halo_kernel<64, true, false>": (101, 1),
    "igemm_kernel<128, 128, false>": (101, 1), "igemm_kernel<128, 128, true>": (101, 1), "igemm_kernel<128, 160, false>": (126, 1),
    "igemm_kernel<64, 128, false>": (45, 1), "igemm_kernel<64, 128, true>": (45, 1), "igemm_kernel<64, 160, false>": (56, 1),
    "igemm_kernel<64, 160, true>": (56, 1),
}


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    ew = _script()
    if not os.path.exists(ew.HIPCC):
        pytest.skip("hipcc not available")
    got = {}
    for name in ew.DEFAULT:
        text = ew.compile_asm(name, str(tmp_path_factory.mktemp("isa_waits") / f"{name}.s"))
        for short, _, loads, stores, drained in ew.table(text):
            got[short] = (loads, stores, drained)
    return got


def test_every_kernel_is_counted(counts):
    main = {k for k in counts if not k.startswith("splitk_finish")}
    assert main == set(COUNTS), sorted(main ^ set(COUNTS))
    for k in main:                  # the count sees an epilogue at all: every kernel loads operands and stores outputs
        assert counts[k][0] >= 20 and counts[k][1] >= 19, (k, counts[k])


@pytest.mark.parametrize("kernel", sorted(COUNTS))
def test_loads_followed_by_a_full_wait(counts, kernel):
    parent, measured = COUNTS[kernel]
    bound = measured + 1
    assert 4 * bound <= parent, (kernel, "the bound itself must stay within a quarter of the earlier count")
    drained = counts[kernel][2]
    print(f"{kernel}: {drained} loads directly followed by vmcnt(0) (bound {bound}, before the batching {parent})")
    assert drained <= bound, (kernel, drained, bound)


def test_split_k_finish_kernels_are_unchanged(counts):
    """They run many waves per SIMD and were left as they are: 3 to 12 such pairs each."""
    fin = {k: v[2] for k, v in counts.items() if k.startswith("splitk_finish")}
    assert len(fin) == 7 and all(v <= 12 for v in fin.values()), fin
