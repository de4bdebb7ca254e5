"""Not-GPU: the host side of the training step - master packing (``unet_grad``), the descriptor table of the one-launch
re-layout and an index-level model of its kernel (tests/relayout_reference.py) against the four torch helpers of
``grad_ops``, the refusals of ``Trainer`` / ``unet_grad`` / the ``prepared=`` keyword, and the binding of
include/dadd_hip_relayout.h."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from progressive_stable_diffusion_amd import grad_ops as G
from progressive_stable_diffusion_amd import lib as L
from progressive_stable_diffusion_amd import optim as O
from progressive_stable_diffusion_amd import training as TR
from progressive_stable_diffusion_amd import unet_grad as UG
from progressive_stable_diffusion_amd import weights as W
from tests import relayout_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "dadd_hip_relayout.h"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
SHAPES = [(8, 8), (16, 72), (72, 16), (136, 200)]          # (N, C): below a tile, ragged both ways, more than one tile


# ---- binding -----------------------------------------------------------------------------------------------------------
def test_header_and_prototype_table_declare_the_same_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    names = set(re.findall(r"\b(dadd_[a-z0-9_]+)\s*\(", text))
    assert names == set(L.RELAYOUT_PROTOTYPES) == {"dadd_relayout_tiles", "dadd_relayout_dst_numel", "dadd_dgrad_relayout_plan",
                                                   "dadd_dgrad_relayout_f16", "dadd_dgrad_relayout_bf16"}
    others = (L.PROTOTYPES, L.HOST_PROTOTYPES, L.GRAD_PROTOTYPES, L.NORM_GRAD_PROTOTYPES, L.ATTN_GRAD_PROTOTYPES,
              L.OPTIM_PROTOTYPES, L.DGRAD_PROTOTYPES, L.END_GRAD_PROTOTYPES, L.COND_GRAD_PROTOTYPES, L.ROWS_GRAD_PROTOTYPES)
    assert not any(names & set(t) for t in others)
    assert L.RELAYOUT_PROTOTYPES["dadd_dgrad_relayout_f16"] == L.RELAYOUT_PROTOTYPES["dadd_dgrad_relayout_bf16"]


def test_entry_points_are_exported_and_the_descriptor_matches_the_header(tmp_path):
    assert {"relayout.hip", "relayout_bf16.hip"} <= set(L.SOURCES)
    handle = ctypes.CDLL(L.build())
    assert not [n for n in L.RELAYOUT_PROTOTYPES if not hasattr(handle, n)]
    fields = [f[0] for f in L.RelayoutDesc._fields_]
    consts = ["DADD_RELAYOUT_T", "DADD_RELAYOUT_S2", "DADD_RELAYOUT_UPS", "DADD_RELAYOUT_COUT4", "DADD_RELAYOUT_TILE"]
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void) {{\n'
                   '  printf("%zu\\n", sizeof(dadd_relayout_desc));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(dadd_relayout_desc, {f}));\n' for f in fields)
                   + "".join(f'  printf("%d\\n", {c});\n' for c in consts) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(L.RelayoutDesc) and out[0] % 8 == 0
    assert out[1:1 + len(fields)] == [getattr(L.RelayoutDesc, f).offset for f in fields]
    assert out[-5:] == [L.RELAYOUT_T, L.RELAYOUT_S2, L.RELAYOUT_UPS, L.RELAYOUT_COUT4, L.RELAYOUT_TILE]
    assert [O.RELAYOUT_KINDS[k] for k in ("T", "S2", "UPS", "COUT4")] == [RR.T, RR.S2, RR.UPS, RR.COUT4] == out[-5:-1]
    assert RR.TILE == L.RELAYOUT_TILE


# ---- master packing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("routing", [True, False])
def test_master_packing_round_trip_is_bit_exact(routing):
    """Every key of ``weights.unet_shapes()`` in its real shape (stand-ins with equal sides would hide a wrong
    permutation), filled with its own flat index; one key at a time, so that the test never holds the whole UNet."""
    shapes = W.unet_shapes(routing_gates=routing)
    for i, (k, s) in enumerate(shapes.items()):
        n = int(np.prod(s)) if s else 1
        v = (torch.arange(n, dtype=F32) * 0.5 + i).reshape(s)
        m = UG.masters_from_state_dict({k: v, "ordinal_embedder.base": torch.ones(8)})     # another prefix: no UNet master
        assert list(m) == [k]
        if len(s) == 4:
            o, c, kh, kw = s
            assert m[k].shape == (o, kh * kw * c) and m[k].is_contiguous()
            assert torch.equal(m[k].reshape(o, kh, kw, c)[o - 1, kh - 1, 0], v[o - 1, :, kh - 1, 0])   # [O][ky][kx][I]
        else:
            assert m[k].shape == tuple(s) and (n == 0 or m[k].data_ptr() != v.data_ptr())
        back = UG.state_dict_from_masters(m)
        assert list(back) == [k] and back[k].shape == v.shape and back[k].dtype == F32 and torch.equal(back[k], v), k
    assert list(UG.masters_from_state_dict({k: torch.zeros(s) for k, s in list(shapes.items())[:40]})) == list(shapes)[:40]
    with pytest.raises(ValueError):
        UG.state_dict_from_masters({"unet.unet.conv_in.weight": torch.zeros(320, 4, 3, 3)})


class _Recorder(dict):
    def __init__(self, *a):
        super().__init__(*a)
        self.read = set()

    def __getitem__(self, k):
        self.read.add(k)
        return super().__getitem__(k)

    def get(self, k, default=None):
        self.read.add(k)
        return super().get(k, default)


def _stub_ops(monkeypatch):
    """Shape-only stand-ins for the operators, so that the wiring of ``unet_forward`` runs without a GPU."""
    def z(*shape):
        return torch.zeros(shape, dtype=F16)
    ops = SimpleNamespace(
        linear=lambda be, x, w, bias=None, prepared=None: z(*x.shape[:-1], w.shape[0]),
        conv3x3=lambda be, x, w, bias=None, stride=1, ups=False, rowvec=None, prepared=None: z(*x.shape[:-1], w.shape[0]),
        downsample2d=lambda be, x, w, bias=None, prepared=None: z(x.shape[0], x.shape[1] // 2, x.shape[2] // 2, w.shape[0]),
        upsample2d=lambda be, x, w, bias=None, prepared=None: z(x.shape[0], x.shape[1] * 2, x.shape[2] * 2, w.shape[0]),
        conv_in=lambda be, x, w, bias=None, dtype=F16: z(x.shape[0], x.shape[2], x.shape[3], w.shape[0]),
        conv_out=lambda be, x, w, bias=None, prepared=None: torch.zeros(x.shape[0], w.shape[0], x.shape[1], x.shape[2]),
        group_norm=lambda be, x, g, b, groups=32, eps=1e-5, silu=False, x2=None: z(*x.shape[:-1], g.shape[0]),
        layer_norm=lambda be, x, g, b, eps=1e-5: z(*x.shape),
        geglu=lambda be, h: z(*h.shape[:-1], h.shape[-1] // 2),
        self_attention=lambda be, qkv, heads: z(*qkv.shape[:-1], qkv.shape[-1] // 3),
        tri_cross_attention=lambda be, q, kv, gates, lam, heads, mode=0: z(*q.shape))

    def time_embedding(be, params, t, proj_keys, dim=320, prefix="unet.unet.time_embedding"):
        for k in (prefix + ".linear_1", prefix + ".linear_2", *proj_keys):
            params[k + ".weight"], params[k + ".bias"]
        return torch.zeros(t.shape[0], sum(params[k + ".weight"].shape[0] for k in proj_keys))
    monkeypatch.setattr(UG, "G", ops)
    monkeypatch.setattr(UG, "CG", SimpleNamespace(time_embedding=time_embedding))


@pytest.mark.parametrize("routing", [True, False])
def test_unet_grad_reads_exactly_the_unet_keys(monkeypatch, routing):
    _stub_ops(monkeypatch)
    shapes = W.unet_shapes(routing_gates=routing)
    lib_shape = {k: ((s[0], s[1] * s[2] * s[3]) if len(s) == 4 else s) for k, s in shapes.items()}
    params = _Recorder({k: torch.zeros(s).expand(s) if not s else torch.zeros(1).expand(s) for k, s in lib_shape.items()})
    out = UG.unet_forward(None, params, torch.zeros(1, 4, 32, 32), torch.tensor([5]), torch.zeros(1, 48 if routing else 32, 768),
                          use_routing_gates=routing)
    assert out.shape == (1, 4, 32, 32)
    assert params.read == set(shapes) == {k for k in shapes if k.startswith("unet.")}
    listed = {e[0]: e[1:] for e in UG.relayout_entries(params)}
    assert all(k.endswith(".weight") and len(shapes[k]) in (2, 4) for k in listed)
    kinds = {k: v[0] for k, v in listed.items()}
    assert sorted(set(kinds.values())) == ["COUT4", "S2", "T", "UPS"]
    assert sum(v == "S2" for v in kinds.values()) == 3 and sum(v == "UPS" for v in kinds.values()) == 3
    assert kinds["unet.unet.conv_out.weight"] == "COUT4" and "unet.unet.conv_in.weight" not in kinds
    assert listed["unet.unet.mid_block.resnets.0.conv1.weight"] == ("T", 9)
    assert listed["unet.unet.up_blocks.0.resnets.0.conv_shortcut.weight"] == ("T", 1)
    assert not any("time_emb" in k for k in kinds)


# ---- the re-layout: model against the torch helpers --------------------------------------------------------------------
def _helper(kind, taps, w16):
    if kind == "T":
        return G.dgrad_weight(w16, taps)
    return {"S2": G.dgrad_weight_stride2, "UPS": G.dgrad_weight_ups, "COUT4": G.dgrad_weight_cout4}[kind](w16)


def _cases():
    out = []
    for n, c in SHAPES:
        out += [("T", 1, n, c), ("T", 9, n, c), ("S2", 9, n, c), ("UPS", 9, n, c)]
    return out + [("COUT4", 9, 4, 8), ("COUT4", 9, 3, 72), ("COUT4", 9, 4, 200), ("COUT4", 9, 1, 16)]


def _weights(cases, dtype, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, taps * c, generator=g).to(dtype) for _, taps, n, c in cases]


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16) if t.dtype == BF16 else t.contiguous().numpy()


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("case", _cases(), ids=lambda c: f"{c[0]}{c[1]}-{c[2]}x{c[3]}")
def test_relayout_model_equals_the_torch_helper(case, dtype):
    kind, taps, n, c = case
    (w,) = _weights([case], dtype)
    want = _helper(kind, taps, w)
    npdt = np.float16 if dtype == F16 else "bf16"
    src = _bits(w).reshape(-1)
    dst = np.full(RR.dst_numel(RR.KIND[kind], taps, n, c), 0x7E01 if dtype == BF16 else np.nan, src.dtype)
    writes = np.zeros(dst.shape, np.int32)
    table, n_tiles = RR.plan([(0, 0, n, c, kind, taps)])
    RR.run(src, dst, table, n_tiles, npdt, writes)
    assert (writes == 1).all()                                # the tiles cover the destination exactly once
    assert dst.shape[0] == want.numel() and np.array_equal(dst.view(np.uint16), _bits(want).reshape(-1).view(np.uint16))


def _mixed_batch(dtype, gap=24):
    """All kinds in one table, the sources packed on 8 elements, ``gap`` elements between (and around) the destinations."""
    cases = _cases()
    ws = _weights(cases, dtype, seed=9)
    items, soff, doff = [], 0, gap
    for (kind, taps, n, c), w in zip(cases, ws):
        items.append((soff, doff, n, c, kind, taps))
        soff += -(-w.numel() // 8) * 8
        doff += -(-RR.dst_numel(RR.KIND[kind], taps, n, c) // 8) * 8 + gap
    return cases, ws, items, soff, doff


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_mixed_batch_with_gaps_and_the_library_plan(dtype):
    cases, ws, items, src_numel, dst_numel = _mixed_batch(dtype)
    table, n_tiles = O.relayout_plan(items, src_numel, dst_numel)
    model, model_tiles = RR.plan(items)
    assert n_tiles == model_tiles and [d.tile0 for d in table] == [d["tile0"] for d in model]
    assert [(d.src_off, d.dst_off, d.N, d.C, d.kind, d.taps) for d in table] == \
        [(d["src_off"], d["dst_off"], d["N"], d["C"], d["kind"], d["taps"]) for d in model]
    src = np.zeros(src_numel, np.uint16)
    for it, w in zip(items, ws):
        src[it[0]:it[0] + w.numel()] = _bits(w).reshape(-1).view(np.uint16)
    src = src.view(np.float16) if dtype == F16 else src
    sentinel = 0x7C55                                         # (a NaN pattern in fp16, a large value in bf16: bits either way)
    dst = np.full(dst_numel, sentinel, np.uint16)
    dst = dst.view(np.float16) if dtype == F16 else dst
    writes = np.zeros(dst_numel, np.int32)
    RR.run(src, dst, model, n_tiles, np.float16 if dtype == F16 else "bf16", writes)
    bits = dst.view(np.uint16)
    covered = np.zeros(dst_numel, bool)
    for (kind, taps, n, c), it, w in zip(cases, items, ws):
        want = _bits(_helper(kind, taps, w)).reshape(-1).view(np.uint16)
        assert np.array_equal(bits[it[1]:it[1] + want.size], want), (kind, taps, n, c)
        covered[it[1]:it[1] + want.size] = True
    assert (writes[covered] == 1).all() and (writes[~covered] == 0).all() and (bits[~covered] == sentinel).all()
    assert (~covered).sum() >= 24 * (len(items) + 1)


def test_plan_refuses_what_the_contract_excludes():
    ok = (0, 0, 16, 24, "T", 9)
    O.relayout_plan([ok], 16 * 9 * 24, 16 * 9 * 24)
    for bad in [(0, 0, 12, 24, "T", 9), (0, 0, 16, 20, "T", 9), (4, 0, 16, 24, "T", 9), (0, 4, 16, 24, "T", 9),
                (0, 0, 16, 24, "T", 3), (0, 0, 16, 24, "S2", 1), (0, 0, 8, 24, "COUT4", 9), (-8, 0, 16, 24, "T", 9)]:
        with pytest.raises(ValueError):
            O.relayout_plan([bad], 1 << 20, 1 << 20)
    with pytest.raises(ValueError):
        O.relayout_plan([ok], 16 * 9 * 24 - 8, 1 << 20)        # the source runs past its array
    with pytest.raises(ValueError):
        O.relayout_plan([ok], 1 << 20, 16 * 9 * 24 - 8)        # the destination runs past its array
    with pytest.raises(ValueError):
        O.relayout_plan([ok, (8, 8, 16, 24, "T", 9)], 1 << 20, 1 << 20)     # overlapping destinations
    with pytest.raises(ValueError):
        O.relayout_plan([(0, 0, 16, 24, "X", 9)], 1 << 20, 1 << 20)
    with pytest.raises(ValueError):
        O.relayout_plan([], 8, 8)
    assert O.relayout_dst_numel("UPS", 9, 16, 24) == 24 * 16 * 16 and O.relayout_dst_numel("COUT4", 9, 4, 24) == 24 * 72


def test_relayout_owner_lays_the_buffer_out_once():
    g = torch.Generator().manual_seed(3)
    t = {"lin.weight": torch.randn(16, 24, generator=g), "lin.bias": torch.randn(16, generator=g),
         "conv.weight": torch.randn(24, 9 * 16, generator=g), "down.weight": torch.randn(8, 9 * 8, generator=g),
         "up.weight": torch.randn(8, 9 * 16, generator=g), "out.weight": torch.randn(4, 9 * 64, generator=g)}
    arena = O.ParamArena(t, {k: 0 for k in t}, working_dtype=F16)
    entries = [("lin.weight", "T"), ("conv.weight", "T", 9), ("down.weight", "S2"), ("up.weight", "UPS"), ("out.weight", "COUT4")]
    r = O.DgradRelayout(None, arena, entries)
    assert r.n_desc == 5 and r.buf.dtype == F16 and r.buf.numel() == r.numel and r.table.numel() == 5 * ctypes.sizeof(L.RelayoutDesc) // 4
    assert r.wt("lin.weight").shape == (24, 16) and r.wt("conv.weight").shape == (16, 9 * 24)
    assert r.wt("down.weight").shape == (8, 72) and r.wt("up.weight").shape == (16, 16 * 8) and r.wt("out.weight").shape == (64, 9, 8)
    for k, _ in [(e[0], e[1]) for e in entries]:
        w16, wt = r.prepared(k)
        assert w16.data_ptr() == arena.param16(k).data_ptr() and wt.data_ptr() % 16 == 0 and wt.is_contiguous()
    # the table the device would read, executed by the model on the arena's own p16
    table = [dict(src_off=d.src_off, dst_off=d.dst_off, N=d.N, C=d.C, kind=d.kind, taps=d.taps, tile0=d.tile0) for d in r._table]
    dst = np.zeros(r.numel, np.float16)
    RR.run(arena.p16.numpy(), dst, table, r.n_tiles)
    for e in entries:
        want = _helper(e[1], e[2] if len(e) > 2 else (1 if e[1] == "T" else 9), arena.param16(e[0]))
        off = r.offsets[e[0]]
        assert np.array_equal(dst[off:off + want.numel()], want.numpy().reshape(-1)), e
    with pytest.raises(RuntimeError):
        r.refresh()
    with pytest.raises(KeyError):
        O.DgradRelayout(None, arena, [("nope", "T")])
    with pytest.raises(ValueError):
        O.DgradRelayout(None, arena, [("lin.bias", "T")])
    with pytest.raises(ValueError):
        O.DgradRelayout(None, arena, [("lin.weight", "T"), ("lin.weight", "T")])
    with pytest.raises(RuntimeError):
        O.DgradRelayout(None, O.ParamArena(t, {k: 0 for k in t}), entries)


# ---- refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [16, 24])
def test_latent_side_that_is_no_multiple_of_32_is_refused(side):
    with pytest.raises(ValueError, match="multiples of 32"):
        UG.unet_forward(None, {}, torch.zeros(1, 4, side, side), torch.tensor([1]), torch.zeros(1, 48, 768))
    mod = SimpleNamespace(latent_side=side)
    with pytest.raises(ValueError, match="multiples of 32"):
        TR.Trainer(mod, 1e-4)


def test_trainer_refuses_bf16_with_a_clear_error():
    with pytest.raises(ValueError, match="fp16"):
        TR.Trainer(SimpleNamespace(latent_side=32), 1e-4, operand_dtype=BF16)


def test_unet_grad_refuses_wrong_operands():
    with pytest.raises(ValueError):
        UG.unet_forward(None, {}, torch.zeros(1, 3, 32, 32), torch.tensor([1]), torch.zeros(1, 48, 768))
    with pytest.raises(ValueError):
        UG.unet_forward(None, {}, torch.zeros(1, 4, 32, 32), torch.tensor([1]), torch.zeros(1, 32, 768))     # split mode: 48
    with pytest.raises(ValueError):
        UG.unet_forward(None, {}, torch.zeros(1, 4, 32, 32), torch.tensor([1]), torch.zeros(1, 48, 768), dtype=F32)


def test_prepared_keyword_refuses_wrong_shape_or_type():
    x, w = torch.zeros(2, 8, 16, dtype=F16), torch.zeros(24, 16)
    good = (torch.zeros(24, 16, dtype=F16), torch.zeros(16, 24, dtype=F16))
    for bad, err in [((good[0], torch.zeros(24, 16, dtype=F16)), ValueError),            # wt not transposed
                     ((torch.zeros(16, 24, dtype=F16), good[1]), ValueError),            # w16 of the wrong shape
                     ((good[0].to(BF16), good[1]), TypeError), ((good[0], good[1].float()), TypeError),
                     ((good[0],), TypeError), (good[0], TypeError), ((good[0], None), TypeError),
                     ((good[0], good[1].t().contiguous().t()), ValueError)]:              # not contiguous
        with pytest.raises(err):
            G.linear(None, x, w, prepared=bad)
    x4, w9 = torch.zeros(1, 4, 4, 16, dtype=F16), torch.zeros(8, 9 * 16)
    w16 = torch.zeros(8, 9 * 16, dtype=F16)
    with pytest.raises(ValueError):
        G.conv3x3(None, x4, w9, prepared=(w16, torch.zeros(16, 8, dtype=F16)))
    with pytest.raises(ValueError):
        G.conv3x3(None, x4.detach(), w9, stride=2, prepared=(w16, torch.zeros(16, 72, dtype=F16)))
    with pytest.raises(ValueError):
        G.upsample2d(None, x4, w9, prepared=(w16, torch.zeros(16, 9 * 8, dtype=F16)))     # UPS takes 16 slabs
    with pytest.raises(ValueError):
        G.downsample2d(None, x4, w9, prepared=(w16, torch.zeros(16, 16 * 8, dtype=F16)))
    with pytest.raises(ValueError):
        G.conv3x3(None, x4, w9, rowvec=torch.zeros(1, 8), prepared=(w16, torch.zeros(16, 9 * 8, dtype=F16).t()))
    xo, wo = torch.zeros(1, 4, 4, 64, dtype=F16), torch.zeros(4, 9 * 64)
    with pytest.raises(ValueError):
        G.conv_out(None, xo, wo, prepared=(torch.zeros(4, 9 * 64, dtype=F16), torch.zeros(64, 9, 4, dtype=F16)))
    with pytest.raises(TypeError):
        G.conv_out(None, xo, wo, prepared=(torch.zeros(4, 9 * 64), torch.zeros(64, 9, 8, dtype=F16)))
