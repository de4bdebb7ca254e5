"""Not-GPU guards of tests/attention_cases.py, the helper behind tests/test_gpu_attention_edges.py:
  * the variant table covers exactly what dadd_init_attention() registers (fp16 and bf16 reading of the source), so an
    instantiation added without a row fails here;
  * every input builder gives finite operands whose logits land where the pattern promises;
  * the `model` reference (float64 with the kernel's two rounding points) stays within the project's bound of the
    `exact` one on its own, so the reference does not eat the bound the GPU test applies to the kernel.
"""
import pytest
import torch

from tests import attention_cases as AC

F16, BF16 = torch.float16, torch.bfloat16
DIMS = {F16: (40, 64, 80, 96, 160, 512), BF16: (40, 80, 160)}
_DT = [pytest.param(dt, d, id=f"{'bf16' if dt == BF16 else 'f16'}-d{d}") for dt in (F16, BF16) for d in DIMS[dt]]
B, HEADS, NQ = 1, 2, 48


@pytest.fixture(scope="module", autouse=True)
def one_thread():
    """The tensors here are tiny: a thread pool per operation costs fifty times the arithmetic."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_variant_table_matches_registered_instantiations(dtype):
    reg = AC.registered_variants(dtype)
    table = {v.key for v in AC.VARIANTS[dtype]}
    assert len(table) == len(AC.VARIANTS[dtype]), "a variant is listed twice"
    assert not (table & set(AC.NOT_REACHED_IN_PROCESS))
    assert reg == table | set(AC.NOT_REACHED_IN_PROCESS), (sorted(reg - table - set(AC.NOT_REACHED_IN_PROCESS)),
                                                            sorted((table | set(AC.NOT_REACHED_IN_PROCESS)) - reg))
    assert {v.d for v in AC.VARIANTS[dtype]} == set(DIMS[dtype])
    for v in AC.VARIANTS[dtype]:          # the rows really ask for the instantiation they name (rules of dadd_attn_f16)
        if v.d == 40:
            assert (v.b * v.heads * ((v.nq + 255) // 256) >= 512) == (v.nw == 8), v
        if v.d == 160:
            assert (v.b * v.heads * ((v.nq + 127) // 128) >= 256) == (v.qf == 2), v


def test_registered_variants_reads_both_storage_types():
    f16, bf16 = AC.registered_variants(F16), AC.registered_variants(BF16)
    assert bf16 < f16 and (512, 1, False, 4) in f16 - bf16 and (40, 2, True, 8) in bf16
    assert AC.Variant(40, 2, True, 8, 1, 64, 2011).kernel_name(BF16) == "flash_kernel_bf16<40, 2, true, 8>"
    assert AC.Variant(160, 1, True, 4, 2, 8, 200).kernel_name(F16) == "flash_kernel<160, 1, true>"


def _spread(a):
    """Six sigma of  (0.5 r + a u) . (0.5 r') / sqrt(d)  plus the r . r' part."""
    return 6.0 * (0.5 * a + 0.3)


@pytest.mark.parametrize("nk", [37, 64, 300, 1041])
@pytest.mark.parametrize("dtype,d", _DT)
def test_builders_place_the_logits(dtype, d, nk):
    for pattern, arg in AC.flash_patterns(nk):
        q, k, v = AC.build(pattern, arg, B, HEADS, d, NQ, nk, dtype, seed=3)
        assert q.dtype == k.dtype == v.dtype == dtype and q.shape == (B, NQ, HEADS * d) and k.shape == v.shape == (B, nk, HEADS * d)
        assert all(bool(torch.isfinite(t.float()).all()) for t in (q, k, v)), (pattern, arg)
        ex, s2 = AC.exact_logits(q, k, HEADS), AC.model_logits(q, k, HEADS)        # natural / log2 units
        nt = (nk + AC.TILE - 1) // AC.TILE
        what = f"{pattern}({arg}) d{d} nk{nk}"
        if pattern in ("first_tile_floor", "all_floor"):
            L = float(arg)
            a = AC.amplitude(L, d)
            nfloor = nk if pattern == "all_floor" else min(nk, AC.TILE)
            lo = ex[..., :nfloor]
            tol = 0.02 * L + 2.0 * _spread(a)          # both operands carry a random part here; 2 % for bf16 operands
            assert float((lo + L).abs().max()) <= tol, (what, float(lo.min()), float(lo.max()))
            if nfloor < nk:
                assert float(ex[..., nfloor:].abs().max()) <= _spread(a), what
            first_max = s2[..., :min(nk, AC.TILE)].max(dim=-1).values          # tile 0's column maximum, log2 units
            if L >= 100:       # below -128 the unfixed kernel's exp2(-dlt) was +inf: most rows must be there
                assert float((first_max < -128.0).double().mean()) > 0.5, (what, float(first_max.max()))
            else:              # the finite neighbour
                assert float(first_max.min()) > -126.0, (what, float(first_max.min()))
        elif pattern == "one_hot":
            p, a = int(arg) % nk, AC.amplitude(150.0, d)
            others = torch.cat([ex[..., :p], ex[..., p + 1:]], dim=-1)
            assert float((ex[..., p] - 150.0).abs().max()) <= 3.0 + 2.0 * _spread(a), what
            if others.numel():
                assert float(others.abs().max()) <= _spread(a), what
        elif pattern == "flat":
            assert float(ex.abs().max()) == 0.0 and float(s2.abs().max()) == 0.0
        elif pattern in ("staircase", "descending"):
            delta = float(arg)
            pos = AC.step_positions(nk)
            tmax = torch.stack([s2[..., t * AC.TILE:min(nk, (t + 1) * AC.TILE)].max(dim=-1).values for t in range(nt)], dim=-1)
            assert torch.equal(tmax, s2[..., pos]), what                  # the step key IS the tile's maximum
            if nt > 1:
                step = tmax[..., 1:] - tmax[..., :-1]
                if pattern == "descending":
                    step = -step
                assert float((step - delta).abs().max()) < 0.1, (what, float(step.min()), float(step.max()))
                # a step of 7.5 stays below the re-centring threshold, one of 8.5 above it
                assert bool(((step > AC.RECENTRE) == (delta > AC.RECENTRE)).all()), what
            rest = s2.clone()             # the other keys of a tile sit 1 .. 6 log2 units below its step key
            rest[..., pos] = float("-inf")
            gap = tmax - torch.stack([rest[..., t * AC.TILE:min(nk, (t + 1) * AC.TILE)].max(dim=-1).values for t in range(nt)], dim=-1)
            assert 0.9 < float(gap.min()) and float(gap.max()) < 6.1, (what, float(gap.min()), float(gap.max()))
        exact, model = AC.references(q, k, v, HEADS)
        assert bool(torch.isfinite(exact).all()) and bool(torch.isfinite(model).all()), what
        ok, msg = AC.within(model, exact, dtype)
        assert ok, f"{what}: model against exact: {msg}"
        if pattern == "one_hot":
            want = v[:, int(arg) % nk][:, None, :].double().expand(-1, NQ, -1)
            assert torch.equal(model, want) and float((exact - want).abs().max()) < 1e-12, what
        if pattern == "flat":
            hv = v.double().reshape(B, nk, HEADS * d).mean(dim=1, keepdim=True)
            assert float((exact - hv).abs().max()) < 1e-12 and float((model - hv).abs().max()) < 1e-12, what


def test_references_in_chunks_agree():
    q, k, v = AC.build("random_spiky", 0, 2, 4, 40, 33, 100, F16, seed=1)
    e1, m1 = AC.references(q, k, v, 4)
    e2, m2 = AC.references(q, k, v, 4, max_elems=33 * 100)            # one head at a time
    assert torch.equal(e1, e2) and torch.equal(m1, m2)
    ref = torch.softmax(AC.exact_logits(q, k, 4), dim=-1) @ v.double().reshape(2, 100, 4, 40).transpose(1, 2)
    assert float((e1 - ref.transpose(1, 2).reshape(2, 33, 160)).abs().max()) < 1e-12


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [40, 80, 160])
@pytest.mark.parametrize("mode", [0, 1])
def test_xattn_builders(dtype, d, mode):
    heads, n = 2, 40
    c = heads * d
    gates = torch.tensor([0.3, 0.7])
    for pattern in AC.XATTN_PATTERNS:
        q, kv = AC.build_xattn(pattern, 1, n, heads, d, mode, dtype, seed=5)
        assert kv.shape == ((1, 48, 4 * c) if mode == 0 else (1, 32, 2 * c))
        assert bool(torch.isfinite(q.float()).all()) and bool(torch.isfinite(kv.float()).all())
        ref = AC.xattn_reference(q, kv, gates, 3.0, mode, heads)
        assert bool(torch.isfinite(ref).all()), pattern
        kd = (kv[:, 0:16, 2 * c:3 * c] if mode == 0 else kv[:, 0:16, :c])      # the pathway one_floor puts at the floor
        lg = AC.exact_logits(q, kd.contiguous(), heads)
        if pattern == "flat":
            mean = lambda tok, col: kv[:, tok, col].double().mean(dim=1)        # noqa: E731
            vm = mean(slice(0, 32), slice(c, 2 * c)) if mode == 1 else \
                (float(gates[0]) * mean(slice(16, 32), slice(c, 2 * c)) + float(gates[1]) * mean(slice(0, 16), slice(3 * c, 4 * c))
                 + 3.0 * mean(slice(32, 48), slice(3 * c, 4 * c)))
            assert float((ref - vm[:, None, :]).abs().max()) < 1e-12
        elif pattern in ("all_floor", "one_floor"):
            assert float(lg.max()) < -100.0, (pattern, float(lg.max()))
        elif pattern == "one_hot":
            assert float(lg.max(dim=-1).values.min()) > 100.0
