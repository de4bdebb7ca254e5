"""The per-launch audit (tests/launch_audit.py) without a GPU: the reference audited against itself stays inside both
criteria, six backends that are wrong in exactly one way fail at the launches they touch and at no other, and every entry
of the measured tiling tables is selected by one of the two B = 4 / 64x64 plans the GPU audit runs.
"""
import gc

import pytest
import torch
import torch.nn.functional as F

from progressive_stable_diffusion_amd import engine as E
from progressive_stable_diffusion_amd import weights as W
from tests import launch_audit as LA
from tests.bf16_backend import DtypeRefBackend
from tests.torch_backend import TorchRefBackend

GATES = {"anatomy": (0.1, 0.9), "disease": (0.9, 0.1), "both": (0.5, 0.5)}


@pytest.fixture(scope="module")
def unet_sd():
    return W.init_state_dict(dict(W.unet_shapes()), 0, gates=GATES, warm_start_dis=False)


@pytest.fixture(autouse=True)
def _free_plans():
    """A plan and its backend refer to each other (recorded bound methods, the pool's hook), so only the cycle collector
    frees its 1.5 GB of packed weights - and tensor storage does not count towards its thresholds.  Collect after each test."""
    yield
    gc.collect()


def _check_reference(be, expected):
    print(LA.report("reference against itself", be))
    be.assert_clean()
    assert be.launches == expected == len(be.log)
    rms = [r["rms_ratio"] for r in be.records if r["rms_ratio"] == r["rms_ratio"]]
    # inner and r32 are the same fp32 arithmetic (the convolutions in another summation order): 1 up to accumulation noise
    assert rms and all(abs(v - 1.0) < 0.02 for v in rms), (min(rms), max(rms))


@pytest.mark.parametrize("b,s,lam", [(1, 16, 3.0), (2, 24, 0.0)])
def test_reference_unet_stays_inside_the_criteria(unet_sd, b, s, lam):
    """(2, 24): ragged attention (576 / 144 / 36 / 9 keys) and lambda = 0 (the delta pathway skipped)."""
    be, plan, expected = LA.audit_unet(TorchRefBackend(), unet_sd, b, s, lam)
    _check_reference(be, expected)
    ops = {op for op, _ in be.log}
    assert {"igemm", "groupnorm", "layernorm", "self_attn", "tri_xattn", "conv_in_nchw", "conv_cout4", "timestep_features",
            "linear_rows"} <= ops


def test_reference_unet_with_statistics_side_outputs(unet_sd, monkeypatch):
    """On the small maps of a CPU test no launch writes GroupNorm partials by the shipped policy (a (sample, group) slab
    fits the single-launch GroupNorm); with that threshold at zero the split-K finish writes them, GroupNorm reads them and
    the 16x16 convs normalise on the way in - the side outputs and their consumers under the audit on the CPU too."""
    monkeypatch.setattr(E, "GN_FUSED_MAX_BYTES", 0)
    be, plan, expected = LA.audit_unet(TorchRefBackend(), unet_sd, 1, 16, 3.0)
    _check_reference(be, expected)
    whats = {(r["op"], r["what"]) for r in be.records}
    assert {("igemm", "gn_ws"), ("conv_in_nchw", "gn_ws")} <= whats
    assert any(op == "groupnorm" and a["ws_chunks"] > 1 for op, a in be.log)
    assert any(op == "igemm" and a["gn_in"] is not None for op, a in be.log)


def test_reference_vae_decoder_stays_inside_the_criteria():
    sd = W.init_state_dict(W.vae_shapes(encoder=False), 0)
    be, plan, expected = LA.audit_vae_decoder(TorchRefBackend(), sd, 1, 8)
    _check_reference(be, expected)
    assert {"pack_latents", "conv_cin8", "conv_cout4", "self_attn"} <= {op for op, _ in be.log}


def test_audit_is_eager_only_and_refuses_unknown_ops():
    be = LA.backend(TorchRefBackend())
    with pytest.raises(RuntimeError):
        be.graph_begin()
    with pytest.raises(AttributeError):
        be.conv_out_ddim


def test_an_input_that_shares_storage_with_the_output_is_refused():
    be = LA.backend(TorchRefBackend())
    x = torch.randn(4, 64).half()
    g = torch.ones(64)
    with pytest.raises(AssertionError, match="shares storage"):
        be.layernorm(x, g, g, x)


# ------------------------------------------------------------------------------------------------ mutants
class _InIgemm(TorchRefBackend):
    """Lets a subclass restate the convolution of ``igemm`` alone (conv_cin8 / conv_cout4 share the hook)."""
    _depth, _odt = 0, None

    def igemm(self, x, w, out, **kw):
        self._depth, self._odt = self._depth + 1, out.dtype
        try:
            super().igemm(x, w, out, **kw)
        finally:
            self._depth -= 1


class DropsLastChannelOfLastTap(TorchRefBackend):
    def igemm(self, x, w, out, **kw):
        w = w.clone()
        w[:, -1] = 0
        super().igemm(x, w, out, **kw)


class SplitKLosesBiasInLastColumnTile(TorchRefBackend):
    def igemm(self, x, w, out, **kw):
        if kw.get("splitk", 1) > 1 and kw.get("bias") is not None:
            n, tile_n = w.shape[0], kw["tile_n"]
            bias = kw["bias"].clone()
            bias[(-(-n // tile_n) - 1) * tile_n:] = 0
            kw = dict(kw, bias=bias)
        super().igemm(x, w, out, **kw)


class ReplicatesBottomRow(_InIgemm):
    def conv2d(self, x, w, bias=None, stride=1, padding=0):
        if self._depth and w.shape[-1] == 3 and padding == 1:
            x = F.pad(x, (1, 1, 1, 0))
            x, padding = torch.cat([x, x[:, :, -1:]], dim=2), 0
        return super().conv2d(x, w, bias, stride, padding)


class GnstatChunkMissesLastRow(TorchRefBackend):
    def igemm(self, x, w, out, **kw):
        super().igemm(x, w, out, **kw)
        ws = kw.get("gn_ws")
        if ws is not None:
            n = out.shape[-1]
            last = out.float().reshape(out.shape[0], kw["gn_nchunk"], -1, 32, n // 32)[0, 0, -1]     # [32][cg]
            st = ws[:64].view(32, 2)
            st[:, 0] -= last.sum(dim=-1)
            st[:, 1] -= (last * last).sum(dim=-1)


class SelfAttnIgnoresLastKeyOfARaggedTile(TorchRefBackend):
    def self_attn(self, qkv, out, heads):
        b, n, c3 = qkv.shape
        if n % 64 == 0:
            return super().self_attn(qkv, out, heads)
        c = c3 // 3
        q, k, v = (t.float().view(b, n, heads, c // heads).transpose(1, 2) for t in qkv.split(c, dim=-1))
        p = torch.softmax(q @ k[:, :, :-1].transpose(-1, -2) / (c // heads) ** 0.5, dim=-1)
        out.copy_((p @ v[:, :, :-1]).transpose(1, 2).reshape(b, n, c).to(out.dtype))


class GroupNormSkipsLastChunk(TorchRefBackend):
    def groupnorm(self, x1, x2, gamma, beta, out, ws, groups, eps, silu, ws_chunks=0):
        if ws_chunks > 1:
            ws = ws.clone()
            ws[: x1.shape[0] * ws_chunks * groups * 2].view(x1.shape[0], ws_chunks, groups, 2)[:, -1] = 0
        super().groupnorm(x1, x2, gamma, beta, out, ws, groups, eps, silu, ws_chunks)


MUTANTS = {
    # name: (backend, policy overrides, the launches it touches: (op, bound arguments) -> bool)
    "a_drops_last_channel_of_last_tap": (DropsLastChannelOfLastTap, {}, lambda op, a: op == "igemm"),
    "b_splitk_loses_bias_in_last_n_tile": (SplitKLosesBiasInLastColumnTile, {},
                                           lambda op, a: op == "igemm" and a["splitk"] > 1 and a["bias"] is not None),
    # (stride 2 over an even map never reads the bottom padding row)
    "c_gather_replicates_bottom_row": (ReplicatesBottomRow, {},
                                       lambda op, a: op == "igemm" and a["taps"] == 9 and a["pad"] == 1 and a["stride"] == 1),
    "d_gnstat_chunk_misses_last_row": (GnstatChunkMissesLastRow, {"GN_FUSED_MAX_BYTES": 0},
                                       lambda op, a: op == "igemm" and a["gn_ws"] is not None),
    "e_self_attn_ignores_last_key": (SelfAttnIgnoresLastKeyOfARaggedTile, {},
                                     lambda op, a: op == "self_attn" and a["qkv"].shape[1] % 64 != 0),
    # (a conv that normalises on the way in reads the same partials: one source, more than one chunk)
    "f_groupnorm_skips_last_chunk": (GroupNormSkipsLastChunk, {"GN_FUSED_MAX_BYTES": 0},
                                     lambda op, a: (op == "groupnorm" and a["ws_chunks"] > 1) or
                                     (op == "igemm" and a["gn_in"] is not None and len(a["gn_in"]) == 5 and a["gn_in"][1] > 1)),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_fails_at_its_own_launches_only(unet_sd, name, monkeypatch):
    """Each launch reads what the (wrong) backend wrote before it and is compared with the reference on the same inputs:
    a launch the mutation does not touch passes although its inputs are off, which is what isolates launches."""
    cls, policy, touches = MUTANTS[name]
    for k, v in policy.items():
        monkeypatch.setattr(E, k, v)
    be, plan, expected = LA.audit_unet(cls(), unet_sd, 1, 16, 3.0)
    assert be.launches == expected
    touched = [i + 1 for i, (op, a) in enumerate(be.log) if touches(op, a)]
    failed = be.failed_launches()
    print(f"{name}: {len(touched)} launches touched, {len(failed)} failed of {be.launches}")
    for r in be.failures()[:3]:
        print("  " + be.describe(r))
    assert touched and failed == touched, (sorted(set(touched) - set(failed)), sorted(set(failed) - set(touched)))
    with pytest.raises(LA.AuditFailure, match="launch"):
        be.assert_clean()


class AccumulatorRoundedTo16Bit(_InIgemm):
    """Not wrong, only less accurate than it could be: the 3x3 convolutions put their accumulator through the storage type
    before the epilogue."""

    def conv2d(self, x, w, bias=None, stride=1, padding=0):
        y = super().conv2d(x, w, bias, stride, padding)
        return y.to(self._odt).to(y.dtype) if self._depth and w.shape[-1] == 3 else y


def test_a_16_bit_accumulator_passes_and_is_listed(unet_sd):
    """A second, independent rounding costs sqrt 2 in RMS (measured here: 1.39 to 1.44 on every 3x3 conv without a residual): inside the 1.5
    limit, and in the report's list of ratios above 1.1.  The variant is stated for the 3x3 convs (K >= 2880) because the
    elementwise bound is a statement about fp32 accumulation: its K 2^-24 A term covers a 16-bit rounding of the
    accumulator, u |acc|, only once K is a few hundred.  The same rounding in the K = 320 / 640 linears with a residual
    that cancels the accumulator lands at up to 3.9 times the bound, and in front of GEGLU at an RMS ratio of 1.86 (both
    measured with this class applied to every igemm) - flagged, as a launch that does not accumulate in fp32 should be."""
    be, plan, expected = LA.audit_unet(AccumulatorRoundedTo16Bit(), unet_sd, 1, 16, 3.0)
    text = LA.report("3x3 accumulator rounded to 16 bit", be)
    print(text)
    be.assert_clean()
    convs = [r for r in be.records if r["op"] == "igemm" and r["what"] == "out" and r["sig"][2] == 9]
    plain = [r["rms_ratio"] for r in convs if not r["sig"][4]]        # (a residual that outweighs the accumulator dilutes it)
    assert plain and all(LA.REPORT_ABOVE < v <= LA.RMS_LIMIT for v in plain), (min(plain), max(plain))
    listed = text[text.index("-- RMS ratio above"):]
    for sig in {r["sig"] for r in convs if not r["sig"][4]}:
        assert f"igemm.out {sig}:" in listed, sig
    others = [r["rms_ratio"] for r in be.records if r not in convs and r["rms_ratio"] == r["rms_ratio"]]
    assert max(others) < 1.02, "only the launches that round twice move"


# ------------------------------------------------------------------------------------------------ census
def _census(plan):
    keys, sigs, n_table = set(), set(), 0
    for fn, a, k in plan.ops:
        if getattr(fn, "__name__", "") != "igemm":
            continue
        x, w, out = a[:3]
        sigs.add(LA.igemm_signature(w, out, k))
        key = E.tiling_key(out.shape[0] * out.shape[1] * out.shape[2], w.shape[0], w.shape[1], k["taps"], bool(k["flags"] & 8),
                           k["residual"] is not None, k["ups"], k["stride"])
        if key in E.TILING_TABLE or key in E.TILING_TABLE_R3:
            keys.add(key)
            n_table += 1
    return keys, len(sigs), n_table


def test_every_tiling_table_entry_is_selected_by_an_audited_plan(unet_sd, monkeypatch):
    """``UNetPlan(4, 64)`` is the benchmark's plan; the tables are keyed on its M = B*H*W.  Counted on the shape backend:

        plan                                launches  igemm  chosen by table  igemm signatures  table keys
        B=4, S=64 (benchmark)                  234     157         76               54           20 of 23
        B=4, S=64, FUSED_FFN/HEAD/ATTN2 off    264     192         96               60           23 of 23
        B=4, S=64, bf16                        264     192         96               60           23 of 23
        B=1, S=64                              284     192         13               56            4 of 23
        B=2, S=24                              260     192          0               50            0

    (signature: N, K, taps, geglu, residual, ups, stride, flags, splitk, tile_m, tile_n.)  An entry neither B = 4 plan
    selects is dead - nothing the suite runs would notice it being wrong - and fails here."""
    table = set(E.TILING_TABLE) | set(E.TILING_TABLE_R3)
    assert len(table) == 23

    def build():            # one B = 4 plan at a time: each holds 2 GB of packed weights and buffers on the host
        plan = E.UNetPlan(DtypeRefBackend(), unet_sd, 4, 64)
        out = (_census(plan), LA.fingerprint(plan))
        del plan
        gc.collect()
        return out
    (keys, nsig, n_table), fp = build()
    assert fp == LA.FINGERPRINTS["bench"] and (fp["ops"], fp["igemm"], n_table, nsig, len(keys)) == (234, 157, 76, 54, 20)
    for sw in ("FUSED_FFN", "FUSED_HEAD", "FUSED_ATTN2"):
        monkeypatch.setattr(E, sw, False)
    (keys_off, nsig_off, n_table_off), fp_off = build()
    assert fp_off == LA.FINGERPRINTS["bench_unfused"]
    assert (fp_off["ops"], fp_off["igemm"], n_table_off, nsig_off, len(keys_off)) == (264, 192, 96, 60, 23)
    assert keys | keys_off == table, sorted(table - keys - keys_off)


@pytest.mark.parametrize("name,b,s,dtype", [("bench_bf16", 4, 64, torch.bfloat16), ("s24", 2, 24, torch.float16),
                                            ("s24", 2, 24, torch.bfloat16)])
def test_fingerprints_of_the_other_audited_plans(unet_sd, name, b, s, dtype):
    plan = E.UNetPlan(DtypeRefBackend(), unet_sd, b, s, dtype=dtype)
    fp = LA.fingerprint(plan)
    del plan
    gc.collect()
    assert fp == LA.FINGERPRINTS[name]
