"""Not-GPU checks of the bf16 operand mode of the UNet.

* ISA: the bf16 twins (csrc/*_bf16.hip) cross-compiled for gfx950 use the bf16 MFMA and round with v_cvt_pk_bf16_f32,
  keep the resource limits of their fp16 twins, and instantiate the same kernels the fp16 sources do (attention: the
  UNet's head dims 40 / 80 / 160 only).
* Wiring: ``UNetPlan(dtype=torch.bfloat16)`` on a CPU operator double stores every 16-bit buffer and packed weight in
  bf16, records no row-block fusion, and computes the oracle's eps within bf16 rounding.
* API: ``operand_dtype`` of the module, its pass-through from ``load_from_checkpoint`` and ``--precision``.
"""
import os
import re
import subprocess

import pytest
import torch

from oracle.sd_unet import unet_forward
from progressive_stable_diffusion_amd import engine as E
from progressive_stable_diffusion_amd import inference_pipeline_ip as PIPE
from progressive_stable_diffusion_amd import lib as L
from progressive_stable_diffusion_amd import weights as W
from progressive_stable_diffusion_amd.config import default_config
from progressive_stable_diffusion_amd.diffusion_module_ip import DiffusionModuleWithIP
from tests.bf16_backend import DtypeRefBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "progressive-stable-diffusion_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BF16 = torch.bfloat16
TWINS = ("igemm", "igemm_dma", "conv_halo", "attention", "norm", "elementwise")
GATES = {"anatomy": (0.1, 0.9), "disease": (0.9, 0.1), "both": (0.5, 0.5)}
TINY_CLIP = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1,
                 image_size=224, patch_size=14, projection_dim=32)


# ---------------------------------------------------------------------------------------------------- ISA
@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    """{source: (fp16 assembly, bf16 assembly)} of every source with a bf16 twin (compiled in parallel)."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("isa_bf16")
    jobs = {}
    for name in TWINS:
        for src in (name, name + "_bf16"):
            out = d / f"{src}.s"
            jobs[src] = (out, subprocess.Popen(
                [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form=1",
                 "--cuda-device-only", "-S", os.path.join(CSRC, src + ".hip"), "-o", str(out)],
                stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    for src, (out, p) in jobs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, (src, err.decode()[-2000:])
    return {n: ((d / f"{n}.s").read_text(), (d / f"{n}_bf16.s").read_text()) for n in TWINS}


def _bodies(text):
    """kernel symbol -> its instruction lines."""
    cur, body, out = None, [], {}
    for line in text.splitlines():
        m = re.match(r"^(_Z\S+):", line)
        if m:
            cur, body = m.group(1), []
        elif line.startswith(".Lfunc_end") and cur:
            out[cur], cur = body, None
        elif cur:
            body.append(line.split(";")[0])
    return out


def _meta(text):
    """kernel symbol -> (scratch bytes, VGPRs, workgroup size limit)."""
    out = {}
    for blk in re.findall(r"^\s+- \.agpr_count:.*?(?=^\s+- \.agpr_count:|\Z)", text, flags=re.S | re.M):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        out[name] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                     int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                     int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", blk).group(1)))
    return out


def _to_bf16(sym):
    """mangled fp16 kernel name -> the name of its bf16 twin (bf16_names.h)"""
    sym = re.sub(r"(\d+)([a-z0-9_]+_kernel)(?=[A-Z]|v)", lambda m: f"{int(m.group(1)) + 5}{m.group(2)}_bf16", sym, count=1)
    return sym.replace("9IgemmArgs", "14IgemmArgs_bf16").replace("DF16_", "DF16b")    # (_Float16 -> __bf16 arguments)


MFMA_KERNELS = ("igemm_kernel", "igemm_dma_kernel", "conv3x3_halo_kernel", "flash_kernel", "xattn_kernel")


def test_bf16_kernels_use_the_bf16_mfma_and_rne_conversions(asm):
    n_mfma = 0
    for name in TWINS:
        bodies = _bodies(asm[name][1])
        assert bodies, name
        for sym, body in bodies.items():
            assert "_bf16" in sym, sym                       # every kernel of a twin carries the suffix
            text = "\n".join(body)
            assert "v_mfma_f32_16x16x32_f16" not in text and "v_mfma_f32_32x32x16_f16" not in text, sym
            assert not re.search(r"v_cvt_(pk_)?(f16_f32|pkrtz)", text), sym     # no fp16 rounding left behind
            if any(k + "_bf16" in sym for k in MFMA_KERNELS):
                assert "v_mfma_f32_16x16x32_bf16" in text, sym
                n_mfma += 1
            if not any(k in sym for k in ("gn_reduce", "gn_stats", "cout4")):
                # every other kernel here writes 16-bit values (statistics and conv_cout4 write fp32: no rounding)
                assert "v_cvt_pk_bf16_f32" in text, sym
    assert n_mfma >= 40, n_mfma


def test_bf16_instantiations_match_their_fp16_twins(asm):
    for name in TWINS:
        f16 = set(_meta(asm[name][0]))
        bf16 = set(_meta(asm[name][1]))
        want = set()
        for s in f16:
            m = re.search(r"(\d+)([a-z0-9_]+_kernel)", s)
            base = m.group(2)
            if name == "elementwise" and base not in ("conv_in_nchw_kernel", "conv_in_nchw_gn_kernel", "conv_cout4_kernel"):
                continue
            if name == "attention" and base == "flash_kernel" and not re.search(r"flash_kernelILi(40|80|160)E", s):
                continue                                     # (CLIP / resampler / VAE head dims stay fp16-only)
            want.add(_to_bf16(s))
        assert bf16 == want, (name, sorted(bf16 ^ want))


def test_bf16_resource_limits(asm):
    for name in TWINS:
        f16, bf16 = _meta(asm[name][0]), _meta(asm[name][1])
        for sym, (scratch, vgpr, wg) in bf16.items():
            assert scratch == 0, (sym, scratch)
            if wg >= 512 and ("igemm_dma" in sym or "halo" in sym):
                assert vgpr <= 256, (sym, vgpr)
            twin = re.sub(r"(\d+)([a-z0-9_]+_kernel)_bf16", lambda m: f"{int(m.group(1)) - 5}{m.group(2)}", sym)
            twin = twin.replace("14IgemmArgs_bf16", "9IgemmArgs").replace("DF16b", "DF16_")
            assert twin in f16, sym
            if any(k + "_bf16" in sym for k in MFMA_KERNELS):      # the MFMA kernels keep their fp16 twins' budget
                assert vgpr <= f16[twin][1] + 8, (sym, vgpr, f16[twin][1])


def test_bf16_flash_loop_and_dma_properties(asm):
    bodies = _bodies(asm["attention"][1])
    d40 = [s for s in bodies if "flash_kernel_bf16ILi40ELi2ELb1ELi8E" in s]
    assert len(d40) == 1, sorted(bodies)
    vgpr = _meta(asm["attention"][1])[d40[0]][1]
    assert vgpr <= 128, vgpr
    for sym, body in bodies.items():
        if "flash_kernel_bf16" not in sym:
            continue
        loops = [i for i, l in enumerate(body) if re.match(r"^\s*s_cbranch_\w+\s+\.LBB", l)]
        # the 64-key tile loop (the last backward branch) exchanges softmax lanes with v_permlane*_swap, never ds_bpermute
        labels = {l.strip().rstrip(":"): i for i, l in enumerate(body) if re.match(r"^\.LBB\S+:", l.strip())}
        back = [(labels[body[i].split()[-1]], i) for i in loops if labels.get(body[i].split()[-1], 1 << 30) < i]
        assert back, sym
        lo, hi = max(back, key=lambda t: t[1] - t[0])
        assert not any("ds_bpermute" in l or "ds_swizzle" in l for l in body[lo:hi]), sym
    for name in ("igemm_dma", "conv_halo"):
        for sym, body in _bodies(asm[name][1]).items():
            dma = [i for i, l in enumerate(body) if "buffer_load_dwordx4" in l and " lds" in l]
            assert dma, sym
            for i in dma:
                looped = any("s_cbranch_execnz" in l for l in body[i + 1:i + 4])
                picked = any("v_readfirstlane" in l for l in body[max(0, i - 10):i])
                assert not (looped and picked), sym


def test_bf16_entry_points_are_declared_and_bound():
    names = [n for n in L.PROTOTYPES if n.endswith("_bf16")]
    assert sorted(names) == sorted(["dadd_conv_igemm_bf16", "dadd_conv_in_nchw_bf16", "dadd_conv3x3_cout4_bf16",
                                    "dadd_conv_out_ddim_bf16", "dadd_groupnorm_bf16", "dadd_layernorm_bf16",
                                    "dadd_self_attn_bf16", "dadd_attn_bf16", "dadd_tri_xattn_bf16"])
    for n in names:                   # same argument lists as the fp16 siblings
        assert L.PROTOTYPES[n] == L.PROTOTYPES[n[:-5] + "_f16"], n
    assert all(s + "_bf16.hip" in L.SOURCES for s in TWINS)


def test_backend_refuses_mixed_16bit_operands():
    from progressive_stable_diffusion_amd.backend import _sfx
    h, b = torch.zeros(2, dtype=torch.float16), torch.zeros(2, dtype=BF16)
    assert _sfx(h, None, torch.zeros(1)) == "f16" and _sfx(b, b) == "bf16"
    with pytest.raises(ValueError):
        _sfx(h, b)
    with pytest.raises(ValueError):
        _sfx(torch.zeros(1))


# ---------------------------------------------------------------------------------------------------- wiring
@pytest.fixture(scope="module")
def full_sd():
    shapes = dict(W.unet_shapes())
    shapes.update(W.vae_shapes(encoder=False))
    shapes.update(W.conditioning_shapes(clip_hidden=TINY_CLIP["hidden_size"], clip_proj=TINY_CLIP["projection_dim"]))
    return W.init_state_dict(shapes, 0, gates=GATES, warm_start_dis=False)


def _names(plan):
    return [getattr(fn, "__name__", "") for fn, _, _ in plan.ops]


def _sig(plan):
    """op name, tensor shapes and flags of every recorded launch"""
    out = []
    for fn, a, k in plan.ops:
        shapes = tuple(tuple(t.shape) for t in a if isinstance(t, torch.Tensor))
        out.append((getattr(fn, "__name__", ""), shapes, k.get("flags"), k.get("splitk"), k.get("tile_n"), k.get("tile_m")))
    return out


@pytest.mark.parametrize("s", [8, 16])
def test_bf16_plan_stores_bf16_and_takes_the_generic_path(full_sd, s, monkeypatch):
    monkeypatch.setattr(E, "A2_MIN_TILES", 1)             # make every attn2 site eligible for the fp16 fusion
    monkeypatch.setattr(E, "FFN_MIN_BLOCKS", 1)
    plan = E.UNetPlan(DtypeRefBackend(), full_sd, 2, s, dtype=BF16)
    assert plan.dtype == BF16 and not plan.a2 and not plan.fused_attn2
    names = _names(plan)
    assert not {"attn2_fused", "ffn_block", "tf_head"} & set(names)
    assert names.count("_xattn") == 16 and names.count("self_attn") == 16
    assert plan.cond16.dtype == BF16 and all(kv.dtype == BF16 for v in plan.kv.values() for kv in v)
    assert all(w.dtype == BF16 for w in plan.kv_w.values())
    for fn, a, k in plan.ops:                             # every 16-bit operand of every launch is bf16
        for t in list(a) + list(k.values()):
            if isinstance(t, torch.Tensor):
                assert t.dtype in (BF16, torch.float32, torch.int32, torch.int64), (fn, t.dtype, tuple(t.shape))
    for t in plan.keep:                                   # packed weights; the time path keeps its fp16 rows (documented)
        if t.dtype == torch.float16:
            assert any(t is w for w in (plan.w_t1, plan.w_t2, plan.w_tp)), tuple(t.shape)
    for lst in plan.pool.free.values():
        assert all(t.dtype != torch.float16 for t in lst)
    # the same tiling / split-K / fold choices as the fp16 plan with its fusions switched off
    monkeypatch.setattr(E, "FUSED_ATTN2", False)
    monkeypatch.setattr(E, "FUSED_FFN", False)
    monkeypatch.setattr(E, "FUSED_HEAD", False)
    ref = E.UNetPlan(DtypeRefBackend(), full_sd, 2, s)
    assert _sig(ref) == _sig(plan)


def test_default_plan_is_unchanged_by_the_dtype_argument(full_sd):
    a = E.UNetPlan(DtypeRefBackend(), full_sd, 2, 8)
    b = E.UNetPlan(DtypeRefBackend(), full_sd, 2, 8, dtype=torch.float16)
    assert _sig(a) == _sig(b) and a.dtype == torch.float16
    assert any(t.dtype == torch.float16 for t in a.keep)
    with pytest.raises(ValueError):
        E.UNetPlan(DtypeRefBackend(), full_sd, 2, 8, dtype=torch.float32)


def test_weight_cache_keys_on_dtype(full_sd):
    cache = {}
    p16 = E.UNetPlan(DtypeRefBackend(), full_sd, 2, 8, wcache=cache)
    n16 = len(cache)
    pb = E.UNetPlan(DtypeRefBackend(), full_sd, 2, 8, wcache=cache, dtype=BF16)
    assert len(cache) > n16
    assert {k[-1] for k in cache} == {torch.float16, BF16}
    w16 = p16.w("conv_in.weight", E.pack_conv_cin8)
    wb = pb.w("conv_in.weight", E.pack_conv_cin8)
    assert w16.dtype == torch.float16 and wb.dtype == BF16


@pytest.mark.parametrize("lam", [0.0, 3.0])
def test_bf16_plan_matches_oracle(full_sd, lam):
    """eps of the bf16 plan (bf16 storage, fp32 arithmetic in the double) against the fp32 oracle."""
    torch.manual_seed(1)
    b, s = 2, 8
    be = DtypeRefBackend()
    plan = E.UNetPlan(be, full_sd, b, s, dtype=BF16)
    x, cond = torch.randn(b, 4, s, s), torch.randn(b, 48, 768) * 0.5
    t = torch.tensor([999, 333])
    with torch.no_grad():
        ref = unet_forward(full_sd, x, t, cond, delta_scale=lam)
        got = plan.forward(x, t, cond, lam=lam)
        got16 = E.UNetPlan(DtypeRefBackend(), full_sd, b, s).forward(x, t, cond, lam=lam)
    err = (ref - got).abs().max().item() / max(1.0, ref.abs().max().item())
    print(f"bf16 plan (CPU double) max|eps - oracle| / max|eps| = {err:.2e}")
    assert err < 4e-2
    assert not torch.equal(got, got16)                   # the rounding is bf16's, not fp16's
    assert {k for _, k in be.calls if k is not None} == {BF16}


# ---------------------------------------------------------------------------------------------------- API
def test_module_operand_dtype_is_validated_and_used(full_sd):
    cfg = default_config(**{"dataset.image_size": 64})
    with pytest.raises(ValueError):
        DiffusionModuleWithIP(cfg, dict(full_sd), backend=DtypeRefBackend(), device="cpu", clip_config=TINY_CLIP,
                              operand_dtype=torch.float32)
    mod = DiffusionModuleWithIP(cfg, dict(full_sd), backend=DtypeRefBackend(), device="cpu", clip_config=TINY_CLIP,
                                operand_dtype=BF16, batch_size=2)
    assert mod.operand_dtype == BF16 and mod.unet._plan.dtype == BF16
    assert mod.ddim_loop(2, 8).u.dtype == BF16
    assert mod._unet_for(1, 8)._plan.dtype == BF16       # every plan of the module
    assert mod.to(torch.float32) is mod and mod.half() is mod and mod.float() is mod
    mod16 = DiffusionModuleWithIP(cfg, dict(full_sd), backend=DtypeRefBackend(), device="cpu", clip_config=TINY_CLIP)
    assert mod16.operand_dtype == torch.float16 and mod16.unet._plan.dtype == torch.float16


def test_load_from_checkpoint_passes_operand_dtype(full_sd, tmp_path):
    cfg = default_config(**{"dataset.image_size": 64})
    path = tmp_path / "sd.pt"
    torch.save(dict(full_sd), path)
    mod = DiffusionModuleWithIP.load_from_checkpoint(str(path), cfg=cfg, backend=DtypeRefBackend(), device="cpu",
                                                     clip_config=TINY_CLIP, operand_dtype=BF16)
    assert mod.unet._plan.dtype == BF16


def test_precision_flag_parses():
    base = ["--checkpoint", "c.ckpt", "--structure-image", "s.png"]
    assert PIPE._parse_args(base).precision == "fp16"
    assert PIPE.PRECISIONS[PIPE._parse_args(base + ["--precision", "bf16"]).precision] == BF16
    with pytest.raises(SystemExit):
        PIPE._parse_args(base + ["--precision", "fp8"])
