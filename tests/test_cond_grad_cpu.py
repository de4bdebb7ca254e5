"""Not-GPU: the binding of the conditioning front-end's training kernels (include/dadd_hip_cond_grad.h,
``lib.COND_GRAD_PROTOTYPES``), the float64 models of tests/cond_grad_reference.py pinned to float64 autograd of
``oracle.conditioning``'s formulas, the attention model at the new shapes (d = 96, ragged key counts), and the three
blocks of ``conditioning_grad`` run on the CPU stand-in backend against float64 autograd of the oracle."""
import ctypes
import gc
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import conditioning as OC
from progressive_stable_diffusion_amd import conditioning_grad as CG
from progressive_stable_diffusion_amd import grad_ops
from progressive_stable_diffusion_amd import lib as L
from tests import attn_grad_reference as R
from tests import cond_grad_reference as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16, F32, F64 = K.F16, K.BF16, K.F32, K.F64


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    """The helper caches its cases per process and nothing after this module needs them in the not-GPU run: drop them,
    collect, and hand the heap that has been freed so far back to the system, so that the modules that follow (whole UNet
    plans and checkpoints, in the same process) start from a small heap."""
    yield
    for fn in (K.ragged_inputs, K.ragged_reference, K.gelu_case, K.tail_case):
        fn.cache_clear()
    gc.collect()
    try:
        ctypes.CDLL("libc.so.6").malloc_trim(0)
    except (OSError, AttributeError):      # (not glibc: nothing to trim)
        pass


# ---- binding ---------------------------------------------------------------------------------------------------------------
def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(dadd_[a-z0-9_]+)\s*\(", text))


def test_header_and_prototype_table_declare_the_same_symbols():
    names = _declared("dadd_hip_cond_grad.h")
    assert names == set(L.COND_GRAD_PROTOTYPES)
    for op in ("gelu", "gelu_grad", "purifier_gate_tail", "purifier_gate_tail_grad"):
        assert {f"dadd_{op}_f16", f"dadd_{op}_bf16"} <= names, op
        assert L.COND_GRAD_PROTOTYPES[f"dadd_{op}_bf16"] == L.COND_GRAD_PROTOTYPES[f"dadd_{op}_f16"], op
    assert "dadd_purifier_gate_tail_grad_ws_floats" in names
    others = set(L.PROTOTYPES) | set(L.GRAD_PROTOTYPES) | set(L.HOST_PROTOTYPES) | set(L.NORM_GRAD_PROTOTYPES) \
        | set(L.ATTN_GRAD_PROTOTYPES) | set(L.OPTIM_PROTOTYPES) | set(L.DGRAD_PROTOTYPES) | set(L.END_GRAD_PROTOTYPES)
    assert not names & others


def test_every_entry_point_is_exported_and_the_workspace_follows_the_layout():
    assert {"cond_grad.hip", "cond_grad_bf16.hip"} <= set(L.SOURCES)
    handle = ctypes.CDLL(L.build())
    assert not [n for n in L.COND_GRAD_PROTOTYPES if not hasattr(handle, n)]
    ws = handle.dadd_purifier_gate_tail_grad_ws_floats
    ws.restype, ws.argtypes = L.COND_GRAD_PROTOTYPES["dadd_purifier_gate_tail_grad_ws_floats"]
    for m, c in K.TAIL_CASES + [(5000, 768)]:
        assert ws(m, c) == min(256, -(-m // 8)) * c * 2      # [nblk][C][2]
    assert ws(4, 2056) == -1 and ws(4, 12) == -1 and ws(0, 8) == -1


def test_attention_backward_accepts_d96_and_ragged_keys_in_the_documented_contract():
    text = open(os.path.join(ROOT, "include", "dadd_hip_attn_grad.h")).read()
    assert "d in {40, 80, 96, 160}" in text and "Nk any positive count" in text


# ---- GELU ------------------------------------------------------------------------------------------------------------------
def test_as_erf_keeps_its_stated_error_and_the_gelu_bounds_follow():
    x = torch.linspace(-8.0, 8.0, 200001, dtype=F64)
    e_erf = float((K.erf_as(x) - torch.erf(x)).abs().max())
    print(f"A&S erf: max |error| {e_erf:.3e} (stated {K.ERF_ERR:.1e})")
    assert e_erf <= K.ERF_ERR
    xg = x.clone().requires_grad_(True)
    F.gelu(xg).backward(torch.ones_like(x))
    e_grad = float((K.gelu_grad_model(x, torch.ones_like(x)) - xg.grad).abs().max())
    e_val = float(((K.gelu_model(x, fp32_point=False) - F.gelu(x)).abs() - 0.5 * x.abs() * K.ERF_ERR).max())
    # the model's fp32 rounding of erf next to 1: half an fp32 step, 2^-25, halved by Phi and multiplied by |x|
    e_f32 = float(((K.gelu_model(x) - K.gelu_model(x, fp32_point=False)).abs() - x.abs() * 2.0 ** -26).max())
    assert e_f32 <= 0.0 and float(K.gelu_model(torch.tensor([-6.0], dtype=F64))) == 0.0
    print(f"gelu' model against autograd of F.gelu: max |error| {e_grad:.3e} (bound {K.GELU_GRAD_ERR:.2e})")
    assert e_grad <= K.GELU_GRAD_ERR and e_val <= 0.0


@pytest.mark.parametrize("m,f,dtype", K.GELU_CASES)
def test_gelu_cases_span_the_range_and_the_model_error_is_below_the_gpu_bound(m, f, dtype):
    x, dy = K.gelu_case(m, f, dtype)
    assert float(x.float().min()) <= -5.9 and float(x.float().max()) >= 5.9
    x64 = x.double().requires_grad_(True)
    F.gelu(x64).backward(dy.double())
    ref = K.gelu_grad_model(x, dy)
    # the approximation's own error sits far inside the elementwise GPU bound: the bound measures the kernel
    assert bool(((ref - x64.grad).abs() <= K.GELU_GRAD_ERR * dy.double().abs() + 1e-300).all())
    assert bool((K.GELU_GRAD_ERR * dy.double().abs() <= 0.01 * K.gelu_grad_bound(ref, dtype)).all())


# ---- the purifier's tail -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifted", [False, True])
def test_gate_tail_models_are_the_autograd_of_the_oracle_formula(shifted):
    img, dis, z, dout, gamma, beta = K.tail_case(32, 768, F16, shifted)
    leaves = [t.double().requires_grad_(True) for t in (img, dis, z, gamma, beta)]
    i64, d64, z64, g64, b64 = leaves
    sd = {"n.weight": g64, "n.bias": b64}
    out = OC._ln(sd, "n", i64 - torch.sigmoid(z64) * d64)          # feature_purifier's last line
    out.backward(dout.double())
    assert float((K.gate_tail_model(img, dis, z, gamma, beta) - out.detach()).abs().max()) <= 1e-10
    r = K.gate_tail_grad_model(img, dis, z, dout, gamma)
    for key, leaf in zip(("dimg", "ddis", "dz", "dgamma", "dbeta"), leaves):
        err = R.rel_l2(r[key], leaf.grad)
        print(f"gate tail model {key} (shifted {shifted}): relative L2 {err:.3e}")
        assert err <= 1e-9, (key, err)
    if shifted:
        u = img.double() - torch.sigmoid(z.double()) * dis.double()
        assert abs(float(u.mean()) - 50.0) < 0.5 and 0.05 < float(u.std(-1).mean()) < 0.2


# ---- the attention model at the new shapes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("run", K.RAGGED_RUNS, ids=K.ragged_id)
def test_attention_model_at_the_new_shapes(run):
    """The model meets max(2 E_model, ulp) trivially; the printed E_model per tensor is what the GPU bound is made of."""
    i, dtype = run
    b, heads, d, nq, nk = K.RAGGED_CASES[i]
    ref = K.ragged_reference(i, dtype)
    q, k, v, do = K.ragged_inputs(i, dtype)
    mo = R.model(q, k, v, do, heads)
    for name, got, ex, e, bound in zip(("dq", "dk", "dv"), mo, ref.exact, ref.e_model, ref.bound):
        print(f"{K.ragged_id(run)} {name}: E_model {e:.3e}, bound {bound:.3e}")
        if nk == 1 and name != "dv":
            assert float(ex.abs().max()) == 0.0 and float(got.abs().max()) <= K.one_key_cap(q, k, v, do)
            continue
        assert e <= bound and bound < 0.05, (name, e, bound)
    unrounded = R.model(q, k, v, do, heads, rounded=False)
    assert all(float((a - b).abs().max()) <= 1e-9 for a, b in zip(unrounded, ref.exact))


def test_attention_model_with_a_dropped_ragged_tile_misses_the_bound():
    """Teeth: leaving out the last key tile of the resampler shape - ONE key of 257 - already breaks dq's bound."""
    i = 0
    heads = K.RAGGED_CASES[i][1]
    q, k, v, do = K.ragged_inputs(i, F16)
    ref = K.ragged_reference(i, F16)
    broken = R.model(q, k, v, do, heads, drop_key_tile=4)
    assert R.rel_l2(broken[0], ref.exact[0]) > ref.bound[0]


# ---- the blocks on the CPU stand-in ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(K.BLOCKS))
def test_block_composition_against_the_oracle(kind):
    """``conditioning_grad``'s own code on ``CpuCondBackend`` (float64 inside, fp16 storage) against float64 autograd of
    the oracle on fp16-rounded weight matrices: every parameter and input gradient within 2e-3 relative L2, half of the
    block bound, so that the reference path alone fits the GPU bound at these shapes."""
    params = K.BLOCKS[kind]()
    inputs, dout = K.block_inputs(kind)
    ref = K.oracle_grads(kind, params, inputs, dout)
    assert set(ref) == set(params) | set(inputs)
    be = K.CpuCondBackend()
    got, out = K.run_block(be, CG, kind, params, inputs, dout)
    assert out.dtype == (F32 if kind == "purifier" else F16)
    assert all(got[k].dtype == F32 for k in params) and all(got[k].dtype == F16 for k in inputs)
    worst = K.check_block(f"stand-in {kind}", got, ref, bound=K.STANDIN_BOUND)
    assert worst <= K.STANDIN_BOUND < K.BLOCK_BOUND
    if kind != "projection":
        nk = {"purifier": K.TOKENS, "resampler": K.CTX}[kind]
        assert be.calls and all(c["nq"] == K.TOKENS and c["nk"] == nk for c in be.calls)


def test_packed_in_proj_master_gets_one_gradient_with_all_three_blocks_filled():
    params = K.purifier_params()
    inputs, dout = K.block_inputs("purifier")
    got, _ = K.run_block(K.CpuCondBackend(), CG, "purifier", params, inputs, dout)
    gw = got["feature_purifier.cross_attn.in_proj_weight"]
    assert gw.shape == (3 * K.E, K.E) and all(float(gw[i * K.E:(i + 1) * K.E].abs().max()) > 0 for i in range(3))


def test_operators_refuse_what_the_kernels_do_not_take():
    be = K.CpuCondBackend()
    with pytest.raises(ValueError):
        grad_ops.gelu(be, torch.zeros(4, 12, dtype=F16))
    with pytest.raises(ValueError):
        grad_ops.gelu(be, torch.zeros(4, 16, dtype=F32))
    g, b = torch.ones(16), torch.zeros(16)
    with pytest.raises(ValueError):
        grad_ops.purifier_gate_tail(be, torch.zeros(4, 16, dtype=F16), torch.zeros(4, 16, dtype=BF16),
                                    torch.zeros(4, 16, dtype=F16), g, b)
    with pytest.raises(ValueError):
        grad_ops.purifier_gate_tail(be, *(torch.zeros(4, 16, dtype=F16) for _ in range(3)), g.double(), b.double())
