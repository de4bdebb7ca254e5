"""Not-GPU: the binding of the attention backward (include/dadd_hip_attn_grad.h, ``lib.ATTN_GRAD_PROTOTYPES``,
``lib.AttnGradDesc``), the algebra and rounding points of csrc/attn_grad.hip restated in plain torch
(tests/attn_grad_reference.py) against float64 autograd, the bound of the GPU suite and its teeth, and the composition of
the triple-pathway gradient from one attention gradient per pathway."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from progressive_stable_diffusion_amd import grad_ops
from progressive_stable_diffusion_amd import lib as L
from tests import attention_cases as A
from tests import attn_grad_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "dadd_hip_attn_grad.h"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
CASE_DTYPES = [(c.name, F16) for c in R.CASES] + [(n, BF16) for n in R.BF16_CASES]


# ---- binding ---------------------------------------------------------------------------------------------------------
def test_header_and_prototype_table_declare_the_same_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    names = set(re.findall(r"\b(dadd_[a-z0-9_]+)\s*\(", text))
    assert names == set(L.ATTN_GRAD_PROTOTYPES) == {"dadd_attn_grad_f16", "dadd_attn_grad_bf16", "dadd_attn_grad_ws_floats"}
    others = set(L.PROTOTYPES) | set(L.GRAD_PROTOTYPES) | set(L.HOST_PROTOTYPES) | set(L.NORM_GRAD_PROTOTYPES)
    assert not names & others


def test_every_entry_point_is_exported_by_the_built_library():
    assert {"attn_grad.hip", "attn_grad_bf16.hip"} <= set(L.SOURCES)
    handle = ctypes.CDLL(L.build())
    missing = [n for n in L.ATTN_GRAD_PROTOTYPES if not hasattr(handle, n)]
    assert not missing, missing


def test_bf16_prototype_equals_the_fp16_one():
    assert L.ATTN_GRAD_PROTOTYPES["dadd_attn_grad_bf16"] == L.ATTN_GRAD_PROTOTYPES["dadd_attn_grad_f16"]
    assert L.ATTN_GRAD_PROTOTYPES["dadd_attn_grad_f16"][1][0]._type_ is L.AttnGradDesc


def test_attn_grad_desc_layout_matches_header(tmp_path):
    fields = [f[0] for f in L.AttnGradDesc._fields_]
    for want in ("q", "k", "v", "dout", "dq", "dk", "dv", "ws", "B", "Nq", "Nk", "heads", "d", "ld_q", "ld_kv", "ld_do",
                 "ld_dq", "ld_dkv", "do_scale", "do_scale_dev"):
        assert want in fields, want
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void) {{\n'
                   '  printf("%zu\\n", sizeof(dadd_attn_grad_desc));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(dadd_attn_grad_desc, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert ctypes.sizeof(L.AttnGradDesc) == out[0]
    assert [getattr(L.AttnGradDesc, f).offset for f in fields] == out[1:]


def test_workspace_size_follows_the_documented_layout():
    """[B][heads][Nq][2] floats; -1 for a size that is not positive."""
    handle = ctypes.CDLL(L.build())
    ws = handle.dadd_attn_grad_ws_floats
    ws.restype, ws.argtypes = L.ATTN_GRAD_PROTOTYPES["dadd_attn_grad_ws_floats"]
    for c in R.CASES:
        assert ws(c.b, c.heads, c.nq) == c.b * c.heads * c.nq * 2
    assert ws(4, 8, 4096) == 4 * 8 * 4096 * 2
    assert ws(0, 8, 64) == -1 and ws(2, 0, 64) == -1 and ws(2, 8, 0) == -1


# ---- the algebra of the kernels, without a GPU -----------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_model_without_roundings_is_the_exact_gradient(name):
    """Proves the algebra: the online LSE, D from dO . V instead of dO . O, the tiling and the scale of dout."""
    c = R.BY_NAME[name]
    q, k, v, do = R.inputs(name, F16)
    ex = R.exact(q, k, v, do, c.heads, R.total_scale(c))
    mo = R.model(q, k, v, do, c.heads, R.total_scale(c), rounded=False)
    for what, a, b in zip(("dq", "dk", "dv"), mo, ex):
        assert R.rel_l2(a, b) < 1e-12, (name, what, R.rel_l2(a, b))


@pytest.mark.parametrize("name,dtype", CASE_DTYPES)
def test_model_error_and_the_bound_of_the_gpu_suite(name, dtype):
    """E_model per tensor, printed; the bound max(2 E_model, ULP) never comes from a kernel."""
    ref = R.reference(name, dtype)
    for what, e, bound in zip(("dq", "dk", "dv"), ref.e_model, ref.bound):
        print(f"{name} {dtype} {what}: E_model {e:.3e}, bound {bound:.3e}")
        assert 0.0 < e < 0.05 and bound == max(2 * e, A.ULP[dtype])


@pytest.mark.parametrize("name,dtype", CASE_DTYPES)
def test_broken_models_land_ten_times_over_the_bound(name, dtype):
    """The bound has teeth: one key tile missing from dq, one query tile missing from dk / dv, or do_scale ignored, is at
    least 10 x over it."""
    c = R.BY_NAME[name]
    q, k, v, do = R.inputs(name, dtype)
    ref = R.reference(name, dtype)
    nkt, nqt = -(-c.nk // R.TILE), -(-c.nq // R.TILE)
    # the last tiles: the partly filled ones where a case has them; the peaked case also loses the tile of the peak
    key_tiles = {nkt - 1} | ({R.PEAK_KEY // R.TILE} if c.layout == "peaked" else set())
    for kt in sorted(key_tiles):
        dq, _, _ = R.model(q, k, v, do, c.heads, R.total_scale(c), drop_key_tile=kt)
        assert R.rel_l2(dq, ref.exact[0]) >= 10 * ref.bound[0], (name, "dq without key tile", kt)
    _, dk, dv = R.model(q, k, v, do, c.heads, R.total_scale(c), drop_query_tile=nqt - 1)
    assert R.rel_l2(dk, ref.exact[1]) >= 10 * ref.bound[1], (name, "dk without a query tile")
    assert R.rel_l2(dv, ref.exact[2]) >= 10 * ref.bound[2], (name, "dv without a query tile")
    if R.total_scale(c) != 1.0:
        got = R.model(q, k, v, do, c.heads, R.total_scale(c), ignore_scale=True)
        for what, a, e, bound in zip(("dq", "dk", "dv"), got, ref.exact, ref.bound):
            assert R.rel_l2(a, e) >= 10 * bound, (name, what, "do_scale ignored")


def test_some_cases_carry_a_scale():
    assert sum(R.total_scale(c) != 1.0 for c in R.CASES) >= 3
    c = R.BY_NAME["pathway shape"]
    assert c.do_scale != 1.0 and c.do_scale_dev not in (None, 1.0) and c.nk == 16


# ---- the triple-pathway composition ------------------------------------------------------------------------------------
def _tri_inputs(mode, b=2, n=32, heads=2, d=40, dtype=F16):
    q, kv = A.build_xattn("one_floor" if mode == 0 else "flat", b, n, heads, d, mode, dtype, seed=7)
    gen = torch.Generator().manual_seed(77)
    q = (0.5 * torch.randn(q.shape, generator=gen)).to(dtype)          # moderate logits
    kv = (0.5 * torch.randn(kv.shape, generator=gen)).to(dtype)
    dy = torch.randn(q.shape, generator=gen).to(dtype)
    return q, kv, dy, torch.tensor([0.8, 0.35], dtype=F32)


@pytest.mark.parametrize("mode,lam", [(0, 0.0), (0, 0.3), (1, 0.0)])
def test_pathway_calls_compose_the_gradient_of_tri_xattn(mode, lam):
    """float64: one masked attention gradient per pathway with the gate / lambda as the scale of dy reproduces autograd of
    the formula of dadd_tri_xattn; the baseline is one softmax over 32 tokens; slices nobody reads stay zero."""
    heads = 2
    q, kv, dy, gates = _tri_inputs(mode)
    c = q.shape[-1]
    dq_ref, dkv_ref = R.tri_exact(q, kv, dy, gates, lam, mode, heads)
    dq, dkv = R.tri_compose(q, kv, dy, gates, lam, mode, heads)
    assert R.rel_l2(dq, dq_ref) < 1e-12 and R.rel_l2(dkv, dkv_ref) < 1e-12
    if mode == 0:
        assert not dkv[:, 16:32, 2 * c:].any() and not dkv[:, :16, :2 * c].any() and not dkv[:, 32:, :2 * c].any()
        assert bool(dkv[:, 32:, 2 * c:].any()) == (lam != 0.0)
        # the model with the kernels' roundings composes too, within the pathway bound scale
        dq_m, dkv_m = R.tri_compose(q, kv, dy, gates, lam, mode, heads, grad=R.model)
        assert R.rel_l2(dq_m, dq_ref) < 4 * A.ULP[F16] and R.rel_l2(dkv_m, dkv_ref) < 4 * A.ULP[F16]


@pytest.mark.parametrize("mode,lam", [(0, 0.0), (0, 0.3), (1, 0.0)])
def test_tri_cross_attention_operator_hands_the_right_slices_to_attn_grad(mode, lam):
    """``grad_ops.tri_cross_attention`` itself on a CPU stand-in backend: number of calls, Nk, scales, and the gradients
    against float64 autograd within the rounding of the 16-bit results."""
    heads = 2
    q, kv, dy, gates = _tri_inputs(mode)
    be = R.CpuAttnBackend()
    qd, kvd = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    out = grad_ops.tri_cross_attention(be, qd, kvd, gates if mode == 0 else None, lam, heads, mode)
    assert R.rel_l2(out, A.xattn_reference(q, kv, gates, lam, mode, heads)) < A.ULP[F16]
    out.backward(dy)
    want = [(16, 0.8), (16, 0.35)] + ([(16, 0.3)] if lam else []) if mode == 0 else [(32, 1.0)]
    assert [(c["nk"], pytest.approx(c["scale"])) for c in be.calls] == [(nk, pytest.approx(s)) for nk, s in want]
    assert all(c["outputs"] == (True, True, True) for c in be.calls)
    dq_ref, dkv_ref = R.tri_exact(q, kv, dy, gates, lam, mode, heads)
    assert qd.grad.dtype == kvd.grad.dtype == F16
    assert R.rel_l2(qd.grad, dq_ref) < 2 * A.ULP[F16] and R.rel_l2(kvd.grad, dkv_ref) < 2 * A.ULP[F16]
    if mode == 0 and lam == 0.0:
        assert not kvd.grad[:, 32:48].any()
    # only what is needed is computed
    be2 = R.CpuAttnBackend()
    q2 = q.clone().requires_grad_(True)
    grad_ops.tri_cross_attention(be2, q2, kv, gates if mode == 0 else None, lam, heads, mode).backward(dy)
    assert all(c["outputs"] == (True, False, False) for c in be2.calls) and torch.equal(q2.grad, qd.grad)


def test_self_attention_and_attention_operators_on_the_stand_in_backend():
    c = R.BY_NAME["one tile"]
    q, k, v, do = R.inputs("one tile", F16)
    ex = R.exact(q, k, v, do, c.heads)
    be = R.CpuAttnBackend()
    qkv = torch.cat([q, k, v], -1).requires_grad_(True)
    grad_ops.self_attention(be, qkv, c.heads).backward(do)
    assert be.calls[0]["outputs"] == (True, True, True)
    assert R.rel_l2(qkv.grad, torch.cat(ex, -1)) < A.ULP[F16]
    qd, kd, vd = q.clone().requires_grad_(True), k.clone(), v.clone().requires_grad_(True)
    grad_ops.attention(be, qd, kd, vd, c.heads).backward(do)
    assert be.calls[1]["outputs"] == (True, False, True) and kd.grad is None
    assert R.rel_l2(qd.grad, ex[0]) < A.ULP[F16] and R.rel_l2(vd.grad, ex[2]) < A.ULP[F16]
    with pytest.raises(ValueError):
        grad_ops.self_attention(be, qkv.float(), c.heads)
    with pytest.raises(ValueError):
        grad_ops.tri_cross_attention(be, q, torch.zeros(1, 48, 2 * q.shape[-1], dtype=F16), torch.ones(2), 0.0, c.heads)
