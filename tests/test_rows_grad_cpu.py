"""Not-GPU: the binding of the fp32 row path's backward (include/dadd_hip_rows_grad.h, ``lib.ROWS_GRAD_PROTOTYPES``), the
float64 models of tests/rows_grad_reference.py pinned to float64 autograd of ``oracle.conditioning`` / ``oracle.sd_unet``
formulas, ``conditioning_grad.ordinal_embedder`` / ``time_embedding`` and ``grad_ops.conv3x3(rowvec=)`` run on the CPU
stand-in backend against float64 autograd of the oracle, and the operators' refusals."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import conditioning as OC
from progressive_stable_diffusion_amd import conditioning_grad as CG
from progressive_stable_diffusion_amd import grad_ops
from progressive_stable_diffusion_amd import lib as L
from tests import norm_grad_reference as N
from tests import rows_grad_reference as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16, F32, F64 = K.F16, K.BF16, K.F32, K.F64


# ---- binding -----------------------------------------------------------------------------------------------------------------
def test_header_and_prototype_table_declare_the_same_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dadd_hip_rows_grad.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(dadd_[a-z0-9_]+)\s*\(", text))
    assert names == set(L.ROWS_GRAD_PROTOTYPES) == {
        "dadd_linear_rows_grad_f32", "dadd_linear_rows_grad_ws_floats", "dadd_aoe_interp_grad_f32", "dadd_rowvec_grad_f16",
        "dadd_rowvec_grad_bf16", "dadd_rowvec_grad_ws_floats"}
    assert L.ROWS_GRAD_PROTOTYPES["dadd_rowvec_grad_bf16"] == L.ROWS_GRAD_PROTOTYPES["dadd_rowvec_grad_f16"]
    others = set(L.PROTOTYPES) | set(L.GRAD_PROTOTYPES) | set(L.HOST_PROTOTYPES) | set(L.NORM_GRAD_PROTOTYPES) \
        | set(L.ATTN_GRAD_PROTOTYPES) | set(L.OPTIM_PROTOTYPES) | set(L.DGRAD_PROTOTYPES) | set(L.END_GRAD_PROTOTYPES) \
        | set(L.COND_GRAD_PROTOTYPES)
    assert not names & others


def test_every_entry_point_is_exported_and_the_workspaces_follow_the_layout():
    assert {"rows_grad.hip", "rows_grad_bf16.hip"} <= set(L.SOURCES)
    handle = ctypes.CDLL(L.build())
    assert not [n for n in L.ROWS_GRAD_PROTOTYPES if not hasattr(handle, n)]
    lin, row = handle.dadd_linear_rows_grad_ws_floats, handle.dadd_rowvec_grad_ws_floats
    lin.restype, lin.argtypes = L.ROWS_GRAD_PROTOTYPES["dadd_linear_rows_grad_ws_floats"]
    row.restype, row.argtypes = L.ROWS_GRAD_PROTOTYPES["dadd_rowvec_grad_ws_floats"]

    def strip(k, n):       # the widest strip of 64 / 32 rows that leaves 512 workgroups, else 16
        kt = -(-k // 512)
        return next((ns for ns in (64, 32) if -(-n // ns) * kt >= 512), 16)

    for m, k, n in K.LINEAR_CASES + [(8, 1536, 12288), (64, 1536, 12288), (8, 1280, 18560), (4, 320, 1280)]:
        assert lin(m, k, n) == -(-n // strip(k, n)) * m * k, (m, k, n)      # [strips][M][K]
    assert strip(1536, 12288) == 64 and strip(1280, 1280) == 16
    assert lin(4, 12, 8) == -1 and lin(4, 2056, 8) == -1 and lin(0, 8, 8) == -1 and lin(4, 8, 0) == -1
    for b, hw, c in K.ROWVEC_CASES + [(8, 4096, 320)]:
        assert row(b, hw, c) == b * -(-hw // 64) * c                        # [B][chunks of 64 pixels][C]
    assert row(2, 64, 12) == -1 and row(0, 64, 8) == -1 and row(2, 0, 8) == -1 and row(65536, 1, 8) == -1


# ---- the models are the autograd of the oracle's formulas --------------------------------------------------------------------
@pytest.mark.parametrize("act_in", [0, 1, 2])
@pytest.mark.parametrize("w_dtype", [F32, F16])
def test_linear_rows_grad_model_is_the_autograd_of_the_oracle_formula(act_in, w_dtype):
    m, k, n = 11, 1536, 130
    x, w, dy = K.linear_case(m, k, n, w_dtype)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    b64 = torch.zeros(n, dtype=F64, requires_grad=True)
    a = x64 if act_in == 0 else F.silu(x64) if act_in == 1 else F.gelu(x64)     # oracle.sd_unet.resnet / conditioning.aoe_project
    OC._lin({"l.weight": w64, "l.bias": b64}, "l", a).backward(dy.double())
    r = K.linear_rows_grad_model(x, w, dy, act_in)
    for key, leaf in (("dx", x64), ("dw", w64), ("db", b64)):
        assert N.rel_l2(r[key], leaf.grad) <= 1e-12, key
    # the sums of absolute terms dominate the results, and a dropped row of dy misses the bound it takes
    assert bool((r["e_dw"] >= r["dw"].abs() - 1e-12).all()) and bool((r["e_dx"] >= r["dx"].abs() - 1e-12).all())
    broken = K.linear_rows_grad_model(x[:-1], w, dy[:-1], act_in)
    bounds = K.linear_bounds(r)
    assert K.share(broken["dw"], r["dw"], bounds["dw"]) > 25 and K.share(broken["db"], r["db"], bounds["db"]) > 25


@pytest.mark.parametrize("b,d,classes", K.AOE_CASES)
def test_aoe_interp_models_are_the_autograd_of_the_oracle_lerp(b, d, classes):
    lab, base, deltas, dout = K.aoe_case(b, d, classes)
    sd = {"e.base": base.double().requires_grad_(True), "e.deltas": deltas.double().requires_grad_(True)}
    out = OC.aoe_lerp(sd, lab.double(), "e")
    out.backward(dout.double())
    assert float((K.aoe_interp_model(lab, base, deltas) - out.detach()).abs().max()) == 0.0
    r = K.aoe_interp_grad_model(lab, dout, classes)
    assert N.rel_l2(r["dbase"], sd["e.base"].grad) <= 1e-12 and N.rel_l2(r["ddeltas"], sd["e.deltas"].grad) <= 1e-12
    assert r["ddeltas"].shape == (classes - 1, d) and bool((r["e_base"] >= r["dbase"].abs() - 1e-12).all())


def test_aoe_labels_hit_every_edge():
    lab = K.labels(9)
    lo, hi, frac = K.aoe_cells(lab, 4)
    assert float(lab.min()) < 0 and float(lab.max()) > 3                      # both clamps
    assert bool(((lo == hi) & (lo == 3)).any())                                # lo == hi at the top
    assert bool(((frac == 0) & (lab == 1.0)).any())                            # an integer label inside
    assert bool(((lo == 0) & (frac > 0)).any()) and int((lo == 0).sum()) >= 2  # two samples in one cell
    assert K.labels(1).tolist() == [-0.5] and len(K.labels(7)) == 7


@pytest.mark.parametrize("b,hw,c", K.ROWVEC_CASES[:3])
def test_rowvec_grad_model_is_the_autograd_of_the_broadcast_add(b, hw, c):
    dy = K.rowvec_case(b, hw, c)
    row = torch.zeros(b, c, dtype=F64, requires_grad=True)
    h = torch.zeros(b, hw, 1, c, dtype=F64)
    (h + row[:, None, None, :]).backward(dy.double().reshape(b, hw, 1, c))     # oracle.sd_unet.resnet's "+ temb" in NHWC
    r = K.rowvec_grad_model(dy)
    assert torch.equal(r["drow"], row.grad) and r["hw"] == hw


# ---- the blocks on the CPU stand-in --------------------------------------------------------------------------------------------
def test_embedder_f32_reference_error_is_the_recorded_one():
    """The block bound is ten times torch's own fp32 error on this path; the recorded figures must describe it."""
    fresh = K.embedder_f32_error()
    for key, err in fresh.items():
        rec = K.EMBEDDER_F32_ERR[key.split(".", 1)[1]]
        print(f"fp32 autograd of the oracle's AOE, d {key}: relative L2 {err:.3e} (recorded {rec:.1e})")
        assert rec / 4 <= err <= 2 * rec, (key, err, rec)
    assert max(K.EMBEDDER_BOUND.values()) < 1e-5 < K.BLOCK_BOUND


def test_ordinal_embedder_on_the_stand_in_against_the_oracle():
    params, lab = K.embedder_params(), K.labels(K.EMB_B)
    dout = K.randn((K.EMB_B, K.EMB_TOKENS, K.EMB_D), 710)
    ref = K.embedder_oracle_grads(params, lab, dout)
    be = K.CpuRowsBackend()
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    out = CG.ordinal_embedder(be, leaves, lab, num_tokens=K.EMB_TOKENS)
    assert out.shape == (K.EMB_B, K.EMB_TOKENS, K.EMB_D) and out.dtype == F32
    sd64 = {k: v.double() for k, v in params.items()}
    assert N.rel_l2(out, OC.aoe_forward(sd64, lab.double(), K.EMB_TOKENS)) <= 1e-6
    out.backward(dout)
    for key in ref:
        err, bound = N.rel_l2(leaves[key].grad, ref[key]), K.EMBEDDER_BOUND[key.split(".", 1)[1]]
        print(f"stand-in embedder d {key}: relative L2 {err:.3e} (bound {bound:.1e})")
        assert leaves[key].grad.dtype == F32 and err <= bound, (key, err, bound)
    unused = [k for k in params if k.split(".", 1)[1] not in K.EMBEDDER_TRAINED]
    assert len(unused) == 3 and all(leaves[k].grad is None for k in unused)        # norm.*, null_embedding


def test_ordinal_embedder_call_forms():
    params, be = K.embedder_params(), K.CpuRowsBackend()
    lab = K.labels(K.EMB_B)
    plain = CG.ordinal_embedder(be, params, lab, num_tokens=K.EMB_TOKENS)
    one = CG.ordinal_embedder(be, params, lab[4], num_tokens=K.EMB_TOKENS)
    assert one.shape == (K.EMB_TOKENS, K.EMB_D) and torch.equal(one, plain[4])
    null = CG.ordinal_embedder(be, params, lab, unconditional=True)
    assert null.shape == (K.EMB_B, K.EMB_D) and torch.equal(null[2], params["ordinal_embedder.null_embedding"][0])
    assert CG.ordinal_embedder(be, params, lab[0], unconditional=True).shape == (1, K.EMB_D)
    torch.manual_seed(5)
    noisy = CG.ordinal_embedder(be, params, lab, is_training=True, noise_std=0.05, num_tokens=K.EMB_TOKENS)
    assert not torch.equal(noisy, plain)
    assert torch.equal(CG.ordinal_embedder(be, params, lab, is_training=True, noise_std=0.0, num_tokens=K.EMB_TOKENS), plain)
    assert torch.equal(CG.ordinal_embedder(be, params, lab, is_training=False, noise_std=0.05, num_tokens=K.EMB_TOKENS), plain)


def test_time_embedding_on_the_stand_in_against_the_oracle():
    params, t = K.time_params(), torch.tensor([17, 640, 999], dtype=torch.int64)
    dout = K.randn((3, sum(K.TIME_WIDTHS)), 820)
    ref_leaves = K.round_matrices(params)
    ref_rows = K.time_rows64(ref_leaves, t)
    ref_rows.backward(dout.double())
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    rows = CG.time_embedding(K.CpuRowsBackend(), leaves, t, K.TIME_PROJ_KEYS, dim=K.TIME_DIM, prefix=K.TIME_PREFIX)
    assert rows.shape == (3, sum(K.TIME_WIDTHS)) and rows.dtype == F32
    assert N.rel_l2(rows, ref_rows.detach()) <= 1e-6
    rows.backward(dout)
    for key, leaf in ref_leaves.items():
        err = N.rel_l2(leaves[key].grad, leaf.grad)
        print(f"stand-in time path d {key}: relative L2 {err:.3e}")
        assert leaves[key].grad.dtype == F32 and leaves[key].grad.shape == params[key].shape and err <= 1e-5, (key, err)


def test_conv3x3_with_a_strided_rowvec_on_the_stand_in():
    """The row enters in the epilogue (one rounding of conv + bias + row) and its gradient is the pixel sum of dy; the
    columns of the wider rows tensor that the conv does not take get a zero gradient."""
    b, hw, c, n = 2, 5, 16, 24
    r = N.R.rnd
    x, w, bias, dy = r((b, hw, hw, c), 900), r((n, 9 * c), 901, (9 * c) ** -0.5, F32), r((n,), 902, 0.1, F32), r((b, hw, hw, n), 903)
    rows = r((b, n + 8), 904, 0.5, F32)
    be = K.CpuRowsBackend()
    xd, wd, bd, rd = (t.clone().requires_grad_(True) for t in (x, w, bias, rows))
    y = grad_ops.conv3x3(be, xd, wd, bd, rowvec=rd[:, :n])
    y.backward(dy)
    x64, w64, b64, r64 = x.double().requires_grad_(True), w.half().double().requires_grad_(True), \
        bias.double().requires_grad_(True), rows.double().requires_grad_(True)
    y64 = N.conv3x3_nhwc(x64, w64, b64) + r64[:, :n][:, None, None, :]
    y64.backward(dy.double())
    assert y.dtype == F16 and torch.equal(y, y64.detach().half())
    assert rd.grad.dtype == F32 and torch.equal(rd.grad, r64.grad.float()) and not rd.grad[:, n:].any()
    N.close16(xd.grad, x64.grad, "conv3x3(rowvec) dx")
    assert N.rel_l2(wd.grad, w64.grad) <= 1e-6 and N.rel_l2(bd.grad, b64.grad) <= 1e-6
    plain = grad_ops.conv3x3(be, x, w, bias)          # without rowvec: the product as before
    assert torch.equal(plain, N.conv3x3_nhwc(x.double(), w.half().double(), bias.double()).half())


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_operators_refuse_what_the_kernels_do_not_take():
    be = K.CpuRowsBackend()
    x16, w = torch.zeros(2, 4, 4, 16, dtype=F16), torch.zeros(8, 9 * 16)
    row = torch.zeros(2, 8)
    for kw in (dict(stride=2), dict(ups=True)):
        with pytest.raises(ValueError):
            grad_ops.conv3x3(be, x16, w, rowvec=row, **kw)
    for bad in (row.double(), torch.zeros(2, 16), torch.zeros(3, 8), torch.zeros(8, 2).t(), torch.zeros(2, 10)[:, 1:9],
                torch.zeros(2, 9)[:, :8]):
        with pytest.raises(ValueError):
            grad_ops.conv3x3(be, x16, w, rowvec=bad)
    xr, wr = torch.zeros(3, 16), torch.zeros(5, 16)
    with pytest.raises(ValueError):
        grad_ops.linear_rows(be, torch.zeros(3, 12), torch.zeros(5, 12))            # K not a multiple of 8
    with pytest.raises(ValueError):
        grad_ops.linear_rows(be, torch.zeros(3, 2056), torch.zeros(5, 2056))        # K > 2048
    with pytest.raises(ValueError):
        grad_ops.linear_rows(be, xr.half(), wr)                                     # rows are fp32
    with pytest.raises(ValueError):
        grad_ops.linear_rows(be, xr, wr.half())                                     # w is the fp32 master
    with pytest.raises(ValueError):
        grad_ops.linear_rows(be, xr, wr, weight_dtype=BF16)                         # the rows multiply in fp16 or fp32
    with pytest.raises(ValueError):
        grad_ops.linear_rows(be, xr, wr, act_in=3)
    with pytest.raises(ValueError):
        grad_ops.linear_rows(be, xr, wr, torch.zeros(4))
    with pytest.raises(ValueError):
        grad_ops.aoe_interp(be, torch.zeros(2), torch.zeros(8), torch.zeros(16, 8))  # 17 classes
    with pytest.raises(ValueError):
        grad_ops.aoe_interp(be, torch.zeros(2), torch.zeros(8), torch.zeros(3, 16))
    with pytest.raises(ValueError):
        be.linear_rows_grad(xr, wr, torch.zeros(3, 5))                               # no output
    with pytest.raises(ValueError):
        be.linear_rows_grad(xr, wr, torch.zeros(3, 5), dx=torch.zeros(3, 16), db=torch.zeros(5), ws=torch.zeros(48))
