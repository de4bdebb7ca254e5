"""Not-GPU: the gradients of the 4-channel end convolutions and of the loss - the binding of the entry points
(include/dadd_hip_end_grad.h, ``lib.END_GRAD_PROTOTYPES``, ``lib.EndWgradDesc``) and the algebra the kernels implement,
as float64 index-level models (tests/end_grad_reference.py) against autograd of ``F.conv2d``: the re-laid weight that
turns ``conv_in_nchw`` into conv_out's data gradient, and both modes of the thin weight-gradient kernel."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from progressive_stable_diffusion_amd import grad_ops
from progressive_stable_diffusion_amd import lib as L
from tests import end_grad_reference as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "dadd_hip_end_grad.h"
F32, F64 = torch.float32, torch.float64
B, H, W = 2, 5, 7


def rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


# ---- the re-laid weight ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("co", [4, 3])
def test_conv_in_kernel_on_relaid_weight_is_conv_out_data_gradient(co):
    c = 16
    w = rnd((co, 9 * c), 10 + co)                                   # library layout [Co][ky][kx][C]
    dy = rnd((B, co, H, W), 20 + co)
    wt = grad_ops.dgrad_weight_cout4(w)
    assert wt.shape == (c, 9, 8) and wt.dtype == F64 and wt.is_contiguous()
    assert not wt[:, :, co:].any()                                  # columns >= Co are zero
    assert torch.equal(wt[:, :, :co], w.reshape(co, 9, c).flip(1).permute(2, 1, 0))
    dx = E.conv_in_nchw_model(dy, wt)                               # NHWC [B,H,W,C]
    dx_ref, _, _ = E.conv2d_grads(rnd((B, c, H, W), 30), w.reshape(co, 3, 3, c).permute(0, 3, 1, 2), dy)
    err = (E.nchw(dx) - dx_ref).abs().max().item()
    assert err <= 1e-12, err
    # without the tap flip the result is a different tensor: the check can tell
    wrong = wt.flip(1)
    assert (E.nchw(E.conv_in_nchw_model(dy, wrong)) - dx_ref).abs().max().item() > 1e-3


# ---- the index algebra of the weight-gradient kernel ---------------------------------------------------------------
@pytest.mark.parametrize("ct", [4, 3])
def test_in_mode_model_is_autograd(ct):
    cw = 8
    lat, dy = rnd((B, ct, H, W), 40 + ct), rnd((B, H, W, cw), 50 + ct)
    dw, db = E.end_wgrad_model(lat, dy, E.IN)
    assert dw.shape == (cw, 9, 8) and db.shape == (cw,)
    _, dw_ref, db_ref = E.conv2d_grads(lat, rnd((cw, ct, 3, 3), 60), E.nchw(dy))
    want = dw_ref.permute(0, 2, 3, 1).reshape(cw, 9, ct)            # [N][ky][kx][c]
    assert (dw[:, :, :ct] - want).abs().max().item() <= 1e-12
    assert not dw[:, :, ct:].any()                                  # the pad channels of the 8 stored
    assert (db - db_ref).abs().max().item() <= 1e-12


@pytest.mark.parametrize("ct", [4, 3])
def test_out_mode_model_is_autograd_and_flips_the_taps(ct):
    cw = 8
    x, dpred = rnd((B, H, W, cw), 70 + ct), rnd((B, ct, H, W), 80 + ct)
    dw, db = E.end_wgrad_model(dpred, x, E.OUT)
    assert dw.shape == (ct, 9, cw) and db.shape == (ct,)
    _, dw_ref, db_ref = E.conv2d_grads(E.nchw(x), rnd((ct, cw, 3, 3), 90), dpred)
    want = dw_ref.permute(0, 2, 3, 1).reshape(ct, 9, cw)            # [o][ky][kx][c]
    assert (dw - want).abs().max().item() <= 1e-12
    assert (db - db_ref).abs().max().item() <= 1e-12
    assert (dw.flip(1) - want).abs().max().item() > 1e-3            # the unflipped taps are a different tensor
    # OUT mode is IN mode with the taps flipped and the output transposed
    dw_in, _ = E.end_wgrad_model(dpred, x, E.IN)
    assert torch.equal(dw_in[:, :, :ct].flip(1).permute(2, 1, 0), dw)


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_header_table_and_library_declare_the_same_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    names = set(re.findall(r"\b(dadd_[a-z0-9_]+)\s*\(", text))
    assert names == set(L.END_GRAD_PROTOTYPES)
    assert {"dadd_conv_end_wgrad_f16", "dadd_conv_end_wgrad_bf16", "dadd_mse_rows_grad_f32"} <= names
    others = set(L.PROTOTYPES) | set(L.GRAD_PROTOTYPES) | set(L.HOST_PROTOTYPES) | set(L.NORM_GRAD_PROTOTYPES) \
        | set(L.ATTN_GRAD_PROTOTYPES) | set(L.OPTIM_PROTOTYPES) | set(L.DGRAD_PROTOTYPES)
    assert not names & others
    assert {"end_grad.hip", "end_grad_bf16.hip"} <= set(L.SOURCES)
    handle = ctypes.CDLL(L.build())
    assert not [n for n in L.END_GRAD_PROTOTYPES if not hasattr(handle, n)]
    assert L.END_GRAD_PROTOTYPES["dadd_conv_end_wgrad_bf16"] == L.END_GRAD_PROTOTYPES["dadd_conv_end_wgrad_f16"]
    assert L.END_GRAD_PROTOTYPES["dadd_conv_end_wgrad_f16"][1][0]._type_ is L.EndWgradDesc
    consts = dict(re.findall(r"#define\s+DADD_END_WGRAD_(IN|OUT)\s+(\d+)", text))
    assert (int(consts["IN"]), int(consts["OUT"])) == (L.END_WGRAD_IN, L.END_WGRAD_OUT) == (E.IN, E.OUT)


def test_desc_layout_matches_header(tmp_path):
    """The ctypes mirror of ``dadd_end_wgrad_desc`` against the C compiler's view of the header (size and the offset of
    every field)."""
    fields = [f[0] for f in L.EndWgradDesc._fields_]
    assert fields == ["thin", "wide", "dw", "dbias", "partial", "B", "H", "W", "Ct", "Cw", "ld_wide", "mode", "splitm"]
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void) {{\n'
                   '  printf("%zu\\n", sizeof(dadd_end_wgrad_desc));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(dadd_end_wgrad_desc, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert ctypes.sizeof(L.EndWgradDesc) == out[0]
    assert [getattr(L.EndWgradDesc, f).offset for f in fields] == out[1:]


def test_partial_size_is_a_host_function():
    """``dadd_end_wgrad_partial_floats`` needs no GPU: per slice dw in its final layout plus the bias sums, padded to whole
    16-byte vectors; nothing for one slice; -1 outside the contract."""
    handle = ctypes.CDLL(L.build())
    fn = handle.dadd_end_wgrad_partial_floats
    fn.restype, fn.argtypes = L.END_GRAD_PROTOTYPES["dadd_end_wgrad_partial_floats"]
    assert fn(E.IN, 4, 320, 1) == 0
    assert fn(E.IN, 4, 320, 5) == 5 * (320 * 72 + 320)
    assert fn(E.OUT, 3, 64, 4) == 4 * (3 * 9 * 64 + 4)
    assert fn(E.OUT, 5, 64, 4) == -1 and fn(E.IN, 4, 96, 2) == -1 and fn(2, 4, 64, 2) == -1
