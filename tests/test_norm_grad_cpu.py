"""Not-GPU: the binding of the norm / GEGLU backward entry points (include/dadd_hip_norm_grad.h, ``lib.NORM_GRAD_PROTOTYPES``,
``lib.GnGradDesc``) and the algebra of csrc/norm_grad.hip, restated in plain fp32 torch with the kernels' chunked
partials (tests/norm_grad_reference.py), against float64 autograd within the bounds of the GPU suite."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from progressive_stable_diffusion_amd import lib as L
from tests import norm_grad_reference as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "dadd_hip_norm_grad.h"


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(dadd_[a-z0-9_]+)\s*\(", text))


def test_header_and_prototype_table_declare_the_same_symbols():
    names = _declared(HEADER)
    assert names == set(L.NORM_GRAD_PROTOTYPES)
    for op in ("groupnorm_grad", "layernorm_grad", "geglu", "geglu_grad"):
        assert {f"dadd_{op}_f16", f"dadd_{op}_bf16"} <= names, op
    assert {"dadd_groupnorm_grad_ws_floats", "dadd_layernorm_grad_ws_floats"} <= names
    assert not names & (set(L.PROTOTYPES) | set(L.GRAD_PROTOTYPES) | set(L.HOST_PROTOTYPES))


def test_every_entry_point_is_exported_by_the_built_library():
    assert {"norm_grad.hip", "norm_grad_bf16.hip"} <= set(L.SOURCES)
    handle = ctypes.CDLL(L.build())
    missing = [n for n in L.NORM_GRAD_PROTOTYPES if not hasattr(handle, n)]
    assert not missing, missing


def test_bf16_prototypes_equal_the_fp16_ones():
    twins = [n for n in L.NORM_GRAD_PROTOTYPES if n.endswith("_bf16")]
    assert len(twins) == 4
    for n in twins:
        assert L.NORM_GRAD_PROTOTYPES[n] == L.NORM_GRAD_PROTOTYPES[n[:-5] + "_f16"], n
    assert L.NORM_GRAD_PROTOTYPES["dadd_groupnorm_grad_f16"][1][0]._type_ is L.GnGradDesc


def test_gn_grad_desc_layout_matches_header(tmp_path):
    fields = [f[0] for f in L.GnGradDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void) {{\n'
                   '  printf("%zu\\n", sizeof(dadd_gn_grad_desc));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(dadd_gn_grad_desc, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert ctypes.sizeof(L.GnGradDesc) == out[0]
    assert [getattr(L.GnGradDesc, f).offset for f in fields] == out[1:]


def test_workspace_sizes_follow_the_documented_layout():
    """Host-only entry points: [B][nchunk][groups][2] twice and [B][nchunk][C][2] for GroupNorm, [nblk][C][2] for LayerNorm;
    -1 outside the contract."""
    handle = ctypes.CDLL(L.build())
    gn, ln = handle.dadd_groupnorm_grad_ws_floats, handle.dadd_layernorm_grad_ws_floats
    gn.restype, gn.argtypes = L.NORM_GRAD_PROTOTYPES["dadd_groupnorm_grad_ws_floats"]
    ln.restype, ln.argtypes = L.NORM_GRAD_PROTOTYPES["dadd_layernorm_grad_ws_floats"]
    for b, c1, c2, h, w, _, _ in N.GN_CASES:
        c = c1 + c2
        nchunk, _ = N.gn_geometry(b, h * w, c)
        assert 1 <= nchunk <= 64
        assert gn(b, h * w, c, 32) == b * nchunk * (4 * 32 + 2 * c), (b, c, h, w)
    assert gn(2, 64, 324, 32) == -1 and gn(2, 64, 320, 48) == -1 and gn(2, 64, 320, 33) == -1 and gn(2, 64, 4104, 27) == -1
    for m, c in N.LN_CASES:
        assert ln(m, c) == min(256, -(-m // 8)) * c * 2
    assert ln(4, 2056) == -1 and ln(4, 12) == -1 and ln(0, 8) == -1


# ---- the algebra of the kernels, without a GPU -----------------------------------------------------------------------
@pytest.mark.parametrize("case", N.GN_CASES[:4])
def test_groupnorm_backward_formulas(case):
    b, c1, c2, h, w, silu, eps = case
    x, dy, gamma, beta, ref = N.gn_case(*case)
    dx, dgamma, dbeta = N.gn_model(x, dy, gamma, beta, eps, bool(silu))
    ref.check(dx, dgamma, dbeta, f"model groupnorm {case}")


def test_groupnorm_backward_formulas_zero_variance_and_bf16():
    for kw in (dict(constant_group=True), dict(dtype=N.BF16)):
        x, dy, gamma, beta, ref = N.gn_case(*N.GN_CASES[0], **kw)
        dx, dgamma, dbeta = N.gn_model(x, dy, gamma, beta, 1e-5, True)
        ref.check(dx, dgamma, dbeta, f"model groupnorm {kw}")
        assert bool(torch.isfinite(ref.dx).all())


@pytest.mark.parametrize("m,c", N.LN_CASES)
def test_layernorm_backward_formulas(m, c):
    x, dy, gamma, beta, ref = N.ln_case(m, c)
    dx, dgamma, dbeta = N.ln_model(x, dy, gamma, 1e-5)
    ref.check(dx, dgamma, dbeta, f"model layernorm {m}x{c}")


@pytest.mark.parametrize("m,f", N.GEGLU_CASES)
def test_geglu_formulas(m, f):
    h, dy, (y_ref, dh_ref) = N.geglu_case(m, f)
    y, dh = N.geglu_model(h, dy)
    N.close16(y, y_ref, f"model geglu {m}x{f} y")
    N.close16(dh, dh_ref, f"model geglu {m}x{f} dh")


def test_a_dropped_row_is_far_over_the_sum_bound():
    """The bound of dgamma / dbeta is not vacuous: leaving one row out of the column sums fails it."""
    x, dy, gamma, beta, ref = N.ln_case(130, 320)
    _, dgamma, dbeta = N.ln_model(x[:-1], dy[:-1], gamma, 1e-5)
    with pytest.raises(AssertionError):
        N.check_sums(dbeta, ref.dbeta, ref.e_beta, ref.m, "one row dropped")
