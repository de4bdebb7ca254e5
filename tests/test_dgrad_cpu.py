"""Not-GPU: the data gradient of the stride-2 and the upsampled 3x3 conv - the binding of its entry points
(include/dadd_hip_dgrad.h, ``lib.DGRAD_PROTOTYPES``, ``lib.DgradDesc`` / ``lib.DgradChoice``), the algebra of the parity
classes and of the pre-summed upsample taps through the re-layout functions of ``grad_ops`` against float64 autograd
(tests/dgrad_reference.py), the rounding points of the kernel against the tolerances of the GPU suite, and the class
table ``dadd_conv_dgrad_resolve`` hands the launcher."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from progressive_stable_diffusion_amd import lib as L
from tests import dgrad_reference as D
from tests import grad_reference as R
from tests import norm_grad_reference as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "dadd_hip_dgrad.h"
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
IDS = [f"{c.mode}-{c.b}x{c.h}x{c.w}-C{c.c}-N{c.n}" for c in D.CASES]


@pytest.fixture(scope="module")
def handle():
    h = ctypes.CDLL(L.build())
    for name, (res, args) in L.DGRAD_PROTOTYPES.items():
        fn = getattr(h, name)
        fn.restype, fn.argtypes = res, args
    h.dadd_last_error.restype = ctypes.c_char_p
    return h


# ---- binding ---------------------------------------------------------------------------------------------------------
def test_header_table_and_library_declare_the_same_symbols(handle):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    names = set(re.findall(r"\b(dadd_[a-z0-9_]+)\s*\(", text))
    assert names == set(L.DGRAD_PROTOTYPES) == {"dadd_conv_dgrad_f16", "dadd_conv_dgrad_bf16", "dadd_conv_dgrad_resolve"}
    others = set(L.PROTOTYPES) | set(L.GRAD_PROTOTYPES) | set(L.HOST_PROTOTYPES) | set(L.NORM_GRAD_PROTOTYPES) \
        | set(L.ATTN_GRAD_PROTOTYPES) | set(L.OPTIM_PROTOTYPES)
    assert not names & others
    assert {"dgrad.hip", "dgrad_bf16.hip"} <= set(L.SOURCES)
    assert not [n for n in L.DGRAD_PROTOTYPES if not hasattr(handle, n)]
    assert L.DGRAD_PROTOTYPES["dadd_conv_dgrad_bf16"] == L.DGRAD_PROTOTYPES["dadd_conv_dgrad_f16"]
    assert L.DGRAD_PROTOTYPES["dadd_conv_dgrad_f16"][1][0]._type_ is L.DgradDesc
    assert L.DGRAD_PROTOTYPES["dadd_conv_dgrad_resolve"][1][1]._type_ is L.DgradChoice
    consts = dict(re.findall(r"#define\s+DADD_DGRAD_(STRIDE2|UPS)\s+(\d+)", text))
    assert (int(consts["STRIDE2"]), int(consts["UPS"])) == (L.DGRAD_STRIDE2, L.DGRAD_UPS)


def test_struct_layouts_match_the_header(tmp_path):
    desc = [f[0] for f in L.DgradDesc._fields_]
    choice = [f[0] for f in L.DgradChoice._fields_]
    cls = [f[0] for f in L.DgradClass._fields_]
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void) {{\n'
                   '  printf("%zu\\n", sizeof(dadd_dgrad_desc));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(dadd_dgrad_desc, {f}));\n' for f in desc)
                   + '  printf("%zu\\n", sizeof(dadd_dgrad_choice));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(dadd_dgrad_choice, {f}));\n' for f in choice)
                   + '  printf("%zu\\n", sizeof(dadd_dgrad_class));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(dadd_dgrad_class, {f}));\n' for f in cls)
                   + '  printf("%d\\n", DADD_DGRAD_MAX_CLASSES);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for struct, fields in ((L.DgradDesc, desc), (L.DgradChoice, choice), (L.DgradClass, cls)):
        want += [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]
    assert out == want + [L.DgradChoice.cls.size // ctypes.sizeof(L.DgradClass)]


# ---- the algebra and the re-layout functions -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_model_in_float64_is_autograd(case):
    """Unrounded W4, float64 sums: the parity classes and the 16 summed taps ARE the gradient (no pixel left NaN)."""
    dy, w, dx_ref = D.case_operands(case)
    dx = D.model(dy.double(), D.relaid(w.double(), case.mode), case.mode, case.h, case.w, acc=F64)
    err = (dx - dx_ref).abs().max().item()
    print(f"{case}: max |model - autograd| = {err:.3e}")
    assert dx.shape == dx_ref.shape and err <= 1e-12


def test_relaid_weights_have_the_documented_slabs():
    n, c = 16, 8
    w = R.rnd((n, 9 * c), 5)
    w4d = w.reshape(n, 3, 3, c)
    ws = D.relaid(w, "stride2")
    assert ws.shape == (c, 9 * n) and ws.is_contiguous() and ws.dtype == F16
    for s, (ky, kx) in enumerate(D.STRIDE2_KYX):
        assert torch.equal(ws[:, s * n:(s + 1) * n], w4d[:, ky, kx].t()), (s, ky, kx)
    wu = D.relaid(w, "ups")
    assert wu.shape == (c, 16 * n) and wu.is_contiguous() and wu.dtype == F16
    sets = {-1: (2,), 0: (1, 2), 1: (0, 1), 2: (0,)}
    for s, (e, f) in enumerate(D.UPS_SRC):
        want = sum(w4d[:, ky, kx].float() for ky in sets[e] for kx in sets[f]).to(F16)      # fp32 sum, rounded once
        assert torch.equal(wu[:, s * n:(s + 1) * n], want.t()), (s, e, f)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_model_with_the_kernels_rounding_points_is_inside_the_tolerance(dtype):
    """16-bit W4, fp32 sums, dx rounded once: elementwise inside the tolerance the GPU suite applies to the kernel."""
    atol, rtol = N.TOL16[dtype]
    worst = 0.0
    for case in D.CASES:
        dy, w, dx_ref = D.case_operands(case, dtype)
        dx = D.model(dy, D.relaid(w, case.mode), case.mode, case.h, case.w)
        assert dx.dtype == dtype
        ratio = D.bound_ratio(dx, dx_ref, atol, rtol)
        alone = D.bound_ratio(dx_ref.to(dtype), dx_ref, atol, rtol)
        print(f"{case} {dtype}: worst err/bound {ratio:.3f} (rounding the float64 dx alone {alone:.3f})")
        worst = max(worst, ratio)
        N.close16(dx, dx_ref, f"model {case}")
    print(f"{dtype}: worst err/bound over the cases {worst:.3f}")


@pytest.mark.parametrize("case", D.EXACT_CASES, ids=["stride2", "ups"])
def test_model_is_exact_on_integers(case):
    dy, w, dx_ref = D.exact_operands(case)
    dx = D.model(dy, D.relaid(w, case.mode), case.mode, case.h, case.w)
    assert dx.dtype == F16 and torch.equal(dx.double(), dx_ref)


# ---- resolve -----------------------------------------------------------------------------------------------------------
def describe(case, **over):
    ho, wo = D.out_hw(case)
    d = L.DgradDesc()
    d.dy, d.wt, d.dx = 4096, 8192, 12288              # resolve reads no buffer: aligned stand-ins
    d.B, d.Hi, d.Wi, d.C, d.Ho, d.Wo, d.N = case.b, case.h, case.w, case.c, ho, wo, case.n
    d.mode, d.ld_dy, d.ld_dx = (L.DGRAD_UPS if case.mode == "ups" else L.DGRAD_STRIDE2), case.n, case.c
    for k, v in over.items():
        setattr(d, k, v)
    return d


def resolve(handle, d):
    ch = L.DgradChoice()
    rc = handle.dadd_conv_dgrad_resolve(ctypes.byref(d), ctypes.byref(ch))
    return rc, ch


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_resolve_classes_cover_every_pixel_once(handle, case):
    rc, ch = resolve(handle, describe(case))
    assert rc == L.DADD_OK, handle.dadd_last_error()
    so = 1 if case.mode == "ups" else 2
    cls = [ch.cls[i] for i in range(ch.nclass)]
    if case.mode == "ups":
        assert [(k.py, k.px, k.first_slab, k.ntaps) for k in cls] == [(0, 0, 0, 16)]
    else:
        assert [(k.py, k.px) for k in cls] == [(0, 0), (0, 1), (1, 0), (1, 1)]
        assert [k.ntaps for k in cls] == [1, 2, 2, 4] and sum(k.ntaps for k in cls) == 9
        assert [(k.first_slab, k.ntaps) for k in cls] == [D.STRIDE2_CLASSES[(k.py, k.px)] for k in cls]
    tile, seen = 0, set()
    for k in cls:                                      # contiguous tile ranges; the pixel set rebuilt from the table
        assert k.first_tile == tile and k.pixels > 0
        tile += -(-k.pixels // 64)
        pix = {(b, y, x) for b in range(case.b) for y in range(k.py, case.h, so) for x in range(k.px, case.w, so)}
        assert len(pix) == k.pixels and not pix & seen
        seen |= pix
    assert len(seen) == case.b * case.h * case.w
    assert (ch.grid_x, ch.grid_y, ch.block) == (tile, case.c // 64, 256)
    assert 0 < ch.smem <= 64 * 1024


def test_resolve_divides_the_larger_operand_among_the_xcds(handle):
    """xcd_by_c: the weight is larger than dy and the grid deals evenly to 8 XCDs (placement only)."""
    for case, want in ((D.Case("ups", 8, 8, 8, 1280, 1280), 1),          # 52 MB of weight, 5 MB of dy
                       (D.Case("stride2", 8, 16, 16, 1280, 1280), 1),
                       (D.Case("stride2", 8, 64, 64, 320, 320), 0),      # dy is the larger operand
                       (D.Case("ups", 8, 32, 32, 640, 640), 0),
                       (D.Case("ups", 1, 3, 5, 1280, 1280), 0)):         # 1 x 20 workgroups: not a multiple of 8
        rc, ch = resolve(handle, describe(case))
        assert rc == L.DADD_OK and ch.xcd_by_c == want, (case, ch.xcd_by_c, ch.grid_x, ch.grid_y)
    for case in D.CASES[7:]:                                             # the cases the GPU suite renumbers with
        rc, ch = resolve(handle, describe(case))
        assert rc == L.DADD_OK and ch.xcd_by_c == 1 and ch.grid_x * ch.grid_y >= 16, (case, ch.grid_x, ch.grid_y)


def test_resolve_drops_the_empty_classes_of_a_one_pixel_map(handle):
    rc, ch = resolve(handle, describe(D.Case("stride2", 3, 1, 1, 64, 64)))
    assert rc == L.DADD_OK and ch.nclass == 1 and (ch.cls[0].py, ch.cls[0].px, ch.cls[0].pixels, ch.grid_x) == (0, 0, 3, 1)


@pytest.mark.parametrize("bad", ["C=96", "N=70", "Ho", "Wo ups", "ld_dx=12", "mode", "B=0", "dy unaligned", "wt null"])
def test_resolve_refuses(handle, bad):
    case = D.CASES[4] if bad == "Wo ups" else D.CASES[0]
    over = {"C=96": dict(C=96, ld_dx=96), "N=70": dict(N=70, ld_dy=72), "Ho": dict(Ho=9), "Wo ups": dict(Wo=15),
            "ld_dx=12": dict(ld_dx=12), "mode": dict(mode=2), "B=0": dict(B=0), "dy unaligned": dict(dy=4104),
            "wt null": dict(wt=None)}[bad]
    ch = L.DgradChoice()
    ch.grid_x = -7
    rc = handle.dadd_conv_dgrad_resolve(ctypes.byref(describe(case, **over)), ctypes.byref(ch))
    assert rc == L.DADD_EINVAL and ch.grid_x == -7
    assert b"dgrad" in handle.dadd_last_error()
