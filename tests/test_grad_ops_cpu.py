"""Not-GPU: the weight re-layout behind the data gradient, checked through the plain-torch igemm of the test-suite
against float64 autograd, and the binding of the weight-gradient entry points."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from progressive_stable_diffusion_amd import lib as L
from progressive_stable_diffusion_amd.grad_ops import dgrad_weight
from tests import grad_reference as R
from tests.torch_backend import TorchRefBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("b,h,c,n", [(2, 12, 64, 128), (2, 8, 128, 64)])
def test_dgrad_weight_through_the_forward_gemm_is_the_data_gradient(b, h, c, n):
    x, dy = R.rnd((b, h, h, c), 1), R.rnd((b, h, h, n), 2)
    w = R.rnd((n, 9 * c), 3, (9 * c) ** -0.5)
    _, dx_ref, _, _ = R.conv_autograd(x, w, dy, 9)
    dx = torch.zeros((b, h, h, c), dtype=torch.float16)
    TorchRefBackend().igemm(dy, dgrad_weight(w, 9), dx, taps=9, pad=1)
    R.close(dx, dx_ref, f"dx {b}x{h}x{h} {n}->{c}")


@pytest.mark.parametrize("taps", [1, 9])
def test_dgrad_weight_is_an_involution(taps):
    w = R.rnd((72, taps * 64), 4)
    wt = dgrad_weight(w, taps)
    assert wt.shape == (64, taps * 72) and wt.is_contiguous()
    assert wt[5, (taps - 1) * 72 + 7] == w[7, 5]                 # first tap of w is the last tap of wt
    assert torch.equal(dgrad_weight(wt, taps), w)


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(dadd_[a-z0-9_]+)\s*\(", text))


def test_wgrad_entry_points_are_declared_exported_and_bound():
    """fp16 form: include/dadd_hip.h and ``lib.PROTOTYPES``; bf16 sibling: include/dadd_hip_grad.h and
    ``lib.GRAD_PROTOTYPES``; both exported by the library with the same argument list."""
    assert "dadd_conv_wgrad_f16" in _declared("dadd_hip.h") and "dadd_conv_wgrad_f16" in L.PROTOTYPES
    assert _declared("dadd_hip_grad.h") == set(L.GRAD_PROTOTYPES) == {"dadd_conv_wgrad_bf16"}
    assert L.GRAD_PROTOTYPES["dadd_conv_wgrad_bf16"] == L.PROTOTYPES["dadd_conv_wgrad_f16"]
    assert L.PROTOTYPES["dadd_conv_wgrad_f16"][1][0]._type_ is L.WgradDesc
    assert {"wgrad.hip", "wgrad_bf16.hip"} <= set(L.SOURCES)
    handle = ctypes.CDLL(L.build())
    assert hasattr(handle, "dadd_conv_wgrad_f16") and hasattr(handle, "dadd_conv_wgrad_bf16")


def test_wgrad_desc_layout_matches_header(tmp_path):
    fields = [f[0] for f in L.WgradDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dadd_hip_grad.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(dadd_wgrad_desc));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(dadd_wgrad_desc, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert ctypes.sizeof(L.WgradDesc) == out[0]
    assert [getattr(L.WgradDesc, f).offset for f in fields] == out[1:]
