"""CPU checks: the C-ABI library builds for gfx950, loads, and exports every symbol that
include/dadd_hip.h declares (no compute calls — there is no GPU here); the ctypes prototype table
covers the header; the parameter inventory reproduces the published SD-1.4 / DADD counts; the
product has no CPU path and says so loudly."""
import ctypes
import os
import re

import pytest
import torch

from progressive_stable_diffusion_amd import lib as L
from progressive_stable_diffusion_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions(header="dadd_hip.h"):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dadd_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    path = L.build()
    assert os.path.exists(path)
    handle = ctypes.CDLL(path)
    names = _header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(handle, n), f"{n} declared in dadd_hip.h but not exported"
    assert set(names) == set(L.PROTOTYPES), set(names) ^ set(L.PROTOTYPES)
    assert handle.dadd_version() == 100


def test_registry_covers_every_header_exactly():
    """``lib.HEADER_PROTOTYPES`` has one table per header under include/, with exactly the functions that header
    declares; the tables are pairwise disjoint, their union is ``lib.ALL_PROTOTYPES``, and the library exports all of it."""
    headers = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h"))
    assert headers == sorted(L.HEADER_PROTOTYPES)
    for h in headers:
        declared = set(_header_functions(h))
        assert declared == set(L.HEADER_PROTOTYPES[h]), (h, declared ^ set(L.HEADER_PROTOTYPES[h]))
    tables = list(L.HEADER_PROTOTYPES.values())
    for i, a in enumerate(tables):
        for b in tables[i + 1:]:
            assert not set(a) & set(b), set(a) & set(b)
    union = {}
    for t in tables:
        union.update(t)
    assert union == L.ALL_PROTOTYPES and len(L.ALL_PROTOTYPES) == sum(len(t) for t in tables)
    handle = ctypes.CDLL(L.build())
    assert not [n for n in L.ALL_PROTOTYPES if not hasattr(handle, n)]
    # ... and the names __graft_entry__.build() requires of the library are that union, no table forgotten
    import __graft_entry__ as G
    assert G.entry_points() == list(L.ALL_PROTOTYPES)


def test_igemm_desc_layout_matches_header(tmp_path):
    """The ctypes mirror of ``dadd_igemm_desc`` against the C compiler's view of include/dadd_hip.h (size and the
    offset of every field)."""
    import subprocess
    fields = [f[0] for f in L.IgemmDesc._fields_]
    assert fields[:8] == ["x", "x2", "w", "out", "partial", "bias", "rowvec", "residual"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dadd_hip.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(dadd_igemm_desc));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(dadd_igemm_desc, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert ctypes.sizeof(L.IgemmDesc) == out[0]
    assert [getattr(L.IgemmDesc, f).offset for f in fields] == out[1:]


def _c_program_output(tmp_path, body):
    """The integers a C program that includes include/dadd_hip.h prints, one per line of ``body``."""
    import subprocess
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dadd_hip.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    return [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]


def test_igemm_choice_layout_matches_header(tmp_path):
    """... and the mirror of ``dadd_igemm_choice`` (what the resolve entry points fill), the same way."""
    fields = [f[0] for f in L.IgemmChoice._fields_]
    assert fields[:2] == ["kernel", "finish"]
    out = _c_program_output(tmp_path, '  printf("%zu\\n", sizeof(dadd_igemm_choice));\n'
                            + "".join(f'  printf("%zu\\n", offsetof(dadd_igemm_choice, {f}));\n' for f in fields))
    assert ctypes.sizeof(L.IgemmChoice) == out[0]
    assert [getattr(L.IgemmChoice, f).offset for f in fields] == out[1:]


def test_host_entry_points_are_declared_exported_and_bound():
    """The bf16 sibling of the resolve entry point: include/dadd_hip_host.h and ``lib.HOST_PROTOTYPES``, same argument
    list as the fp16 form of include/dadd_hip.h."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dadd_hip_host.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(dadd_[a-z0-9_]+)\s*\(", text)) == set(L.HOST_PROTOTYPES) == {"dadd_conv_igemm_resolve_bf16"}
    assert L.HOST_PROTOTYPES["dadd_conv_igemm_resolve_bf16"] == L.PROTOTYPES["dadd_conv_igemm_resolve_f16"]
    assert L.PROTOTYPES["dadd_conv_igemm_resolve_f16"][1][2]._type_ is L.IgemmChoice
    handle = ctypes.CDLL(L.build())
    assert hasattr(handle, "dadd_conv_igemm_resolve_bf16")


def test_flag_constants_match_header(tmp_path):
    """Every EPI_* / PRE_* / TUNE_* constant of lib.py against the header's #define of the same name, through the C
    compiler; and the header defines no such flag that lib.py lacks."""
    names = sorted(n for n in vars(L) if re.match(r"(EPI|PRE|TUNE)_[A-Z0-9_]+$", n))
    assert len(names) >= 17
    header = re.findall(r"#define\s+DADD_((?:EPI|PRE|TUNE)_[A-Z0-9_]+)\b", open(os.path.join(ROOT, "include", "dadd_hip.h")).read())
    assert set(header) - {"EPI_ACT_MASK"} == set(names), set(header) ^ set(names)
    out = _c_program_output(tmp_path, "".join(f'  printf("%d\\n", DADD_{n});\n' for n in names))
    assert out == [getattr(L, n) for n in names]
    assert _c_program_output(tmp_path, '  printf("%d\\n", DADD_EPI_ACT_MASK);\n') == [L.EPI_QUICKGELU | L.EPI_GELU | L.EPI_SIGMOID]


def test_status_codes_map_to_reference_exceptions():
    L.load()
    L.check(0)
    with pytest.raises(ValueError):
        L.check(L.DADD_EINVAL)
    with pytest.raises(RuntimeError):
        L.check(L.DADD_EHIP)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_product_has_no_cpu_path():
    from progressive_stable_diffusion_amd.backend import HipBackend
    from progressive_stable_diffusion_amd.config import default_config
    from progressive_stable_diffusion_amd.diffusion_module_ip import DiffusionModuleWithIP
    with pytest.raises(RuntimeError):
        HipBackend(torch.device("cuda:0"))
    with pytest.raises(RuntimeError):
        DiffusionModuleWithIP(default_config(), state_dict={}, device="cuda:0")


def test_parameter_inventory_matches_published_counts():
    u = W.unet_shapes()
    base = {k: s for k, s in u.items() if ".processor." not in k}
    assert W.count_params(base) == 859_520_964                      # SD-1.x UNet2DConditionModel
    assert W.count_params(u) - W.count_params(base) == 2 * 768 * 12480   # to_k_dis/to_v_dis, 16 sites
    assert W.count_params(W.vae_shapes()) == 83_653_863             # SD-1.x AutoencoderKL
    assert W.count_params(W.vae_shapes(encoder=False)) == 49_490_199
    c = W.conditioning_shapes()
    for prefix, n in (("ordinal_embedder", 20_096_256), ("image_projection", 14_976_768),
                      ("feature_purifier", 5_908_224)):
        assert W.count_params({k: s for k, s in c.items() if k.startswith(prefix)}) == n
    assert W.count_params(W.conditioning_shapes(projection_plus=False, purifier=False)) - 20_096_256 == 9_451_008
    assert len([k for k in u if k.endswith("anat_gate")]) == 16


def test_seeded_init_is_order_independent_and_reference_like():
    sh = W.conditioning_shapes()
    a = W.init_state_dict(sh, 3)
    keys = list(sh)[::-1]
    b = W.init_state_dict(sh, 3, keys=keys)
    assert all(torch.equal(a[k], b[k]) for k in sh)
    assert not torch.equal(a["ordinal_embedder.base"], W.init_state_dict(sh, 4)["ordinal_embedder.base"])
    d = a["ordinal_embedder.deltas"]
    assert d.shape == (3, 768) and 0.03 < d[0].mean() < 0.07 and d[2].mean() > d[0].mean()   # monotone init
    u = W.unet_shapes()
    ap = "unet.unet.mid_block.attentions.0.transformer_blocks.0.attn2"
    ks = [k for k in u if k.startswith(ap)]
    warm = W.init_state_dict(u, 0, keys=ks)
    assert torch.equal(warm[ap + ".processor.to_k_dis.weight"], warm[ap + ".to_k.weight"])   # routing_gates.py:308-314
    cold = W.init_state_dict(u, 0, keys=ks, warm_start_dis=False)
    assert not torch.equal(cold[ap + ".processor.to_k_dis.weight"], cold[ap + ".to_k.weight"])
    g = W.init_state_dict(u, 0, keys=ks, gates={"disease": (0.9, 0.1)})
    assert float(g[ap + ".processor.anat_gate"]) == pytest.approx(0.9)
