"""TEST-ONLY harness (no tests here): every launch of a plan against a float64 restatement of the same op.

``AuditBackend(inner, ref64, ref32)`` has the backend interface the plans use.  A plan built with it records its bound
methods, so running the plan runs, per launch: the launch itself on ``inner`` (a ``HipBackend``; on the CPU a
``TorchRefBackend`` or a deliberately wrong subclass of it), then the same op from the same input tensors twice more -
``r`` in float64 and ``r32`` with fp32 arithmetic rounded to the output type, which is what the kernel tests compare
with - and two comparisons.  The next launch reads what ``inner`` wrote: nothing accumulates from launch to launch
(teacher forcing), and a wrong launch is reported where it happens and nowhere else.

Criteria (u = 2^-11 for fp16, 2^-9 for bf16; fp32 accumulation has unit 2^-24):
  elementwise  linear igemm (bias / rowvec / residual / split-K, with or without statistics side outputs):
                   |o - r| <= 2 u |r| + K 2^-24 A + tiny,   K = taps * Cin,
               A = the same launch on absolute values, |x| conv |w| + |bias| + |rowvec| + |residual| in float64: the
               worst case of ANY fp32 summation order of the K products plus the rounding of the result, so a correct
               kernel cannot exceed it whatever its tiling or slice count;
               every other 16-bit output: the tolerance the kernel tests give that op (``TOL`` below, one table),
               atol * max(1, rms(r)) + rtol |r|;   fp32 outputs: the kernel tests' tolerances as they stand;
               statistics side outputs (GroupNorm chunk partials, LayerNorm row partials): against float64 sums over
               the 16-bit output THE SAME LAUNCH STORED, within n_terms 2^-24 sum|term|.
  RMS          16-bit outputs only: rms(o - r) <= 1.5 rms(r32 - r).  r32 carries one rounding of the result; a kernel with
               an independent second rounding of the same size costs sqrt 2; 1.5 is that plus slack.  This assumes the
               float64 reference rounds where the kernel documents a 16-bit intermediate (the model references below).

The float64 reference writes its convolutions as im2col + matmul (nothing depends on a convolution library's kernel
search) in bands that fit beside the VAE's 512x512 maps, and its attention per sample.
"""
from __future__ import annotations

import inspect
import math
import time
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from progressive_stable_diffusion_amd.lib import (EPI_GEGLU, EPI_GELU, EPI_GNAPPLY_SILU, EPI_LNFOLD, EPI_QUICKGELU, EPI_SIGMOID,
                                                 PRE_GN)
from tests import attention_cases as AC
from tests.torch_backend import TorchRefBackend

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
U = {F16: 2.0 ** -11, BF16: 2.0 ** -9}
U32 = 2.0 ** -24
RMS_LIMIT = 1.5
REPORT_ABOVE = 1.1
# (op, tensor) -> why its RMS ratio sits above 1.1 although the launch is right.  A ratio above 1.1 with no entry here is
# printed as unexplained.  Empty today: on MI355X every launch of the audited plans measures 0.73 to 1.004 once the
# reference of conv_in_nchw rounds the latents to the plan's storage type as the kernel does (bf16 plans: 1.43 before).
REASONS = {}

EPI_ACT = EPI_QUICKGELU | EPI_GELU | EPI_SIGMOID
NONLINEAR = EPI_GEGLU | EPI_LNFOLD | EPI_ACT | PRE_GN

# (dtype, key) -> (atol, rtol, the test the pair comes from).  One place; nothing else in the audit holds a tolerance.
TOL = {
    (F16, "igemm.lnfold"): (6e-3, 6e-3, "test_gpu_kernels.py::test_igemm_layernorm_fold"),
    (F16, "igemm.geglu"): (3e-3, 3e-3, "test_gpu_kernels.py::test_igemm_geglu"),
    (F16, "igemm.act"): (3e-3, 3e-3, "test_gpu_kernels.py::test_igemm_activation_epilogues"),
    (F16, "igemm.pre_gn"): (2e-3, 1e-3, "test_gpu_kernels.py::test_conv3x3_halo_groupnorm_on_the_way_in"),
    (F16, "igemm.pre_gn_cat"): (3e-3, 2e-3, "test_gpu_kernels.py::test_conv3x3_halo_groupnorm_over_skip_concat"),
    (F16, "igemm.gn_apply"): (6e-3, 6e-3, "test_gpu_kernels.py::test_splitk_finish_with_groupnorm_apply"),
    (F16, "groupnorm"): (3e-3, 2e-3, "test_gpu_kernels.py::test_groupnorm"),
    (F16, "layernorm"): (2e-3, 2e-3, "test_gpu_kernels.py::test_layernorm"),
    (F16, "self_attn"): (3e-3, 3e-3, "test_gpu_kernels.py::test_self_attention"),
    (F16, "attention"): (3e-3, 3e-3, "test_gpu_kernels.py::test_attention_separate_query_and_key_lengths"),
    (F16, "tri_xattn"): (4e-3, 4e-3, "test_gpu_kernels.py::test_tri_xattn"),
    (F16, "attn2_fused"): (4e-3, 3e-3, "test_gpu_kernels.py::test_attn2_fused"),
    (F16, "attn2_fused.lnfold"): (8e-3, 6e-3, "test_gpu_kernels.py::test_attn2_fused (norm2 folded)"),
    (F16, "ffn_block"): (6e-3, 4e-3, "test_gpu_kernels.py::test_ffn_block"),
    (F16, "tf_head.hs"): (3e-3, 3e-3, "test_gpu_kernels.py::test_tf_head"),
    (F16, "tf_head.qkv"): (6e-3, 4e-3, "test_gpu_kernels.py::test_tf_head"),
    (F16, "pack_latents"): (2e-3, 2e-3, "test_gpu_kernels.py::test_thin_convs_and_pack"),
    (F16, "conv_cin8"): (3e-3, 2e-3, "test_gpu_kernels.py::test_thin_convs_and_pack"),
    (F16, "conv_in_nchw"): (3e-3, 2e-3, "test_gpu_kernels.py::test_thin_convs_and_pack"),
    (BF16, "igemm.lnfold"): (3e-2, 2e-2, "test_gpu_bf16.py::test_igemm_bf16_layernorm_fold_and_statistics"),
    (BF16, "igemm.geglu"): (2e-2, 1.6e-2, "test_gpu_bf16.py::test_igemm_bf16"),
    (BF16, "igemm.act"): (2e-2, 1.6e-2, "test_gpu_bf16.py::test_igemm_bf16"),
    (BF16, "igemm.pre_gn"): (3e-2, 2e-2, "test_gpu_bf16.py::test_halo_conv_bf16"),
    (BF16, "igemm.pre_gn_cat"): (3e-2, 2e-2, "test_gpu_bf16.py::test_halo_conv_bf16"),
    (BF16, "igemm.gn_apply"): (4e-2, 3e-2, "test_gpu_bf16.py::test_splitk_finish_gn_and_gnapply_bf16"),
    (BF16, "groupnorm"): (2e-2, 1.6e-2, "test_gpu_bf16.py::test_groupnorm_bf16"),
    (BF16, "layernorm"): (1.6e-2, 1.6e-2, "test_gpu_bf16.py::test_layernorm_bf16"),
    (BF16, "self_attn"): (2e-2, 2e-2, "test_gpu_bf16.py::test_self_attention_bf16"),
    (BF16, "attention"): (2e-2, 2e-2, "test_gpu_bf16.py::test_self_attention_bf16"),
    (BF16, "tri_xattn"): (2.5e-2, 2.5e-2, "test_gpu_bf16.py::test_tri_xattn_bf16"),
    (BF16, "conv_in_nchw"): (1.6e-2, 1.6e-2, "test_gpu_bf16.py::test_conv_in_and_conv_out_bf16"),
    # fp32 outputs: the tolerance as the kernel test states it, no scale factor
    (F32, "conv_cout4"): (1e-3, 1e-3, "test_gpu_kernels.py::test_thin_convs_and_pack, test_gpu_bf16.py::test_conv_in_and_conv_out_bf16"),
    (F32, "timestep_features"): (2e-4, 0.0, "test_gpu_kernels.py::test_time_rows_and_linear"),
    (F32, "linear_rows"): (2e-4, 2e-4, "test_gpu_kernels.py::test_time_rows_and_linear"),
}
# gaussian_sample has no kernel-level tolerance of its own.  It is three fp32 operations on fp32 inputs and one expf whose
# argument 0.5 * logvar is at most 15 in magnitude (the clamp): the argument's rounding costs 15 * 2^-24 ~ 1e-6 relative,
# expf and the three roundings a few 2^-24 more - 1e-5 of (|mean| + |std * noise|) * scale is ten times that.
GAUSSIAN_RTOL, GAUSSIAN_ATOL = 1e-5, 1e-6

# Launch counts of the audited plans as the CPU census sees them (tests/test_launch_audit_cpu.py builds each plan on the
# shape backend and asserts these; tests/test_gpu_launch_audit.py asserts them of the plan it runs on the GPU).
FINGERPRINT_NAMES = ("igemm", "tf_head", "attn2_fused", "ffn_block", "self_attn", "_xattn", "groupnorm", "layernorm")
FINGERPRINTS = {
    # UNetPlan(4, 64) fp16, the benchmark's plan
    "bench": dict(igemm=157, tf_head=5, attn2_fused=5, ffn_block=5, self_attn=16, _xattn=11, groupnorm=22, layernorm=11, ops=234),
    # ... with FUSED_FFN = FUSED_HEAD = FUSED_ATTN2 = False, and the bf16 plan (no row-block fusions): the same launches
    "bench_unfused": dict(igemm=192, tf_head=0, attn2_fused=0, ffn_block=0, self_attn=16, _xattn=16, groupnorm=27, layernorm=11, ops=264),
    "bench_bf16": dict(igemm=192, tf_head=0, attn2_fused=0, ffn_block=0, self_attn=16, _xattn=16, groupnorm=27, layernorm=11, ops=264),
    # UNetPlan(2, 24), fp16 and bf16
    "s24": dict(igemm=192, tf_head=0, attn2_fused=0, ffn_block=0, self_attn=16, _xattn=16, groupnorm=18, layernorm=16, ops=260),
}


def fingerprint(plan):
    names = [getattr(fn, "__name__", "") for fn, _, _ in plan.ops]
    fp = {n: names.count(n) for n in FINGERPRINT_NAMES}
    fp["ops"] = len([n for n in names if not n.startswith("prefetch")])
    return fp


def igemm_signature(w, out, kw):
    """N, K, taps, geglu, residual, ups, stride, flags, splitk, tile_m, tile_n of one igemm launch."""
    flags = int(kw.get("flags", 0))
    return (int(w.shape[0]), int(w.shape[1]), int(kw.get("taps", 1)), bool(flags & EPI_GEGLU), kw.get("residual") is not None,
            int(bool(kw.get("ups", 0))), int(kw.get("stride", 1)), flags, int(kw.get("splitk", 1)), int(kw.get("tile_m", 0)),
            int(kw.get("tile_n", 0)))


# ------------------------------------------------------------------------------------------------ float64 reference
class Im2colRefBackend(TorchRefBackend):
    """``TorchRefBackend`` with the convolution written as im2col (``F.unfold`` after the explicit padding) + matmul, per
    sample and in bands of output rows: the result depends on GEMM only, not on a convolution library's kernel search,
    and the 512x512 maps of the VAE fit.  In fp32 this is the audit's ``r32``."""
    name = "torch-ref-im2col"
    MAX_COLS = 1 << 27          # elements of one im2col band (1 GiB in float64)

    def conv2d(self, x, w, bias=None, stride=1, padding=0):
        if padding:
            x = F.pad(x, (padding,) * 4)
        n, cin, kh, kw = w.shape
        bsz, _, h, wd = x.shape
        ho, wo = (h - kh) // stride + 1, (wd - kw) // stride + 1
        wm = w.reshape(n, cin * kh * kw)                 # (c, ky, kx): the row order of F.unfold
        out = x.new_empty(bsz, n, ho, wo)
        rows = max(1, min(ho, self.MAX_COLS // (cin * kh * kw * wo)))
        for bi in range(bsz):
            for r0 in range(0, ho, rows):
                r1 = min(ho, r0 + rows)
                band = x[bi:bi + 1, :, r0 * stride:(r1 - 1) * stride + kh, :]
                cols = band.reshape(cin, -1) if (kh, kw, stride) == (1, 1, 1) else F.unfold(band, (kh, kw), stride=stride)[0]
                out[bi, :, r0:r1] = (wm @ cols).reshape(n, r1 - r0, wo)
        if bias is not None:
            out += bias[None, :, None, None]
        return out


class Float64RefBackend(Im2colRefBackend):
    """The audit's ``r``: float64, with the attention kernels' documented 16-bit intermediates in place."""
    name = "torch-ref-f64"

    def __init__(self, device="cpu"):
        super().__init__(device, compute=F64)

    # flash_kernel (csrc/attention.hip) rounds twice on the way: q * log2(e)/sqrt(d) to the storage type (the scale rides
    # on Q) and P = exp2(s - rowmax) to the storage type before P v and before the row sum.  tests/attention_cases.py
    # states that model in float64; it takes (batch, head) slices in chunks, here one sample at a time.
    def _flash(self, q, k, v, out, heads):
        for bi in range(q.shape[0]):
            _, model = AC.references(q[bi:bi + 1], k[bi:bi + 1], v[bi:bi + 1], heads)
            out[bi:bi + 1].copy_(model.to(out.dtype))

    def self_attn(self, qkv, out, heads):
        c = qkv.shape[-1] // 3
        self._flash(qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:], out, heads)

    def attention(self, q, k, v, out, heads):
        c = out.shape[-1]
        self._flash(q[..., :c], k[..., :c], v[..., :c], out, heads)

    # xattn_kernel rounds once on the way: the normalised, gate-weighted probabilities gate * softmax(s) go to the storage
    # type for the P v MFMA (pack_p); the logits and the softmax are fp32 from unrounded q.
    def tri_xattn(self, q, kv, out, gates, lam, mode, heads, lam_dev=None):
        if lam_dev is not None:
            lam = float(lam_dev.reshape(-1)[0])
        b, n, c = q.shape
        d = c // heads
        qh = self.c(q).view(b, n, heads, d).transpose(1, 2)

        def path(wgt, tok0, ntok, kcol, vcol):
            k = self.c(kv[:, tok0:tok0 + ntok, kcol:kcol + c]).view(b, ntok, heads, d).transpose(1, 2)
            v = self.c(kv[:, tok0:tok0 + ntok, vcol:vcol + c]).view(b, ntok, heads, d).transpose(1, 2)
            p = wgt * torch.softmax(qh @ k.transpose(-1, -2) / math.sqrt(d), dim=-1)
            return self.c(p.float().to(q.dtype)) @ v

        if mode == 0:
            z = path(self.c(gates[0]), 16, 16, 0, c) + path(self.c(gates[1]), 0, 16, 2 * c, 3 * c)
            if lam != 0.0:
                z = z + path(float(torch.tensor(lam, dtype=F32)), 32, 16, 2 * c, 3 * c)
        else:
            z = path(1.0, 0, 32, 0, c)
        out.copy_(z.transpose(1, 2).reshape(b, n, c).to(out.dtype))


# ------------------------------------------------------------------------------------------------ the wrapper
PLUMBING = ("name", "device", "ctx", "empty", "zeros", "to_device", "copy_", "zero_", "clone", "synchronize", "wait_current",
            "release_to_current", "prefetch", "prefetch_join", "graph_launch", "graph_destroy", "stream", "lib")


def _tensors(v):
    if isinstance(v, torch.Tensor):
        yield v
    elif isinstance(v, (tuple, list)):
        for e in v:
            yield from _tensors(e)


def _extent(t):
    lo = t.data_ptr()
    return lo, lo + (sum((s - 1) * st for s, st in zip(t.shape, t.stride()) if s > 0) + 1) * t.element_size() if t.numel() else lo


def _rms(t):
    return float(torch.sqrt((t * t).mean())) if t.numel() else 0.0


class AuditFailure(AssertionError):
    pass


class AuditBackend:
    """See the module docstring.  ``records`` holds one dict per compared tensor; ``launches`` counts audited launches."""

    def __init__(self, inner, ref64, ref32):
        self.inner, self.ref64, self.ref32 = inner, ref64, ref32
        self.records, self.launches = [], 0
        self.log = []               # (op, bound arguments) of launch 1, 2, ...: what the tests select launches by

    def __getattr__(self, name):                    # plumbing goes straight through; anything else is an error
        if name in PLUMBING:
            return getattr(self.inner, name)
        raise AttributeError(f"AuditBackend has no pass-through for {name!r}: the audit is eager and covers the plans' ops only")

    def graph_begin(self):
        raise RuntimeError("the launch audit is eager only: run the plan with use_graph=False")

    # -- bookkeeping ---------------------------------------------------------------------------------
    def failures(self):
        return [r for r in self.records if not r["ok"]]

    def failed_launches(self):
        return sorted({r["launch"] for r in self.records if not r["ok"]})

    @staticmethod
    def describe(r):
        return (f"launch {r['launch']} {r['op']}.{r['what']} {r['sig']}: worst element {r['worst_index']} got {r['got']:.6e} "
                f"ref {r['ref']:.6e} at {r['elem_ratio']:.3f} of its bound; rms ratio {r['rms_ratio']:.3f} (limit {RMS_LIMIT})")

    def assert_clean(self):
        bad = self.failures()
        if bad:
            raise AuditFailure(f"{len(bad)} of {len(self.records)} compared tensors outside the criteria:\n"
                               + "\n".join(self.describe(r) for r in bad[:20]))

    # -- comparison ----------------------------------------------------------------------------------
    def _record(self, op, what, sig, o, r, bound, r32=None, t0=None):
        """``o`` what the launch stored, ``r`` float64, ``bound`` float64 elementwise, ``r32`` the rounded fp32 reference
        (16-bit outputs: adds the RMS criterion)."""
        o64 = o.to(F64)
        err = (o64 - r).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf"))
        flat = ratio.flatten()
        i = int(flat.argmax()) if flat.numel() else 0
        elem = float(flat[i]) if flat.numel() else 0.0
        rms_ratio = float("nan")
        if r32 is not None:
            mine, base = _rms((o64 - r).nan_to_num(nan=float("inf"))), _rms(r32.to(F64) - r)
            rms_ratio = mine / base if base > 0 else (1.0 if mine == 0 else float("inf"))
        ok = elem <= 1.0 and (r32 is None or rms_ratio <= RMS_LIMIT)
        self.records.append(dict(launch=self.launches, op=op, what=what, sig=sig, elem_ratio=elem, rms_ratio=rms_ratio, ok=ok,
                                 worst_index=tuple(int(x) for x in np.unravel_index(i, tuple(o.shape))) if flat.numel() else (),
                                 got=float(o64.flatten()[i]) if flat.numel() else 0.0, ref=float(r.flatten()[i]) if flat.numel() else 0.0,
                                 seconds=0.0 if t0 is None else time.perf_counter() - t0))

    def _tol_bound(self, key, r, dtype):
        atol, rtol, _ = TOL[(dtype, key)]
        s = 1.0 if dtype == F32 else max(1.0, _rms(r))
        return atol * s + rtol * r.abs()

    def _stats(self, op, what, sig, got, terms, dims, t0):
        """Statistics side output: (sum, sum of squares) over ``dims`` of ``terms`` (float64 view of the stored 16-bit
        output), stacked on a last axis, against ``got``: n_terms 2^-24 sum|term| each."""
        n = 1
        for d in dims:
            n *= terms.shape[d]
        sq = terms * terms
        want = torch.stack([terms.sum(dim=dims), sq.sum(dim=dims)], dim=-1)
        bound = n * U32 * torch.stack([terms.abs().sum(dim=dims), sq.sum(dim=dims)], dim=-1)
        return want, bound

    # -- one launch ----------------------------------------------------------------------------------
    def _launch(self, op, args, kwargs, outs, strip=(), work=()):
        """Run ``op`` on ``inner`` and on both references.  ``outs``: names of the compared outputs; ``strip``: side
        outputs the references do not write (compared apart, from what the launch stored); ``work``: workspaces.
        -> (bound arguments, {name: (o, r64, r32)})."""
        sig = inspect.signature(getattr(TorchRefBackend, op))
        ba = sig.bind(self.ref32, *args, **kwargs)
        ba.apply_defaults()
        a = OrderedDict(list(ba.arguments.items())[1:])
        written = [t for n in (*outs, *strip, *work) for t in _tensors(a[n])]
        reads = [t for n, v in a.items() if n not in outs and n not in strip and n not in work for t in _tensors(v)]
        for w in written:                       # no input may share storage with what the launch writes: then the
            wl, wh = _extent(w)                 # references below would read what the kernel already overwrote
            for rd in reads:
                rl, rh = _extent(rd)
                assert rh <= wl or wh <= rl, f"{op}: an input {tuple(rd.shape)} shares storage with an output {tuple(w.shape)}"
        getattr(self.inner, op)(*args, **kwargs)
        self.launches += 1
        self.log.append((op, a))
        res = {}
        with self.inner.ctx():
            calls = []
            for ref, dt in ((self.ref64, F64), (self.ref32, None)):
                b = OrderedDict(a)
                for n in strip:
                    b[n] = None
                for n in work:
                    b[n] = None
                for n in outs:
                    b[n] = torch.zeros(a[n].shape, dtype=dt or a[n].dtype, device=a[n].device)
                pos = [b[p.name] for p in list(sig.parameters.values())[1:] if p.kind == p.POSITIONAL_OR_KEYWORD]
                kw = {p.name: b[p.name] for p in sig.parameters.values() if p.kind == p.KEYWORD_ONLY}
                getattr(ref, op)(*pos, **kw)
                calls.append(b)
            for n in outs:
                res[n] = (a[n], calls[0][n], calls[1][n])
        return a, res

    def _simple(self, op, args, kwargs, outs, key=None, sig=None, **kw):
        t0 = time.perf_counter()
        a, res = self._launch(op, args, kwargs, outs, **kw)
        with self.inner.ctx():
            for n, (o, r, r32) in res.items():
                k = key[n] if isinstance(key, dict) else (key or op)
                self._record(op, n, sig(a) if sig else tuple(a[outs[0]].shape), o, r, self._tol_bound(k, r, o.dtype),
                             r32 if o.dtype in U else None, t0)
        return a, res

    # -- the ops -------------------------------------------------------------------------------------
    def igemm(self, x, w, out, **kw):
        t0 = time.perf_counter()
        flags = int(kw.get("flags", 0))
        sig = igemm_signature(w, out, kw)
        a, res = self._launch("igemm", (x, w, out), kw, ("out",), strip=("gn_ws", "ln_stats_out", "gn_apply"),
                              work=("partial", "counters"))
        with self.inner.ctx():
            o, r, r32 = res["out"]
            if flags & NONLINEAR:
                key = ("igemm.lnfold" if flags & EPI_LNFOLD else "igemm.geglu" if flags & EPI_GEGLU else
                       ("igemm.pre_gn_cat" if len(a["gn_in"]) > 5 else "igemm.pre_gn") if flags & PRE_GN else "igemm.act")
                bound = self._tol_bound(key, r, o.dtype)
            else:                                   # |x| conv |w| + |bias| + |rowvec| + |residual|: the same launch on absolute values
                ab = lambda t: None if t is None else t.abs()           # noqa: E731
                amag = torch.zeros_like(r)
                self.ref64.igemm(x.abs(), w.abs(), amag, x2=ab(a["x2"]), bias=ab(a["bias"]), rowvec=ab(a["rowvec"]),
                                 residual=ab(a["residual"]), taps=a["taps"], stride=a["stride"], ups=a["ups"], pad=a["pad"],
                                 flags=flags & 7)
                fi = torch.finfo(o.dtype)
                bound = 2 * U[o.dtype] * r.abs() + w.shape[1] * U32 * amag + fi.smallest_normal * fi.eps
            self._record("igemm", "out", sig, o, r, bound, r32, t0)
            o64 = o.to(F64)
            b, ho, wo, n = o.shape
            if a["ln_stats_out"] is not None:       # [P][M][2] over blocks of N / P columns of the stored output
                st = a["ln_stats_out"]
                want, bound = self._stats("igemm", "ln_stats_out", sig, st, o64.reshape(b * ho * wo, st.shape[0], -1), (2,), t0)
                self._record("igemm", "ln_stats_out", sig, st, want.permute(1, 0, 2), bound.permute(1, 0, 2), None, t0)
            if a["gn_ws"] is not None:              # [B][nchunk][32][2] of the stored output
                nch = a["gn_nchunk"]
                want, bound = self._stats("igemm", "gn_ws", sig, None, o64.reshape(b, nch, -1, 32, n // 32), (2, 4), t0)
                self._record("igemm", "gn_ws", sig, a["gn_ws"][:want.numel()].reshape(want.shape), want, bound, None, t0)
            if a["gn_apply"] is not None:           # GroupNorm (+ SiLU) of the stored output, written beside it
                g_out, gam, bet, eps_o = a["gn_apply"]
                silu = bool(flags & EPI_GNAPPLY_SILU)
                g64, g32 = torch.zeros(g_out.shape, dtype=F64, device=g_out.device), torch.zeros_like(g_out)
                self.ref64.groupnorm(o, None, gam, bet, g64, None, 32, eps_o, silu)
                self.ref32.groupnorm(o, None, gam, bet, g32, None, 32, eps_o, silu)
                self._record("igemm", "gn_apply", sig, g_out, g64, self._tol_bound("igemm.gn_apply", g64, g_out.dtype), g32, t0)

    def groupnorm(self, *args, **kw):
        chunks = kw.get("ws_chunks", args[9] if len(args) > 9 else 0)
        self._simple("groupnorm", args, kw, ("out",), work=() if chunks else ("ws",),
                     sig=lambda a: (tuple(a["out"].shape), 0 if a["x2"] is None else int(a["x2"].shape[-1]), int(a["silu"]), int(a["ws_chunks"])))

    def layernorm(self, *args, **kw):
        self._simple("layernorm", args, kw, ("out",))

    def self_attn(self, *args, **kw):
        self._simple("self_attn", args, kw, ("out",), sig=lambda a: (tuple(a["out"].shape), int(a["heads"])))

    def attention(self, *args, **kw):
        self._simple("attention", args, kw, ("out",), sig=lambda a: (tuple(a["out"].shape), int(a["k"].shape[1]), int(a["heads"])))

    def tri_xattn(self, *args, **kw):
        self._simple("tri_xattn", args, kw, ("out",), sig=lambda a: (tuple(a["out"].shape), int(a["mode"]), float(a["lam"])))

    def _row_stats(self, op, sig, st, o, t0):
        o64 = o.to(F64)
        want, bound = self._stats(op, "ln_stats_out", sig, st, o64.reshape(-1, st.shape[0], o.shape[-1] // st.shape[0]), (2,), t0)
        self._record(op, "ln_stats_out", sig, st, want.permute(1, 0, 2), bound.permute(1, 0, 2), None, t0)

    def _chunk_stats(self, op, sig, ws, nch, o, t0):
        b, c = o.shape[0], o.shape[-1]
        want, bound = self._stats(op, "gn_ws", sig, None, o.to(F64).reshape(b, nch, -1, 32, c // 32), (2, 4), t0)
        self._record(op, "gn_ws", sig, ws[:want.numel()].reshape(want.shape), want, bound, None, t0)

    def attn2_fused(self, *args, **kw):
        t0 = time.perf_counter()
        fold = kw.get("ln_stats_in") is not None
        a, res = self._simple("attn2_fused", args, kw, ("out",), key="attn2_fused.lnfold" if fold else "attn2_fused",
                              strip=("ln_stats_out",), sig=lambda a: (tuple(a["out"].shape), fold, a["ln_stats_out"] is not None))
        if a["ln_stats_out"] is not None:
            with self.inner.ctx():
                self._row_stats("attn2_fused", tuple(a["out"].shape), a["ln_stats_out"], a["out"], t0)

    def ffn_block(self, *args, **kw):
        t0 = time.perf_counter()
        a, res = self._simple("ffn_block", args, kw, ("out",), strip=("gn_ws",),
                              sig=lambda a: (tuple(a["out"].shape), int(a["gn_nchunk"])))
        if a["gn_ws"] is not None:
            with self.inner.ctx():
                self._chunk_stats("ffn_block", tuple(a["out"].shape), a["gn_ws"], a["gn_nchunk"], a["out"], t0)

    def tf_head(self, *args, **kw):
        self._simple("tf_head", args, kw, ("hs", "qkv"), key={"hs": "tf_head.hs", "qkv": "tf_head.qkv"},
                     sig=lambda a: (tuple(a["hs"].shape), int(a["gn_nchunk"])))

    def conv_in_nchw(self, *args, **kw):
        t0 = time.perf_counter()
        a, res = self._simple("conv_in_nchw", args, kw, ("out",), strip=("gn_ws",),
                              sig=lambda a: (tuple(a["out"].shape), int(a["gn_nchunk"])))
        if a["gn_ws"] is not None:
            with self.inner.ctx():
                self._chunk_stats("conv_in_nchw", tuple(a["out"].shape), a["gn_ws"], a["gn_nchunk"], a["out"], t0)

    def conv_cin8(self, *args, **kw):
        self._simple("conv_cin8", args, kw, ("out",))

    def pack_latents(self, *args, **kw):
        self._simple("pack_latents", args, kw, ("out",))

    def conv_cout4(self, *args, **kw):
        self._simple("conv_cout4", args, kw, ("out",), sig=lambda a: (tuple(a["out"].shape), int(a["x"].shape[-1]), int(a["mode"])))

    def timestep_features(self, *args, **kw):
        self._simple("timestep_features", args, kw, ("out",))

    def linear_rows(self, *args, **kw):
        self._simple("linear_rows", args, kw, ("out",),
                     sig=lambda a: (tuple(a["out"].shape), int(a["x"].shape[1]), int(a["act_in"]), int(a["act_out"])))

    def gaussian_sample(self, mean, logvar, noise, out, scale=1.0):
        t0 = time.perf_counter()
        a, res = self._launch("gaussian_sample", (mean, logvar, noise, out, scale), {}, ("out",))
        with self.inner.ctx():
            o, r, _ = res["out"]
            mag = (mean.double().abs() + (torch.exp(0.5 * logvar.double().clamp(-30.0, 20.0)) * noise.double()).abs()) * abs(scale)
            self._record("gaussian_sample", "out", tuple(out.shape), o, r, GAUSSIAN_ATOL + GAUSSIAN_RTOL * mag, None, t0)


# ------------------------------------------------------------------------------------------------ the audited runs
def backend(inner, device="cpu"):
    return AuditBackend(inner, Float64RefBackend(device), Im2colRefBackend(device))


def unet_inputs(b, s):
    """Seeded like test_gpu_parity.py::test_unet_call_512_matches_oracle; the timesteps mixed over the batch."""
    g = torch.Generator().manual_seed(17)
    x = torch.randn(b, 4, s, s, generator=g)
    cond = torch.randn(b, 48, 768, generator=g) * 0.5
    return x, torch.tensor([650, 999, 0, 261, 37, 820, 444, 5])[:b], cond


def audit_unet(inner, sd, b, s, lam, dtype=F16, device="cpu"):
    """-> (AuditBackend, plan, expected number of audited launches) after one ``forward`` of ``UNetPlan(b, s)``."""
    from progressive_stable_diffusion_amd.engine import UNetPlan
    be = backend(inner, device)
    plan = UNetPlan(be, sd, b, s, dtype=dtype)
    x, t, cond = (v.to(device) for v in unet_inputs(b, s))
    with torch.no_grad():
        plan.forward(x, t, cond, lam=lam)
    inner.synchronize()
    # the recorded ops (prefetches launch no kernel), the 16 K/V projections of set_cond, the 4 launches of time_rows
    return be, plan, fingerprint(plan)["ops"] + len(plan.sites) + 4


def audit_vae_decoder(inner, sd, b, s, device="cpu"):
    from progressive_stable_diffusion_amd.engine import VaeDecoderPlan
    be = backend(inner, device)
    plan = VaeDecoderPlan(be, sd, b, s, latent_scale=0.18215)
    z = torch.randn(b, 4, s, s, generator=torch.Generator().manual_seed(8)) * 0.18215 * 1.5
    inner.copy_(plan.z_in, z.to(device))
    with torch.no_grad():
        plan.run()
    inner.synchronize()
    return be, plan, fingerprint(plan)["ops"]


def audit_vae_encoder(inner, sd, b, s, device="cpu"):
    """Geometry and inputs of test_gpu_parity.py::test_vae_encode_matches_oracle, the reparameterised sample behind it."""
    from progressive_stable_diffusion_amd.engine import VaeEncoderPlan
    be = backend(inner, device)
    plan = VaeEncoderPlan(be, sd, b, s)
    g = torch.Generator().manual_seed(21)
    x = torch.rand(b, 3, s * 8, s * 8, generator=g) * 2 - 1
    noise = torch.randn(b, 4, s, s, generator=g)
    inner.copy_(plan.img_in, x.to(device))
    with torch.no_grad():
        plan.run()
        be.gaussian_sample(plan.mean, plan.logvar, inner.to_device(noise.to(device)), inner.zeros((b, 4, s, s), F32), 0.18215)
    inner.synchronize()
    return be, plan, fingerprint(plan)["ops"] + 1


# ------------------------------------------------------------------------------------------------ report
def report(title, be, wall=None):
    """One line per (op, tensor, signature): launches, worst elementwise ratio, worst RMS ratio, audit seconds; then the
    signatures whose RMS ratio is above 1.1."""
    groups = OrderedDict()
    for r in be.records:
        g = groups.setdefault((r["op"], r["what"], r["sig"]), dict(n=0, elem=0.0, rms=float("nan"), sec=0.0, ok=True))
        g["n"] += 1
        g["elem"] = max(g["elem"], r["elem_ratio"])
        if r["rms_ratio"] == r["rms_ratio"]:
            g["rms"] = r["rms_ratio"] if g["rms"] != g["rms"] else max(g["rms"], r["rms_ratio"])
        g["sec"] += r["seconds"] if r["what"] in ("out", "hs") else 0.0
        g["ok"] = g["ok"] and r["ok"]
    lines = [f"== {title}: {be.launches} launches, {len(be.records)} tensors compared, {len(groups)} signatures, "
             f"{len(be.failures())} outside the criteria" + ("" if wall is None else f", {wall:.1f} s")]
    lines.append(f"{'op.tensor':<26}{'n':>4}{'elem':>9}{'rms':>8}{'sec':>8}  signature")
    for (op, what, sig), g in groups.items():
        lines.append(f"{op + '.' + what:<26}{g['n']:>4}{g['elem']:>9.3f}{g['rms']:>8.3f}{g['sec']:>8.2f}  {sig}{'' if g['ok'] else '   <-- FAIL'}")
    above = [(k, g) for k, g in groups.items() if g["rms"] == g["rms"] and g["rms"] > REPORT_ABOVE]
    lines.append(f"-- RMS ratio above {REPORT_ABOVE}: {len(above)}")
    for (op, what, sig), g in above:
        lines.append(f"   {op}.{what} {sig}: {g['rms']:.3f} - {REASONS.get((op, what), 'unexplained')}")
    return "\n".join(lines)
