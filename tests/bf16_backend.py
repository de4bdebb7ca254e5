"""TEST-ONLY: ``TorchRefBackend`` for plans in either 16-bit storage type.

The parent rounds every result to ``out.dtype`` already; two things are fp16-specific there and are restated here:
conv_in's latent rounding (the fused kernel rounds the fp32 latents to the storage type in registers), and the rule
of ``HipBackend`` that one op takes one 16-bit dtype.  Every op call is also logged as (name, 16-bit dtypes seen)
so the wiring tests can check what a plan hands the kernels.
"""
from __future__ import annotations

import torch

from tests.torch_backend import TorchRefBackend

_16 = (torch.float16, torch.bfloat16)


class DtypeRefBackend(TorchRefBackend):
    name = "torch-ref-dtype"

    def __init__(self, device="cpu"):
        super().__init__(device)
        self.calls = []

    def _log(self, name, *ts):
        kinds = {t.dtype for t in ts if isinstance(t, torch.Tensor) and t.dtype in _16}
        if len(kinds) > 1:
            raise ValueError(f"{name}: mixed 16-bit operands {sorted(map(str, kinds))}")
        self.calls.append((name, kinds.pop() if kinds else None))

    def conv_in_nchw(self, x, w, bias, out, gn_ws=None, gn_nchunk=0):
        self._log("conv_in_nchw", w, out)
        x8 = torch.zeros(x.shape[0], x.shape[2], x.shape[3], 8, dtype=out.dtype, device=x.device)
        self.pack_latents(x, x8)
        self.conv_cin8(x8, w, bias, out)
        if gn_ws is not None:
            b, h, wd, c = out.shape
            o = out.float().reshape(b, gn_nchunk, (h * wd) // gn_nchunk, 32, c // 32)
            st = torch.stack([o.sum(dim=(2, 4)), (o * o).sum(dim=(2, 4))], dim=-1)
            gn_ws[:b * gn_nchunk * 64].copy_(st.reshape(-1))

    def igemm(self, x, w, out, **kw):
        g = kw.get("gn_apply")
        self._log("igemm", x, kw.get("x2"), w, out, kw.get("residual"), None if g is None else g[0])
        super().igemm(x, w, out, **kw)

    def groupnorm(self, x1, x2, gamma, beta, out, *a, **k):
        self._log("groupnorm", x1, x2, out)
        super().groupnorm(x1, x2, gamma, beta, out, *a, **k)

    def layernorm(self, x, gamma, beta, out, eps=1e-5):
        self._log("layernorm", x, out)
        super().layernorm(x, gamma, beta, out, eps)

    def self_attn(self, qkv, out, heads):
        self._log("self_attn", qkv, out)
        super().self_attn(qkv, out, heads)

    def tri_xattn(self, q, kv, out, *a, **k):
        self._log("tri_xattn", q, kv, out)
        super().tri_xattn(q, kv, out, *a, **k)

    def conv_cout4(self, x, w, bias, out, mode=0):
        self._log("conv_cout4", x, w)
        super().conv_cout4(x, w, bias, out, mode)

    def conv_out_ddim(self, x, w, bias, latents, coef):
        self._log("conv_out_ddim", x, w)
        super().conv_out_ddim(x, w, bias, latents, coef)
