"""Static execution plans for the UNet epsilon-prediction, the VAE decoder and the DDIM loop.

A plan is built once per (batch, latent side): weights are repacked into the kernels' layouts
(fp16, ``[Cout][ky][kx][Cin]``), every intermediate gets a fixed buffer from a pool, and the
operator sequence is recorded as a list of bound launches.  Running the plan allocates nothing and
never synchronises, so one denoising step (``begin_step`` + UNet + DDIM update) is captured into a
hipGraph and replayed ``steps`` times with a device-side step counter.

What replaces what (reference paths):
  * ``UNetPlan``      — ``DiffusionModuleWithIP.forward`` -> ``OrdinalUNet.forward`` ->
                        diffusers ``UNet2DConditionModel`` (src/models/diffusion_module_ip.py:383-390,
                        src/models/unet/unet.py:96-146) incl. the 16 attention processors
                        (src/models/attention_processor_routing_gates.py:84-196 / _base.py:39-138)
  * ``VaeDecoderPlan``— ``SDVAE.decode`` (src/models/vae/vae.py:90-112)
  * ``DdimLoop``      — the loop body of ``_ddim_sample_ip``
                        (src/pipelines/inference/inference_pipeline_ip.py:423-468)
Step-invariant work is hoisted exactly: the K/V projections of the conditioning
tokens (16 sites) and the whole time-embedding MLP + 22 ``time_emb_proj`` rows for all steps are
computed once per sampling run.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from . import lib as L
from .backend import on_backend
from .routing import get_block_type  # noqa: F401  (re-exported for callers)

F16, F32, BF16 = torch.float16, torch.float32, torch.bfloat16
OPERAND_DTYPES = (F16, BF16)     # 16-bit storage of the UNet plan: fp16 (default) or bf16 (csrc/*_bf16.hip)
UNET_CH = (320, 640, 1280, 1280)
VAE_CH = (128, 256, 512, 512)
HEADS = 8
GROUPS = 32
N_CU = 256
# attn2 folded into one kernel (csrc/attn2_fused.hip).  Used where one launch has at least A2_MIN_TILES 128-token
# tiles (B=4: the 64x64 sites; same-box A/B +0.9 % end to end); on the smaller maps its 32 / 8 workgroups leave the
# chip idle (-6 % when forced everywhere), so those keep to_q + xattn + to_out.  FUSED_ATTN2 = False switches it off.
FUSED_ATTN2 = True
A2_MIN_TILES = 128


# ----------------------------------------------------------------------------- weight packing
def pack_conv(w: torch.Tensor, dtype=F16) -> torch.Tensor:
    """[Cout,Cin,kh,kw] (or [Cout,Cin]) fp32 -> [Cout, kh*kw*Cin] fp16 (or ``dtype``), K = (tap, cin)."""
    if w.dim() == 2:
        return w.to(dtype).contiguous()
    co, ci, kh, kw = w.shape
    return w.permute(0, 2, 3, 1).reshape(co, kh * kw * ci).to(dtype).contiguous()


def pack_conv_cin8(w: torch.Tensor, dtype=F16) -> torch.Tensor:
    """[Cout,Cin<=8,3,3] -> [Cout,9,8] fp16 (or ``dtype``), input channels zero-padded to 8."""
    co, ci, _, _ = w.shape
    out = torch.zeros(co, 9, 8, dtype=dtype)
    out[:, :, :ci] = w.permute(0, 2, 3, 1).reshape(co, 9, ci).to(dtype)
    return out.contiguous()


def pack_conv_cout4(w: torch.Tensor, dtype=F16) -> torch.Tensor:
    """[Cout<=4,C,3,3] -> [Cout,9,C] fp16 (or ``dtype``)."""
    co, ci, _, _ = w.shape
    return w.permute(0, 2, 3, 1).reshape(co, 9, ci).to(dtype).contiguous()


def geglu_interleave(w: torch.Tensor, b: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Row order for the fused GEGLU epilogue: every 128-row tile = 2 waves x [32 hidden | 32 gate]
    rows of the same 32 output columns (diffusers GEGLU: ``hidden, gate = proj(x).chunk(2)``)."""
    n2 = w.shape[0] // 2
    idx = torch.arange(w.shape[0])
    tile, r = idx // 128, idx % 128
    wn, rr = r // 64, r % 64
    col = tile * 64 + wn * 32 + (rr % 32)
    src = torch.where(rr < 32, col, n2 + col)
    return w[src].contiguous(), b[src].contiguous()


def fold_layernorm(w: torch.Tensor, b: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor, dtype=F16):
    """LayerNorm folded into the linear that consumes it (csrc/igemm_args.h, DADD_EPI_LNFOLD):
    LN(x) W^T + b = rstd (x (gamma o W)^T - mu c1) + (W beta + b).  Returns (gamma o W in fp16, c1, composed bias);
    c1 sums the ROUNDED weights, so that the mean term cancels exactly against what the MFMAs accumulate."""
    w, gamma, beta = w.double(), gamma.double(), beta.double()
    w16 = (w * gamma[None, :]).to(dtype)
    bias = w @ beta + (b.double() if b is not None else 0.0)
    return w16, w16.double().sum(dim=1).float(), bias.float()


def fold_ups_weight(w9: torch.Tensor) -> torch.Tensor:
    """Packed 3x3 weight ``[N][9*Cin]`` (``pack_conv``) of a "nearest 2x upsample -> conv3x3" -> ``[4][N][4*Cin]``: the
    four 2x2 phase convs on the un-upsampled input that compute the same thing (csrc/igemm_ups_fold.hip).  Output
    pixel (2y + py, 2x + px) reads input rows y + py - 1 + dy, dy in {0, 1}; the nine taps collapse onto them as
    py = 0: {ky 0} | {ky 1, 2}, py = 1: {ky 0, 1} | {ky 2}, columns alike.  Phase = 2 py + px, taps in (dy, dx) order.
    Every entry is the sum of 1, 2 or 4 of the 16-bit weights, taken in float64 and rounded ONCE to the weight's type
    (as ``grad_ops.dgrad_weight_ups`` does for the backward)."""
    n, cin = w9.shape[0], w9.shape[1] // 9
    assert w9.dim() == 2 and w9.shape[1] == 9 * cin
    w = w9.reshape(n, 3, 3, cin).double()
    sets = (((0,), (1, 2)), ((0, 1), (2,)))                      # [parity][d] -> the ky (kx) summed
    phases = []
    for py in range(2):
        for px in range(2):
            taps = [w[:, list(sets[py][dy])][:, :, list(sets[px][dx])].sum((1, 2)) for dy in range(2) for dx in range(2)]
            phases.append(torch.stack(taps, 1).reshape(n, 4 * cin))
    return torch.stack(phases, 0).to(w9.dtype).contiguous()


def lds_image(w: torch.Tensor) -> torch.Tensor:
    """[R, 64] fp16 slab -> the LDS image the DMA kernels read fragments from: 128-byte rows, the eight 16-byte chunks
    of row r stored at position ``chunk ^ ((r >> 1) & 7)`` (csrc/igemm_dma.hip ``lds_off``; an involution)."""
    r = w.shape[0]
    sw = (torch.arange(r) >> 1) & 7
    idx = (torch.arange(8)[None, :] ^ sw[:, None])                       # image position p holds chunk p ^ sw
    return w.reshape(r, 8, 8).gather(1, idx[:, :, None].expand(r, 8, 8)).reshape(r, 64).contiguous()


def pack_ffn_stream(w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, wp: torch.Tensor):
    """Weights of a transformer block's tail in the order ``csrc/ffn_block.hip`` consumes them, as ready LDS images:
    per 64 hidden channels five [128 x 64] pieces of ``ff.net.0.proj`` (rows: wave column wn -> [h0 g0 h1 g1], 16 rows
    each, hidden index = chunk*64 + wn*32 + u*16 + e, gate row = 4C + hidden: diffusers ``GEGLU`` is
    ``hidden, gate = proj(x).chunk(2)``), then two [160 x 64] pieces of ``ff.net.2`` (output channels x the chunk's
    hidden channels); after the 20 chunks the ten [160 x 64] pieces of ``proj_out``.  Returns (stream fp16 1-D, bias of
    the GEGLU rows in the same order)."""
    c, hid = 320, 1280
    assert tuple(w1.shape) == (2 * hid, c) and tuple(w2.shape) == (c, hid) and tuple(wp.shape)[:2] == (c, c)
    w1, w2, wp = w1.to(F16), w2.to(F16), wp.reshape(c, c).to(F16)
    pieces, bias = [], []
    e = torch.arange(16)
    for ch in range(hid // 64):
        rows = []
        for wn in range(2):
            for u in range(2):
                h = ch * 64 + wn * 32 + u * 16 + e
                rows += [h, hid + h]
                bias += [b1[h].float(), b1[hid + h].float()]
        rows = torch.cat(rows)                                   # 128 rows of ff.net.0.proj
        for kt in range(c // 64):
            pieces.append(lds_image(w1[rows][:, kt * 64:(kt + 1) * 64]))
        for nh in range(2):
            pieces.append(lds_image(w2[nh * 160:(nh + 1) * 160, ch * 64:(ch + 1) * 64]))
    for nh in range(2):
        for kt in range(c // 64):
            pieces.append(lds_image(wp[nh * 160:(nh + 1) * 160, kt * 64:(kt + 1) * 64]))
    return torch.cat([p.reshape(-1) for p in pieces]).contiguous(), torch.cat(bias).contiguous()


def pack_head_stream(wp: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor) -> torch.Tensor:
    """Weights of a transformer block's head in the order ``csrc/tf_head.hip`` consumes them: ten [160 x 64] LDS images of
    ``proj_in`` (column half, K tile), then thirty of ``to_q | to_k | to_v`` (six column blocks of 160, K tile)."""
    c = 320
    wp = wp.reshape(c, c).to(F16)
    wqkv = torch.cat([wq, wk, wv]).to(F16)
    assert tuple(wqkv.shape) == (3 * c, c)
    pieces = []
    for w in (wp, wqkv):
        for nh in range(w.shape[0] // 160):
            for kt in range(c // 64):
                pieces.append(lds_image(w[nh * 160:(nh + 1) * 160, kt * 64:(kt + 1) * 64]))
    return torch.cat([p.reshape(-1) for p in pieces]).contiguous()


class Recipe:
    """Where a packed device tensor of a plan came from: the state-dict keys, the kind of packing and the destination
    tensor(s) - what ``optim.PlanRefresh`` needs to write the tensor again from a flat array of fp32 masters
    (csrc/plan_refresh.hip) without rebuilding the plan.  A source is a key or ``(key, lo, hi)``, a row slice.
      ``copy32``       src: sources concatenated                        dst: (fp32 tensor,)              ``f()``, ``b_tp``
      ``cast``         src: sources concatenated by rows                dst: (16-bit tensor,)            ``pack_conv``, qkv, kv
      ``cast_cin8``    src: (key,)                                      dst: (16-bit [N][9][8],)         ``pack_conv_cin8``
      ``geglu``        src: (weight, bias)                              dst: (16-bit weight, fp32 bias)  ``geglu_interleave``
      ``lnfold``       src: (weights, biases or None, gamma, beta)      dst: (w16, c1, bias)             ``fold_layernorm``
      ``upsfold``      src: (key,)                                      dst: (16-bit [4][N][4 Cin],)     ``fold_ups_weight``
      ``head_stream``  src: (proj_in, to_q, to_k, to_v)                 dst: (stream,)                   ``pack_head_stream``
      ``ffn_stream``   src: (ff.net.0.proj w, b, ff.net.2 w, proj_out)  dst: (stream, permuted bias)     ``pack_ffn_stream``
    ``geglu``: an ``lnfold`` whose rows are in ``geglu_interleave``'s order."""
    __slots__ = ("kind", "src", "dst", "geglu")
    KINDS = ("copy32", "cast", "cast_cin8", "geglu", "lnfold", "upsfold", "head_stream", "ffn_stream")

    def __init__(self, kind, src, dst, geglu=False):
        assert kind in self.KINDS, kind
        self.kind, self.src, self.dst, self.geglu = kind, tuple(src), tuple(dst), bool(geglu)

    def keys(self):
        """Every state-dict key the recipe reads."""
        out = []

        def walk(x):
            if isinstance(x, str):
                out.append(x)
            elif isinstance(x, tuple) and len(x) == 3 and isinstance(x[0], str) and isinstance(x[1], int):
                out.append(x[0])
            elif x is not None:
                for y in x:
                    walk(y)
        walk(self.src)
        return out


FROZEN = object()        # ``recipe=FROZEN``: an upload of something no training changes (routing gates)
STAGED = object()        # ``recipe=STAGED``: an upload that only feeds a stacked copy; the copy carries the recipe
_PACK_RECIPE = {"pack_conv": "cast", "pack_conv_cout4": "cast", "pack_conv_cin8": "cast_cin8"}


# GroupNorm (+ SiLU) applied inside the consuming 3x3 conv (DADD_PRE_GN, csrc/conv_halo.hip GNIN): the halo is normalised
# in LDS by the loader waves; needs the producer's chunk partials, one source, <= 1024 input channels, the halo kernel
GN_IN_CONV = True

# conv3x3_halo_kernel with two MFMA waves per SIMD (csrc/conv_halo.hip, DUO): measured equal to the one-wave build
# (profiles/r02_zn_halo_duo_ab.txt), so off; True is the A/B switch
HALO_DUO = False

# On the 8x8 maps the split-K finish kernel of a conv also writes the GroupNorm (+ SiLU) of its output for the next conv
# (DADD_EPI_GNAPPLY, csrc/igemm.hip splitk_finish_gnapply_kernel): one launch instead of finish + single-launch GroupNorm
FINISH_GN_APPLY = True

# Weight prefetch on a side branch of the graph (csrc/api.hip dadd_prefetch): how many weight-bearing launches ahead of
# its consumer a weight tensor is read into the Infinity Cache (0 = off), and the smallest tensor worth a branch.
# MEASURED AND OFF (profiles/r03_zh_weight_prefetch_ab.txt, same box, A B A B): 385.7 / 385.0 ms per pass without, 535.4 /
# 534.8 ms with - a captured graph with ~80 side branches per step makes hipGraphLaunch host-bound (host queue time 277 ->
# 504 ms per pass), far more than the 3-8 us per launch that hot weights save (profiles/r03_zg_cold_hot_weights.txt).
WEIGHT_PREFETCH_AHEAD = 0
WEIGHT_PREFETCH_MIN_BYTES = 2 * 1024 * 1024

# GroupNorm statistics written by the producing GEMM's epilogue (no gn_stats launch, one read of the tensor less).
GN_FROM_EPILOGUE = True
GN_FUSED_MAX_BYTES = 16 * 1024       # csrc/norm.hip: below this slab size the single-launch LDS GroupNorm runs
SPLITK_GN_ROWS = 16                  # rows per block / per GroupNorm chunk of splitk_finish_gn_kernel (16 or 64)


# "Nearest 2x upsample -> conv3x3" as four 2x2 phase convs on pre-summed weights (fold_ups_weight, DADD_TUNE_UPS_FOLD):
# K = 4 Cin instead of 9 Cin, 2.25x fewer MFMAs.  The folded copy is built once per plan, beside the packed weight.
# Sites the split-K rule serves (the 8x8 -> 16x16 conv of the UNet: 256 rows per phase, weight-stream-bound) stay on
# the gather kernel; False is the A/B switch.
UPS_FOLD = True


def ups_fold_tiling(m: int, n: int, cin: int) -> Optional[Tuple[int, int, int, int]]:
    """(tile_m, tile_n, 1, tune | TUNE_UPS_FOLD) of an upsample conv that runs as four phase convs, None where it stays
    on the gather: a table entry under the fold's own key (K = 4 Cin) decides; without one the fold runs where the
    gather needs no K slices and every phase has whole 128-row tiles."""
    if not UPS_FOLD:
        return None
    key = tiling_key(m, n, 4 * cin, 9, False, False, 1, 1)
    hit = TILING_OVERRIDE.get(key) or TILING_TABLE.get(key)
    if hit is not None:
        return tuple(hit) if hit[3] & L.TUNE_UPS_FOLD else None
    tile_m, tile_n, sk, tune = plan_tiling(m, n, 9 * cin, 9, False, False, 1, 1)
    if sk != 1 or tile_m != 128 or (m // 4) % 128 or (tune & L.TUNE_NODMA):
        return None
    return tile_m, tile_n, 1, tune | L.TUNE_UPS_FOLD


# LayerNorm folded into the consuming linear (qkv, attn2.to_q, GEGLU projection) instead of a LayerNorm launch and a
# normalised copy of the hidden states.  Measured in situ (profiles/r02_d_step_profile_lnfold_everywhere.txt): the row
# statistics are 64 v_dot2c per K tile in the MFMA waves — free where those waves wait on the LDS fill (64-row tiles:
# 15.7 vs 15.3 us, minus a 4.7 us LayerNorm launch), but +11..19 us on the 128-row tiles, whose MFMA waves are the
# critical path (qkv 64x64: 45 vs 26 us).  So "auto" folds exactly the linears planned on 64-row tiles; True / False
# force it everywhere / nowhere (tests, A/B measurements).
LN_FOLD = "auto"
# ... and on the 128-row tiles the fold is epilogue arithmetic only when the row statistics come from the GEMM that
# produced the hidden states (DADD_EPI_LNSTAT partials of its output, csrc/igemm_epilogue.h): no LayerNorm launch, no
# normalised copy, no statistics in the consumer's K loop.
LN_STATS_FROM_PRODUCER = True
LN_STATS_MAX_PARTS = 8          # what the consumer stages in LDS (csrc/ln_lds.h); more parts (1280 channels from 64-column
                                # tiles: 40) would be read from global memory in the epilogue — slower than the LayerNorm launch


# The tail of a 320-channel transformer block (norm3 -> GEGLU -> FF-out -> proj_out) as ONE launch per 64-token row block
# (csrc/ffn_block.hip): the (B*N) x 4C GEGLU output never leaves the CU.  Each workgroup streams the block's 2.6 MB of
# weights, so it pays only while there are about as many row blocks as CUs (B = 4 at 64x64: 256); below FFN_MIN_BLOCKS
# the three GEMM launches stay.
FUSED_FFN = True
FFN_MIN_BLOCKS = 128
# ... and its head (GroupNorm -> proj_in -> norm1 -> q|k|v) the same way (csrc/tf_head.hip), where the block's input
# comes with GroupNorm chunk partials from its producer
FUSED_HEAD = True


def fold_here(m: int, n: int, k: int, geglu: bool = False) -> bool:
    if LN_FOLD == "auto":
        tile_m, _, _, tune = plan_tiling(m, n, k, 1, geglu, False)
        return tile_m == 64 and not (tune & L.TUNE_NODMA)       # the statistics live in the LDS-DMA kernel
    return bool(LN_FOLD)


def choose_tiling(m: int, n: int, k: int, tile_n: int, geglu: bool = False,
                  residual: bool = True) -> Tuple[int, int, int]:
    """(tile_m, splitk, tune_flags) for one implicit GEMM with 128- or 160-column tiles, from measurements over
    every layer shape of the B=4 / 512x512 step on MI355X (scripts/op_bench.py, profiles/r01_*_op_bench.txt):
      * K >= 12 tiles: the wave-specialised LDS-DMA ring kernel, 128-row tiles, ONE workgroup per CU;
        split K only while a slice keeps >= 16 K tiles (8-10 on the small 8x8..32x32 grids) and the grid
        stays near 256 workgroups — the fp32 slabs and the finish kernel cost more than idle CUs below that;
        with >= 8 tiles per CU (VAE) the ring is kept running over a run of tiles (DADD_TUNE_PERSIST);
      * short K with more 128-row tiles than CUs (qkv, the GEGLU projection at 32x32): the same kernel
        with its ring kept running over a run of output tiles per workgroup (DADD_TUNE_PERSIST);
      * other short-K linears: without a residual input the LDS-DMA kernel (its loaders run no vector
        arithmetic), with one the register-staged kernel, two workgroups per CU, 64-row tiles when 128-row
        tiles would not give ~512 workgroups;
      * GEGLU at 64x64 (2560 tiles, erf epilogue as long as the MFMAs): register-staged 64-row tiles."""
    nkt = k // 64
    nt = math.ceil(n / tile_n)
    t128 = math.ceil(m / 128) * nt
    if geglu:
        if m >= 16384:
            return 64, 1, L.TUNE_NODMA | L.TUNE_SHALLOW
        return 128, 1, (L.TUNE_PERSIST if t128 >= 4 * N_CU else 0)
    if nkt >= 12:
        if n <= 128 and nkt <= 18:      # VAE 128-channel convs: one column tile, the DMA stream is the longer side
            return 128, 1, L.TUNE_NODMA
        per = 16 if t128 > 64 else (10 if t128 > 16 else 8)
        sk = max(1, min(round(N_CU / t128), nkt // per, 32))
        if not residual and nkt <= 20:      # plain projections: one pass beats slabs + finish (15.0 vs 18.9 us)
            sk = 1
        return 128, sk, (L.TUNE_PERSIST if sk == 1 and t128 >= 8 * N_CU else 0)   # VAE: >= 8 tiles per CU
    if t128 > N_CU:
        return 128, 1, L.TUNE_PERSIST
    if not residual and nkt >= 5:           # q / proj_in style linears without a residual read: DMA ring wins
        return 128, 1, 0
    return (128 if t128 >= 2 * N_CU else 64), 1, L.TUNE_NODMA


def choose_splitk(m: int, n: int, k: int, tile_n: int) -> int:
    return choose_tiling(m, n, k, tile_n)[1]


# Measured tile table: (m, n, k, taps, geglu, residual, ups, stride) -> (tile_m, tile_n, splitk, tune), written by
# scripts/tile_sweep.py from in-situ per-launch timings of the B=4 / 512x512 step; shapes outside it use the rules of
# choose_tiling().  TILING_OVERRIDE (same keys) is the sweep's own hook and wins over both.
TILING_OVERRIDE: Dict[Tuple, Tuple[int, int, int, int]] = {}
try:
    from .tiling_table import TABLE as TILING_TABLE, TABLE_R3 as TILING_TABLE_R3
except ImportError:          # no table committed yet
    TILING_TABLE, TILING_TABLE_R3 = {}, {}
TILING_R3 = True             # the round-3 entries of the table (64-row tiles with K slices on the small maps)


def tiling_key(m, n, k, taps, geglu, residual, ups=0, stride=1):
    return (int(m), int(n), int(k), int(taps), bool(geglu), bool(residual), int(bool(ups)), int(stride))


def plan_tiling(m, n, k, taps, geglu, residual, ups=0, stride=1) -> Tuple[int, int, int, int]:
    """(tile_m, tile_n, splitk, tune) of one implicit GEMM."""
    key = tiling_key(m, n, k, taps, geglu, residual, ups, stride)
    hit = TILING_OVERRIDE.get(key) or (TILING_TABLE_R3.get(key) if TILING_R3 else None) or TILING_TABLE.get(key)
    if hit is not None:
        return tuple(hit)
    tile_n = 128 if geglu or n % 160 else 160
    tile_m, sk, tune = choose_tiling(m, n, k, tile_n, geglu, residual)
    # short linears of the small maps (<= 128 tiles of 128 rows): 64x64 LDS-DMA tiles, two workgroups per CU, fill
    # the chip without fp32 slabs and a finish launch
    if (taps == 1 and not geglu and not ups and n % 64 == 0 and k // 64 <= 40
            and math.ceil(m / 128) * math.ceil(n / tile_n) <= N_CU // 2):
        return 64, 64, 1, 0
    return tile_m, tile_n, sk, tune


class Pool:
    """Plan-time buffer pool: fixed addresses, explicit release, reuse by (shape, dtype)."""

    def __init__(self, be, dtype=F16):
        self.be = be
        self.dtype = dtype              # of get() without an explicit dtype: the plan's 16-bit activations
        self.free: Dict[Tuple, List[torch.Tensor]] = {}
        self.bytes = 0
        self.on_put = None

    def get(self, shape, dtype=None) -> torch.Tensor:
        dtype = dtype or self.dtype
        key = (tuple(shape), dtype)
        lst = self.free.get(key)
        if lst:
            return lst.pop()
        t = self.be.empty(shape, dtype)
        self.bytes += t.numel() * t.element_size()
        return t

    def put(self, *ts):
        for t in ts:
            if t is not None:
                if self.on_put is not None:
                    self.on_put(t)
                self.free.setdefault((tuple(t.shape), t.dtype), []).append(t)


class _Plan:
    def __init__(self, be, wcache=None, dtype=F16, sd=None, prefix=""):
        if dtype not in OPERAND_DTYPES:
            raise ValueError(f"plan dtype must be torch.float16 or torch.bfloat16, got {dtype}")
        self.be = be
        self.wcache = wcache
        self.dtype = dtype              # 16-bit storage of activations and packed weights
        self.sd, self.prefix = sd, prefix + "."
        self.pool = Pool(be, dtype)
        self.ops: List = []
        self.keep: List[torch.Tensor] = []  # weights & persistent buffers
        self.gn_partials: Dict[int, Tuple[torch.Tensor, int]] = {}   # output buffer -> (chunk partials, chunks)
        self.ln_partials: Dict[int, torch.Tensor] = {}               # output buffer -> LayerNorm row partials [P][M][2]
        self._memo: Dict = {}
        self.gn_ready: Dict[int, Tuple] = {}      # output buffer -> (its GroupNorm written by the finish kernel, gamma, beta, eps, silu)
        self.pool.on_put = self._forget
        self.gn_ws = None
        # Split-K slabs are combined by the finish kernel.  The in-launch combine (last-arriving slice
        # reduces; `counters` of dadd_conv_igemm_f16) is implemented and tested but measured 2-4x SLOWER
        # on MI355X for these shapes (M=256 N=1280 K=11520, 16 slices: 122 us vs 27 us): every slice
        # pays an agent-scope release (L2 write-back) — cdna_hip_programming.md "cut GEMM->GEMM seams".
        self.sk_counters = None
        # every device tensor derived from ``sd`` has a Recipe; an upload without one is listed in ``unrefreshable``.
        # ``frozen`` plans (VAE) record neither: nothing trains their weights.
        self.recipes: List[Recipe] = []
        self.unrefreshable: List = []
        self.frozen = False
        self._src_key: Dict[int, str] = {}      # packed 3x3 weight -> its state-dict key (ups_fold)

    def rec(self, fn, *a, **k):
        self.ops.append((fn, a, k))

    def run(self):
        for fn, a, k in self.ops:
            fn(*a, **k)

    def _forget(self, t):
        """``pool.on_put``: a recycled buffer loses its statistics.  A normalised copy of it (``gn_ready``) must have been
        taken by then: only the consuming ``gn()`` hands that pool buffer on, so dropping the entry would leak it."""
        assert t.data_ptr() not in self.gn_ready, f"GroupNorm of a {tuple(t.shape)} buffer written by a finish kernel, never consumed"
        self.gn_partials.pop(t.data_ptr(), None)
        self.ln_partials.pop(t.data_ptr(), None)

    def _end_build(self, prefetch_weights=False):
        """Every ``_build`` ends here."""
        assert not self.gn_ready, f"GroupNorm written by a finish kernel, never consumed: {[tuple(r[0].shape) for r in self.gn_ready.values()]}"
        if prefetch_weights:
            self._insert_weight_prefetch()

    def _insert_weight_prefetch(self):
        """Every layer's weights are cold when its kernel starts (1.76 GB per step against 256 MB of Infinity Cache).  A
        launch whose weights are at least WEIGHT_PREFETCH_MIN_BYTES gets a ``be.prefetch`` of them WEIGHT_PREFETCH_AHEAD
        weight-bearing launches earlier - a side branch of the captured graph (``dadd_prefetch``) - and the plan ends with
        the join.  Reads only: results are unchanged."""
        if not WEIGHT_PREFETCH_AHEAD:
            return
        wops = []                       # (op index, weight tensor) of the launches that stream a weight operand
        for i, (fn, a, k) in enumerate(self.ops):
            name = getattr(fn, "__name__", "")
            if name == "igemm":
                wops.append((i, a[1]))
            elif name in ("ffn_block", "tf_head"):
                wops.append((i, a[1]))
        inserts = []
        for j, (i, w) in enumerate(wops):
            if w.numel() * w.element_size() < WEIGHT_PREFETCH_MIN_BYTES or j < WEIGHT_PREFETCH_AHEAD:
                continue
            inserts.append((wops[j - WEIGHT_PREFETCH_AHEAD][0], w))
        for at, w in sorted(inserts, key=lambda t: -t[0]):       # back to front: earlier indices stay valid
            self.ops.insert(at, (self.be.prefetch, (w,), {}))
        if inserts:
            self.ops.append((self.be.prefetch_join, (), {}))

    def dev(self, t, dtype=None, recipe=None):
        """A parameter or I/O buffer the plan uploads directly (not shared between plans).  ``recipe``: ``(kind, src)`` of
        the ``Recipe`` that writes it again, ``FROZEN`` or ``STAGED``."""
        d = self.be.to_device(t, dtype)
        self.keep.append(d)
        if recipe is not FROZEN and recipe is not STAGED and not self.frozen:
            if recipe is None:
                self.unrefreshable.append(("dev", tuple(d.shape), d.dtype))
            else:
                self.recipes.append(Recipe(recipe[0], recipe[1], (d,)))
        return d

    def cached(self, key, make, recipe=None):
        """Packed device tensor(s) for ``key``: ``make()`` uploads one tensor or a tuple (``be.to_device``) on the first
        request - of any plan that shares the optional cross-plan cache (``wcache``: plans for other batch sizes or tilings
        over the same state dict share the packed weights instead of re-packing 1.9 GB each).  The plan-local memo gives one
        entry per key (fuse_gn hints name the same tensors twice) and puts each tensor into ``keep`` once.  The key carries
        the plan's dtype: fp16 and bf16 plans over one cache never hand each other their packed weights.
        ``recipe``: ``value -> [Recipe, ...]`` for what ``make()`` returns, recorded by every plan that takes the entry (plans
        over one ``wcache`` share destinations: a refresh writes each once)."""
        key = (*key, self.dtype)
        t = self._memo.get(key)
        if t is None:
            t = self.wcache.get(key) if self.wcache is not None else None
            if t is None:
                t = make()
                if self.wcache is not None:
                    self.wcache[key] = t
            self._memo[key] = t
            self.keep += t if isinstance(t, tuple) else (t,)
            if not self.frozen:
                if recipe is None:
                    self.unrefreshable.append(key)
                else:
                    self.recipes += recipe(t)
        return t

    def w(self, key, pack=pack_conv):
        full = self.prefix + key
        t = self.cached((full, pack.__name__), lambda: self.be.to_device(pack(self.sd[full], self.dtype)),
                        (lambda t: [Recipe(_PACK_RECIPE[pack.__name__], (full,), (t,))]) if pack.__name__ in _PACK_RECIPE else None)
        self._src_key[t.data_ptr()] = full
        return t

    def ups_fold(self, w9):
        """The folded copy ``[4][N][4 Cin]`` of the packed upsample-conv weight ``w9``, kept as long as ``w9`` (same cache,
        same ``keep``) and registered with a backend that runs the phase convs (``register_ups_fold``); others ignore
        DADD_TUNE_UPS_FOLD and run the 9-tap gather."""
        src = self._src_key.get(w9.data_ptr())
        w4 = self.cached(("ups_fold", w9.data_ptr()), lambda: self.be.to_device(fold_ups_weight(w9.cpu())),
                         (lambda t: [Recipe("upsfold", (src,), (t,))]) if src is not None else None)
        if hasattr(self.be, "register_ups_fold"):
            self.be.register_ups_fold(w9, w4)
        return w4

    def f(self, key):
        full = self.prefix + key
        return self.cached((full, "f32"), lambda: self.be.to_device(self.sd[full].float()),
                           lambda t: [Recipe("copy32", (full,), (t,))])

    def _gn_partials_for(self, out, nchunk, extra=0):
        """GroupNorm chunk partials [B][nchunk + extra][32][2] of ``out``, written by the launch that takes the returned
        keywords and found by the consumers of ``out`` in ``gn_partials``."""
        ws = self.be.zeros((out.shape[0] * (nchunk + extra) * GROUPS * 2,), F32)
        self.keep.append(ws)
        self.gn_partials[out.data_ptr()] = (ws, nchunk)
        return dict(gn_ws=ws, gn_nchunk=nchunk)

    def _ln_partials_for(self, out, parts):
        """LayerNorm row partials [parts][M][2] of ``out`` (DADD_EPI_LNSTAT), found by its folded consumer in ``ln_partials``."""
        st = self.be.zeros((parts, out.numel() // out.shape[-1], 2), F32)
        self.keep.append(st)
        self.ln_partials[out.data_ptr()] = st
        return st

    # ---- recorded building blocks -----------------------------------------------------------
    def conv(self, x, w, out_shape, *, x2=None, bias=None, rowvec=None, residual=None, taps=9,
             stride=1, ups=0, pad=1, flags=0, ln_c1=None, ln_eps=1e-5, gn_stats=False, ln_stats=False,
             ln_stats_in=None, gn_in=None, fuse_gn=None):
        """``gn_in`` = (partials, nchunk, gamma, beta, eps, silu): GroupNorm of ``x`` on the way in (``gn_in_conv_ok``).
        ``fuse_gn`` = (gamma, beta, eps, silu) of the GroupNorm that consumes the output: on the small maps, where the
        conv runs split-K and a (sample, group) slab is <= 16 KiB, the finish kernel writes the normalised copy too
        (DADD_EPI_GNAPPLY) and the consuming ``gn()`` finds it in ``self.gn_ready`` instead of launching.
        ``ln_stats``: the output feeds a LayerNorm whose consumer is a folded linear — have the epilogue write the row
        partials (DADD_EPI_LNSTAT) where the launch allows (plain linear, one K pass, whole wave column blocks); they
        are found again through ``self.ln_partials``.  ``ln_stats_in``: such partials of ``x`` for this folded linear.
        ``gn_stats``: the output feeds a GroupNorm — have the epilogue write its chunk partials (DADD_EPI_GNSTAT)
        where the tiling allows (full 128/160-column tiles holding whole groups, row blocks inside one sample, <= 128
        chunks, no split-K); the consuming ``gn()`` then skips its statistics pass."""
        out = self.pool.get(out_shape)
        n = w.shape[0]
        m = out_shape[0] * out_shape[1] * out_shape[2]
        tile_m, tile_n, sk, tune = plan_tiling(m, n, w.shape[1], taps, bool(flags & L.EPI_GEGLU), residual is not None,
                                               ups, stride)
        fold = ups_fold_tiling(m, n, w.shape[1] // 9) if ups and x2 is None and residual is None and rowvec is None else None
        if fold is not None:
            tile_m, tile_n, sk, tune = fold
            self.ups_fold(w)
        if taps == 9 and HALO_DUO:
            tune |= L.TUNE_SHALLOW
        if ln_c1 is not None:
            sk = 1                      # the row statistics come from whole rows of A: no K slices
        partial = self.pool.get((sk * m * n,), F32) if sk > 1 else None
        gkw = {}
        if gn_stats and GN_FROM_EPILOGUE and not (flags & L.EPI_GEGLU) and n % 32 == 0:
            howo, cg = out_shape[1] * out_shape[2], n // 32
            if sk == 1:     # the GEMM's own epilogue writes the partials: one chunk per MFMA wave's row block
                wm_rows = tile_m // 2
                ok = tile_n in (128, 160) and (tile_n // 2) % cg == 0 and m % tile_m == 0 and n % tile_n == 0
            else:           # split-K: the finish kernel writes them, per 16 rows x 160 (128) columns
                wm_rows = SPLITK_GN_ROWS if howo // SPLITK_GN_ROWS <= 128 else 64      # (<= 128 chunks keeps GroupNorm-in-conv eligible)
                cb = 160 if n % 160 == 0 else 128
                ok = n % cb == 0 and cb % cg == 0 and m % wm_rows == 0
            nchunk = howo // wm_rows
            # (maps whose (batch, group) slab fits the single-launch LDS GroupNorm keep that path)
            # (> 128 chunks — the VAE maps — are folded to 64 per sample by gn_reduce_kernel inside dadd_groupnorm_f16:
            # one small launch instead of a statistics pass over the tensor; `ws` carries the room for them)
            if ok and howo % wm_rows == 0 and nchunk >= 1 and howo * cg * 2 > GN_FUSED_MAX_BYTES:
                gkw = self._gn_partials_for(out, nchunk, extra=64 if nchunk > 128 else 0)
                flags |= L.EPI_GNSTAT
        if (ln_stats and LN_STATS_FROM_PRODUCER and not (flags & (L.EPI_GEGLU | L.EPI_GNSTAT)) and sk == 1
                and n % (tile_n // 2) == 0 and n // (tile_n // 2) <= LN_STATS_MAX_PARTS):
            gkw["ln_stats_out"] = self._ln_partials_for(out, n // (tile_n // 2))
            flags |= L.EPI_LNSTAT
        f = flags | (L.EPI_BIAS if bias is not None else 0) | (L.EPI_ROWVEC if rowvec is not None else 0) \
            | (L.EPI_RESIDUAL if residual is not None else 0) | (L.EPI_LNFOLD if ln_c1 is not None else 0) | tune
        kw = dict(ln_c1=ln_c1, ln_eps=ln_eps) if ln_c1 is not None else {}
        if (fuse_gn is not None and FINISH_GN_APPLY and sk > 1 and self.sk_counters is None and not (f & L.EPI_GNSTAT)
                and n % 64 == 0 and out_shape[1] * out_shape[2] * (n // 32) * 2 <= GN_FUSED_MAX_BYTES):
            g_out = self.pool.get(out_shape)
            f |= L.EPI_GNAPPLY | (L.EPI_GNAPPLY_SILU if fuse_gn[3] else 0)
            kw["gn_apply"] = (g_out, fuse_gn[0], fuse_gn[1], fuse_gn[2])
            self.gn_ready[out.data_ptr()] = (g_out, fuse_gn[0].data_ptr(), fuse_gn[1].data_ptr(), float(fuse_gn[2]), bool(fuse_gn[3]))
        if gn_in is not None:       # (partials, chunks, gamma, beta, eps, silu[, partials of x2, chunks of x2])
            f |= L.PRE_GN | (L.PRE_GN_SILU if gn_in[5] else 0)
            kw["gn_in"] = tuple(gn_in[:5]) + tuple(gn_in[6:])
        if ln_c1 is not None and ln_stats_in is not None:
            kw["ln_stats_in"] = ln_stats_in
        self.rec(self.be.igemm, x, w, out, x2=x2, bias=bias, rowvec=rowvec, residual=residual,
                 taps=taps, stride=stride, ups=ups, pad=pad, flags=f, splitk=sk, partial=partial,
                 tile_n=tile_n, tile_m=tile_m, counters=self.sk_counters if sk > 1 else None, **kw, **gkw)  # None: finish kernel
        self.pool.put(partial)
        return out

    def gn_in_conv_ok(self, x, x2, w, out_shape, residual) -> Optional[Tuple]:
        """(partials, chunks) of ``x`` if the 3x3 conv (x -> out_shape, weights w) can apply the GroupNorm itself: the conv
        must land on the halo kernel (csrc/igemm.hip: stride 1 / pad 1, 64-, 32- or 16-wide square map in whole 128-pixel
        tiles, 128x160 LDS-DMA tiles, no persistent ring) and ``x`` must be a single source of <= 1152 / 2048 / 2432 channels whose
        producer wrote <= 128 chunk partials."""
        cmax = {64: 1152, 32: 2048, 16: 2432}.get(x.shape[2], 0)      # (scale, shift) pairs that fit beside the halo in LDS
        cin = x.shape[-1] + (0 if x2 is None else x2.shape[-1])
        if not GN_IN_CONV or cin > cmax or x.shape[-1] % 64 or cin % 64:
            return None
        part = self.gn_partials.get(x.data_ptr())
        if part is None or part[1] > 128:
            return None
        if x2 is not None:          # skip-concat: both sources' partials, nesting group widths (DADD_PRE_GN contract)
            part2 = self.gn_partials.get(x2.data_ptr())
            c1_, c2_, cgc = x.shape[-1], x2.shape[-1], cin // 32
            if (part2 is None or part2[1] > 128 or c1_ % 32 or c2_ % 32 or cgc % (c1_ // 32) or cgc % (c2_ // 32)
                    or c1_ % cgc):
                return None
            part = (part[0], part[1], part2[0], part2[1])
        b, h, w_, _ = x.shape
        n, m = w.shape[0], out_shape[0] * out_shape[1] * out_shape[2]
        if tuple(out_shape[1:3]) != (h, w_) or h != w_ or w_ not in (16, 32, 64) or (h * w_) % 128:
            return None
        tile_m, tile_n, _, tune = plan_tiling(m, n, w.shape[1], 9, False, residual is not None, 0, 1)
        if tile_m != 128 or tile_n != 160 or (tune & (L.TUNE_NODMA | L.TUNE_PERSIST)) or HALO_DUO:
            return None
        return part

    def gn(self, x1, x2, gamma, beta, eps, silu):
        c = x1.shape[-1] + (0 if x2 is None else x2.shape[-1])
        ready = self.gn_ready.get(x1.data_ptr()) if x2 is None else None
        if ready is not None and ready[1:] == (gamma.data_ptr(), beta.data_ptr(), float(eps), bool(silu)):
            del self.gn_ready[x1.data_ptr()]       # written by the producer's split-K finish (DADD_EPI_GNAPPLY)
            return ready[0]
        out = self.pool.get((*x1.shape[:3], c))
        part = self.gn_partials.get(x1.data_ptr()) if x2 is None else None
        if part is not None:            # statistics already written by the producing epilogue
            self.rec(self.be.groupnorm, x1, None, gamma, beta, out, part[0], GROUPS, eps, silu, ws_chunks=part[1])
        else:
            self.rec(self.be.groupnorm, x1, x2, gamma, beta, out, self.gn_ws, GROUPS, eps, silu)
        return out


# ----------------------------------------------------------------------------- UNet
class UNetPlan(_Plan):
    """SD-1.x UNet forward for a fixed (B, S); eps = plan(latents) with cond/time prepared apart."""

    def __init__(self, be, sd: Dict[str, torch.Tensor], batch: int, side: int, *,
                 prefix="unet.unet", use_routing_gates=True, use_frequency_strategy=True, wcache=None, dtype=F16):
        """``dtype``: 16-bit storage of activations, packed weights, conditioning and K/V caches (fp32 accumulation either
        way).  bf16 takes the generic path at the sites where fp16 uses a row-block fusion (tf_head, ffn_block,
        attn2_fused have no bf16 form); every other tiling / split-K / fold choice is the fp16 plan's.  The time-embedding
        rows stay as in fp16 (fp32 rows from fp16 weights, dadd_linear_rows_f32)."""
        super().__init__(be, wcache, dtype, sd, prefix)
        assert side % 8 == 0, "latent side must be a multiple of 8 (three stride-2 levels)"
        self.B, self.S = batch, side
        self.gates_mode = use_routing_gates
        self.lam = 0.0
        # device-side scalars read by the kernels of a captured step: [0] = lambda (delta steering), [1] = CFG scale
        self.params = be.zeros((2,), F32)
        self.params_dev = False      # True while a DdimLoop drives the plan: kernels take lambda from `params`
        self.ddim_coef = None        # set by DdimLoop for a step without CFG: conv_out applies the DDIM update itself
        self.gn_ws = be.empty((batch * L.GN_MAX_CHUNKS * GROUPS * 2,), F32)
        u = self.prefix
        # ---- time path: linear_1, linear_2, all 22 time_emb_proj concatenated
        te = u + "time_embedding.linear_"
        self.w_t1 = self.dev(sd[te + "1.weight"], F16, ("cast", (te + "1.weight",)))
        self.b_t1 = self.dev(sd[te + "1.bias"], None, ("copy32", (te + "1.bias",)))
        self.w_t2 = self.dev(sd[te + "2.weight"], F16, ("cast", (te + "2.weight",)))
        self.b_t2 = self.dev(sd[te + "2.bias"], None, ("copy32", (te + "2.bias",)))
        names = self._resnet_names()
        self.temb_off, off = {}, 0
        for nme in names:
            self.temb_off[nme] = off
            off += sd[u + nme + ".time_emb_proj.weight"].shape[0]
        self.temb_cols = off
        tp_w, tp_b = [u + n + ".time_emb_proj.weight" for n in names], [u + n + ".time_emb_proj.bias" for n in names]
        self.w_tp = self.dev(torch.cat([sd[k] for k in tp_w]), F16, ("cast", tp_w))
        self.b_tp = self.dev(torch.cat([sd[k] for k in tp_b]), None, ("copy32", tp_b))
        self.temb_rows = be.zeros((batch, self.temb_cols), F32)     # current step's rows
        # ---- cross-attention conditioning caches (step invariant)
        self.sites = self._attn_sites()
        self.T = 48 if use_routing_gates else 32
        self.kv_w, self.kv, self.gates = {}, {}, {}
        for site, c in self.sites:
            ap = f"{u}{site}.transformer_blocks.0.attn2"
            kv_keys = [ap + ".to_k.weight", ap + ".to_v.weight"]
            if use_routing_gates:
                kv_keys += [ap + ".processor.to_k_dis.weight", ap + ".processor.to_v_dis.weight"]
                self.gates[site] = self.dev(torch.stack([sd[ap + ".processor.anat_gate"],
                                                         sd[ap + ".processor.dis_gate"]]).float(), None, FROZEN)
            else:
                self.gates[site] = None
            self.kv_w[site] = self.dev(torch.cat([sd[k] for k in kv_keys]), dtype, ("cast", kv_keys))
            self.kv[site] = [be.zeros((batch, 1, self.T, self.kv_w[site].shape[0]), dtype)
                             for _ in range(2)]                     # [cond, uncond]
        self.cond16 = be.zeros((batch, 1, self.T, 768), dtype)
        self.kv_slot = 0
        self.cond_gen = 0      # advanced by every set_cond(): callers that cache projections key on it
        self.weights_gen = 0   # advanced when the packed weights are rewritten in place (training.Trainer.sync_module):
                               # what was computed FROM them and cached (DdimLoop's time-row table) keys on it
        # ---- attn2 folded into ONE kernel per block (dadd_attn2_fused_f16): with 16 keys per pathway
        # q K^T = x (W_q K^T) and P V W_o^T = P (V W_o^T), so the step-invariant conditioning absorbs both
        # projections.  Sites whose map is smaller than one 128-token tile (8x8) keep the three-kernel path.
        self.fused_attn2 = bool(use_routing_gates) and FUSED_ATTN2 and dtype == F16
        self.a2, self._a2_dirty, self._a2_lam = {}, True, None
        if self.fused_attn2:
            for site, c in self.sites:
                hw = self._site_hw(site)
                # one workgroup per 128-token tile: sites with few tiles leave most of the chip idle
                if hw % 128 == 0 and c % 320 == 0 and batch * hw // 128 >= A2_MIN_TILES:
                    ap = f"{u}{site}.transformer_blocks.0.attn2"
                    self.a2[site] = dict(
                        # (read once by _a2_group, which stacks them: the stacked copies are what a refresh rewrites)
                        wq=self.dev(sd[ap + ".to_q.weight"].float(), None, STAGED),
                        wo=self.dev(sd[ap + ".to_out.0.weight"].float(), None, STAGED),
                        mcat=be.zeros((batch, 384, c), F16), vw=be.zeros((batch, c, 384), F16),
                        # norm2 folded into the score GEMM (set by _transformer when the producer supplies row partials)
                        fold=False, ln_c1=be.zeros((batch, 384), F32), ln_d=be.zeros((batch, 384), F32),
                        gamma=self.f(f"{site}.transformer_blocks.0.norm2.weight"),
                        beta=self.f(f"{site}.transformer_blocks.0.norm2.bias"))
        # The fold runs once per conditioning (every sampler pass): sites of equal width share ONE set of batched torch
        # ops over stacked weights / buffers (five sites at 64x64: ~25 launches instead of ~125, profiles/r03_*_pass_breakdown)
        self.a2_groups = []
        by_c: Dict[int, List[str]] = {}
        for site, c in self.sites:
            if site in self.a2:
                by_c.setdefault(c, []).append(site)
        for c, names in by_c.items():
            self.a2_groups.append(self._a2_group(c, names, batch))
        # ---- I/O
        self.lat_in = be.zeros((batch, 4, side, side), F32)
        self.eps_out = [be.zeros((batch, 4, side, side), F32) for _ in range(2)]
        self._build()

    def _a2_group(self, c, names, batch):
        """Stacked weights and output buffers of the fused-attn2 sites of width ``c`` (``prepare_attn2``)."""
        be = self.be
        ns, d = len(names), c // HEADS
        with be.ctx():                      # (the stacking reads tensors uploaded on the backend's stream)
            grp = dict(sites=names, c=c,
                       wq=torch.stack([self.a2[n]["wq"].view(HEADS, d, c) for n in names]),
                       wo=torch.stack([self.a2[n]["wo"].view(c, HEADS, d) for n in names]),
                       gamma=torch.stack([self.a2[n]["gamma"] for n in names]).view(ns, 1, 1, c),
                       beta=torch.stack([self.a2[n]["beta"] for n in names]).view(ns, 1, 1, c),
                       gates=torch.stack([self.gates[n] for n in names]).float(),
                       mcat=be.zeros((ns, batch, 384, c), F16), vw=be.zeros((ns, batch, c, 384), F16),
                       ln_c1=be.zeros((ns, batch, 384), F32), ln_d=be.zeros((ns, batch, 384), F32))
        for i, n in enumerate(names):       # the per-site tensors the kernels read are slices of the stacked ones
            tb = f"{self.prefix}{n}.transformer_blocks.0"
            for key, src in (("wq", ".attn2.to_q.weight"), ("wo", ".attn2.to_out.0.weight"), ("gamma", ".norm2.weight"),
                             ("beta", ".norm2.bias")):
                self.recipes.append(Recipe("copy32", (tb + src,), (grp[key][i],)))      # the stacked copies
            for key in ("mcat", "vw", "ln_c1", "ln_d"):
                self.a2[n][key] = grp[key][i]
            del self.a2[n]["wq"], self.a2[n]["wo"]
        self.keep += [grp[k] for k in ("wq", "wo", "gamma", "beta", "gates", "mcat", "vw", "ln_c1", "ln_d")]
        return grp

    # -- inventory -------------------------------------------------------------------------------
    @staticmethod
    def _resnet_names():
        n = [f"down_blocks.{i}.resnets.{j}" for i in range(4) for j in range(2)]
        n += ["mid_block.resnets.0", "mid_block.resnets.1"]
        n += [f"up_blocks.{i}.resnets.{j}" for i in range(4) for j in range(3)]
        return n

    def _site_hw(self, site: str) -> int:
        """Tokens per sample at an attention site (latent side S: 64x64 -> S^2, S^2/4, S^2/16, mid S^2/64)."""
        if site.startswith("down_blocks."):
            r = self.S >> int(site.split(".")[1])
        elif site.startswith("up_blocks."):
            r = self.S >> (3 - int(site.split(".")[1]))
        else:
            r = self.S >> 3
        return r * r

    @staticmethod
    def _attn_sites():
        s = [(f"down_blocks.{i}.attentions.{j}", UNET_CH[i]) for i in range(3) for j in range(2)]
        s.append(("mid_block.attentions.0", 1280))
        s += [(f"up_blocks.{i}.attentions.{j}", UNET_CH[3 - i]) for i in (1, 2, 3) for j in range(3)]
        return s

    # -- blocks ----------------------------------------------------------------------------------
    def _gn_of(self, key, eps, silu):
        """(gamma, beta, eps, silu) of the GroupNorm ``key`` — the ``fuse_gn`` hint of the conv that feeds it."""
        return (self.f(key + ".weight"), self.f(key + ".bias"), eps, silu)

    def _norm_conv(self, name, n, x, skip, cout, release_x=False, **kw):
        """``conv<n>(SiLU(norm<n>(x | skip)))`` of ResNet ``name``: the GroupNorm runs inside the 3x3 conv where the halo
        kernel can apply it (``gn_in_conv_ok``), else through ``gn()``.  ``release_x``: ``x`` returns to the pool right after
        its last reader is recorded - in the second arm BEFORE the conv, whose output may then take its place."""
        b, h, w_, _ = x.shape
        shp = (b, h, w_, cout)
        w = self.w(f"{name}.conv{n}.weight")
        norm = self._gn_of(f"{name}.norm{n}", 1e-5, 1)
        kw.update(bias=self.f(f"{name}.conv{n}.bias"), gn_stats=True)
        part = self.gn_in_conv_ok(x, skip, w, shp, kw.get("residual"))
        if part is not None:         # (part carries the skip's partials too when there is one)
            out = self.conv(x, w, shp, x2=skip, gn_in=tuple(part[:2]) + norm + tuple(part[2:]), **kw)
            if release_x:
                self.pool.put(x)
        else:
            g = self.gn(x, skip, *norm)
            if release_x:
                self.pool.put(x)
            out = self.conv(g, w, shp, **kw)
            self.pool.put(g)
        return out

    def _resnet(self, name, x, skip=None, next_gn=None):
        """``next_gn``: the GroupNorm that consumes this block's output first (``_gn_of``), if the caller knows it."""
        b, h, w_, _ = x.shape
        cin = x.shape[-1] + (0 if skip is None else skip.shape[-1])
        cout = self.sd[self.prefix + name + ".conv1.weight"].shape[0]
        off = self.temb_off[name]
        h1 = self._norm_conv(name, 1, x, skip, cout, rowvec=self.temb_rows[:, off:off + cout],
                             fuse_gn=self._gn_of(name + ".norm2", 1e-5, 1))
        if cin != cout:
            res = self.conv(x, self.w(name + ".conv_shortcut.weight"), (b, h, w_, cout), x2=skip,
                            bias=self.f(name + ".conv_shortcut.bias"), taps=1, pad=0)
        else:
            assert skip is None
            res = x
        out = self._norm_conv(name, 2, h1, None, cout, release_x=True, residual=res, fuse_gn=next_gn)
        if res is not x:
            self.pool.put(res)
        return out

    def _ln_linear(self, tb, norm, name, wkey_list, bias_key=None, geglu=False):
        """Device tensors (w16, c1, bias) of ``norm`` folded into the linear(s) ``wkey_list`` (rows concatenated)."""
        u = self.prefix

        def make():
            w = torch.cat([self.sd[u + tb + k] for k in wkey_list])
            b = self.sd[u + tb + bias_key] if bias_key else None
            w16, c1, bias = fold_layernorm(w, b, self.sd[u + tb + norm + ".weight"], self.sd[u + tb + norm + ".bias"],
                                           self.dtype)
            if geglu:               # row order of the fused GEGLU epilogue; c1 / bias follow their rows
                idx = geglu_interleave(torch.arange(w16.shape[0])[:, None].float(), torch.zeros(w16.shape[0]))[0][:, 0].long()
                w16, c1, bias = w16[idx], c1[idx], bias[idx]
            return tuple(self.be.to_device(t.contiguous()) for t in (w16, c1, bias))
        src = ([u + tb + k for k in wkey_list], [u + tb + bias_key] if bias_key else None, u + tb + norm + ".weight",
               u + tb + norm + ".bias")
        return self.cached((u + tb, "lnfold", name), make, lambda t: [Recipe("lnfold", src, t, geglu=geglu)])

    def _ln_then_linear(self, x, out_shape, fold, folded, plain, ln, flags=0):
        """The linear that consumes a LayerNorm of ``x``: folded into the GEMM where the policy says so (``fold``: row
        statistics in the GEMM's own K loop) or the producer of ``x`` left row partials (``ln_partials``), else a LayerNorm
        launch (``ln()`` returns the normalised copy) and the plain linear.  ``folded()`` gives (w, c1, bias) as
        ``_ln_linear`` does, ``plain()`` gives (w, bias)."""
        st = self.ln_partials.get(x.data_ptr())
        if fold or st is not None:
            w, c1, bias = folded()
            return self.conv(x, w, out_shape, bias=bias, taps=1, pad=0, flags=flags, ln_c1=c1,
                             ln_stats_in=None if fold else st)
        w, bias = plain()
        return self.conv(ln(), w, out_shape, bias=bias, taps=1, pad=0, flags=flags)

    def _transformer(self, site, x):
        b, h, w_, c = x.shape
        shp = (b, h, w_, c)
        u, tb = self.prefix, site + ".transformer_blocks.0"
        m_rows = b * h * w_
        fold1, fold2, fold3 = (fold_here(m_rows, 3 * c, c), fold_here(m_rows, c, c) and site not in self.a2,
                               fold_here(m_rows, 8 * c, c, True))
        rowblock = self.dtype == F16          # (the row-block fusions have no bf16 form)
        fused_tail = rowblock and FUSED_FFN and c == 320 and (h * w_) % 64 == 0 and m_rows // 64 >= FFN_MIN_BLOCKS
        xpart = self.gn_partials.get(x.data_ptr())
        fused_head = (rowblock and FUSED_HEAD and c == 320 and (h * w_) % 64 == 0 and m_rows // 64 >= FFN_MIN_BLOCKS
                      and xpart is not None and xpart[1] <= 256)
        ext = LN_STATS_FROM_PRODUCER and LN_FOLD == "auto"
        qkv_keys = [f".attn1.to_{n}.weight" for n in "qkv"]
        ln_box = [None]                 # the normalised copy, allocated only if some LayerNorm still runs as a kernel

        def ln_of(src, norm):
            if ln_box[0] is None:
                ln_box[0] = self.pool.get(shp)
            self.rec(self.be.layernorm, src, self.f(tb + norm + ".weight"), self.f(tb + norm + ".bias"), ln_box[0])
            return ln_box[0]
        # attn1 (self)
        if fused_head:               # norm -> proj_in -> norm1 -> q|k|v in one launch (csrc/tf_head.hip)
            hstream = self.cached((u + tb, "head_stream"), lambda: self.be.to_device(pack_head_stream(
                self.sd[u + site + ".proj_in.weight"], *[self.sd[u + tb + k] for k in qkv_keys])),
                lambda t: [Recipe("head_stream", [u + site + ".proj_in.weight"] + [u + tb + k for k in qkv_keys], (t,))])
            hs = self.pool.get(shp)
            qkv = self.pool.get((b, h, w_, 3 * c))
            self.rec(self.be.tf_head, x.view(b, h * w_, c), hstream, xpart[0], xpart[1], self.f(site + ".norm.weight"),
                     self.f(site + ".norm.bias"), self.f(site + ".proj_in.bias"), self.f(tb + ".norm1.weight"),
                     self.f(tb + ".norm1.bias"), hs.view(b, h * w_, c), qkv.view(b, h * w_, 3 * c))
        else:
            g = self.gn(x, None, self.f(site + ".norm.weight"), self.f(site + ".norm.bias"), 1e-6, 0)
            hs = self.conv(g, self.w(site + ".proj_in.weight"), shp, bias=self.f(site + ".proj_in.bias"),
                           taps=1, pad=0, ln_stats=ext and not fold1)
            self.pool.put(g)

            def _qkv():
                return self.be.to_device(torch.cat([self.sd[u + tb + k] for k in qkv_keys]), self.dtype)
            qkv = self._ln_then_linear(hs, (b, h, w_, 3 * c), fold1, lambda: self._ln_linear(tb, ".norm1", "qkv", qkv_keys),
                                       lambda: (self.cached((u + tb, "qkv"), _qkv, lambda t: [
                                           Recipe("cast", [u + tb + k for k in qkv_keys], (t,))]), None),
                                       lambda: ln_of(hs, ".norm1"))
        att = self.pool.get(shp)
        self.rec(self.be.self_attn, qkv.view(b, h * w_, 3 * c), att.view(b, h * w_, c), HEADS)
        self.pool.put(qkv)
        h2 = self.conv(att, self.w(tb + ".attn1.to_out.0.weight"), shp,
                       bias=self.f(tb + ".attn1.to_out.0.bias"), residual=hs, taps=1, pad=0,
                       ln_stats=ext and not fold2)
        self.pool.put(hs)
        # attn2 (DADD cross-attention); its output h3 comes with row partials where the GEGLU projection can fold norm3 with them
        if site in self.a2:          # one kernel: x (W_q K^T) -> 24 softmaxes -> P (V W_o^T) + bias + residual
            st = self.a2[site]
            st2 = self.ln_partials.get(h2.data_ptr())
            kw2 = {}
            if st2 is not None:          # norm2 folded into the score GEMM: mcat carries gamma (prepare_attn2)
                st["fold"] = True
                lnx = h2
                kw2 = dict(ln_stats_in=st2, ln_c1=st["ln_c1"], ln_d=st["ln_d"], ln_eps=1e-5)
            else:
                lnx = ln_of(h2, ".norm2")
            h3 = self.pool.get(shp)
            if ext and not fold3 and c % 80 == 0 and not fused_tail:
                kw2["ln_stats_out"] = self._ln_partials_for(h3, c // 80)
            self.rec(self.be.attn2_fused, lnx.view(b, h * w_, c), st["mcat"], st["vw"],
                     self.f(tb + ".attn2.to_out.0.bias"), h2.view(b, h * w_, c), h3.view(b, h * w_, c), **kw2)
        else:
            q = self._ln_then_linear(
                h2, shp, fold2, lambda: self._ln_linear(tb, ".norm2", "to_q", [".attn2.to_q.weight"]),
                lambda: (self.w(tb + ".attn2.to_q.weight"), None), lambda: ln_of(h2, ".norm2"))
            self.rec(self._xattn, site, q.view(b, h * w_, c), att.view(b, h * w_, c))
            self.pool.put(q)
            h3 = self.conv(att, self.w(tb + ".attn2.to_out.0.weight"), shp,
                           bias=self.f(tb + ".attn2.to_out.0.bias"), residual=h2, taps=1, pad=0,
                           ln_stats=ext and not fold3 and not fused_tail)
        self.pool.put(h2, att)
        if fused_tail:               # norm3 -> GEGLU -> FF-out + h3 -> proj_out + x in one launch (csrc/ffn_block.hip)
            def _tail():
                st, b1p = pack_ffn_stream(self.sd[u + tb + ".ff.net.0.proj.weight"], self.sd[u + tb + ".ff.net.0.proj.bias"],
                                          self.sd[u + tb + ".ff.net.2.weight"], self.sd[u + site + ".proj_out.weight"])
                return self.be.to_device(st), self.be.to_device(b1p)
            stream, b1p = self.cached((u + tb, "ffn_stream"), _tail, lambda t: [Recipe("ffn_stream", (
                u + tb + ".ff.net.0.proj.weight", u + tb + ".ff.net.0.proj.bias", u + tb + ".ff.net.2.weight",
                u + site + ".proj_out.weight"), t)])
            out = self.pool.get(shp)
            nchunk = (h * w_) // 32
            gkw = {}
            if GN_FROM_EPILOGUE and nchunk <= 128 and (h * w_) * (c // 32) * 2 > GN_FUSED_MAX_BYTES:
                gkw = self._gn_partials_for(out, nchunk)
            if ln_box[0] is not None:
                self.pool.put(ln_box[0])
            self.rec(self.be.ffn_block, h3.view(b, h * w_, c), stream, self.f(tb + ".norm3.weight"), self.f(tb + ".norm3.bias"),
                     b1p, self.f(tb + ".ff.net.2.bias"), self.f(site + ".proj_out.bias"), x.view(b, h * w_, c),
                     out.view(b, h * w_, c), **gkw)
            self.pool.put(h3)
            return out

        def _geglu():
            wf, bf = geglu_interleave(self.sd[u + tb + ".ff.net.0.proj.weight"], self.sd[u + tb + ".ff.net.0.proj.bias"])
            return self.be.to_device(wf, self.dtype), self.be.to_device(bf.float())
        # GEGLU feed-forward
        ff = self._ln_then_linear(
            h3, (b, h, w_, 4 * c), fold3,
            lambda: self._ln_linear(tb, ".norm3", "geglu", [".ff.net.0.proj.weight"], ".ff.net.0.proj.bias", geglu=True),
            lambda: self.cached((u + tb, "geglu"), _geglu, lambda t: [Recipe("geglu", (
                u + tb + ".ff.net.0.proj.weight", u + tb + ".ff.net.0.proj.bias"), t)]),
            lambda: ln_of(h3, ".norm3"), flags=L.EPI_GEGLU)
        self.pool.put(ln_box[0])
        h4 = self.conv(ff, self.w(tb + ".ff.net.2.weight"), shp, bias=self.f(tb + ".ff.net.2.bias"),
                       residual=h3, taps=1, pad=0)
        self.pool.put(ff, h3)
        out = self.conv(h4, self.w(site + ".proj_out.weight"), shp, bias=self.f(site + ".proj_out.bias"),
                        residual=x, taps=1, pad=0, gn_stats=True)
        self.pool.put(h4)
        return out

    def _xattn(self, site, q, out):
        mode = L.XATTN_SPLIT if self.gates_mode else L.XATTN_BASELINE
        kv = self.kv[site][self.kv_slot]
        self.be.tri_xattn(q, kv.view(self.B, self.T, -1), out, self.gates[site], self.lam, mode, HEADS,
                          lam_dev=self.params[0:1] if (self.params_dev and self.gates_mode) else None)

    def _emit_eps(self, x, w, bias):
        if self.ddim_coef is not None:      # sampler step without CFG: conv_out and the DDIM update in one launch
            self.be.conv_out_ddim(x, w, bias, self.lat_in, self.ddim_coef)
        else:
            self.be.conv_cout4(x, w, bias, self.eps_out[self.kv_slot], 0)

    def _build(self):
        b, s = self.B, self.S
        h = self.pool.get((b, s, s, 320))
        gkw = {}
        if GN_FROM_EPILOGUE and (s * s) % 256 == 0 and (s * s) // 256 <= 128 and s * s * 10 * 2 > GN_FUSED_MAX_BYTES:
            # conv_in writes the GroupNorm chunk partials of its output (256 pixels per chunk): no statistics pass for the
            # first ResNet's norm1 nor for the last up block's skip-concat, and both can normalise inside their 3x3 conv
            gkw = self._gn_partials_for(h, (s * s) // 256)
        self.rec(self.be.conv_in_nchw, self.lat_in, self.w("conv_in.weight", pack_conv_cin8), self.f("conv_in.bias"), h, **gkw)
        skips = [h]
        for i in range(4):
            for j in range(2):
                if i < 3:
                    nxt = self._gn_of(f"down_blocks.{i}.attentions.{j}.norm", 1e-6, 0)
                else:
                    nxt = self._gn_of("down_blocks.3.resnets.1.norm1" if j == 0 else "mid_block.resnets.0.norm1", 1e-5, 1)
                hn = self._resnet(f"down_blocks.{i}.resnets.{j}", h, next_gn=nxt)
                if h is not skips[-1]:
                    self.pool.put(h)
                h = hn
                if i < 3:
                    hn = self._transformer(f"down_blocks.{i}.attentions.{j}", h)
                    self.pool.put(h)
                    h = hn
                skips.append(h)
            if i < 3:
                c = h.shape[-1]
                h = self.conv(h, self.w(f"down_blocks.{i}.downsamplers.0.conv.weight"),
                              (b, h.shape[1] // 2, h.shape[2] // 2, c),
                              bias=self.f(f"down_blocks.{i}.downsamplers.0.conv.bias"), stride=2, pad=1, gn_stats=True,
                              fuse_gn=self._gn_of(f"down_blocks.{i + 1}.resnets.0.norm1", 1e-5, 1))
                skips.append(h)
        hn = self._resnet("mid_block.resnets.0", h, next_gn=self._gn_of("mid_block.attentions.0.norm", 1e-6, 0))        # h is skips[-1]: keep
        h = hn
        hn = self._transformer("mid_block.attentions.0", h)
        self.pool.put(h)
        h = self._resnet("mid_block.resnets.1", hn)
        self.pool.put(hn)
        for i in range(4):
            for j in range(3):
                skip = skips.pop()
                hn = self._resnet(f"up_blocks.{i}.resnets.{j}", h, skip,
                                  next_gn=self._gn_of(f"up_blocks.{i}.attentions.{j}.norm", 1e-6, 0) if i > 0 else None)
                self.pool.put(h, skip)
                h = hn
                if i > 0:
                    hn = self._transformer(f"up_blocks.{i}.attentions.{j}", h)
                    self.pool.put(h)
                    h = hn
            if i < 3:
                c = h.shape[-1]
                hn = self.conv(h, self.w(f"up_blocks.{i}.upsamplers.0.conv.weight"),
                               (b, h.shape[1] * 2, h.shape[2] * 2, c),
                               bias=self.f(f"up_blocks.{i}.upsamplers.0.conv.bias"), ups=1, pad=1)
                self.pool.put(h)
                h = hn
        g = self.gn(h, None, self.f("conv_norm_out.weight"), self.f("conv_norm_out.bias"), 1e-5, 1)
        self.rec(self._emit_eps, g, self.w("conv_out.weight", pack_conv_cout4), self.f("conv_out.bias"))
        self.pool.put(h, g)
        self._end_build(prefetch_weights=True)

    # -- step-invariant preparation ----------------------------------------------------------------
    def set_cond(self, cond: torch.Tensor, slot: int = 0):
        """Project the conditioning tokens through to_k/to_v(/to_k_dis/to_v_dis) of all 16 sites."""
        if cond.dim() == 2:
            cond = cond.unsqueeze(1)
        if cond.dim() != 3:
            raise ValueError(f"cond_embed must have shape (B, D) or (B, seq_len, D), got {tuple(cond.shape)}")
        if cond.shape[0] != self.B or cond.shape[1] != self.T or cond.shape[2] != 768:
            raise ValueError(f"cond_embed must be ({self.B}, {self.T}, 768) for this plan, got {tuple(cond.shape)}")
        self.be.copy_(self.cond16, cond)
        for site, _ in self.sites:
            self.be.igemm(self.cond16, self.kv_w[site], self.kv[site][slot], taps=1, pad=0)
        self.cond_gen += 1
        if slot == 0:
            self._a2_dirty = True

    def prepare_attn2(self, lam: float):
        """Fold W_q / W_o and the gates into the conditioning of the fused attn2 sites (once per run;
        never inside a graph capture: a no-op when neither the conditioning nor lambda changed)."""
        if not self.a2 or (not self._a2_dirty and self._a2_lam == float(lam)):
            return
        B = self.B
        with self.be.ctx(), torch.no_grad():
            for grp in self.a2_groups:
                names, c = grp["sites"], grp["c"]
                ns, d = len(names), c // HEADS
                kv = torch.stack([self.kv[n][0].view(B, self.T, 4 * c) for n in names]).float()     # s b t 4c
                hd = lambda t: t.reshape(ns, B, 16, HEADS, d)                     # noqa: E731
                ks = [hd(kv[:, :, 16:32, 0:c]), hd(kv[:, :, 0:16, 2 * c:3 * c]), hd(kv[:, :, 32:48, 2 * c:3 * c])]
                vs = [hd(kv[:, :, 16:32, c:2 * c]), hd(kv[:, :, 0:16, 3 * c:4 * c]), hd(kv[:, :, 32:48, 3 * c:4 * c])]
                g = grp["gates"]                                                  # [s][anat, dis]
                gp = [g[:, 0].view(ns, 1, 1, 1, 1), g[:, 1].view(ns, 1, 1, 1, 1),
                      torch.full((), float(lam), device=g.device)]                # (a fill, not an upload: no host wait)
                scale = math.log2(math.e) / math.sqrt(d)
                m = torch.stack([torch.einsum("sbthd,shdc->sbhtc", k, grp["wq"]) for k in ks], dim=3) * scale   # s b h p t c
                v = torch.stack([torch.einsum("snhd,sbthd->sbnht", grp["wo"], x) * gg for x, gg in zip(vs, gp)], dim=4)  # s b n h p t
                if float(lam) == 0.0:      # routing_gates.py:160,177-178: the delta pathway is skipped, not scaled —
                    m[:, :, :, 2] = 0.0    # zero scores and zero values: garbage (NaN) delta tokens cannot leak
                    v[:, :, :, :, 2] = 0.0
                m = m.reshape(ns, B, 384, c)
                folds = [bool(self.a2[n]["fold"]) for n in names]
                if any(folds):             # LayerNorm 2 folded in: S = rstd (x (gamma o M)^T - mu c1) + M beta
                    assert all(folds), "fused attn2 sites of one width fold norm2 alike"
                    grp["ln_d"].copy_((m * grp["beta"]).sum(dim=-1))
                    m = m * grp["gamma"]
                grp["mcat"].copy_(m)
                if any(folds):             # c1 sums the ROUNDED rows, so that the mean term cancels exactly
                    grp["ln_c1"].copy_(grp["mcat"].float().sum(dim=-1))
                grp["vw"].copy_(v.reshape(ns, B, c, 384))
        self._a2_dirty, self._a2_lam = False, float(lam)

    def time_rows(self, t: torch.Tensor, out: torch.Tensor):
        """rows[m] = cat_r time_emb_proj_r(SiLU(MLP(sinusoid(t[m]))))  for a vector of timesteps."""
        m = t.shape[0]
        feat = self.be.empty((m, 320), F32)
        t1 = self.be.empty((m, 1280), F32)
        t2 = self.be.empty((m, 1280), F32)
        self.be.timestep_features(t, feat)
        self.be.linear_rows(feat, self.w_t1, self.b_t1, t1, 0, 1)      # Linear -> SiLU
        self.be.linear_rows(t1, self.w_t2, self.b_t2, t2, 0, 0)        # Linear  (= temb)
        self.be.linear_rows(t2, self.w_tp, self.b_tp, out, 1, 0)       # SiLU -> 22 x Linear
        return t2

    def run_slot(self, slot: int, lam: float):
        self.kv_slot, self.lam = slot, lam
        self.run()

    def forward(self, latents: torch.Tensor, t: torch.Tensor, cond: Optional[torch.Tensor],
                lam: float = 0.0) -> torch.Tensor:
        """General ``module(latents, t, cond)`` call: eps for arbitrary per-sample timesteps.
        ``cond=None`` reuses the projections of the previous ``set_cond``."""
        if tuple(latents.shape) != tuple(self.lat_in.shape):
            raise ValueError(f"latents must be {tuple(self.lat_in.shape)}, got {tuple(latents.shape)}")
        if t.dim() == 0:
            t = t[None]
        t = t.reshape(-1).long()
        if t.shape[0] == 1:
            t = t.expand(self.B)
        if t.shape[0] != self.B:
            raise ValueError(f"timesteps must have {self.B} entries, got {t.shape[0]}")
        if cond is not None:
            self.set_cond(cond, 0)
        self.time_rows(self.be.to_device(t.contiguous()), self.temb_rows)
        self.be.copy_(self.lat_in, latents.float())
        self.prepare_attn2(lam)
        self.run_slot(0, lam)
        return self.be.clone(self.eps_out[0])


# ----------------------------------------------------------------------------- VAE
class _VaePlan(_Plan):
    """What the decoder and the encoder plans share: fp16 storage, the ResNet and the attention block."""

    def __init__(self, be, sd, batch: int, side: int, prefix):
        super().__init__(be, sd=sd, prefix=prefix)
        self.frozen = True               # nothing trains the VAE: no recipes
        self.B, self.S = batch, side
        self.gn_ws = be.empty((batch * L.GN_MAX_CHUNKS * GROUPS * 2,), F32)

    def _res(self, name, x):
        b, h, w_, cin = x.shape
        cout = self.sd[self.prefix + name + ".conv1.weight"].shape[0]
        g1 = self.gn(x, None, self.f(name + ".norm1.weight"), self.f(name + ".norm1.bias"), 1e-6, 1)
        h1 = self.conv(g1, self.w(name + ".conv1.weight"), (b, h, w_, cout), bias=self.f(name + ".conv1.bias"),
                       gn_stats=True)
        self.pool.put(g1)
        g2 = self.gn(h1, None, self.f(name + ".norm2.weight"), self.f(name + ".norm2.bias"), 1e-6, 1)
        self.pool.put(h1)
        res = x
        if cin != cout:
            res = self.conv(x, self.w(name + ".conv_shortcut.weight"), (b, h, w_, cout),
                            bias=self.f(name + ".conv_shortcut.bias"), taps=1, pad=0)
        out = self.conv(g2, self.w(name + ".conv2.weight"), (b, h, w_, cout),
                        bias=self.f(name + ".conv2.bias"), residual=res, gn_stats=True)
        self.pool.put(g2)
        if res is not x:
            self.pool.put(res)
        return out

    def _attn(self, name, x):
        b, h, w_, c = x.shape
        g = self.gn(x, None, self.f(name + ".group_norm.weight"), self.f(name + ".group_norm.bias"), 1e-6, 0)
        wqkv = self.dev(torch.cat([self.sd[self.prefix + name + f".to_{n}.weight"] for n in "qkv"]), F16)
        bqkv = self.dev(torch.cat([self.sd[self.prefix + name + f".to_{n}.bias"] for n in "qkv"]).float())
        qkv = self.conv(g, wqkv, (b, h, w_, 3 * c), bias=bqkv, taps=1, pad=0)
        self.pool.put(g)
        att = self.pool.get((b, h, w_, c))
        self.rec(self.be.self_attn, qkv.view(b, h * w_, 3 * c), att.view(b, h * w_, c), 1)
        self.pool.put(qkv)
        out = self.conv(att, self.w(name + ".to_out.0.weight"), (b, h, w_, c),
                        bias=self.f(name + ".to_out.0.bias"), residual=x, taps=1, pad=0, gn_stats=True)
        self.pool.put(att)
        return out

    def _mid(self, side, h):
        """ResNet, attention, ResNet of ``side`` ("decoder." / "encoder."); ``h`` returns to the pool."""
        for blk, name in ((self._res, "resnets.0"), (self._attn, "attentions.0"), (self._res, "resnets.1")):
            hn = blk(f"{side}mid_block.{name}", h)
            self.pool.put(h)
            h = hn
        return h


# ----------------------------------------------------------------------------- VAE decoder
class VaeDecoderPlan(_VaePlan):
    def __init__(self, be, sd, batch: int, side: int, *, prefix="vae.vae", latent_scale=0.18215):
        super().__init__(be, sd, batch, side, prefix)
        self.z_in = be.zeros((batch, 4, side, side), F32)
        self.img_out = be.zeros((batch, 3, side * 8, side * 8), F32)
        self.inv_scale = 1.0 / latent_scale
        self._build()

    def _build(self):
        b, s = self.B, self.S
        d = "decoder."
        z8 = self.pool.get((b, s, s, 8))
        pq_w = self.dev(self.sd[self.prefix + "post_quant_conv.weight"].reshape(4, 4).float())
        pq_b = self.f("post_quant_conv.bias")
        self.rec(self.be.pack_latents, self.z_in, z8, self.inv_scale, pq_w, pq_b)
        h = self.pool.get((b, s, s, 512))
        self.rec(self.be.conv_cin8, z8, self.w(d + "conv_in.weight", pack_conv_cin8), self.f(d + "conv_in.bias"), h)
        h = self._mid(d, h)
        for i in range(4):
            for j in range(3):
                hn = self._res(d + f"up_blocks.{i}.resnets.{j}", h)
                self.pool.put(h)
                h = hn
            if i < 3:
                c = h.shape[-1]
                hn = self.conv(h, self.w(d + f"up_blocks.{i}.upsamplers.0.conv.weight"),
                               (b, h.shape[1] * 2, h.shape[2] * 2, c),
                               bias=self.f(d + f"up_blocks.{i}.upsamplers.0.conv.bias"), ups=1, pad=1, gn_stats=True)
                self.pool.put(h)
                h = hn
        g = self.gn(h, None, self.f(d + "conv_norm_out.weight"), self.f(d + "conv_norm_out.bias"), 1e-6, 1)
        self.rec(self.be.conv_cout4, g, self.w(d + "conv_out.weight", pack_conv_cout4),
                 self.f(d + "conv_out.bias"), self.img_out, 1)
        self.pool.put(h, g)
        self._end_build()


# ----------------------------------------------------------------------------- VAE encoder
class VaeEncoderPlan(_VaePlan):
    """``SDVAE.encode`` (src/models/vae/vae.py:71-88) -> diffusers ``AutoencoderKL.encode``: images (B,3,H,W) in
    [-1,1] -> moments (mean, logvar), each (B,4,H/8,W/8) fp32 NCHW.  Same kernels as the decoder; the three
    downsamplers are 3x3 / stride-2 convolutions with the asymmetric (0,1,0,1) padding folded into the gather
    (pad = 0: the window runs one pixel past the bottom / right edge, where the gather returns zeros), and
    ``quant_conv`` (1x1, 8 -> 8) is composed into ``conv_out`` at plan time (two linear maps: exact algebra, one
    rounding of the composed weights to fp16).  ``side`` is the LATENT side (image side / 8)."""

    def __init__(self, be, sd, batch: int, side: int, *, prefix="vae.vae"):
        super().__init__(be, sd, batch, side, prefix)
        self.img_in = be.zeros((batch, 3, side * 8, side * 8), F32)
        self.mean = be.zeros((batch, 4, side, side), F32)
        self.logvar = be.zeros((batch, 4, side, side), F32)
        self._build()

    def _build(self):
        b, s = self.B, self.S * 8
        e = "encoder."
        x8 = self.pool.get((b, s, s, 8))
        self.rec(self.be.pack_latents, self.img_in, x8)
        h = self.pool.get((b, s, s, VAE_CH[0]))
        self.rec(self.be.conv_cin8, x8, self.w(e + "conv_in.weight", pack_conv_cin8), self.f(e + "conv_in.bias"), h)
        self.pool.put(x8)
        for i in range(4):
            for j in range(2):
                hn = self._res(e + f"down_blocks.{i}.resnets.{j}", h)
                self.pool.put(h)
                h = hn
            if i < 3:
                c = h.shape[-1]
                hn = self.conv(h, self.w(e + f"down_blocks.{i}.downsamplers.0.conv.weight"),
                               (b, h.shape[1] // 2, h.shape[2] // 2, c),
                               bias=self.f(e + f"down_blocks.{i}.downsamplers.0.conv.bias"), stride=2, pad=0,
                               gn_stats=True)
                self.pool.put(h)
                h = hn
        h = self._mid(e, h)
        g = self.gn(h, None, self.f(e + "conv_norm_out.weight"), self.f(e + "conv_norm_out.bias"), 1e-6, 1)
        # moments = quant_conv(conv_out(g)):  W' = Q W,  b' = Q b + q   (Q: 8x8 of the 1x1 conv)
        u = self.prefix
        q = self.sd[u + "quant_conv.weight"].reshape(8, 8).double()
        w = self.sd[u + e + "conv_out.weight"].double()
        wq = torch.einsum("oc,cikl->oikl", q, w).float()
        bq = (q @ self.sd[u + e + "conv_out.bias"].double() + self.sd[u + "quant_conv.bias"].double()).float()
        self.rec(self.be.conv_cout4, g, self.dev(pack_conv_cout4(wq[:4])), self.dev(bq[:4].contiguous()), self.mean, 0)
        self.rec(self.be.conv_cout4, g, self.dev(pack_conv_cout4(wq[4:])), self.dev(bq[4:].contiguous()), self.logvar, 2)
        self.pool.put(h, g)
        self._end_build()


# ----------------------------------------------------------------------------- DDIM loop
class DdimLoop:
    """Deterministic (eta = 0) DDIM loop over a UNetPlan: ONE captured step graph, replayed."""

    def __init__(self, unet: UNetPlan, max_steps: int = 1000):
        self.u = unet
        self.be = unet.be
        self.step = self.be.zeros((2,), torch.int32)       # row of the next step, block ticket of dadd_begin_step
        self.cur_coef = self.be.zeros((4,), F32)
        self.graphs: Dict[Tuple, object] = {}
        self.cap = 0
        self.table = None
        self.coef = None
        self.nsteps = 0
        self._prepared = None           # (timestep grid, schedule identity) the tables on the device were built for
        self._params = None             # (lambda, guidance) held by ``unet.params`` on the device
        self._reserve(64)

    def _reserve(self, n: int):
        if n <= self.cap:
            return
        for g in self.graphs.values():       # captured graphs hold the old table addresses
            self.be.graph_destroy(g)
        self.graphs.clear()
        self.cap = n
        self._prepared = None
        self.table = self.be.zeros((n, self.u.temb_cols), F32)
        self.coef = self.be.zeros((n, 4), F32)

    def prepare(self, timesteps: torch.Tensor, alphas_cumprod: torch.Tensor):
        """Coefficient rows computed on the host in fp32 exactly as the reference does per step
        (inference_pipeline_ip.py:434-450), and the time-embedding rows of every step.  Both depend on the timestep
        grid and the weights only: a repeated grid (every pass of a sweep) reuses the tables on the device — no
        device-to-host read of the grid, no upload, nothing that makes the host wait for the GPU, so the next pass is
        queued while the current one runs.  Callers on the hot path hand in a CPU grid (``torch.linspace`` gives the
        same integers on both devices: tests/test_gpu_parity.py::test_ddim_timestep_grid_on_device)."""
        ts = timesteps.detach()
        ts = (ts if ts.device.type == "cpu" else ts.cpu()).long()
        n = ts.shape[0]
        key = (tuple(ts.tolist()), alphas_cumprod.data_ptr(), alphas_cumprod._version, self.u.weights_gen)
        if key == self._prepared and n <= self.cap:
            self.nsteps = n
            return
        self._reserve(n)
        ac = alphas_cumprod.detach().cpu().float()
        coef = torch.empty(n, 4, dtype=F32)
        for i in range(n):
            a_t = ac[int(ts[i])]
            coef[i, 0], coef[i, 1] = torch.sqrt(a_t), torch.sqrt(1.0 - a_t)
            if i == n - 1:
                coef[i, 2], coef[i, 3] = -1.0, 0.0          # last step returns x0 (:441-443)
            else:
                a_p = ac[int(ts[i + 1])]
                coef[i, 2], coef[i, 3] = torch.sqrt(a_p), torch.sqrt(1.0 - a_p)
        self.be.copy_(self.coef[:n], self.be.to_device(coef))
        self.u.time_rows(self.be.to_device(ts), self.table[:n])
        self.nsteps = n
        self._prepared = key

    def set_params(self, lam: float, guidance: float):
        """lambda and the CFG scale live in device memory (``unet.params``): the captured step reads them there, so
        ONE graph per (cfg on/off) serves every (lambda, guidance) — the reference reads ``delta_scale`` per call
        (attention_processor_routing_gates.py:160).  The fused attn2 sites fold lambda into their step-invariant
        conditioning (``prepare_attn2``), which is device memory too."""
        if self._params != (float(lam), float(guidance)):      # (an upload from pageable memory blocks the host)
            self.be.copy_(self.u.params, torch.tensor([float(lam), float(guidance)], dtype=F32))
            self._params = (float(lam), float(guidance))
        self.u.prepare_attn2(lam)

    def sample(self, latents: torch.Tensor, timesteps: torch.Tensor, alphas_cumprod: torch.Tensor, lam: float,
               do_cfg: bool = False, guidance: float = 1.0, use_graph: bool = True,
               trace: Optional[list] = None) -> torch.Tensor:
        """All prepared steps from ``latents`` -> final latents, WITH both stream hand-offs: the backend stream waits
        for whatever torch's current stream has queued (conditioning caches written by torch ops, the latents), and
        the current stream waits for the returned tensor.  Callers that drive ``prepare`` / ``run`` by hand owe the
        same bracket (``with on_backend(be):``)."""
        be = self.be
        with on_backend(be):
            self.prepare(timesteps, alphas_cumprod)
            be.copy_(self.u.lat_in, latents)
            self.run(lam, do_cfg, guidance, use_graph=use_graph, trace=trace)
            return be.clone(self.u.lat_in)

    def _one_step(self, lam: float, do_cfg: bool, guidance: float, keep_eps: bool = False):
        """``keep_eps``: eps of the step stays readable in ``unet.eps_out`` (traces); otherwise, without CFG, conv_out
        applies the DDIM update itself (``dadd_conv_out_ddim_f16``) and eps is never stored."""
        u = self.u
        u.params_dev = True
        fused = not do_cfg and not keep_eps
        try:
            self.be.begin_step(self.table, u.temb_rows, self.coef, self.cur_coef, self.step)
            u.ddim_coef = self.cur_coef if fused else None
            u.run_slot(0, lam)
            if do_cfg:
                u.run_slot(1, lam)
            if not fused:
                self.be.ddim_update(u.lat_in, u.eps_out[0], u.eps_out[1] if do_cfg else None, guidance,
                                    self.cur_coef, guidance_dev=u.params[1:2])
        finally:
            u.params_dev = False
            u.ddim_coef = None

    def run(self, lam: float, do_cfg: bool = False, guidance: float = 1.0, use_graph: bool = True,
            trace: Optional[list] = None):
        """Runs all prepared steps in place on ``unet.lat_in``."""
        self.be.zero_(self.step)
        self.set_params(lam, guidance)
        if trace is not None or not use_graph:
            for _ in range(self.nsteps):
                self._one_step(lam, do_cfg, guidance, keep_eps=trace is not None)
                if trace is not None:
                    trace.append((self.be.clone(self.u.eps_out[0]), self.be.clone(self.u.lat_in)))
            return
        key = bool(do_cfg)
        g = self.graphs.get(key)
        if g is None:
            self.be.synchronize()
            self.be.graph_begin()
            try:
                self._one_step(lam, do_cfg, guidance)
            finally:
                g = self.be.graph_end()
            self.graphs[key] = g
        for _ in range(self.nsteps):
            self.be.graph_launch(g)
