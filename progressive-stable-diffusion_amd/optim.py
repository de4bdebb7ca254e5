"""The optimizer of a training step on the HIP kernels of csrc/optim.hip (include/dadd_hip_optim.h): AdamW over parameter
groups with global-norm gradient clipping, a loss scale with skip-on-overflow (``precision: 16-mixed``), the EMA of the
weights, the 16-bit working copy of the weights and the zeroing of the gradients.  One step is three launches (gradient
statistics, one workgroup of scalar work, one fused pass over the parameters) and no host synchronisation.

``ParamArena`` owns the flat fp32 buffers the kernels work on: master weights ``p``, gradients ``g``, the moments ``m``
and ``v``, optionally the EMA and the 16-bit copy ``p16``.  It is plain torch and lives on any device.  ``FusedAdamW``
owns the device-resident state block (step count, loss scale, per-group constants) and launches the kernels.
``reference_param_groups`` restates the grouping of the reference's ``configure_optimizers`` (src/models/
diffusion_module_ip.py: UNet and ordinal embedder at ``lr``, image projection and feature purifier at ``2 * lr``).

``DgradRelayout`` stands next to the arena: it owns the second 16-bit buffer that holds every weight in the layout its
data gradient reads, refreshed from ``p16`` by one launch of csrc/relayout.hip after each optimizer step.

``PlanRefresh`` goes the other way: it writes the packed weights of live inference plans again from the arena's fp32
masters or their EMA, by one launch of csrc/plan_refresh.hip per 16-bit type.

``training.Trainer`` wires these into a training step; ``DiffusionModuleWithIP.configure_optimizers()`` itself still
raises.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import torch

from . import lib as L
from .backend import on_backend

CHUNK = L.OPTIM_CHUNK
_ALIGN = 8          # elements: 32 bytes of fp32, 16 bytes of the 16-bit copy
_P16_FLAG = {torch.float16: L.OPTIM_P16_F16, torch.bfloat16: L.OPTIM_P16_BF16}


def _round_up(x: int, to: int) -> int:
    return -(-x // to) * to


class ParamArena:
    """Flat fp32 storage of a set of named parameters, laid out group by group.

    ``tensors``: ordered mapping name -> fp32 tensor (the initial values; copied).  ``group_of``: name -> group index.
    Every tensor starts on a multiple of 8 elements, so its fp32 view and its 16-bit view are both 16-byte aligned;
    every group is padded to a multiple of ``CHUNK`` elements, so one workgroup of the kernels never sees two groups.
    The padding is zero in every array and stays zero under the update (zero gradient, zero moments: the update term is
    0 / (0 + eps)).  ``names`` is the arena order: group 0's tensors in mapping order, then group 1's, ...
    """

    def __init__(self, tensors: Mapping[str, torch.Tensor], group_of: Mapping[str, int], *, device=None,
                 working_dtype: Optional[torch.dtype] = None, ema: bool = False):
        if not tensors:
            raise ValueError("ParamArena needs at least one tensor")
        for k, t in tensors.items():
            if t.dtype != torch.float32:
                raise ValueError(f"{k}: the arena holds fp32 masters, got {t.dtype}")
            if k not in group_of or int(group_of[k]) < 0:
                raise ValueError(f"{k}: no group index")
        self.n_groups = max(int(group_of[k]) for k in tensors) + 1
        if self.n_groups > L.OPTIM_MAX_GROUPS:
            raise ValueError(f"{self.n_groups} groups, the kernels take {L.OPTIM_MAX_GROUPS}")
        self.device = torch.device(device) if device is not None else next(iter(tensors.values())).device
        self.names: List[str] = []
        self.shapes: Dict[str, torch.Size] = {}
        self.offsets: Dict[str, int] = {}
        self.group_of: Dict[str, int] = {}
        self.group_names: List[List[str]] = [[] for _ in range(self.n_groups)]
        self.group_start: List[int] = []
        self.group_chunks: List[int] = []
        off = 0
        for gi in range(self.n_groups):
            self.group_start.append(off)
            for k, t in tensors.items():
                if int(group_of[k]) != gi:
                    continue
                off = _round_up(off, _ALIGN)
                self.names.append(k)
                self.shapes[k], self.offsets[k], self.group_of[k] = t.shape, off, gi
                self.group_names[gi].append(k)
                off += t.numel()
            off = _round_up(off, CHUNK)
            self.group_chunks.append((off - self.group_start[gi]) // CHUNK)
        self.numel = off
        self.n_chunks = off // CHUNK

        def flat():
            return torch.zeros(self.numel, dtype=torch.float32, device=self.device)
        self.p, self.g, self.m, self.v = flat(), flat(), flat(), flat()
        self.ema: Optional[torch.Tensor] = None
        self.p16: Optional[torch.Tensor] = None
        with torch.no_grad():
            for k in self.names:
                self._view(self.p, k).copy_(tensors[k])
        if ema:
            self.ensure_ema()
        if working_dtype is not None:
            self.ensure_p16(working_dtype)

    # -- optional arrays
    def ensure_ema(self) -> torch.Tensor:
        """Allocate the EMA (a copy of the current weights) unless it exists."""
        if self.ema is None:
            self.ema = self.p.clone()
        return self.ema

    def ensure_p16(self, dtype: torch.dtype) -> torch.Tensor:
        """Allocate the 16-bit working copy (the current weights, rounded) unless it exists; the type is fixed then."""
        if dtype not in _P16_FLAG:
            raise ValueError(f"the working copy is fp16 or bf16, not {dtype}")
        if self.p16 is None:
            self.p16 = self.p.to(dtype)
        elif self.p16.dtype != dtype:
            raise ValueError(f"the arena's working copy is {self.p16.dtype}, not {dtype}")
        return self.p16

    # -- views
    def _view(self, flat: torch.Tensor, name: str) -> torch.Tensor:
        off, shape = self.offsets[name], self.shapes[name]
        return flat[off:off + shape.numel()].view(shape)

    def param(self, name: str) -> torch.Tensor:
        """fp32 master weight, a view of ``p`` in the tensor's own shape."""
        return self._view(self.p, name)

    def grad(self, name: str) -> torch.Tensor:
        return self._view(self.g, name)

    def param16(self, name: str) -> torch.Tensor:
        """The 16-bit working copy the optimizer step refreshes: what a forward kernel reads instead of casting."""
        if self.p16 is None:
            raise RuntimeError("the arena has no 16-bit working copy (working_dtype / ensure_p16)")
        return self._view(self.p16, name)

    def exp_avg(self, name: str) -> torch.Tensor:
        return self._view(self.m, name)

    def exp_avg_sq(self, name: str) -> torch.Tensor:
        return self._view(self.v, name)

    def ema_param(self, name: str) -> torch.Tensor:
        if self.ema is None:
            raise RuntimeError("the arena has no EMA (ema=True / ensure_ema)")
        return self._view(self.ema, name)

    def attach(self, params: Mapping[str, torch.Tensor]) -> None:
        """Make each given leaf tensor a view of ``p`` with ``.grad`` preset to the matching view of ``g``: autograd
        then accumulates in place into the arena (torch adds into an existing ``.grad``), which is gradient
        accumulation over micro-batches and leaves one flat gradient buffer.  The tensor's current values are dropped:
        the arena's are the truth."""
        for k, t in params.items():
            if k not in self.offsets:
                raise KeyError(f"{k} is not in the arena")
            if not t.is_leaf or t.shape != self.shapes[k] or t.dtype != torch.float32:
                raise ValueError(f"{k}: expected an fp32 leaf of shape {tuple(self.shapes[k])}, got {tuple(t.shape)} {t.dtype}")
            t.data = self.param(k)
            t.grad = self.grad(k)


RELAYOUT_KINDS = {"T": L.RELAYOUT_T, "S2": L.RELAYOUT_S2, "UPS": L.RELAYOUT_UPS, "COUT4": L.RELAYOUT_COUT4}


def relayout_plan(items: Sequence[Tuple[int, int, int, int, str, int]], src_numel: int, dst_numel: int):
    """The descriptor table of one re-layout launch.  ``items``: ``(src_off, dst_off, N, C, kind, taps)`` per tensor, in
    ascending ``dst_off`` order; ``kind`` one of ``RELAYOUT_KINDS``.  -> ``(table, n_tiles)``: a ctypes array of
    ``lib.RelayoutDesc`` with ``tile0`` filled in and the grid of the launch.  The library checks the contract of
    include/dadd_hip_relayout.h (alignment, multiples of 8, every range inside its array, destinations disjoint) and a
    breach is a ``ValueError``; nothing here needs a GPU."""
    if not items:
        raise ValueError("relayout_plan: no tensors")
    table = (L.RelayoutDesc * len(items))()
    for d, (src_off, dst_off, n, c, kind, taps) in zip(table, items):
        if kind not in RELAYOUT_KINDS:
            raise ValueError(f"relayout_plan: kind {kind!r} is none of {sorted(RELAYOUT_KINDS)}")
        d.src_off, d.dst_off, d.N, d.C, d.kind, d.taps = int(src_off), int(dst_off), int(n), int(c), RELAYOUT_KINDS[kind], int(taps)
    lib = L.load()
    n_tiles = lib.dadd_dgrad_relayout_plan(table, len(items), int(src_numel), int(dst_numel))
    if n_tiles < 0:
        raise ValueError((lib.dadd_last_error() or b"").decode())
    return table, int(n_tiles)


def relayout_dst_numel(kind: str, taps: int, n: int, c: int) -> int:
    """Elements of the re-laid copy of an ``[N][taps*C]`` weight of ``kind``; ``ValueError`` outside the contract."""
    r = L.load().dadd_relayout_dst_numel(RELAYOUT_KINDS.get(kind, -1), int(taps), int(n), int(c))
    if r < 0:
        raise ValueError(f"relayout: kind {kind!r}, taps {taps}, N {n}, C {c} is outside the contract (N and C multiples of "
                         "8; COUT4: N 1..4; taps 1 or 9 for T, 9 otherwise)")
    return int(r)


class _Launcher:
    """What ``DgradRelayout``, ``PlanRefresh`` and ``FusedAdamW`` share: ``be`` (``None``: the owner holds its device
    blocks but cannot launch), the upload of a ctypes block, and the stream bracket around ``launch()``."""
    _HOLDS = ""         # how the "built without a backend" error ends, in the owner's words

    def _need_backend(self) -> None:
        if self.be is None:
            raise RuntimeError(f"{type(self).__name__} was built without a backend: {self._HOLDS}")

    def _upload_words(self, block, dst: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A ctypes block as int32 words into ``dst`` (default: a new tensor on the arena's device), through the backend's
        stream when there is one."""
        words = torch.frombuffer(bytearray(bytes(block)), dtype=torch.int32)
        if dst is None:
            dst = torch.zeros(words.numel(), dtype=torch.int32, device=self.arena.device)
        if self.be is not None:
            # half a hand-off: ``dst`` (and the moments a load wrote) were produced on torch's stream; only the backend's
            # stream reads the block, and the bracket of the next refresh() / step() releases
            self.be.wait_current()
            self.be.copy_(dst, words)
        else:
            dst.copy_(words)
        return dst

    def _bracketed_launch(self, *args) -> None:
        """``launch(*args)`` ordered after torch's current stream and before what it does next; in a graph capture the
        bracket does nothing and the bare launches are recorded."""
        self._need_backend()
        with on_backend(self.be):
            self.launch(*args)


class DgradRelayout(_Launcher):
    """Owner of the data-gradient layouts of an arena's weights: a flat 16-bit buffer ``wt`` beside ``arena.p16`` and the
    device-resident descriptor table of the launch that fills it.

    ``entries``: ``(name, kind)`` or ``(name, kind, taps)`` per weight; the arena holds it as ``[N][taps*C]``.  ``kind``:
    ``"T"`` (``grad_ops.dgrad_weight``; ``taps`` 1 unless given as 9), ``"S2"`` (``dgrad_weight_stride2``), ``"UPS"``
    (``dgrad_weight_ups``), ``"COUT4"`` (``dgrad_weight_cout4``).  Buffer and table are allocated once; ``refresh()`` is
    one launch on the backend's stream, ordered like ``FusedAdamW.step``.  ``w16(name)`` / ``wt(name)`` are the views a
    ``grad_ops`` product takes as ``prepared=``.  ``be=None`` gives an owner that holds the table but cannot launch."""
    _HOLDS = "it holds the table but cannot launch"

    def __init__(self, be, arena: ParamArena, entries: Sequence[tuple]):
        if arena.p16 is None:
            raise RuntimeError("DgradRelayout reads the arena's 16-bit working copy (working_dtype / ensure_p16)")
        if be is not None and arena.device != be.device:
            raise ValueError(f"the arena lives on {arena.device}, the backend on {be.device}")
        self.be, self.arena = be, arena
        self.kinds: Dict[str, Tuple[str, int]] = {}
        self.offsets: Dict[str, int] = {}
        self.shapes: Dict[str, Tuple[int, ...]] = {}
        items, off = [], 0
        for e in entries:
            name, kind = e[0], e[1]
            taps = int(e[2]) if len(e) > 2 else (1 if kind == "T" else 9)
            if name not in arena.offsets:
                raise KeyError(f"{name} is not in the arena")
            if name in self.kinds:
                raise ValueError(f"{name} is listed twice")
            shape = arena.shapes[name]
            if len(shape) != 2 or shape[1] % taps:
                raise ValueError(f"{name}: expected the library layout [N][{taps}*C], got {tuple(shape)}")
            n, c = int(shape[0]), int(shape[1]) // taps
            numel = relayout_dst_numel(kind, taps, n, c)
            self.kinds[name], self.offsets[name] = (kind, taps), off
            self.shapes[name] = (c, 9, 8) if kind == "COUT4" else (c, numel // c)
            items.append((arena.offsets[name], off, n, c, kind, taps))
            off += _round_up(numel, _ALIGN)
        self.numel = off
        self._table, self.n_tiles = relayout_plan(items, arena.numel, self.numel)
        self.n_desc = len(items)
        self.buf = torch.zeros(self.numel, dtype=arena.p16.dtype, device=arena.device)
        self.table = self._upload_words(self._table)

    def launch(self) -> None:
        """The one launch on the backend's stream, nothing else: what a graph capture records."""
        self._need_backend()
        self.be.dgrad_relayout(self.arena.p16, self.buf, self.table, self.n_desc, self.n_tiles)

    def refresh(self) -> None:
        """Re-lay every listed weight from the arena's current ``p16``.  Ordered after torch's current stream and before
        what it does next, like ``FusedAdamW.step``; no host sync."""
        self._bracketed_launch()

    def w16(self, name: str) -> torch.Tensor:
        """The 16-bit working copy of ``name``: ``arena.param16``."""
        return self.arena.param16(name)

    def wt(self, name: str) -> torch.Tensor:
        """The re-laid copy of ``name`` as of the last ``refresh()``: ``[C][slabs*N]``, COUT4 ``[C][9][8]``."""
        off, shape = self.offsets[name], self.shapes[name]
        numel = 1
        for v in shape:
            numel *= v
        return self.buf[off:off + numel].view(shape)

    def prepared(self, name: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(w16, wt)`` of ``name``: the ``prepared=`` argument of the ``grad_ops`` products."""
        return self.w16(name), self.wt(name)


PLAN_REFRESH_KINDS = {"COPY32": L.PLAN_REFRESH_COPY32, "CAST": L.PLAN_REFRESH_CAST, "GEGLU_W": L.PLAN_REFRESH_GEGLU_W,
                      "GEGLU_B": L.PLAN_REFRESH_GEGLU_B, "LNFOLD": L.PLAN_REFRESH_LNFOLD, "UPSFOLD": L.PLAN_REFRESH_UPSFOLD,
                      "HEAD_STREAM": L.PLAN_REFRESH_HEAD_STREAM, "FFN_STREAM": L.PLAN_REFRESH_FFN_STREAM,
                      "FFN_BIAS": L.PLAN_REFRESH_FFN_BIAS}
_PR_F32 = ("COPY32", "GEGLU_B", "FFN_BIAS")


def plan_refresh_table(items: Sequence[dict], src_numel: int):
    """The descriptor table of one refresh launch.  ``items``: dicts with ``kind`` (a key of ``PLAN_REFRESH_KINDS``),
    ``N``, ``K``, ``Cs``, ``flags``, ``src`` (up to four element offsets into the flat fp32 source, -1 = absent) and
    ``dst`` (up to three ``(address, room in elements)`` pairs).  -> ``(table, n_wgs)``: a ctypes array of
    ``lib.PlanRefreshDesc`` with ``wg0`` filled in and the grid of the launch.  The library checks the contract of
    include/dadd_hip_plan_refresh.h (sizes, alignment, every source range inside the array, room behind every
    destination, destinations disjoint) and a breach is a ``ValueError``; nothing here needs a GPU: the addresses are
    compared, never read."""
    if not items:
        raise ValueError("plan_refresh_table: no tensors")
    table = (L.PlanRefreshDesc * len(items))()
    for d, it in zip(table, items):
        if it["kind"] not in PLAN_REFRESH_KINDS:
            raise ValueError(f"plan_refresh_table: kind {it['kind']!r} is none of {sorted(PLAN_REFRESH_KINDS)}")
        d.kind, d.N, d.K, d.Cs = PLAN_REFRESH_KINDS[it["kind"]], int(it["N"]), int(it.get("K", 0)), int(it.get("Cs", 0))
        d.flags = int(it.get("flags", 0))
        src, dst = list(it["src"]), list(it["dst"])
        for i in range(4):
            d.src_off[i] = int(src[i]) if i < len(src) else -1
        for i in range(3):
            d.dst[i], d.dst_room[i] = (int(dst[i][0]), int(dst[i][1])) if i < len(dst) else (None, 0)
    lib = L.load()
    n_wgs = lib.dadd_plan_refresh_plan(table, len(items), int(src_numel))
    if n_wgs < 0:
        raise ValueError((lib.dadd_last_error() or b"").decode())
    return table, int(n_wgs)


class PlanRefresh(_Launcher):
    """Owner of the launch that writes the packed weights of live plans again from an arena's fp32 masters: the
    device-resident descriptor tables of csrc/plan_refresh.hip, built from the ``engine.Recipe`` lists of the plans
    (``UNetPlan.recipes``) and of the conditioning modules (``conditioning._Params.recipes``).

    Every source key of a recipe must be in the arena, in the library layout.  Recipes that name the same destination
    (plans over one weight cache) are written once.  The tables are built and uploaded once; ``refresh(source)`` is one
    launch per 16-bit type among the destinations on the backend's stream (fp16 plans: one; bf16 plans: two, their time
    path is fp16), ordered like ``FusedAdamW.step``.  The destinations keep their addresses: a captured graph that
    reads them reads the new weights.  ``be=None`` gives an owner that holds the tables but cannot launch."""
    _HOLDS = "it holds the tables but cannot launch"

    def __init__(self, be, arena: ParamArena, recipes: Sequence):
        if be is not None and arena.device != be.device:
            raise ValueError(f"the arena lives on {arena.device}, the backend on {be.device}")
        self.be, self.arena = be, arena
        self.items: Dict[torch.dtype, List[dict]] = {}
        self._dst: List[torch.Tensor] = []          # the destinations stay alive as long as their addresses are in a table
        # Recipes count as the same when their FIRST destination starts at the same address (plans over one weight
        # cache record identical recipes).  The library checks that destinations are disjoint within one table only;
        # across the two tables nothing checks it: it holds because a table takes destinations of one 16-bit type and
        # all fp32 destinations go to a single table, and a tensor has one type.
        seen, expanded = set(), []
        for r in recipes:
            ptr = r.dst[0].data_ptr()
            if ptr in seen:
                continue
            seen.add(ptr)
            self._dst += list(r.dst)
            expanded += self._expand(r)
        if not expanded:
            raise ValueError("PlanRefresh: no recipes")
        # one table (= one launch) per 16-bit type among the destinations; the fp32 kinds ride with the larger one
        count = {dt: sum(1 for it in expanded if it["kind"] not in _PR_F32 and it["out"][0][0].dtype == dt)
                 for dt in (torch.float16, torch.bfloat16)}
        major = torch.bfloat16 if count[torch.bfloat16] > count[torch.float16] else torch.float16
        for it in expanded:
            self.items.setdefault(major if it["kind"] in _PR_F32 else it["out"][0][0].dtype, []).append(it)
        self.tables: Dict[torch.dtype, Tuple[torch.Tensor, int, int]] = {}
        self.bytes_read = self.bytes_written = 0
        for dtype, items in self.items.items():
            for it in items:
                it["dst"] = [(t.data_ptr() + off * t.element_size(), t.numel() - off) for t, off in it["out"]]
                self.bytes_read += 4 * sum(it["reads"])
                self.bytes_written += sum(n * t.element_size() for (t, _), n in zip(it["out"], it["writes"]))
            host, n_wgs = plan_refresh_table(items, arena.numel)
            self.tables[dtype] = (self._upload_words(host), len(items), n_wgs)
        self.n_launches = len(self.tables)

    # -- recipes -> descriptors
    def _src(self, s) -> Tuple[int, int, int]:
        """(offset, rows, row length) of a source: a key or a row slice ``(key, lo, hi)``."""
        key, lo, hi = (s, None, None) if isinstance(s, str) else s
        if key not in self.arena.offsets:
            raise KeyError(f"{key}: a recipe reads it, the arena does not hold it")
        shape = tuple(self.arena.shapes[key])
        rows = shape[0] if shape else 1
        rowlen = (self.arena.shapes[key].numel() // rows) if rows else 0
        lo, hi = (0 if lo is None else int(lo)), (rows if hi is None else int(hi))
        if not 0 <= lo < hi <= rows:
            raise ValueError(f"{key}: rows [{lo}, {hi}) of {rows}")
        return self.arena.offsets[key] + lo * rowlen, hi - lo, rowlen

    def _expand(self, r) -> List[dict]:
        def item(kind, n, k, srcs, out, reads, writes, cs=0, flags=0):
            return dict(kind=kind, N=n, K=k, Cs=cs, flags=flags, src=srcs, out=out, reads=reads, writes=writes)
        out: List[dict] = []
        if r.kind in ("copy32", "cast"):
            off = 0
            for s in r.src:
                so, n, k = self._src(s)
                if r.kind == "copy32":
                    out.append(item("COPY32", n * k, 0, [so], [(r.dst[0], off)], [n * k], [n * k]))
                else:
                    out.append(item("CAST", n, k, [so], [(r.dst[0], off)], [n * k], [n * k], cs=k))
                off += n * k
            if off != r.dst[0].numel():
                raise ValueError(f"{r.kind} of {r.src}: {off} source elements for a destination of {r.dst[0].numel()}")
        elif r.kind == "cast_cin8":
            so, n, k = self._src(r.src[0])
            out.append(item("CAST", n * 9, 8, [so], [(r.dst[0], 0)], [n * k], [n * 72], cs=k // 9))
        elif r.kind == "geglu":
            so, n, k = self._src(r.src[0])
            bo, nb, _ = self._src(r.src[1])
            out.append(item("GEGLU_W", n, k, [so], [(r.dst[0], 0)], [n * k], [n * k]))
            out.append(item("GEGLU_B", nb, 0, [bo], [(r.dst[1], 0)], [nb], [nb]))
        elif r.kind == "lnfold":
            ws, bs, gamma, beta = r.src
            go, bo = self._src(gamma)[0], self._src(beta)[0]
            if r.geglu and len(ws) != 1:
                raise ValueError("lnfold in GEGLU order takes one weight")
            row = 0
            for i, s in enumerate(ws):
                so, n, k = self._src(s)
                b = self._src(bs[i])[0] if bs else -1
                out.append(item("LNFOLD", n, k, [so, go, bo, b], [(r.dst[0], row * k), (r.dst[1], row), (r.dst[2], row)],
                                [n * k + 2 * k + (n if bs else 0)], [n * k, n, n],
                                flags=L.PLAN_REFRESH_GEGLU if r.geglu else 0))
                row += n
            if row != r.dst[1].numel():
                raise ValueError(f"lnfold of {ws}: {row} source rows for a destination of {r.dst[1].numel()}")
        elif r.kind == "upsfold":
            so, n, k = self._src(r.src[0])
            out.append(item("UPSFOLD", n, k // 9, [so], [(r.dst[0], 0)], [n * k], [16 * n * (k // 9)]))
        elif r.kind == "head_stream":
            srcs = [self._src(s) for s in r.src]
            if any((n, k) != (320, 320) for _, n, k in srcs):
                raise ValueError(f"head_stream of {r.src}: every source must be [320][320]")
            out.append(item("HEAD_STREAM", 320, 320, [s[0] for s in srcs], [(r.dst[0], 0)], [4 * 320 * 320], [r.dst[0].numel()]))
        elif r.kind == "ffn_stream":
            (w1, n1, k1), (b1, nb, _), (w2, n2, k2), (wp, n3, k3) = [self._src(s) for s in r.src]
            if (n1, k1, nb, n2, k2, n3, k3) != (2560, 320, 2560, 320, 1280, 320, 320):
                raise ValueError(f"ffn_stream of {r.src}: the sources must be [2560][320], [2560], [320][1280], [320][320]")
            out.append(item("FFN_STREAM", 2560, 320, [w1, w2, wp], [(r.dst[0], 0)], [2560 * 320 + 320 * 1280 + 320 * 320],
                            [r.dst[0].numel()]))
            out.append(item("FFN_BIAS", 2560, 320, [b1], [(r.dst[1], 0)], [2560], [2560]))
        else:
            raise ValueError(f"recipe kind {r.kind!r}")
        return out

    # -- the launch
    def source(self, which: str) -> torch.Tensor:
        if which == "raw":
            return self.arena.p
        if which == "ema":
            if self.arena.ema is None:
                raise RuntimeError("the arena has no EMA (ema=True / ensure_ema)")
            return self.arena.ema
        raise ValueError(f"source must be 'ema' or 'raw', got {which!r}")

    def launch(self, source: str = "ema") -> None:
        """The launches on the backend's stream, nothing else: what a graph capture records."""
        self._need_backend()
        src = self.source(source)
        for dtype, (table, n_desc, n_wgs) in self.tables.items():
            self.be.plan_refresh(src, table, n_desc, n_wgs, dtype)

    def refresh(self, source: str = "ema") -> None:
        """Write every destination again from the arena's EMA (``"ema"``) or its raw masters (``"raw"``).  Ordered after
        torch's current stream and before what it does next, like ``FusedAdamW.step``; no host sync."""
        self._bracketed_launch(source)


def reference_param_groups(names: Sequence[str], lr: float, weight_decay: float = 0.0) -> List[dict]:
    """The reference's four parameter groups over state-dict key names: ``unet.`` and ``ordinal_embedder.`` at ``lr``,
    ``image_projection.`` and ``feature_purifier.`` at ``2 * lr`` (left out when no key has that prefix), all with the
    one ``weight_decay``.  ``vae.`` and ``image_encoder.`` are frozen in the reference and excluded; any other key is an
    error.  -> list of ``{"name", "params", "lr", "weight_decay"}`` in that order."""
    spec = (("unet.", 1.0, False), ("ordinal_embedder.", 1.0, False), ("image_projection.", 2.0, False),
            ("feature_purifier.", 2.0, True))
    frozen = ("vae.", "image_encoder.")
    buckets: "OrderedDict[str, List[str]]" = OrderedDict((pre, []) for pre, _, _ in spec)
    for k in names:
        if k.startswith(frozen):
            continue
        for pre in buckets:
            if k.startswith(pre):
                buckets[pre].append(k)
                break
        else:
            raise ValueError(f"{k}: no parameter group takes this key")
    return [{"name": pre[:-1], "params": buckets[pre], "lr": mult * lr, "weight_decay": weight_decay}
            for pre, mult, optional in spec if buckets[pre] or not optional]


def arena_from_groups(tensors: Mapping[str, torch.Tensor], groups: Sequence[dict], **kw) -> ParamArena:
    """``ParamArena`` over the tensors that ``groups`` (``reference_param_groups``' list) names, group k = groups[k]."""
    group_of = {k: gi for gi, g in enumerate(groups) for k in g["params"]}
    return ParamArena(OrderedDict((k, tensors[k]) for g in groups for k in g["params"]), group_of, **kw)


class FusedAdamW(_Launcher):
    """AdamW over a ``ParamArena`` on the kernels of csrc/optim.hip.

    ``groups``: one ``{"lr", "weight_decay"}`` per arena group (further keys are ignored, so the list of
    ``reference_param_groups`` passes as it is).  ``max_grad_norm`` > 0 clips by the global norm
    (``clip_grad_norm_``'s rule); ``init_scale`` > 0 switches the loss scale on: the gradients in the arena are then
    taken to be ``scale`` times the true ones, a step with a non-finite gradient is skipped and halves the scale, and
    ``growth_interval`` clean steps double it (torch.amp.GradScaler).  The caller multiplies its loss by ``scale()``'s
    tensor (a device scalar, no sync).  ``ema_decay`` allocates the arena's EMA; ``working_dtype`` its 16-bit copy
    (default: what the arena already has).  ``be=None`` gives an optimizer that holds state but cannot step (CPU).
    """
    _HOLDS = "it holds state but cannot step"

    def __init__(self, be, arena: ParamArena, groups: Sequence[Mapping], *, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: float = 0.0, ema_decay: Optional[float] = None,
                 working_dtype: Optional[torch.dtype] = None, init_scale: float = 0.0, growth_interval: int = 2000,
                 growth_factor: float = 2.0, backoff_factor: float = 0.5, max_blocks: int = 0):
        if len(groups) != arena.n_groups:
            raise ValueError(f"{len(groups)} groups for an arena of {arena.n_groups}")
        if be is not None and arena.device != be.device:
            raise ValueError(f"the arena lives on {arena.device}, the backend on {be.device}")
        self.be, self.arena = be, arena
        self.max_blocks = int(max_blocks)
        self.ema_decay = ema_decay
        if ema_decay is not None:
            arena.ensure_ema()
        if working_dtype is not None:
            arena.ensure_p16(working_dtype)
        self.betas = [tuple(float(b) for b in g.get("betas", betas)) for g in groups]
        host = L.OptimState()
        host.n_groups, host.growth_interval = arena.n_groups, int(growth_interval)
        host.scale, host.max_norm = float(init_scale), float(max_grad_norm)
        host.growth_factor, host.backoff_factor = float(growth_factor), float(backoff_factor)
        for k, g in enumerate(groups):
            b1, b2 = self.betas[k]
            hg = host.group[k]
            host.lr[k] = float(g["lr"])
            hg.beta1, hg.beta2, hg.eps, hg.weight_decay = b1, b2, float(g.get("eps", eps)), float(g["weight_decay"])
            hg.one_minus_beta1, hg.one_minus_beta2 = 1.0 - b1, 1.0 - b2
        self.state = self._upload_words(host)
        self.partials = torch.empty(arena.n_chunks, dtype=torch.float32, device=arena.device)
        self.flags = torch.empty(arena.n_chunks, dtype=torch.int32, device=arena.device)
        self._group_chunks = (C.c_int * arena.n_groups)(*arena.group_chunks)
        self._lr_words = self.state[L.OptimState.lr.offset // 4:L.OptimState.lr.offset // 4 + arena.n_groups].view(torch.float32)
        self._scale_word = self.state[L.OptimState.scale.offset // 4:L.OptimState.scale.offset // 4 + 1].view(torch.float32)

    # -- the state block
    def _upload(self, host: "L.OptimState") -> None:
        self._upload_words(host, self.state)

    def _download(self) -> "L.OptimState":
        if self.be is not None:
            self.be.synchronize()
        return L.OptimState.from_buffer_copy(self.state.cpu().numpy().tobytes())

    def set_lrs(self, lrs: Sequence[float]) -> None:
        """The learning rates of the next step, one per group (``lr_scheduler.warmup_cosine_lr``'s list): one small copy
        into the state block, ordered on the backend's stream."""
        if len(lrs) != self.arena.n_groups:
            raise ValueError(f"{len(lrs)} learning rates for {self.arena.n_groups} groups")
        src = torch.tensor([float(x) for x in lrs], dtype=torch.float32)
        if self.be is not None:
            self.be.copy_(self._lr_words, src)
        else:
            self._lr_words.copy_(src)

    def scale(self) -> torch.Tensor:
        """The loss scale as a one-element device tensor (a view of the state block; 0 = no loss scaling)."""
        return self._scale_word

    def stats(self) -> dict:
        """``step, grad_norm, coef, found_inf, scale, growth_tracker`` of the last step.  Synchronises: for logging and
        tests."""
        h = self._download()
        return {"step": h.step, "grad_norm": h.grad_norm, "coef": h.coef, "found_inf": bool(h.found_inf), "scale": h.scale,
                "growth_tracker": h.growth_tracker}

    # -- the step
    def _flags(self, update_ema: bool, zero_grad: bool) -> int:
        a = self.arena
        if update_ema and (a.ema is None or self.ema_decay is None):
            raise RuntimeError("update_ema needs ema_decay")
        return (L.OPTIM_EMA if update_ema else 0) | (_P16_FLAG[a.p16.dtype] if a.p16 is not None else 0) | \
            (L.OPTIM_ZERO_GRAD if zero_grad else 0)

    def launch(self, update_ema: bool = False, zero_grad: bool = True) -> None:
        """The three launches on the backend's stream, nothing else: what a graph capture records."""
        self._need_backend()
        a, be = self.arena, self.be
        flags = self._flags(update_ema, zero_grad)
        be.optim_grad_stats(a.g, self.partials, self.flags, max_blocks=self.max_blocks)
        be.optim_finalize(self.partials, self.flags, self.state)
        be.optim_adamw_step(a.p, a.g, a.m, a.v, self.state, self._group_chunks, ema=a.ema if update_ema else None,
                            p16=a.p16, ema_weight=(1.0 - self.ema_decay) if update_ema else 0.0, flags=flags,
                            max_blocks=self.max_blocks)

    def step(self, update_ema: bool = False, zero_grad: bool = True) -> None:
        """One optimizer step on the gradients in the arena: clip, unscale, AdamW, and in the same pass the 16-bit copy,
        with ``update_ema`` the EMA and with ``zero_grad`` the zeroed gradient.  Ordered after torch's current stream
        (the backward that produced the gradients) and before what torch's current stream does next; no host sync."""
        self._bracketed_launch(update_ema, zero_grad)

    # -- checkpoints: torch.optim.AdamW's layout
    def state_dict(self) -> dict:
        """``{"state": {i: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups": [...], "scaler": {...}}`` with the
        parameters numbered in arena order: what ``torch.optim.AdamW.state_dict()`` gives for the same parameters in
        the same groups (a Lightning checkpoint's ``optimizer_states[0]``), plus the loss scale under ``"scaler"``.
        ``exp_avg`` / ``exp_avg_sq`` are views of the arena, not copies.  Synchronises."""
        h, a = self._download(), self.arena
        state, groups, i = {}, [], 0
        for gi in range(a.n_groups):
            idx = []
            for k in a.group_names[gi]:
                if h.step > 0:
                    state[i] = {"step": torch.tensor(float(h.step)), "exp_avg": a.exp_avg(k), "exp_avg_sq": a.exp_avg_sq(k)}
                idx.append(i)
                i += 1
            hg = h.group[gi]
            groups.append({"lr": float(h.lr[gi]), "betas": self.betas[gi], "eps": float(hg.eps),
                           "weight_decay": float(hg.weight_decay), "amsgrad": False, "maximize": False, "foreach": None,
                           "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": True,
                           "params": idx})
        return {"state": state, "param_groups": groups,
                "scaler": {"scale": float(h.scale), "growth_tracker": int(h.growth_tracker)}}

    def load_state_dict(self, sd: Mapping) -> None:
        """Take moments, step count, learning rates, betas, eps and weight decay from a ``torch.optim.AdamW`` state dict
        over the same parameters in the same groups (or one of ``state_dict()``); ``"scaler"`` is optional.  The kernels
        keep one step count for all parameters, so the dict's must agree (parameters without state count as step 0 only
        when every parameter is without)."""
        a = self.arena
        pg = sd["param_groups"]
        if len(pg) != a.n_groups or any(len(g["params"]) != len(a.group_names[gi]) for gi, g in enumerate(pg)):
            raise ValueError("param_groups do not match the arena's groups")
        state = sd["state"]
        steps = set()
        names = [k for gi in range(a.n_groups) for k in a.group_names[gi]]
        order = [i for g in pg for i in g["params"]]
        with torch.no_grad():
            for k, i in zip(names, order):
                st = state.get(i)
                if st is None:
                    steps.add(0)
                    a.exp_avg(k).zero_()
                    a.exp_avg_sq(k).zero_()
                    continue
                steps.add(int(float(st["step"])))
                if st["exp_avg"].shape != a.shapes[k]:
                    raise ValueError(f"{k}: exp_avg has shape {tuple(st['exp_avg'].shape)}, the arena {tuple(a.shapes[k])}")
                a.exp_avg(k).copy_(st["exp_avg"])
                a.exp_avg_sq(k).copy_(st["exp_avg_sq"])
        if len(steps) != 1:
            raise ValueError(f"the parameters carry different step counts {sorted(steps)}; the fused step keeps one")
        h = self._download()
        h.step = steps.pop()
        for gi, g in enumerate(pg):
            b1, b2 = (float(b) for b in g["betas"])
            self.betas[gi] = (b1, b2)
            hg = h.group[gi]
            h.lr[gi] = float(g["lr"])
            hg.beta1, hg.beta2, hg.eps, hg.weight_decay = b1, b2, float(g["eps"]), float(g["weight_decay"])
            hg.one_minus_beta1, hg.one_minus_beta2 = 1.0 - b1, 1.0 - b2
        if "scaler" in sd:
            h.scale, h.growth_tracker = float(sd["scaler"]["scale"]), int(sd["scaler"]["growth_tracker"])
        self._upload(h)

    def ema_state(self) -> "OrderedDict[str, torch.Tensor]":
        """name -> view of the EMA: the ``state_dict`` a checkpoint stores and ``checkpoint.load_state`` reads with
        ``which="ema"``."""
        return OrderedDict((k, self.arena.ema_param(k)) for k in self.arena.names)
