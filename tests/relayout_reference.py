"""Index-level numpy model of csrc/relayout.hip (include/dadd_hip_relayout.h): the mapping from a workgroup index to a
descriptor and a tile, and what each kind writes for that tile.  Written from the header's text, independently of the
library's own planning function: ``tiles`` / ``dst_numel`` restate the counts, ``run`` executes a table workgroup by
workgroup.  The torch helpers of ``grad_ops`` are the reference of the VALUES; this model pins the decomposition (that
the tiles of a tensor cover its destination exactly once and nothing else) and the fp32 summation order of the UPS kind."""
import numpy as np

TILE = 64
T, S2, UPS, COUT4 = 0, 1, 2, 3
KIND = {"T": T, "S2": S2, "UPS": UPS, "COUT4": COUT4}
S2_TAPS = (4, 3, 5, 1, 7, 0, 2, 6, 8)          # 3 * ky + kx of grad_ops.STRIDE2_SLABS
UPS_SETS = ((2,), (1, 2), (0, 1), (0,))        # grad_ops.UPS_TAP_SETS


def slabs(kind, taps):
    return taps if kind == T else 16 if kind == UPS else 9


def tiles(kind, taps, n, c):
    if kind == COUT4:
        return -(-c * 9 // 256)
    return slabs(kind, taps) * (-(-n // TILE)) * (-(-c // TILE))


def dst_numel(kind, taps, n, c):
    return c * 72 if kind == COUT4 else c * slabs(kind, taps) * n


def plan(items):
    """items: (src_off, dst_off, N, C, kind name, taps) -> (list of dicts with tile0, total tiles)."""
    out, t0 = [], 0
    for src_off, dst_off, n, c, kind, taps in items:
        out.append(dict(src_off=src_off, dst_off=dst_off, N=n, C=c, kind=KIND[kind], taps=taps, tile0=t0))
        t0 += tiles(KIND[kind], taps, n, c)
    return out, t0


def _round16(a32, dtype):
    """fp32 -> the 16-bit type, round to nearest even (numpy has fp16; bf16 travels as uint16 bit patterns)."""
    if dtype == np.float16:
        return a32.astype(np.float16)
    u = a32.astype(np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _to32(a, dtype):
    if dtype == np.float16:
        return a.astype(np.float32)
    return (a.astype(np.uint32) << 16).view(np.float32)


def run(src, dst, table, n_tiles, dtype=np.float16, writes=None):
    """Execute every workgroup of the launch on the flat arrays (fp16 arrays, or uint16 bit patterns with
    ``dtype='bf16'``).  ``writes``: optional int array like dst that counts the stores per element."""
    tile0 = [d["tile0"] for d in table]
    for wg in range(n_tiles):
        lo, hi = 0, len(table) - 1                      # the kernel's search: last descriptor with tile0 <= wg
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if tile0[mid] <= wg:
                lo = mid
            else:
                hi = mid - 1
        d = table[lo]
        n, c, kind, taps = d["N"], d["C"], d["kind"], d["taps"]
        local = wg - d["tile0"]
        assert 0 <= local < tiles(kind, taps, n, c)
        if kind == COUT4:
            s = src[d["src_off"]:d["src_off"] + n * 9 * c].reshape(n, 9, c)
            o = dst[d["dst_off"]:d["dst_off"] + c * 72].reshape(c * 9, 8)
            for idx in range(local * 256, min(local * 256 + 256, c * 9)):
                ch, slab = divmod(idx, 9)
                o[idx, :] = 0
                o[idx, :n] = s[:, 8 - slab, ch]
                if writes is not None:
                    writes[d["dst_off"] + idx * 8:d["dst_off"] + idx * 8 + 8] += 1
            continue
        st = taps if kind == T else 9
        ns = slabs(kind, taps)
        tn, tc = -(-n // TILE), -(-c // TILE)
        slab, rem = divmod(local, tn * tc)
        n0, c0 = (rem // tc) * TILE, (rem % tc) * TILE
        n1, c1 = min(n0 + TILE, n), min(c0 + TILE, c)
        s = src[d["src_off"]:d["src_off"] + n * st * c].reshape(n, st, c)
        o = dst[d["dst_off"]:d["dst_off"] + c * ns * n].reshape(c, ns, n)
        if kind == UPS:
            kys, kxs = UPS_SETS[slab >> 2], UPS_SETS[slab & 3]
            acc = None
            for kx in kxs:                               # (sum over ky) per kx, then over kx; every sum starts at 0
                col = np.zeros((n1 - n0, c1 - c0), np.float32)
                for ky in kys:
                    col = col + _to32(s[n0:n1, 3 * ky + kx, c0:c1], dtype)
                acc = (np.zeros_like(col) + col) if acc is None else acc + col
            val = _round16(acc, dtype)
        else:
            tap = S2_TAPS[slab] if kind == S2 else taps - 1 - slab
            val = s[n0:n1, tap, c0:c1]
        o[c0:c1, slab, n0:n1] = val.T
        if writes is not None:
            w = writes[d["dst_off"]:d["dst_off"] + c * ns * n].reshape(c, ns, n)
            w[c0:c1, slab, n0:n1] += 1
