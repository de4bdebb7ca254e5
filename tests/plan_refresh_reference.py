"""CPU executor of the descriptor items of ``optim.PlanRefresh`` with the index arithmetic and the rounding sequence of
csrc/plan_refresh.hip, and the cases the CPU and GPU tests of the kernel share (sources, recipes, what the packers of
``engine`` give for them).

The executor works on the python-level items (``PlanRefresh.items``: kind, sizes, source offsets, destination tensors
with element offsets) - the same numbers the ctypes table carries.  Rounding: fp64 -> fp32 -> 16 bits, each to nearest
even; LNFOLD's row sums in the kernel's order (lane l of 64 adds k = 8 l + 512 j + e ascending, then a butterfly over
lane distances 32 .. 1).
"""
from collections import OrderedDict

import torch

from progressive_stable_diffusion_amd import engine as E
from progressive_stable_diffusion_amd import optim as O

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64


# ----------------------------------------------------------------------------------------------- index arithmetic
def geglu_row(r, n2):
    tile, wn, q = r >> 7, (r >> 6) & 1, r & 63
    col = tile * 64 + wn * 32 + (q & 31)
    return torch.where(q < 32, col, n2 + col)


def ffn_row(ch, rr):
    q, e = rr >> 4, rr & 15
    return (q & 1) * 1280 + ch * 64 + (q >> 2) * 32 + ((q >> 1) & 1) * 16 + e


def _image(g):
    """(row, source chunk) of group ``g`` inside a run of [R][64] LDS images (8 groups per row)."""
    r = g >> 3
    return r, (g & 7) ^ ((r >> 1) & 7)


def head_group_src(g, off):
    piece, w = g // 1280, g % 1280
    r, chunk = _image(w)
    q = torch.where(piece < 10, piece, piece - 10)
    row = (q // 5) * 160 + r
    which = torch.where(piece < 10, torch.zeros_like(row), 1 + row // 320)
    row = torch.where(piece < 10, row, row % 320)
    base = torch.tensor(off, dtype=torch.int64)[which]
    return base + row * 320 + (q % 5) * 64 + chunk * 8


def ffn_group_src(g, off):
    per = 7680
    ch, w = g // per, g % per
    # ff.net.0.proj: five [128][64] pieces
    r1, c1 = _image(w & 1023)
    a = off[0] + ffn_row(ch, r1) * 320 + (w >> 10) * 64 + c1 * 8
    # ff.net.2: two [160][64] pieces
    w2 = w - 5 * 1024
    r2, c2 = _image(w2 % 1280)
    b = off[1] + ((w2 // 1280) * 160 + r2) * 1280 + ch * 64 + c2 * 8
    # proj_out: ten [160][64] pieces behind the 20 chunks
    q = g - 20 * per
    r3, c3 = _image(q % 1280)
    piece = q // 1280
    c = off[2] + ((piece // 5) * 160 + r3) * 320 + (piece % 5) * 64 + c3 * 8
    return torch.where(g < 20 * per, torch.where(w < 5 * 1024, a, b), c)


def _wave_sum(part):
    """[N][64] lane partials -> lane 0 of the butterfly (distances 32, 16, .., 1)."""
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lane ^ o]
    return part[:, 0]


def _lane_sums(x):
    """[N][K] fp64 terms -> [N][64]: lane l adds its k = 8 l + 512 j + e in ascending order."""
    n, k = x.shape
    kp = -(-k // 512) * 512
    x = torch.cat([x, torch.zeros(n, kp - k, dtype=F64)], 1).view(n, kp // 512, 64, 8)
    acc = torch.zeros(n, 64, dtype=F64)
    for j in range(kp // 512):
        for e in range(8):
            acc = acc + x[:, j, :, e]
    return acc


# ----------------------------------------------------------------------------------------------- the executor
def run_item(it, src):
    """One descriptor item on the CPU: reads the flat fp32 ``src``, writes ``it["out"]`` (CPU tensors) in place."""
    kind, n, k = it["kind"], it["N"], it["K"]
    so = list(it["src"])
    outs = [(t.view(-1), off) for t, off in it["out"]]
    d0, o0 = outs[0]
    dt = d0.dtype

    def put(which, vals):
        d, o = outs[which]
        d[o:o + vals.numel()] = vals.reshape(-1).to(d.dtype)

    if kind == "COPY32":
        put(0, src[so[0]:so[0] + n])
    elif kind == "GEGLU_B":
        put(0, src[so[0] + geglu_row(torch.arange(n), n // 2)])
    elif kind == "FFN_BIAS":
        e = torch.arange(2560)
        put(0, src[so[0] + ffn_row(e >> 7, e & 127)])
    elif kind == "CAST":
        cs = it["Cs"]
        if cs == k:
            put(0, src[so[0]:so[0] + n * k].to(dt))
        else:
            rows = torch.zeros(n, 8, dtype=dt)
            rows[:, :cs] = src[so[0]:so[0] + n * cs].view(n, cs).to(dt)
            put(0, rows)
    elif kind == "GEGLU_W":
        g = torch.arange(n * k // 8)
        base = so[0] + geglu_row(g // (k // 8), n // 2) * k + (g % (k // 8)) * 8
        put(0, src[base[:, None] + torch.arange(8)].to(dt))
    elif kind == "HEAD_STREAM":
        base = head_group_src(torch.arange(51200), so)
        put(0, src[base[:, None] + torch.arange(8)].to(dt))
    elif kind == "FFN_STREAM":
        base = ffn_group_src(torch.arange(166400), so)
        put(0, src[base[:, None] + torch.arange(8)].to(dt))
    elif kind == "UPSFOLD":
        w = src[so[0]:so[0] + n * 9 * k].view(n, 3, 3, k).to(dt).to(F64)            # every tap rounded to 16 bits first
        sets = (((0,), (1, 2)), ((0, 1), (2,)))
        out = torch.zeros(4, n, 4, k, dtype=F64)
        for ph in range(4):
            for t in range(4):
                for ky in sets[ph >> 1][t >> 1]:
                    for kx in sets[ph & 1][t & 1]:
                        out[ph, :, t] = out[ph, :, t] + w[:, ky, kx]
        put(0, out.to(F32).to(dt))                                                   # fp64 -> fp32 -> 16 bits
    elif kind == "LNFOLD":
        r = torch.arange(n)
        s = geglu_row(r, n // 2) if it["flags"] & 1 else r
        w = src[so[0]:so[0] + n * k].view(n, k)[s]
        gamma, beta = src[so[1]:so[1] + k], src[so[2]:so[2] + k]
        w16 = (w * gamma[None]).to(dt)                                               # the fp32 product = round32 of the exact one
        c1 = _wave_sum(_lane_sums(w16.to(F64)))
        bias = _wave_sum(_lane_sums(w.to(F64) * beta.to(F64)[None]))
        if so[3] >= 0:
            bias = bias + src[so[3]:so[3] + n][s].to(F64)
        put(0, w16)
        put(1, c1.to(F32))
        put(2, bias.to(F32))
    else:
        raise ValueError(kind)


def execute(pr, src):
    """Every item of a ``PlanRefresh`` whose destinations are CPU tensors."""
    src = src.detach().cpu()
    for items in pr.items.values():
        for it in items:
            run_item(it, src)


# ----------------------------------------------------------------------------------------------- the shared cases
def _oihw(w, taps):
    """library layout [N][taps * C] -> OIHW, what the packers of ``engine`` take."""
    n = w.shape[0]
    if taps == 1:
        return w
    return w.view(n, 3, 3, -1).permute(0, 3, 1, 2).contiguous()


def sum_bound(ref, terms_abs, k):
    """|got - ref| allowed for c1 / bias: one fp32 spacing for a rounding that lands on the other side plus the error of
    two fp64 summations of k + 1 terms in different orders."""
    return 2.0 ** -23 * ref.double().abs() + (k + 2) * 2.0 ** -52 * terms_abs


def lnfold_bounds(r, arena, ref):
    """The c1 / bias bounds (``sum_bound``) of one ``lnfold`` recipe ``r``, from the masters in ``arena`` and the reference
    tensors ``ref`` = (w16, c1, bias) a packer gave for them."""
    def view(s):
        return arena.param(s) if isinstance(s, str) else arena.param(s[0])[s[1]:s[2]]
    ws, bs, _, beta = r.src
    w = torch.cat([view(s) for s in ws]).double()
    n, k = w.shape
    terms_b = (w * view(beta).double()[None]).abs().sum(1)
    if bs:
        terms_b = terms_b + torch.cat([view(s) for s in bs]).double().abs()
    if r.geglu:
        terms_b = terms_b[geglu_row(torch.arange(n), n // 2).to(w.device)]
    return sum_bound(ref[1], ref[0].double().abs().sum(1), k), sum_bound(ref[2], terms_b, k)


def restore_check(recipes, arena, run):
    """Keep a copy of every destination of ``recipes``, overwrite it with NaN, ``run()`` the refresh, and compare: bit-equal
    but for c1 / bias of an ``lnfold``, which must be inside ``lnfold_bounds``.  -> (destinations compared, worst share
    of a bound)."""
    seen, want = set(), []
    for r in recipes:
        if r.dst[0].data_ptr() in seen:
            continue
        seen.add(r.dst[0].data_ptr())
        want.append((r, [d.clone() for d in r.dst]))
        for d in r.dst:
            d.fill_(float("nan"))
    run()
    worst, n = 0.0, 0
    for r, refs in want:
        bounds = lnfold_bounds(r, arena, refs) if r.kind == "lnfold" else None
        for i, (d, ref) in enumerate(zip(r.dst, refs)):
            n += 1
            if bounds is not None and i > 0:
                share = ((d.double() - ref.double()).abs() / bounds[i - 1]).max().item()
                assert share <= 1.0, (r.kind, r.src, i, share)
                worst = max(worst, share)
            else:
                assert torch.equal(d, ref), (r.kind, r.src, i, tuple(d.shape))
    return n, worst


class Cases:
    """Sources (library layout, scaled like real weights), the recipes over them and, per destination name, what the
    packer of ``engine`` gives on the CPU.  ``alloc(name, shape, dtype)`` supplies the destination tensors (CPU tensors
    here, guarded device views in the GPU test)."""

    def __init__(self, dtype, alloc=None, streams=None, seed=0, device=None):
        g = torch.Generator().manual_seed(seed)
        self.dtype = dtype
        alloc = alloc or (lambda name, shape, dt: torch.full(shape, float("nan"), dtype=dt))
        streams = (dtype == F16) if streams is None else streams
        rnd = lambda *shape, s=0.05: torch.randn(*shape, generator=g) * s             # noqa: E731
        T: "OrderedDict[str, torch.Tensor]" = OrderedDict()
        self.recipes, self.expect, self.dst, self.bounds = [], {}, {}, {}

        def add(kind, src, names, shapes, dtypes, want, geglu=False):
            dst = tuple(alloc(nm, sh, dt) for nm, sh, dt in zip(names, shapes, dtypes))
            self.recipes.append(E.Recipe(kind, src, dst, geglu=geglu))
            for nm, d, w in zip(names, dst, want):
                self.dst[nm], self.expect[nm] = d, w.contiguous()

        # CAST
        for n, taps, c in ((8, 1, 8), (16, 9, 72), (136, 1, 200)):
            key = f"cast.{n}.{taps}.{c}"
            T[key] = rnd(n, taps * c)
            add("cast", (key,), [key], [(n, taps * c)], [dtype], [E.pack_conv(_oihw(T[key], taps), dtype)])
        cat = [f"cat.{i}" for i in range(3)]
        for key, n in zip(cat, (8, 24, 16)):
            T[key] = rnd(n, 72)
        add("cast", cat, ["cat"], [(48, 72)], [dtype], [torch.cat([T[k] for k in cat]).to(dtype)])
        T["conv_in"] = rnd(8, 9 * 4)
        add("cast_cin8", ("conv_in",), ["conv_in"], [(8, 9, 8)], [dtype], [E.pack_conv_cin8(_oihw(T["conv_in"], 9), dtype)])
        for n in (1, 2, 3, 4):
            key = f"conv_out.{n}"
            T[key] = rnd(n, 9 * 16)
            add("cast", (key,), [key], [(n, 9, 16)], [dtype], [E.pack_conv_cout4(_oihw(T[key], 9), dtype)])
        # COPY32: lengths 1, 8, 200 into one destination: offsets 0, 1, 9
        c32 = [f"copy.{n}" for n in (1, 8, 200)]
        for key, n in zip(c32, (1, 8, 200)):
            T[key] = rnd(n)
        add("copy32", c32, ["copy"], [(209,)], [F32], [torch.cat([T[k] for k in c32])])
        # GEGLU
        for rows, c in ((256, 8), (384, 72)):
            kw, kb = f"geglu.{rows}.w", f"geglu.{rows}.b"
            T[kw], T[kb] = rnd(rows, c), rnd(rows)
            wf, bf = E.geglu_interleave(T[kw], T[kb])
            add("geglu", (kw, kb), [kw, kb], [(rows, c), (rows,)], [dtype, F32], [wf.to(dtype), bf.float()])
        # LNFOLD: gamma ~ 1 +- 0.2, beta ~ +-0.2 with a non-zero mean
        for name, ns, k, has_b, geglu in (("ln.8", (8,), 8, False, False), ("ln.24", (24,), 72, True, False),
                                          ("ln.136", (136,), 200, True, False), ("ln.geglu", (256,), 72, True, True),
                                          ("ln.cat", (16, 40), 72, True, False),
                                          # more than one group per lane (K > 512): the second and third round of a wave
                                          ("ln.640", (24,), 640, True, False), ("ln.1288", (8,), 1288, True, False)):
            ws, bs = [f"{name}.w{i}" for i in range(len(ns))], [f"{name}.b{i}" for i in range(len(ns))]
            for kw, kb, n in zip(ws, bs, ns):
                T[kw] = rnd(n, k)
                if has_b:
                    T[kb] = rnd(n)
            T[name + ".gamma"] = 1.0 + rnd(k, s=0.2)
            T[name + ".beta"] = 0.05 + rnd(k, s=0.2)
            w = torch.cat([T[x] for x in ws])
            b = torch.cat([T[x] for x in bs]) if has_b else None
            w16, c1, bias = E.fold_layernorm(w, b, T[name + ".gamma"], T[name + ".beta"], dtype)
            terms_c1 = w16.double().abs().sum(1)
            terms_b = (w.double() * T[name + ".beta"].double()[None]).abs().sum(1) + (b.double().abs() if has_b else 0.0)
            if geglu:
                idx = E.geglu_interleave(torch.arange(w16.shape[0])[:, None].float(), torch.zeros(w16.shape[0]))[0][:, 0].long()
                w16, c1, bias, terms_c1, terms_b = w16[idx], c1[idx], bias[idx], terms_c1[idx], terms_b[idx]
            n = sum(ns)
            add("lnfold", (ws, bs if has_b else None, name + ".gamma", name + ".beta"),
                [name + ".w16", name + ".c1", name + ".bias"], [(n, k), (n,), (n,)], [dtype, F32, F32], [w16, c1, bias],
                geglu=geglu)
            self.bounds[name + ".c1"] = sum_bound(c1, terms_c1, k)
            self.bounds[name + ".bias"] = sum_bound(bias, terms_b, k)
        # ... and rows built to sit on the double rounding (tests/test_plan_refresh_cpu.py): (1 + h + 2^-23)(1 - 2^-24) lies
        # above the 16-bit tie 1 + h and below the fp32 midpoint; the taps 1, h, 2^-24 sum to an fp32 tie above it
        h = 2.0 ** -11 if dtype == F16 else 2.0 ** -8
        T["pin.w"] = torch.zeros(8, 72)
        T["pin.w"][:, ::3] = 1.0 + h + 2.0 ** -23
        T["pin.gamma"], T["pin.beta"] = torch.full((72,), 1.0 - 2.0 ** -24), 0.05 + rnd(72, s=0.2)
        w16, c1, bias = E.fold_layernorm(T["pin.w"], None, T["pin.gamma"], T["pin.beta"], dtype)
        add("lnfold", (["pin.w"], None, "pin.gamma", "pin.beta"), ["pin.w16", "pin.c1", "pin.bias"], [(8, 72), (8,), (8,)],
            [dtype, F32, F32], [w16, c1, bias])
        self.bounds["pin.c1"] = sum_bound(c1, w16.double().abs().sum(1), 72)
        self.bounds["pin.bias"] = sum_bound(bias, (T["pin.w"].double() * T["pin.beta"].double()[None]).abs().sum(1), 72)
        T["pin.ups"] = torch.zeros(8, 9 * 8)
        taps = T["pin.ups"].view(8, 3, 3, 8)
        taps[:, 1, 1], taps[:, 1, 2], taps[:, 2, 1], taps[:, 0, 0], taps[:, 0, 1] = 1.0, h, 2.0 ** -24, 1.0 + 2 * h, h
        add("upsfold", ("pin.ups",), ["pin.ups"], [(4, 8, 32)], [dtype], [E.fold_ups_weight(E.pack_conv(_oihw(T["pin.ups"], 9), dtype))])
        # UPSFOLD
        for n, cin in ((8, 8), (16, 72)):
            key = f"ups.{n}.{cin}"
            T[key] = rnd(n, 9 * cin)
            add("upsfold", (key,), [key], [(4, n, 4 * cin)], [dtype], [E.fold_ups_weight(E.pack_conv(_oihw(T[key], 9), dtype))])
        # the row-block streams (C = 320, fp16 only)
        if streams:
            for key, shape in (("s.proj_in", (320, 320)), ("s.q", (320, 320)), ("s.k", (320, 320)), ("s.v", (320, 320)),
                               ("s.ff0.w", (2560, 320)), ("s.ff0.b", (2560,)), ("s.ff2", (320, 1280)), ("s.proj_out", (320, 320))):
                T[key] = rnd(*shape)
            add("head_stream", ("s.proj_in", "s.q", "s.k", "s.v"), ["head"], [(409600,)], [F16],
                [E.pack_head_stream(T["s.proj_in"], T["s.q"], T["s.k"], T["s.v"])])
            st, b1p = E.pack_ffn_stream(T["s.ff0.w"], T["s.ff0.b"], T["s.ff2"], T["s.proj_out"])
            add("ffn_stream", ("s.ff0.w", "s.ff0.b", "s.ff2", "s.proj_out"), ["ffn", "ffn.b"], [(1331200,), (2560,)],
                [F16, F32], [st, b1p])
        self.tensors = T
        self.arena = O.ParamArena(T, {k: 0 for k in T}, device=device)

    def compare(self, got=None):
        """-> (names that are not bit-equal, worst share of the c1 / bias bound, its name).  ``got``: name -> CPU tensor
        (default: the destinations themselves)."""
        bad, worst, worst_name = [], 0.0, None
        for name, want in self.expect.items():
            have = (got[name] if got is not None else self.dst[name]).detach().cpu().reshape(want.shape)
            if name in self.bounds:
                share = ((have.double() - want.double()).abs() / self.bounds[name]).max().item()
                if not share <= worst:      # (also catches NaN)
                    worst, worst_name = share, name
            elif not torch.equal(have.view(torch.int16) if have.dtype != F32 else have.view(torch.int32),
                                 want.view(torch.int16) if want.dtype != F32 else want.view(torch.int32)):
                bad.append(name)
        return bad, worst, worst_name
