#!/usr/bin/env python
"""How far from zero a group or a row may sit before each norm route leaves its tolerance, measured on the GPU.

Runs every route of tests/norm_cases.py (the cases of tests/test_gpu_norm_conditioning.py, same small shapes, no second
copy) at r = |mu| / sigma in {0, 8, 32, 128, 512} and in the constant case, once, and prints per route and type the worst
error as a share of the route's tolerance (above 1 would fail the test; the tests assert r <= 32, and r <= 128 on the
two-pass routes in fp16).  It asserts nothing and measures no speed.  A route that raises (a refused contract, a HIP error)
ends the run there: what was measured so far is in the file.

    python scripts/norm_envelope.py [--route SUBSTRING ...] [--out profiles/r13_a_norm_envelope.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--route", action="append", default=[], help="run the routes whose name contains this (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_a_norm_envelope.txt"))
    args = ap.parse_args(argv)
    from progressive_stable_diffusion_amd.backend import HipBackend
    from tests import norm_cases as NC
    hip = HipBackend(torch.device("cuda:0"))
    cols = [*NC.R_ENVELOPE, "const"]
    head = ("Norm routes on MI355X: worst error as a share of the route's tolerance (scripts/norm_envelope.py; cases, references\n"
            "and bounds: tests/norm_cases.py).  Columns: r = |mu| / sigma of every group / row (sigma 2 for GroupNorm, 1 for\n"
            "LayerNorm), then the constant case (a slab / rows exactly 64.0, r = 8 elsewhere; '-' where the route has none).\n"
            "Per cell: the worst share over the route's 16-bit / fp32 outputs, then after '|' over the statistics tensors its\n"
            "epilogue writes, or over the fp32 dgamma / dbeta of a backward route.\n"
            "'*' marks a cell the tests assert; 'NaN' a non-finite output.\n")
    lines = [head, f"{'route':<34}{'type':<6}" + "".join(f"{'r=' + str(c) if c != 'const' else c:>16}" for c in cols)]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    print("\n".join(lines), flush=True)
    for name, rt in NC.ROUTES.items():
        if args.route and not any(s in name for s in args.route):
            continue
        for dt in rt.dtypes:
            cells = []
            for c in cols:
                if c == "const" and not rt.constant:
                    cells.append("-")
                    continue
                try:
                    recs = NC.run(hip, name, dt, c)
                except (ValueError, AssertionError) as e:      # refused on the host: nothing was launched
                    print(f"{name} {NC.name_of(dt)} {c}: refused: {e}", file=sys.stderr, flush=True)
                    cells.append("refused")
                    continue
                side = ("gn_ws", "ln_stats_out", "dgamma", "dbeta")
                stats, outs = [r for r in recs if r.what in side], [r for r in recs if r.what not in side]
                cell = "NaN" if not all(NC.finite(r) for r in recs) else f"{NC.worst(outs):.2f}"
                if stats:
                    cell += f"|{NC.worst(stats):.2f}"
                asserted = c == "const" or c in NC.rs_of(name, dt)
                cells.append(cell + ("*" if asserted else ""))
            line = f"{name:<34}{NC.name_of(dt):<6}" + "".join(f"{c:>16}" for c in cells)
            print(line, flush=True)
            lines.append(line)
            with open(args.out, "w") as f:      # (rewritten after every line: a run that is cut short leaves what it had)
                f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
