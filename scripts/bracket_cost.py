"""Host cost of the stream bracket alone: ``with on_backend(hip): pass`` on the ``HipBackend``, microseconds per entry
on the host clock, median (min .. max) over the rounds.  A training step enters the bracket a few thousand times, so
this is the number to compare between two trees when the bracket or the two calls under it change.

    python scripts/bracket_cost.py [--entries 20000] [--rounds 9]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from progressive_stable_diffusion_amd.backend import HipBackend  # noqa: E402
from progressive_stable_diffusion_amd.grad_ops import on_backend  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    be = HipBackend(torch.device("cuda:0"))

    def loop():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.entries):
            with on_backend(be):
                pass
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return (t1 - t0) / args.entries * 1e6

    loop()
    vals = [loop() for _ in range(args.rounds)]
    print(f"on_backend(HipBackend) enter + exit, empty body: {statistics.median(vals):.3f} us per entry "
          f"({min(vals):.3f} .. {max(vals):.3f}), host clock, {args.entries} entries x {args.rounds} rounds", flush=True)


if __name__ == "__main__":
    main()
