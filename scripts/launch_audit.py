#!/usr/bin/env python
"""Per-launch audit of the benchmarked plans on the GPU (tests/launch_audit.py), written as a report.

For every plan one table: a line per (op, compared tensor, signature) with the number of launches, the worst elementwise
ratio (error over the op's bound; above 1 fails), the worst RMS ratio rms(o - r) / rms(r32 - r) (above 1.5 fails) and the
seconds the audit of those launches took; then the signatures whose RMS ratio is above 1.1.  The same runs are the tests of
tests/test_gpu_launch_audit.py; this writes what they print.  It measures no speed.

    python scripts/launch_audit.py [--plan SUBSTRING ...] [--out profiles/r05_a_launch_audit.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

GATES = {"anatomy": (0.1, 0.9), "disease": (0.9, 0.1), "both": (0.5, 0.5)}
UNFUSED = dict(FUSED_FFN=False, FUSED_HEAD=False, FUSED_ATTN2=False)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--plan", action="append", default=[], help="run the plans whose title contains this (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_a_launch_audit.txt"))
    args = ap.parse_args(argv)
    from progressive_stable_diffusion_amd import engine as E
    from progressive_stable_diffusion_amd import weights as W
    from progressive_stable_diffusion_amd.backend import HipBackend
    from tests import launch_audit as LA
    dev = torch.device("cuda:0")
    hip = HipBackend(dev)
    F16, BF16 = torch.float16, torch.bfloat16
    sds = {}

    def sd(kind):
        if kind not in sds:
            shapes = dict(W.unet_shapes()) if kind == "unet" else W.vae_shapes(encoder=kind == "enc", decoder=kind == "dec")
            sds[kind] = W.init_state_dict(shapes, 0, **(dict(gates=GATES, warm_start_dis=False) if kind == "unet" else {}))
        return sds[kind]

    def unet(b, s, lam, dtype=F16, policy=None):
        old = {k: getattr(E, k) for k in (policy or {})}
        for k, v in (policy or {}).items():
            setattr(E, k, v)
        try:
            return LA.audit_unet(hip, sd("unet"), b, s, lam, dtype=dtype, device=dev)
        finally:
            for k, v in old.items():
                setattr(E, k, v)

    plans = [
        ("UNetPlan(4, 64) fp16, lambda 3 (the benchmark's plan)", lambda: unet(4, 64, 3.0)),
        ("UNetPlan(4, 64) fp16, FUSED_FFN / HEAD / ATTN2 off", lambda: unet(4, 64, 3.0, policy=UNFUSED)),
        ("UNetPlan(4, 64) bf16, lambda 3", lambda: unet(4, 64, 3.0, dtype=BF16)),
        ("UNetPlan(2, 24) fp16, lambda 0", lambda: unet(2, 24, 0.0)),
        ("UNetPlan(2, 24) bf16, lambda 0", lambda: unet(2, 24, 0.0, dtype=BF16)),
        ("VaeDecoderPlan(4, 64)", lambda: LA.audit_vae_decoder(hip, sd("dec"), 4, 64, device=dev)),
        ("VaeEncoderPlan(2, 16)", lambda: LA.audit_vae_encoder(hip, sd("enc"), 2, 16, device=dev)),
        ("VaeEncoderPlan(1, 32)", lambda: LA.audit_vae_encoder(hip, sd("enc"), 1, 32, device=dev)),
    ]
    head = ("Per-launch audit of the benchmarked plans (scripts/launch_audit.py; criteria and references: tests/launch_audit.py).\n"
            "Columns: launches of the signature, worst |o - r| over the op's elementwise bound (above 1 fails), worst\n"
            "rms(o - r) / rms(r32 - r) (16-bit outputs; above 1.5 fails), seconds the audit of those launches took (launch,\n"
            "both references, comparison).  igemm signature: N, K, taps, geglu, residual, ups, stride, flags, splitk, tile_m, tile_n.")
    out, bad, above = [head], 0, 0
    for title, run in plans:
        if args.plan and not any(p in title for p in args.plan):
            continue
        t0 = time.perf_counter()
        be, plan, expected = run()
        text = LA.report(title, be, time.perf_counter() - t0)
        for r in be.failures():
            text += "\n   FAIL " + be.describe(r)
        if be.launches != expected:
            text += f"\n   FAIL {be.launches} launches audited, {expected} expected"
        bad += len(be.failures()) + (be.launches != expected)
        above += sum(1 for r in be.records if r["rms_ratio"] == r["rms_ratio"] and r["rms_ratio"] > LA.REPORT_ABOVE)
        print(text, flush=True)
        out.append(text)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        tail = (f"== all plans: {bad} outside the criteria, {above} compared tensors with an RMS ratio above {LA.REPORT_ABOVE}"
                + ("" if bad or above else ": the audit found nothing to fix and nothing to explain"))
        with open(args.out, "w") as f:          # (rewritten after every plan: a run that is cut short leaves what it had)
            f.write("\n\n".join(out + [tail]) + "\n")
    print(tail)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
