#!/usr/bin/env python
"""The evaluation-metric kernels (csrc/metrics.hip through HipBackend) next to the torch formula on the device, at the
reference's sizes: N = M = 5000, D = 768 (CLIP features) and N = M = 10000, D = 4096 (VGG fc7, ``max_samples``).
  mmd     feat_prepare + rbf_mmd (4 bandwidths)        vs  3 x cdist(...).pow(2), 12 x exp, sums (three N x N fp32 matrices)
  ipr     feat_prepare + 2 knn_radius + 2 manifold_hits vs  3 x cdist, 2 x topk(4), 2 x any
  clip    clip_features on 64 frames of 512 x 512 (device preprocessing + the tower on the kernels; ``--tower tiny|l14``)
          vs the host round trip of the reference: frames to the host, PIL, CLIPImageProcessor, pixel values back, same tower
Time: device events around ``--iters`` back-to-back calls after ``--warmup`` (the host round trip: host clock around calls
that end in a synchronise), median of ``--repeats`` such measurements.  The values of both sides are printed: they must
agree, a fast wrong kernel is no result.
usage: python scripts/metrics_bench.py [--shapes 5000x768,10000x4096] [--iters 5] [--warmup 2] [--repeats 3] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from progressive_stable_diffusion_amd import evaluation as EV  # noqa: E402
from progressive_stable_diffusion_amd.backend import HipBackend, on_backend  # noqa: E402

SIGMAS = EV.DEFAULT_SIGMAS


def timed_events(fn, warmup, iters, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return statistics.median(out)               # ms per call


def torch_mmd(x, y):
    n, m = x.shape[0], y.shape[0]
    xx, yy, xy = torch.cdist(x, x).pow(2), torch.cdist(y, y).pow(2), torch.cdist(x, y).pow(2)
    total = torch.zeros((), device=x.device)
    for sigma in SIGMAS:
        g = 1.0 / (2.0 * sigma ** 2)
        kxx, kyy, kxy = torch.exp(-g * xx), torch.exp(-g * yy), torch.exp(-g * xy)
        total = total + (kxx.sum() - kxx.diagonal().sum()) / (n * (n - 1)) + (kyy.sum() - kyy.diagonal().sum()) / (m * (m - 1)) \
            - 2 * kxy.sum() / (n * m)
    return total


def torch_ipr(x, y, k=3):
    rx = torch.cdist(x, x).topk(k + 1, largest=False).values[:, -1]
    ry = torch.cdist(y, y).topk(k + 1, largest=False).values[:, -1]
    cross = torch.cdist(y, x)
    return (cross <= rx.unsqueeze(0)).any(dim=1).float().mean(), (cross.T <= ry.unsqueeze(0)).any(dim=1).float().mean()


def features(n, d, seed, shift, dev):
    g = torch.Generator().manual_seed(99)
    base, mix = torch.randn(1, d, generator=g), 0.25 * torch.randn(16, d, generator=g)
    gs = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 16, generator=gs) @ mix + base + 0.05 * torch.randn(n, d, generator=gs) + shift * mix[0]
    return (x / x.norm(dim=1, keepdim=True)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="5000x768,10000x4096")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--frame-size", type=int, default=512)
    ap.add_argument("--tower", choices=("tiny", "l14", "none"), default="l14")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    be = HipBackend(dev)
    lines = [f"metrics_bench: {torch.cuda.get_device_name(0)}, iters {args.iters}, warmup {args.warmup}, median of {args.repeats}",
             f"{'shape':>14} {'op':>5} {'kernels ms':>11} {'torch ms':>10} {'speed-up':>9}   values (kernels | torch)"]

    for shape in args.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        x, y = features(n, d, 1, 0.0, dev), features(n, d, 2, 0.2, dev)
        p = EV._Prepared(be, x, y, False, len(SIGMAS))
        out = be.empty((3 * len(SIGMAS) + 1,), torch.float64)
        r_x, r_y = be.empty((n,), torch.float32), be.empty((n,), torch.float32)
        h_x, h_y = be.empty((n,), torch.int32), be.empty((n,), torch.int32)

        def k_mmd():
            with on_backend(be):
                be.feat_prepare(x, y, p.xc, p.yc, p.sqx, p.sqy, p.center, p.scratch)
                be.rbf_mmd(p.xc, p.sqx, p.yc, p.sqy, d, SIGMAS, out, p.scratch)

        def k_ipr():
            with on_backend(be):
                be.feat_prepare(x, y, p.xc, p.yc, p.sqx, p.sqy, p.center, p.scratch)
                be.knn_radius(p.xc, p.sqx, d, 3, r_x)
                be.knn_radius(p.yc, p.sqy, d, 3, r_y)
                be.manifold_hits(p.yc, p.sqy, p.xc, p.sqx, r_x, d, h_y)
                be.manifold_hits(p.xc, p.sqx, p.yc, p.sqy, r_y, d, h_x)

        t_k, t_t = timed_events(k_mmd, args.warmup, args.iters, args.repeats), timed_events(lambda: torch_mmd(x, y), args.warmup, args.iters, args.repeats)
        lines.append(f"{shape:>14} {'mmd':>5} {t_k:11.3f} {t_t:10.3f} {t_t / t_k:8.2f}x   {float(out[-1]):+.6e} | {float(torch_mmd(x, y)):+.6e}")
        t_k, t_t = timed_events(k_ipr, args.warmup, args.iters, args.repeats), timed_events(lambda: torch_ipr(x, y), args.warmup, args.iters, args.repeats)
        pr, rc = torch_ipr(x, y)
        lines.append(f"{shape:>14} {'ipr':>5} {t_k:11.3f} {t_t:10.3f} {t_t / t_k:8.2f}x   {float(h_y.sum()) / n:.4f} {float(h_x.sum()) / n:.4f} | "
                     f"{float(pr):.4f} {float(rc):.4f}")
        del p, x, y
        torch.cuda.empty_cache()

    if args.tower != "none":
        from PIL import Image
        from transformers import CLIPImageProcessor

        from progressive_stable_diffusion_amd import conditioning as PC
        from progressive_stable_diffusion_amd import weights as W
        cfg = dict(W.CLIP_VIT_L14) if args.tower == "l14" else dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                                                                    num_attention_heads=1, image_size=224, patch_size=14, projection_dim=32)
        enc = PC.ImageEncoder(W.init_state_dict(W.clip_shapes(cfg), 5), dev, be=be)
        proc = CLIPImageProcessor(do_resize=True, size={"shortest_edge": 224}, resample=3, do_center_crop=True,
                                  crop_size={"height": 224, "width": 224}, do_rescale=True, rescale_factor=1 / 255, do_normalize=True,
                                  image_mean=list(EV.CLIP_MEAN), image_std=list(EV.CLIP_STD))
        frames = torch.rand(args.frames, 3, args.frame_size, args.frame_size, generator=torch.Generator().manual_seed(3)).to(dev)

        def host_round_trip():
            pil = [Image.fromarray(f.permute(1, 2, 0).mul(255).to(torch.uint8).cpu().numpy()) for f in frames]
            return enc(proc(images=pil, return_tensors="pt", do_rescale=True).pixel_values.to(dev))

        def host_clock(fn):
            fn()
            ts = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(ts), r
        t_k = timed_events(lambda: EV.clip_features(enc, frames), 1, max(1, args.iters // 2), args.repeats)
        t_h, want = host_clock(host_round_trip)
        got = EV.clip_features(enc, frames)
        rel = float((got - want).abs().max() / want.abs().max())
        shape = f"{args.frames}x{args.frame_size}^2"
        lines.append(f"{shape:>14} {'clip':>5} {t_k:11.3f} {t_h:10.3f} {t_h / t_k:8.2f}x   tower {args.tower}, max rel difference of the features {rel:.2e}")

    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
