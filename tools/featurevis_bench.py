#!/usr/bin/env python
"""Times and peak memory of the PCA colouring of a feature map (gags_amd/featurevis.py, include/gags_next.h N11) on a seeded
[C, H, W] map (default C = 512, 1080 x 1920; a mixture of 6 embeddings with smooth spatial weights plus noise), in both
layouts -- channel-major and the pixel-major memory behind the decoders' permuted view: the four kernels one by one (moments,
project, select, colour) and feature_visualize end to end (moments, the C x C readback and float64 eigh on the host, project,
select and its 4-float readback, colour), against the obvious torch composition of the same function on the same GPU --
F.normalize, the sample's float32 Gram matrix by matmul, the same host eigh, a matmul projection, torch.quantile, clamp.
HIP events, median of --reps runs after one warm-up; peak memory = torch.cuda.max_memory_allocated over one call, above what
the map itself occupies.  `max_abs_diff` is the largest difference between the two paths' images.  Prints one JSON line.

    python tools/featurevis_bench.py [--c 512] [--h 1080] [--w 1920] [--reps 5]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gags_amd import featurevis as FV  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return round(peak / 2 ** 20, 1)


def make_map(c, h, w, seed, device):
    """[c, h, w] float32, channel-major: 3.7 (softmax-weighted mixture of 6 embeddings + 0.05 noise)."""
    g = torch.Generator(device=device).manual_seed(seed)
    emb = torch.randn(6, c, generator=g, device=device)
    yy = torch.linspace(0, 1, h, device=device)[:, None]
    xx = torch.linspace(0, 1, w, device=device)[None, :]
    par = torch.rand(6, 4, generator=g, device=device)
    z = torch.stack([3.0 * 0.8 ** k * (torch.sin(2 * math.pi * ((0.5 + 2 * par[k, 0]) * yy + par[k, 1]))
                                       + torch.cos(2 * math.pi * ((0.5 + 2 * par[k, 2]) * xx + par[k, 3]))) for k in range(6)])
    f = torch.einsum("khw,kc->chw", torch.softmax(z, dim=0), emb)
    f.add_(torch.randn(c, h, w, generator=g, device=device), alpha=0.05).mul_(3.7)
    return f


def torch_visualize(feature):
    """render.py:33-48 as torch ops on the GPU (the PCA fit as this package's: moments, host eigh)."""
    c, h, w = feature.shape
    x = torch.nn.functional.normalize(feature, dim=0).permute(1, 2, 0).reshape(-1, c)
    xs = x[::3]
    n = xs.shape[0]
    mean, comps = FV.pca_from_moments(xs.sum(dim=0), xs.t() @ xs, n)
    mean, comps = mean.to(x.device, torch.float32), comps.to(x.device, torch.float32)
    t = (x - mean) @ comps.t()
    q = torch.quantile(t[::3].reshape(-1), torch.tensor([0.01, 0.99], device=x.device))
    return ((t - q[0]) / (q[1] - q[0])).clamp_(0, 1).reshape(h, w, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c", type=int, default=512)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    C, H, W = args.c, args.h, args.w
    dev = torch.device("cuda")
    P, S = H * W, (H * W + 2) // 3
    res = {"tool": "featurevis_bench", "unit": "ms (median, min, max)", "reps": args.reps, "C": C, "H": H, "W": W,
           "device": torch.cuda.get_device_name(0), "map_MiB": round(C * P * 4 / 2 ** 20, 1), "samples": S,
           "moments_GFLOP": round(2 * S * C * C / 1e9, 1)}
    cm = make_map(C, H, W, 0, dev)
    for name in ("channel_major", "pixel_major"):
        x = cm if name == "channel_major" else cm.permute(1, 2, 0).contiguous().permute(2, 0, 1)
        r = {}
        mean, comps, q1, q99 = FV.feature_pca_basis(x)
        t = FV.feature_project(x, mean, comps)
        r["moments_ms"] = timed(lambda: FV.feature_moments(x), args.reps)
        r["moments_TFLOPs"] = round(2 * S * C * C / (r["moments_ms"][0] * 1e-3) / 1e12, 1)
        r["project_ms"] = timed(lambda: FV.feature_project(x, mean, comps), args.reps)
        r["project_GBps"] = round(C * P * 4 / (r["project_ms"][0] * 1e-3) / 1e9, 1)
        r["select_ms"] = timed(lambda: FV.order_statistics(t, [10, 11, 3 * S - 12, 3 * S - 11], group=3, stride=9, n=3 * S), args.reps)
        r["colour_ms"] = timed(lambda: FV.feature_colour(t, q1, q99, H, W, return_uint8=True), args.reps)
        r["hip_feature_visualize_ms"] = timed(lambda: FV.feature_visualize(x), args.reps)
        r["hip_feature_visualize_peak_MiB"] = peak_mib(lambda: FV.feature_visualize(x))
        r["torch_feature_visualize_ms"] = timed(lambda: torch_visualize(x), args.reps)
        r["torch_feature_visualize_peak_MiB"] = peak_mib(lambda: torch_visualize(x))
        r["max_abs_diff"] = float((FV.feature_visualize(x) - torch_visualize(x)).abs().max())
        res[name] = r
        del x, t
    print(json.dumps(res))


if __name__ == "__main__":
    main()
