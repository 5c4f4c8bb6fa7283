#!/usr/bin/env python
"""Times of the min-depth prompt grids (gags_amd/prompts.py, include/gags_next.h N13) against the host composition of the same
step: the numpy restatement of the reference's builders (tests/prompts_ref.py mindepth_grid) on maps copied from the device,
as a user of the reference's host code would run it after gags_amd.depthsample.

  mindepth_point_grids  depths, samples [C, 1080, 1920] on the GPU, n_per_side = 8, for C = 1, 16, 200.  Reported: the whole call
                        (wall clock, synchronised) and its three parts -- the statistics kernel (HIP events), the readback of
                        the statistics (wall clock), the host draws (wall clock).
  host composition      device -> host copy of both maps, then per camera the restatement (64 crop sums, 64 masked sums, 6400
                        counts, the draws).  Timed on --host-cams cameras of each C (it is a per-image loop: its time per image
                        does not depend on C) and reported per image; `host_total_s` = per image x C is an extrapolation and is
                        labelled so.

Both paths draw from random.Random(0); the points are compared.  Prints one JSON line.

    python tools/prompts_bench.py [--h 1080] [--w 1920] [--cams 1 16 200] [--reps 5] [--host-cams 2]"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gags_amd import prompts as P  # noqa: E402


def make_maps(c, h, w, device, seed=0):
    """depths: a ramp from 0.6 to 14 with 10 % noise; samples: 20 % of the pixels, a fraction of the depth there."""
    g = torch.Generator(device=device).manual_seed(seed)
    yy = torch.linspace(0, 1, h, device=device)[None, :, None]
    xx = torch.linspace(0, 1, w, device=device)[None, None, :]
    depths = (0.6 + 13.4 * (0.65 * xx + 0.35 * yy)) * (0.9 + 0.2 * torch.rand(c, h, w, generator=g, device=device))
    frac = (0.15 + 0.95 * torch.rand(c, h, w, generator=g, device=device)) * (0.3 + 0.7 * yy)
    samples = torch.where(torch.rand(c, h, w, generator=g, device=device) < 0.2, depths * frac, torch.zeros((), device=device))
    return depths.contiguous(), samples.contiguous()


def stats_ms(xs):
    xs = sorted(xs)
    return [round(xs[len(xs) // 2], 4), round(xs[0], 4), round(xs[-1], 4)]


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--cams", type=int, nargs="+", default=[1, 16, 200])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-cams", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prompts_bench needs a GPU: there is nothing to time without one")
    import prompts_ref as R
    H, W, n = args.h, args.w, args.n
    res = {"tool": "prompts_bench", "unit": "ms (median, min, max)", "device": torch.cuda.get_device_name(0), "H": H, "W": W,
           "n_per_side": n, "reps": args.reps}
    L = P.crop_layout(H, W, n)
    for c in args.cams:
        depths, samples = make_maps(c, H, W, "cuda")
        P.crop_stats(depths, samples, n, layout=L)  # warm-up
        kern, back, draws, whole = [], [], [], []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            st = P.crop_stats(depths, samples, n, layout=L)
            b.record()
            b.synchronize()
            kern.append(a.elapsed_time(b))
            host, t = wall(lambda: P.stats_to_host(st))
            back.append(t)
            t0 = time.perf_counter()
            P.mindepth_grids_from_stats(host, L, 4, rng=random.Random(0))
            draws.append((time.perf_counter() - t0) * 1e3)
            ours, t = wall(lambda: P.mindepth_point_grids(depths, samples, n, rng=random.Random(0)))
            whole.append(t)
        # the host composition on the first --host-cams cameras, from one stream
        k = min(c, args.host_cams)
        rng = random.Random(0)
        (dh, sh), copy_ms = wall(lambda: (depths[:k].cpu().numpy(), samples[:k].cpu().numpy()))
        t0 = time.perf_counter()
        theirs = [R.mindepth_grid(n, dh[i], sh[i], 4, rng) for i in range(k)]
        host_ms = (time.perf_counter() - t0) * 1e3
        per_image = (copy_ms + host_ms) / k
        nbytes = 2 * c * H * W * 4
        res[f"C{c}"] = {
            "kernel_ms": stats_ms(kern), "readback_ms": stats_ms(back), "host_draws_ms": stats_ms(draws), "whole_call_ms": stats_ms(whole),
            "kernel_GBps": round(nbytes / stats_ms(kern)[0] / 1e6, 1),
            "host_cams_timed": k, "host_copy_ms_per_image": round(copy_ms / k, 3), "host_builder_ms_per_image": round(host_ms / k, 3),
            "host_total_s_extrapolated": round(per_image * c / 1e3, 3),
            "ratio_host_over_gpu_per_image": round(per_image / (stats_ms(whole)[0] / c), 2),
            "points_equal": all(np.array_equal(ours[i][0][0], theirs[i][0]) for i in range(k)),
            "points_per_image": int(ours[0][0][0].shape[0])}
        del depths, samples
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
