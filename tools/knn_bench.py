#!/usr/bin/env python
"""gags_amd.knn.dist2 (include/gags_next.h N9, csrc/knn.hip) against the torch composition of the same computation -- the
only baseline there is: chunked torch.cdist(x_chunk, x) -> topk(4, largest=False) -> drop self -> mean of squares, with the
largest chunk whose distance matrix fits 8 GiB -- on the same machine, in the same process.

Sizes: N = 1.8e5 (a typical COLMAP cloud) and 1.5e6 (the point count of the depth-sample documents); clouds: uniform in the
unit cube, and the two_clusters recipe of tests/knn_ref.py scaled up (half the points within 1e-3 of the origin, half within 1
of (50, 50, 50), one far outlier, one triple).  Per (size, cloud):
  * the kernel: two warm-up calls, then --reps calls, HIP events around each: median, minimum and maximum;
  * the per-phase split (keys + sort, boxes, query) from one profiled call, taken after the timed ones: kernel durations summed
    by name (knn_bbox* / knn_key / rs_* / knn_gather; knn_box; knn_query);
  * the composition: its first two chunks as warm-up, then whole runs until --baseline-reps or --baseline-seconds is reached
    (at least one), a host clock around work that ends in a synchronise;
  * a check: 256 sampled points against the contract's float32 expression evaluated by torch element-wise kernels over ALL
    points (no matrix product, no FMA), bit for bit.
Prints one JSON line; needs a GPU.

    python tools/knn_bench.py [--sizes 180000,1500000] [--reps 10] [--baseline-reps 3] [--baseline-seconds 60]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import knn_ref as K  # noqa: E402
from gags_amd import knn  # noqa: E402

DEV = "cuda"
CHUNK_BYTES = 8 << 30
PHASES = {"keys_sort": ("knn_bbox", "knn_key", "rs_", "knn_gather"), "boxes": ("knn_box_kernel",), "query": ("knn_query",)}


def make_cloud(kind, n):
    if kind == "uniform":
        return np.random.default_rng(101).random((n, 3)).astype(np.float32)
    return K.two_clusters_scaled(n)


def torch_composition(x, n_chunks=None):
    """The baseline: x [N, 3] on the device -> [N]; n_chunks: stop after that many chunks (warm-up)."""
    n = x.shape[0]
    chunk = max(1, CHUNK_BYTES // (4 * n))
    out = torch.empty(n, device=x.device)
    for c, s in enumerate(range(0, n, chunk)):
        if n_chunks is not None and c >= n_chunks:
            break
        d = torch.cdist(x[s:s + chunk], x)
        near = torch.topk(d, 4, dim=1, largest=False).values[:, 1:]
        out[s:s + chunk] = (near * near).mean(dim=1)
        del d, near
    return out


def check_sample(x, got, m=256, step=32):
    """got at m sampled points == the contract evaluated by element-wise float32 torch kernels (each op its own kernel: no FMA)."""
    n = x.shape[0]
    idx = torch.randperm(n, device=x.device, generator=torch.Generator(device=x.device).manual_seed(9))[:m]
    idx[:4] = torch.tensor([0, n - 1, n - 2, n - 4], device=x.device)[:4]  # (two_clusters: the last four are outlier + triple)
    bad = 0
    for s in range(0, m, step):
        i = idx[s:s + step]
        q = x[i]
        dx = x[None, :, 0] - q[:, None, 0]
        dy = x[None, :, 1] - q[:, None, 1]
        dz = x[None, :, 2] - q[:, None, 2]
        d2 = dx * dx
        d2 += dy * dy
        d2 += dz * dz
        d2[torch.arange(i.shape[0], device=x.device), i] = float("inf")
        b = torch.topk(d2, 3, dim=1, largest=False).values.sort(dim=1).values
        want = ((b[:, 0] + b[:, 1]) + b[:, 2]) / 3.0
        bad += int((want != got[i]).sum())
        del dx, dy, dz, d2
    return bad


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def phase_split(x):
    """ms per phase of one call, from the profiler's kernel records."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        knn.dist2(x)
        torch.cuda.synchronize()
    ms = {k: 0.0 for k in PHASES}
    other = 0.0
    for e in prof.events():
        if e.device_type != torch.autograd.DeviceType.CUDA:
            continue
        t = getattr(e, "device_time", None)
        t = getattr(e, "cuda_time", 0.0) if t is None else t
        for k, pats in PHASES.items():
            if any(p in e.name for p in pats):
                ms[k] += t / 1e3
                break
        else:
            other += t / 1e3
    return {**{k: round(v, 4) for k, v in ms.items()}, "other": round(other, 4)}


def bench(kind, n, reps, base_reps, base_seconds):
    x = torch.from_numpy(make_cloud(kind, n)).to(DEV)
    n = x.shape[0]
    row = {"cloud": kind, "n": n, "reps": reps, "scratch_MB": round(knn._lib.load().gags_knn3_dist2_scratch_bytes(n) / 2 ** 20, 1)}
    for _ in range(2):
        got = knn.dist2(x)
    ts = sorted(event_ms(lambda: knn.dist2(x))[0] for _ in range(reps))
    row.update(kernel_ms_median=round(ts[len(ts) // 2], 4), kernel_ms_min=round(ts[0], 4), kernel_ms_max=round(ts[-1], 4))
    row["phases_ms"] = phase_split(x)
    row["sample_mismatches"] = check_sample(x, got)
    torch_composition(x, n_chunks=2)
    torch.cuda.synchronize()
    bt, t_all = [], time.perf_counter()
    while len(bt) < base_reps and (not bt or time.perf_counter() - t_all < base_seconds):
        t0 = time.perf_counter()
        ref = torch_composition(x)
        torch.cuda.synchronize()
        bt.append((time.perf_counter() - t0) * 1e3)
    bt.sort()
    rel = ((ref - got).abs() / got.clamp_min(1e-30))
    row.update(torch_chunk=max(1, CHUNK_BYTES // (4 * n)), torch_runs=len(bt), torch_ms_median=round(bt[len(bt) // 2], 2),
               torch_ms_min=round(bt[0], 2), torch_ms_max=round(bt[-1], 2),
               torch_median_rel_diff=float(rel.median()),  # (cdist goes through a matrix product: it is NOT exact)
               speedup_median=round(bt[len(bt) // 2] / ts[len(ts) // 2], 1))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="180000,1500000")
    ap.add_argument("--clouds", default="uniform,two_clusters")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--baseline-seconds", type=float, default=60.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench: needs a GPU (no time is reported without one)")
    res = {"tool": "knn_bench", "unit": "ms", "box": knn.BOX, "runs": []}
    for n in (int(s) for s in args.sizes.split(",") if s):
        for kind in (c for c in args.clouds.split(",") if c):
            row = bench(kind, n, args.reps, args.baseline_reps, args.baseline_seconds)
            res["runs"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
