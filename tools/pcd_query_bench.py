#!/usr/bin/env python
"""Stage times of the 3-D open-vocabulary query (gags_amd/pointquery.py, include/gags_next.h N5) on synthetic Gaussians:
decode (CNN_decoder 16 -> 512, chunks of 1 M), relevancy (3 phrases), normalise + threshold, and the neighbour vote
(gags_point_mask_smooth: grid + sorts + capped scan).  The vote is timed on coherent masks of about 1 %, 10 % and 50 %
(balls around points of the cloud, K = 3 at once) at the reference's r = 0.05 and at a radius that puts ~100 or more
masked neighbours around a typical masked point.  HIP events, median of --reps runs.  Prints one JSON line.

    python tools/pcd_query_bench.py [--n 1500000,4000000] [--reps 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gags_amd import synthetic as syn  # noqa: E402
from gags_amd import pointquery as PQ  # noqa: E402
from gags_amd.decoders import CNN_decoder  # noqa: E402
from gags_amd.relevancy import RelevancyHead  # noqa: E402


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return round(ts[len(ts) // 2], 3), out


def coherent(xyz, frac, n_masks, g):
    """Balls around random points of the cloud holding ~frac of the points each (a 100 k sample sets the radius)."""
    masks = []
    for _ in range(n_masks):
        c = xyz[torch.randint(0, xyz.shape[0], (1,), device=xyz.device, generator=g)]
        d = (xyz - c).norm(dim=1)
        R = torch.quantile(d[torch.randint(0, xyz.shape[0], (100000,), device=xyz.device, generator=g)], frac)
        masks.append(d < R)
    return torch.stack(masks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1500000,4000000")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    dec = CNN_decoder(16, 512).to(dev)
    head = RelevancyHead(torch.nn.functional.normalize(torch.randn(3, 512, device=dev, generator=g), dim=-1),
                         torch.nn.functional.normalize(torch.randn(4, 512, device=dev, generator=g), dim=-1))
    res = {"tool": "pcd_query_bench", "unit": "ms", "reps": args.reps, "runs": []}
    for n in [int(v) for v in args.n.split(",")]:
        xyz = syn.make_gaussians(n, 0, 1920, 1080, seed=0, device="cuda")["xyz"].contiguous()
        sem = torch.randn(n, 16, device=dev, generator=g) * 0.25
        run = {"n": n}
        chunks = [sem[s:s + 1_000_000] for s in range(0, n, 1_000_000)]
        with torch.no_grad():
            run["decode"], feats = timed(lambda: [dec(c.t()[..., None]).squeeze(-1).t() for c in chunks], args.reps)
            run["relevancy"], probs = timed(lambda: [head._all(f) for f in feats], args.reps)
            del feats
            probs = torch.cat(probs, dim=1)
            lib = PQ._lib.load()
            nb = lib.gags_point_relevancy_mask_scratch_bytes(3, n)
            scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
            nrm = torch.empty(3, n, device=dev)
            mraw = torch.empty(3, n, dtype=torch.uint8, device=dev)

            def normalise():
                PQ.check(lib.gags_point_relevancy_mask(3, n, PQ.ptr(probs), 0.4, PQ.ptr(nrm), PQ.ptr(mraw), PQ.ptr(scratch), nb,
                                                       PQ._lib.stream()), "gags_point_relevancy_mask")
            run["normalise"], _ = timed(normalise, args.reps)
            run["query_total_r0.05"], _ = timed(lambda: PQ.query_points(sem, xyz, dec, head), max(1, args.reps // 2))
        votes = []
        for frac in (0.01, 0.10, 0.50):
            masks = coherent(xyz, frac, 3, g)
            for r in (0.05, 0.15):
                t, (out, cnt) = timed(lambda: PQ.smooth_point_mask(masks, xyz, r, 20, return_counts=True), args.reps)
                # typical (median) count over the masked points, capped at 21
                med = int(cnt[masks].float().median().item()) if masks.any() else 0
                votes.append({"mask_frac": round(masks.float().mean().item(), 4), "radius": r, "vote_ms": t,
                              "median_capped_count": med, "kept": int(out.sum().item())})
            # uncapped neighbour density at r = 0.15: the threshold that makes the scan visit ~every neighbour
            t, (_, cnt) = timed(lambda: PQ.smooth_point_mask(masks, xyz, 0.15, 1000, return_counts=True), args.reps)
            votes.append({"mask_frac": round(masks.float().mean().item(), 4), "radius": 0.15, "threshold": 1000, "vote_ms": t,
                          "median_count": int(cnt[masks].float().median().item())})
        run["vote"] = votes
        res["runs"].append(run)
        del probs, nrm, mraw, scratch, xyz, sem
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
