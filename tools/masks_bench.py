#!/usr/bin/env python
"""Times and peak memory of the SAM mask post-processing (gags_amd/sam_masks.py, include/gags_next.h N10) on M random
rectangle masks of H x W with 10 % holes (default M = 256, 1080 x 1920): the four kernels one by one (pack, pair
intersections, column maxima, paint with every mask kept) and mask_nms end to end (sort, the fused pack + pairs + colmax
entry, the threshold tests, the one readback), against the obvious torch composition on the same GPU --
m.float() @ m.float().T, then the element-wise operations of the restatement (tests/sam_masks_ref.py) as GPU tensor ops --
and, on the host at a reduced size, a Python pair loop in the reference's style (two full-image logical ops and two sums per
pair).  HIP events, median of --reps runs after one warm-up; peak memory = torch.cuda.max_memory_allocated over one call,
above what the masks themselves occupy.  The two GPU paths must select the same masks (reported as `same_selection`).
Prints one JSON line.

    python tools/masks_bench.py [--m 256] [--h 1080] [--w 1920] [--reps 7] [--loop-m 48] [--loop-h 270] [--loop-w 480]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gags_amd import sam_masks as SM  # noqa: E402


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


def rect_masks(m, h, w, seed, device):
    """[m, h, w] bool: rectangles (a third of them nested in the previous one), each losing 10 % of its pixels."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = torch.empty(m, h, w, dtype=torch.bool, device=device)
    ys, xs = torch.arange(h, device=device)[:, None], torch.arange(w, device=device)[None, :]
    gd = torch.Generator(device=device).manual_seed(seed)
    box = (0, h, 0, w)
    for k in range(m):
        r = torch.rand(5, generator=g).tolist()
        y0, y1, x0, x1 = box if (k and r[4] < 0.33) else (0, h, 0, w)
        bh, bw = max(2, int((y1 - y0) * (0.15 + 0.6 * r[0]))), max(2, int((x1 - x0) * (0.15 + 0.6 * r[1])))
        ya, xa = y0 + int((y1 - y0 - bh) * r[2]), x0 + int((x1 - x0 - bw) * r[3])
        box = (ya, ya + bh, xa, xa + bw)
        out[k] = (ys >= ya) & (ys < ya + bh) & (xs >= xa) & (xs < xa + bw) & (torch.rand(h, w, generator=gd, device=device) >= 0.1)
    return out


def torch_nms(masks, scores, iou_thr=0.7, score_thr=0.1, inner_thr=0.2):
    """The obvious composition: a float matmul for the intersections, then the matrix form of the pair loop."""
    n = masks.shape[0]
    mf = masks.reshape(n, -1).float()
    inter = mf @ mf.t()
    s_sorted, idx = torch.sort(scores, descending=True, stable=True)
    I = inter[idx][:, idx]
    a = torch.diagonal(I)
    rate = I / a[:, None]
    r_i, r_j = rate, rate.t()
    upper = torch.ones(n, n, dtype=torch.bool, device=masks.device).triu(1)
    zero = torch.zeros((), device=masks.device)
    iou = torch.where(upper, I / (a[:, None] + a[None, :] - I), zero)
    val = 1 - r_j * r_i
    inner = torch.where(upper & (r_i < 0.5) & (r_j >= 0.85), val, zero) + \
        torch.where(upper & (r_i >= 0.85) & (r_j < 0.5), val, zero).t()
    keeps = torch.stack([iou.max(dim=0).values <= iou_thr, s_sorted > score_thr,
                         inner.triu(1).max(dim=0).values <= 1 - inner_thr, inner.tril(1).max(dim=0).values <= 1 - inner_thr])
    top3 = torch.arange(n, device=masks.device) < 3
    none = ~keeps.any(dim=1, keepdim=True)
    none[0] = False
    keeps = torch.where(none, top3[None], keeps)
    return idx[keeps.all(dim=0)]


def pair_loop(masks, scores):
    """The reference's style on the host: per pair two full-image logical ops and two sums (IoU and the two rates only)."""
    order = torch.argsort(scores, descending=True)
    m = masks[order]
    n = m.shape[0]
    area = m.sum(dim=(1, 2), dtype=torch.float)
    iou = torch.zeros(n, n)
    for i in range(n):
        for j in range(i, n):
            inter = torch.sum(torch.logical_and(m[i], m[j]), dtype=torch.float)
            union = torch.sum(torch.logical_or(m[i], m[j]), dtype=torch.float)
            iou[i, j] = inter / union
            _ = inter / area[i] < 0.5 and inter / area[j] >= 0.85
    return iou


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loop-m", type=int, default=48)
    ap.add_argument("--loop-h", type=int, default=270)
    ap.add_argument("--loop-w", type=int, default=480)
    args = ap.parse_args()
    M, H, W = args.m, args.h, args.w
    dev = torch.device("cuda")
    masks = rect_masks(M, H, W, 0, dev)
    scores = torch.rand(M, generator=torch.Generator().manual_seed(1), dtype=torch.float64).mul(0.5).add(0.5).to(dev)
    res = {"tool": "masks_bench", "unit": "ms (median, min, max)", "reps": args.reps, "M": M, "H": H, "W": W,
           "device": torch.cuda.get_device_name(0), "masks_MiB": round(masks.numel() / 2 ** 20, 1)}

    bits, area = SM.pack_masks(masks)
    inter = SM.pair_intersections(bits)
    order = torch.argsort(scores, descending=True)
    kept = torch.arange(M, dtype=torch.int32, device=dev)
    res["bits_MiB"] = round(bits.numel() * 8 / 2 ** 20, 1)
    res["pack_ms"] = timed(lambda: SM.pack_masks(masks), args.reps)
    res["pairs_ms"] = timed(lambda: SM.pair_intersections(bits), args.reps)
    res["colmax_ms"] = timed(lambda: SM.column_maxima(inter, area, order), args.reps)
    res["paint_ms"] = timed(lambda: SM.seg_map(bits, kept, H, W), args.reps)
    res["hip_mask_nms_ms"] = timed(lambda: SM.mask_nms(masks, scores), args.reps)
    res["hip_mask_nms_peak_MiB"] = peak_mib(lambda: SM.mask_nms(masks, scores))
    nw = bits.shape[1]
    res["pairs_G_word_pairs_per_s"] = round(M * (M + 1) / 2 * nw / (res["pairs_ms"][0] * 1e-3) / 1e9, 1)
    res["pack_GBps"] = round(masks.numel() / (res["pack_ms"][0] * 1e-3) / 1e9, 1)
    del bits, inter
    res["torch_mask_nms_ms"] = timed(lambda: torch_nms(masks, scores).cpu(), args.reps)
    res["torch_mask_nms_peak_MiB"] = peak_mib(lambda: torch_nms(masks, scores).cpu())
    res["same_selection"] = bool(torch.equal(SM.mask_nms(masks, scores), torch_nms(masks, scores)))
    res["selected"] = int(SM.mask_nms(masks, scores).numel())

    lm = rect_masks(args.loop_m, args.loop_h, args.loop_w, 2, torch.device("cpu"))
    ls = torch.rand(args.loop_m, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    t0 = time.perf_counter()
    pair_loop(lm, ls)
    res["host_pair_loop"] = {"M": args.loop_m, "H": args.loop_h, "W": args.loop_w, "threads": torch.get_num_threads(),
                             "s": round(time.perf_counter() - t0, 3)}
    lm_d, ls_d = lm.to(dev), ls.to(dev)
    res["hip_mask_nms_at_loop_size_ms"] = timed(lambda: SM.mask_nms(lm_d, ls_d), args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
