#!/usr/bin/env python
"""The bilateral grid (gags_amd.bilagrid, include/gags_next.h N24): slice forward + backward (gradients to the grid and to the
image) and the TV term forward + backward, against the float32 torch composition of the same rule -- F.grid_sample plus
element-wise operators, differentiated by autograd, written below: the only baseline there is -- at 1920 x 1080 with the
default 16 x 16 x 8 grid.  The image is the [3,H,W] view of [H,W,3] memory (what render() returns).  Both paths are timed in
one process, alternating, HIP events around forward + backward, two warm-up rounds of each, then the median (and minimum) of
--reps rounds.  Algorithmic bytes of the fused slice pair: forward reads and writes one image, backward reads two and writes
one = 5 x 12 H W (0.12 GB at 1080p; the grid and its gradient are ~0.1 MB each); GB/s = that over the fused time.  TV: --grids
grids of the default size.  Prints one JSON line.

    python tools/bilagrid_bench.py [--size 1920x1080] [--grid 16x16x8] [--grids 200] [--reps 30]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from gags_amd import bilagrid  # noqa: E402


def slice_composition(grid, chw):
    """The rule in torch operators: grid [12,L,Gh,Gw], chw [3,H,W] -> [3,H,W]."""
    _, h, w = chw.shape
    xs = (torch.arange(w, dtype=chw.dtype, device=chw.device) + 0.5) / w
    ys = (torch.arange(h, dtype=chw.dtype, device=chw.device) + 0.5) / h
    gray = (0.299 * chw[0] + 0.587 * chw[1]) + 0.114 * chw[2]
    coords = torch.stack([(2 * xs - 1)[None, :].expand(h, w), (2 * ys - 1)[:, None].expand(h, w), 2 * gray - 1], -1)
    A = F.grid_sample(grid[None], coords[None, None], mode="bilinear", align_corners=True, padding_mode="border")[0, :, 0]
    A = A.reshape(3, 4, h, w)
    return (A[:, :3] * chw[None]).sum(1) + A[:, 3]


def tv_composition(grids):
    b = grids.shape[0]
    total = 0.0
    for d in (2, 3, 4):
        diff = grids.narrow(d, 1, grids.shape[d] - 1) - grids.narrow(d, 0, grids.shape[d] - 1)
        total = total + (diff ** 2).sum() / (diff.numel() // b)
    return 2.0 * total / b


def slice_round(fn, grid, img, v):
    g, x = grid.detach().requires_grad_(True), img.detach().requires_grad_(True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn(g, x)
    out.backward(v)
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out.detach(), g.grad, x.grad


def tv_round(fn, grids):
    g = grids.detach().requires_grad_(True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    loss = fn(g)
    loss.backward()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), loss.detach(), g.grad


def stats(ts):
    ts = sorted(ts)
    return round(ts[len(ts) // 2], 4), round(ts[0], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--grid", default="16x16x8", help="grid_X x grid_Y x grid_W")
    ap.add_argument("--grids", type=int, default=200, help="number of grids of the TV term")
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bilagrid_bench: needs a GPU (no time is reported without one)")
    if args.reps < 20:
        raise SystemExit("bilagrid_bench: at least 20 rounds")
    dev = "cuda"
    w, h = (int(v) for v in args.size.split("x"))
    gx, gy, gl = (int(v) for v in args.grid.split("x"))
    gen = torch.Generator(device=dev).manual_seed(w)
    img = torch.rand(h, w, 3, device=dev, generator=gen).permute(2, 0, 1)
    v = torch.randn(h, w, 3, device=dev, generator=gen).permute(2, 0, 1)
    model = bilagrid.BilateralGrid(args.grids, gx, gy, gl).to(dev)
    with torch.no_grad():
        model.grids.add_(0.1 * torch.randn(model.grids.shape, device=dev, generator=gen))
    grid = model.grids.detach()[0].clone()
    res = {"tool": "bilagrid_bench", "unit": "ms", "reps": args.reps, "width": w, "height": h, "grid": [gl, gy, gx], "grids": args.grids}

    paths = {"fused": bilagrid.slice, "torch": slice_composition}
    ts, out = {k: [] for k in paths}, {}
    for fn in paths.values():
        for _ in range(2):
            slice_round(fn, grid, img, v)
    for _ in range(args.reps):  # alternating
        for k, fn in paths.items():
            t, *out[k] = slice_round(fn, grid, img, v)
            ts[k].append(t)
    nbytes = 5 * 12 * h * w
    row = {"alg_GB": round(nbytes / 1e9, 4)}
    for k in paths:
        row[k + "_ms_median"], row[k + "_ms_min"] = stats(ts[k])
    row["fused_GBps"] = round(nbytes / (row["fused_ms_median"] * 1e-3) / 1e9, 1)
    row["speedup_median"] = round(row["torch_ms_median"] / row["fused_ms_median"], 2)
    for name, a, b in zip(("out", "v_grid", "v_rgb"), out["fused"], out["torch"]):
        row[name + "_diff_rel"] = float((a - b).abs().max() / b.abs().max())
    res["slice"] = row

    paths = {"fused": bilagrid.total_variation_loss, "torch": tv_composition}
    ts, out = {k: [] for k in paths}, {}
    grids = model.grids.detach()
    for fn in paths.values():
        for _ in range(2):
            tv_round(fn, grids)
    for _ in range(args.reps):
        for k, fn in paths.items():
            t, *out[k] = tv_round(fn, grids)
            ts[k].append(t)
    row = {"alg_GB": round(3 * 4 * grids.numel() / 1e9, 4)}  # forward reads the grids, backward reads them and writes a gradient
    for k in paths:
        row[k + "_ms_median"], row[k + "_ms_min"] = stats(ts[k])
    row["speedup_median"] = round(row["torch_ms_median"] / row["fused_ms_median"], 2)
    row["loss_diff"] = abs(float(out["fused"][0]) - float(out["torch"][0]))
    row["grad_diff_rel"] = float((out["fused"][1] - out["torch"][1]).abs().max() / out["torch"][1].abs().max())
    res["tv"] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
