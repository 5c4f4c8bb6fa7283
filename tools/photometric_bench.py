#!/usr/bin/env python
"""The RGB stage's photometric loss (gags_amd.losses.photometric_loss, include/gags_next.h N7), forward + backward, against
the torch composition of the same formula -- F.conv2d(groups=3) with the reference's 11 x 11 window plus element-wise ops,
written below: the reference's formulation on the same GPU, the only baseline there is -- at 1920 x 1080 x 3 and
1280 x 720 x 3.  The image is the [3,H,W] view of [H,W,3] memory (what render() returns) and, second, a contiguous [3,H,W];
the target is contiguous.  Both paths are timed in one process, alternating, HIP events around forward + backward, one
warm-up round of each, then the median (and minimum) of --reps rounds.  Algorithmic bytes of the fused pair: forward reads 2
images and writes 3 maps, backward reads 5 and writes 1 = 11 x 4 x 3 H W (0.27 GB at 1080p); GB/s = that over the fused time.
Launches per forward + backward are counted from one profiled round of each path (after the timing).  Prints one JSON line.

    python tools/photometric_bench.py [--sizes 1920x1080,1280x720] [--reps 30] [--no-count]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from gags_amd import losses  # noqa: E402


def torch_composition(window2d):
    """(1 - lambda) l1 + lambda (1 - ssim) as utils/loss_utils.py:20,178-196 spells it."""
    C1, C2 = 0.01 ** 2, 0.03 ** 2

    def loss(img, gt, lam=0.2):
        x, y = img[None], gt[None]
        mu1, mu2 = F.conv2d(x, window2d, padding=5, groups=3), F.conv2d(y, window2d, padding=5, groups=3)
        mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        s1 = F.conv2d(x * x, window2d, padding=5, groups=3) - mu1_sq
        s2 = F.conv2d(y * y, window2d, padding=5, groups=3) - mu2_sq
        s12 = F.conv2d(x * y, window2d, padding=5, groups=3) - mu1_mu2
        ssim_map = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
        return (1.0 - lam) * torch.abs(img - gt).mean() + lam * (1.0 - ssim_map.mean())
    return loss


def one_round(fn, img, gt):
    x = img.detach().requires_grad_(True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    loss = fn(x, gt)
    loss.backward()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), loss.detach(), x.grad


def count_launches(fn, img, gt):
    from torch.profiler import ProfilerActivity, profile
    x = img.detach().requires_grad_(True)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn(x, gt).backward()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def stats(ts):
    ts = sorted(ts)
    return round(ts[len(ts) // 2], 4), round(ts[0], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,1280x720")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--no-count", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("photometric_bench: needs a GPU (no time is reported without one)")
    if args.reps < 20:
        raise SystemExit("photometric_bench: at least 20 rounds")
    dev = "cuda"
    w1 = torch.tensor(losses.SSIM_WINDOW, dtype=torch.float32, device=dev)[:, None]
    window2d = (w1 @ w1.t())[None, None].expand(3, 1, 11, 11).contiguous()
    paths = {"fused": losses.photometric_loss, "torch": torch_composition(window2d)}
    res = {"tool": "photometric_bench", "unit": "ms", "reps": args.reps, "runs": []}
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        g = torch.Generator(device=dev).manual_seed(w)
        gt = torch.rand(3, h, w, device=dev, generator=g)
        hwc = (gt.permute(1, 2, 0) + 0.05 * torch.randn(h, w, 3, device=dev, generator=g)).clamp(0, 1).contiguous()
        layouts = {"pixel_major_view": hwc.permute(2, 0, 1), "contiguous": hwc.permute(2, 0, 1).contiguous()}
        nbytes = 11 * 4 * 3 * h * w
        for lname, img in layouts.items():
            ts = {k: [] for k in paths}
            out = {}
            for k, fn in paths.items():  # warm-up: code objects, the convolution's algorithm choice, the allocator's blocks
                for _ in range(2):
                    one_round(fn, img, gt)
            for _ in range(args.reps):  # alternating
                for k, fn in paths.items():
                    t, loss, grad = one_round(fn, img, gt)
                    ts[k].append(t)
                    out[k] = (loss, grad)
            row = {"width": w, "height": h, "layout": lname, "alg_GB": round(nbytes / 1e9, 4)}
            for k in paths:
                row[k + "_ms_median"], row[k + "_ms_min"] = stats(ts[k])
            row["fused_GBps"] = round(nbytes / (row["fused_ms_median"] * 1e-3) / 1e9, 1)
            row["speedup_median"] = round(row["torch_ms_median"] / row["fused_ms_median"], 2)
            row["loss_diff"] = abs(float(out["fused"][0]) - float(out["torch"][0]))
            row["grad_diff_rel"] = float((out["fused"][1] - out["torch"][1]).abs().max() / out["torch"][1].abs().max())
            if not args.no_count:
                for k, fn in paths.items():
                    try:
                        row[k + "_launches"] = count_launches(fn, img, gt)
                    except Exception as e:  # the timing above stands without the count
                        row[k + "_launches"] = f"not counted ({type(e).__name__})"
            res["runs"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
