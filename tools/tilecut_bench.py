#!/usr/bin/env python
"""Times of the tile cut (gags_amd/tilecut.py, include/gags_next.h N14) on K random rectangle masks with 10 % holes over one
H x W image (default K = 300, 1080 x 1920): the tile kernel with the fp32 output CLIP takes, with the uint8 output and with
both, the box kernel, and cut_tiles end to end (box validation on the host, upload, launch) -- against the host composition of
tests/tilecut_ref.py for the same masks (crop, mask, pad and the integer resize in numpy, then stack, float conversion,
permute, / 255 and the upload, as preprocess.py:476-489 does them; --host-tiles of the K, extrapolated).  HIP events, median of
--reps runs after one warm-up.  written_GBps counts the bytes the kernel stores.  The GPU tiles must equal the host
composition's (reported as `same_tiles`).  Prints one JSON line.

    python tools/tilecut_bench.py [--k 300] [--h 1080] [--w 1920] [--reps 7] [--host-tiles 30]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import tilecut_ref as R  # noqa: E402
from gags_amd import _lib, sam_masks as SM, tilecut as TC  # noqa: E402
from gags_amd._lib import ptr  # noqa: E402


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


def rect_masks(k, h, w, seed):
    """(masks [k, h, w] bool, boxes [k, 4] (x, y, w, h) covering each rectangle): sides between 5 % and 60 % of the image."""
    g = np.random.default_rng(seed)
    masks, boxes = np.zeros((k, h, w), bool), np.zeros((k, 4), np.int32)
    for i in range(k):
        bh, bw = max(2, int(h * g.uniform(0.05, 0.6))), max(2, int(w * g.uniform(0.05, 0.6)))
        y, x = int(g.integers(0, h - bh + 1)), int(g.integers(0, w - bw + 1))
        masks[i, y:y + bh, x:x + bw] = g.random((bh, bw)) >= 0.1
        boxes[i] = (x, y, bw, bh)
    return masks, boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-tiles", type=int, default=30)
    args = ap.parse_args()
    K, H, W = args.k, args.h, args.w
    dev = torch.device("cuda")
    image = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    masks, boxes = rect_masks(K, H, W, 0)
    dimage = torch.from_numpy(image).to(dev)
    bits = torch.cat([SM.pack_masks(torch.from_numpy(masks[i:i + 50]).to(dev))[0] for i in range(0, K, 50)])
    res = {"tool": "tilecut_bench", "unit": "ms (median, min, max)", "reps": args.reps, "K": K, "H": H, "W": W,
           "device": torch.cuda.get_device_name(0), "bits_MiB": round(bits.numel() * 8 / 2 ** 20, 1),
           "mean_box_side": round(float(boxes[:, 2:].max(axis=1).mean()), 1)}

    lib = _lib.load()
    index = torch.arange(K, dtype=torch.int32, device=dev)
    dboxes = torch.from_numpy(boxes).to(dev)
    u8 = torch.empty(K, 224, 224, 3, dtype=torch.uint8, device=dev)
    f32 = torch.empty(K, 3, 224, 224, dtype=torch.float32, device=dev)

    def kernel(a, b):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.gags_tilecut(K, H, W, ptr(dimage), 0, K, ptr(bits), ptr(index), ptr(dboxes), ptr(a), ptr(b), st)
        assert rc == 0, rc
    n = K * 224 * 224 * 3
    for name, a, b, nbytes in (("f32", None, f32, 4 * n), ("u8", u8, None, n), ("both", u8, f32, 5 * n)):
        res[f"kernel_{name}_ms"] = timed(lambda: kernel(a, b), args.reps)
        res[f"kernel_{name}_written_GBps"] = round(nbytes / (res[f"kernel_{name}_ms"][0] * 1e-3) / 1e9, 1)
    res["mask_boxes_ms"] = timed(lambda: TC.mask_boxes(bits, H, W), args.reps)
    res["cut_tiles_ms"] = timed(lambda: TC.cut_tiles(dimage, bits, boxes), args.reps)

    n_host = min(args.host_tiles, K)
    t0 = time.perf_counter()
    tiles = R.tiles_ref(image, masks[:n_host], boxes[:n_host])
    host = (torch.from_numpy(tiles.astype("float32")).permute(0, 3, 1, 2) / 255.0).to(dev)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res["host_composition"] = {"tiles": n_host, "s": round(dt, 3), "ms_per_tile": round(dt / max(n_host, 1) * 1e3, 2),
                               "extrapolated_s_for_K": round(dt / max(n_host, 1) * K, 2)}
    res["same_tiles"] = bool(torch.equal(f32[:n_host], host) and np.array_equal(u8[:n_host].cpu().numpy(), tiles))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
