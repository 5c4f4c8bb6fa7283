#!/usr/bin/env python
"""Times of the query images and the loss maps (gags_amd/queryvis.py, include/gags_next.h N12) against the obvious torch
composition of the same steps on the same GPU.

  query_images  valid_map [n_phrases, 1080, 1920] -> heat map, lerf and mask composites (float and uint8) and the mask, for 1, 4
                and 16 phrases.  torch: the two box means as F.conv2d with a ones / 900 kernel over a reflect-padded map, min / max
                normalisation, the 7 x 7 majority vote as a zero-padded conv2d (its interior rule; the border rows differ from
                eval/utils.py's), LUT gathers and torch.where.
  feature_loss_maps  two [512, 1080, 1920] maps (one channel-major, one the pixel-major memory behind the decoder's permuted view;
                and both channel-major) -> three [1080, 1920] maps.  torch: compute_relvancy.py:440-446 as written.

HIP events; the two paths are timed alternately, --reps times each after a warm-up of both; median, min, max.  GB/s = the bytes
the computation must move (inputs read once, outputs written once) over the median.  Prints one JSON line.

    python tools/query_images_bench.py [--h 1080] [--w 1920] [--c 512] [--reps 20] [--loss-reps 5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from gags_amd import queryvis as QV  # noqa: E402


def timed_pair(fa, fb, reps):
    """(stats of fa, stats of fb) in ms, the two alternating."""
    fa(), fb()
    torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(reps):
        for fn, acc in ((fa, ts[0]), (fb, ts[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            del out
            acc.append(a.elapsed_time(b))
    return tuple((round(sorted(t)[len(t) // 2], 4), round(min(t), 4), round(max(t), 4)) for t in ts)


def make_valid(k, h, w, device, seed=0):
    g = torch.Generator(device=device).manual_seed(seed)
    base = F.interpolate(torch.rand(k, 1, 14, 24, generator=g, device=device), size=(h, w), mode="bicubic")[:, 0]
    return (base + 0.05 * torch.randn(k, h, w, generator=g, device=device)).clamp_(0, 1).contiguous()


def box_mean(x, box=30):
    a = box // 2
    pad = F.pad(x[:, None], (a, box - 1 - a, a, box - 1 - a), mode="reflect")
    return F.conv2d(pad, torch.full((1, 1, box, box), 1.0 / (box * box), device=x.device))[:, 0]


def torch_query_images(valid, image, thresh, lut):
    k = valid.shape[0]
    heat = 0.5 * (box_mean(valid) + valid)
    mn, mx = heat.flatten(1).amin(1)[:, None, None], heat.flatten(1).amax(1)[:, None, None]
    output = torch.clip(((heat - mn) / (mx - mn + 1e-9)) * 2 - 1, 0, 1)
    pred = (output > thresh).float()
    mask = F.conv2d(pred[:, None], torch.ones(1, 1, 7, 7, device=valid.device), padding=3)[:, 0] > 24
    heatmap = lut[(output * 255).long()]
    p = torch.clip(heat - 0.5, 0, 1)
    q = torch.clip(p / (p.flatten(1).amax(1)[:, None, None] + 1e-6), 0, 1)
    img = image[None].expand(k, -1, -1, -1)
    lerf = torch.where((heat < 0.5)[..., None], img * 0.3, lut[(q * 255).long()])
    b = torch.clip(0.5 * output + 0.5 * box_mean(output), 0, 1)
    maskc = torch.where(mask[..., None], lut[(b * 255).long()], img * 0.4 + 0.1)
    res = {"heatmap": heatmap, "lerf_composited": lerf, "mask_composited": maskc, "mask": mask.to(torch.uint8)}
    res.update({key + "_u8": QV.to_uint8(res[key]) for key in QV.IMAGE_KEYS})
    return res


def torch_loss_maps(feature, gt, mask):
    gtm, fm = gt * mask, feature * mask
    return torch.sqrt(torch.sum((gtm - fm) ** 2, dim=0)), torch.mean(torch.abs(fm), dim=0), torch.mean(torch.abs(gtm), dim=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--c", type=int, default=512)
    ap.add_argument("--phrases", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loss-reps", type=int, default=5)
    args = ap.parse_args()
    H, W, C = args.h, args.w, args.c
    if not torch.cuda.is_available():
        raise SystemExit("query_images_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda")
    res = {"tool": "query_images_bench", "unit": "ms (median, min, max)", "device": torch.cuda.get_device_name(0), "H": H, "W": W,
           "reps": args.reps, "loss_reps": args.loss_reps}
    lut = QV.turbo_lut(dev)
    image = torch.rand(H, W, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    for k in args.phrases:
        valid = make_valid(k, H, W, dev)
        hip, ref = timed_pair(lambda: QV.query_images(valid, image, thresh=0.4, return_uint8=True),
                              lambda: torch_query_images(valid, image, 0.4, lut), args.reps)
        a, b = QV.query_images(valid, image, thresh=0.4), torch_query_images(valid, image, 0.4, lut)
        # per map and pixel: valid_map in (4 B), three float RGB (36 B) and three uint8 RGB (9 B) out, the mask (1 B); the image
        # (12 B per pixel) once per frame
        nbytes = k * H * W * (4 + 36 + 9 + 1) + H * W * 12
        res[f"query_images_{k}"] = {
            "hip_ms": hip, "torch_ms": ref, "speedup": round(ref[0] / hip[0], 2), "hip_GBps_of_needed_bytes": round(nbytes / hip[0] / 1e6, 1),
            "pixels_differing": {key: float((a[key] != b[key]).any(-1).float().mean()) for key in QV.IMAGE_KEYS}}
        del valid, a, b
    torch.cuda.empty_cache()
    # loss maps
    g = torch.Generator(device=dev).manual_seed(2)
    gt = torch.randn(C, H, W, device=dev, generator=g)
    feat_cm = gt + 0.1 * torch.randn(C, H, W, device=dev, generator=g)
    mask = torch.rand(1, H, W, device=dev, generator=g) > 0.3
    nbytes = 2 * C * H * W * 4 + 4 * H * W * 4
    r = {"C": C, "needed_GB": round(nbytes / 1e9, 2)}
    hip, ref = timed_pair(lambda: QV.feature_loss_maps(feat_cm, gt, mask), lambda: torch_loss_maps(feat_cm, gt, mask), args.loss_reps)
    r["channel_major"] = {"hip_ms": hip, "torch_ms": ref, "speedup": round(ref[0] / hip[0], 2), "hip_GBps": round(nbytes / hip[0] / 1e6, 1)}
    ours, theirs = QV.feature_loss_maps(feat_cm, gt, mask), torch_loss_maps(feat_cm, gt, mask)
    r["max_abs_diff"] = [float((o - t).abs().max()) for o, t in zip(ours, theirs)]
    del theirs
    feat_pm = feat_cm.permute(1, 2, 0).contiguous().permute(2, 0, 1)   # the decoder's output layout
    del feat_cm
    torch.cuda.empty_cache()
    hip, ref = timed_pair(lambda: QV.feature_loss_maps(feat_pm, gt, mask), lambda: torch_loss_maps(feat_pm, gt, mask), args.loss_reps)
    r["pixel_major_prediction"] = {"hip_ms": hip, "torch_ms": ref, "speedup": round(ref[0] / hip[0], 2),
                                   "hip_GBps": round(nbytes / hip[0] / 1e6, 1)}
    r["layouts_bit_equal"] = all(torch.equal(o, t) for o, t in zip(ours, QV.feature_loss_maps(feat_pm, gt, mask)))
    res["feature_loss_maps"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
