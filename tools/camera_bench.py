#!/usr/bin/env python
"""Projection forward and backward under the three camera models (gags_project_fwd_cam / gags_project_bwd_cam)
in one process, alternating, one warm-up round of each, then the median, minimum, 90th percentile and maximum of --reps
rounds, HIP events around each call.  The pinhole's minimum .. 90th percentile is the run-to-run spread the other models are
read against.

Per model ("pinhole", "ortho", "fisheye") at N = 1.5 M (C3's N), a 1920 x 1080 image:
  fwd          the plain forward (activated parameters, classic)            fwd_all   RAW | AA (stored parameters, antialiased)
  bwd          the plain backward                                          bwd_all   RAW | AA | POSE (v_viewmat on the way)
The scene is drawn in the camera frame so that about the same share of Gaussians is on screen under each model (fisheye: off
axis up to 80 degrees).  Prints one JSON line; no threshold: the stage is HBM-bound (72 B per Gaussian forward) and what
atan2f and the extra divisions of the fisheye cost on it is what this tool is for.

    python tools/camera_bench.py [--n 1500000] [--reps 20]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gags_amd import _lib  # noqa: E402
from gags_amd._lib import check, ptr  # noqa: E402

DEV = "cuda"
W, H = 1920, 1080


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "p90": round(ts[(9 * len(ts)) // 10], 4),
            "max": round(ts[-1], 4)}


def scene(model, n, gen):
    """(means [N,3] in the camera frame = world frame, K) with most Gaussians on screen under `model`."""
    u = torch.rand(n, 3, device=DEV, generator=gen)
    dist = 2.0 + 10.0 * u[:, 2]
    if model == "fisheye":
        fx = fy = 0.5 * W / math.radians(80.0)
        th, ph = math.radians(80.0) * u[:, 0], 2 * math.pi * u[:, 1]
        p = dist[:, None] * torch.stack([th.sin() * ph.cos(), th.sin() * ph.sin(), th.cos()], 1)
    elif model == "ortho":
        fx = fy = W / 12.0
        p = torch.stack([(u[:, 0] - 0.5) * 1.05 * W / fx, (u[:, 1] - 0.5) * 1.05 * H / fy, dist], 1)
    else:
        fx = fy = 0.9 * W
        p = torch.stack([(u[:, 0] - 0.5) * 1.05 * W / fx * dist, (u[:, 1] - 0.5) * 1.05 * H / fy * dist, dist], 1)
    K = torch.tensor([[fx, 0, 0.5 * W], [0, fy, 0.5 * H], [0, 0, 1]], device=DEV)
    return p.contiguous(), K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_500_000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("camera_bench: needs a GPU (no time is reported without one)")
    lib = _lib.load()
    n = args.n
    stream = _lib.stream(torch.device(DEV, 0))
    gen = torch.Generator(device=DEV).manual_seed(0)
    rot = torch.randn(n, 4, device=DEV, generator=gen)
    slog = math.log(0.0063) + 0.5 * torch.randn(n, 3, device=DEV, generator=gen)
    logit = 1.5 * torch.randn(n, device=DEV, generator=gen)
    quats, scales = torch.nn.functional.normalize(rot), slog.exp()
    vm = torch.eye(4, device=DEV)
    cot = dict(m2=torch.randn(n, 2, device=DEV, generator=gen), z=torch.randn(n, device=DEV, generator=gen),
               con=torch.randn(n, 3, device=DEV, generator=gen), op=torch.randn(n, device=DEV, generator=gen))
    o = dict(radii=torch.empty(n, dtype=torch.int32, device=DEV), m2=torch.empty(n, 2, device=DEV), z=torch.empty(n, device=DEV),
             con=torch.empty(n, 3, device=DEV), tiles=torch.empty(n, dtype=torch.int32, device=DEV), op=torch.empty(n, device=DEV),
             comp=torch.empty(n, device=DEV))
    g = dict(means=torch.empty(n, 3, device=DEV), quats=torch.empty(n, 4, device=DEV), scales=torch.empty(n, 3, device=DEV),
             logit=torch.empty(n, device=DEV), vm=torch.empty(4, 4, device=DEV))
    partials = torch.empty(lib.gags_project_pose_partials(n), 12, device=DEV)
    RAW, AA, POSE = _lib.GAGS_PROJ_RAW, _lib.GAGS_PROJ_AA, _lib.GAGS_PROJ_POSE
    row = {"tool": "camera_bench", "unit": "ms", "n": n, "width": W, "height": H, "reps": args.reps, "models": {}}
    paths, keep = {}, []
    for model, cam in _lib.CAMERA_MODELS.items():
        means, K = scene(model, n, gen)
        keep.append((means, K))

        def fwd(flags, cam=cam, means=means, K=K):
            raw = flags & RAW
            check(lib.gags_project_fwd_cam(cam, flags, n, ptr(means), ptr(rot if raw else quats), ptr(slog if raw else scales),
                                           ptr(logit), 1.0, ptr(vm), ptr(K), W, H, 0.3, 0.01, 1e10, 0.0, ptr(o["radii"]),
                                           ptr(o["m2"]), ptr(o["z"]), ptr(o["con"]), ptr(o["tiles"]), ptr(o["op"]), None, None,
                                           None, ptr(o["comp"]), stream), "gags_project_fwd_cam")

        def bwd(flags, cam=cam, means=means, K=K):
            raw = flags & RAW
            check(lib.gags_project_bwd_cam(cam, flags, n, ptr(means), ptr(rot if raw else quats), ptr(slog if raw else scales),
                                           ptr(logit), 1.0, ptr(vm), ptr(K), W, H, 0.3, ptr(o["radii"]), ptr(cot["m2"]),
                                           ptr(cot["z"]), ptr(cot["con"]), ptr(cot["op"]), None, ptr(g["means"]), ptr(g["quats"]),
                                           ptr(g["scales"]), ptr(g["logit"]), ptr(g["vm"]), ptr(partials), partials.numel() * 4,
                                           stream), "gags_project_bwd_cam")
        # (each backward follows a forward of its own model, which leaves that model's radii in place)
        paths[model] = {"fwd": lambda f=fwd: f(0), "bwd": lambda b=bwd: b(0), "fwd_all": lambda f=fwd: f(RAW | AA),
                        "bwd_all": lambda b=bwd: b(RAW | AA | POSE)}
    ts = {m: {k: [] for k in p} for m, p in paths.items()}
    for rep in range(args.reps + 1):
        for m, p in paths.items():
            for k, fn in p.items():
                t = timed(fn)
                if rep:
                    ts[m][k].append(t)
            if rep == 0:
                row["models"][m] = {"visible": int((o["radii"] > 0).sum())}
    for m in ts:
        row["models"][m].update({k: stats(v) for k, v in ts[m].items()})
    for m in ("ortho", "fisheye"):
        row["models"][m]["median_over_pinhole"] = {k: round(row["models"][m][k]["median"] / row["models"]["pinhole"][k]["median"], 3)
                                                   for k in ("fwd", "bwd", "fwd_all", "bwd_all")}
    print(json.dumps(row))


if __name__ == "__main__":
    main()
