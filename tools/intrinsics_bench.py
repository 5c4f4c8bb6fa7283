#!/usr/bin/env python
"""The projection backward with the intrinsics' gradients (gags_project_bwd_calib) against the pose kernel and
the plain backward of the same commit, per camera model, in one process, alternating, one warm-up round of each, then the
median, minimum, 90th percentile and maximum of --reps rounds, HIP events around each call (the calls include their second
stage: the column sums of the partial rows).

Per model ("pinhole", "ortho", "fisheye", "fisheye_kb" = the fisheye with distortion coefficients) at N = 1 M, a 1920 x 1080
image, stored parameters, antialiased (RAW | AA: the variant render() runs):
  bwd     gags_project_bwd_cam                       pose    gags_project_bwd_cam, GAGS_PROJ_POSE
  calib   gags_project_bwd_calib, GAGS_PROJ_POSE     calib_frozen   the same with every scene output NULL (a frozen scene)
The comparison point is `pose`: the calib kernel is the pose kernel with eight more sums.  Prints one JSON line; no threshold.

    python tools/intrinsics_bench.py [--n 1000000] [--reps 20]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from camera_bench import DEV, H, W, scene, stats, timed  # noqa: E402
from gags_amd import _lib  # noqa: E402
from gags_amd._lib import check, ptr  # noqa: E402

COEFFS = (-0.0290, -0.0049, 0.0012, -0.0004)   # (mild: g' >= 0.66 up to 88 degrees)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("intrinsics_bench: needs a GPU (no time is reported without one)")
    lib = _lib.load()
    n = args.n
    stream = _lib.stream(torch.device(DEV, 0))
    gen = torch.Generator(device=DEV).manual_seed(0)
    rot = torch.randn(n, 4, device=DEV, generator=gen)
    slog = math.log(0.0063) + 0.5 * torch.randn(n, 3, device=DEV, generator=gen)
    logit = 1.5 * torch.randn(n, device=DEV, generator=gen)
    vm = torch.eye(4, device=DEV)
    cot = dict(m2=torch.randn(n, 2, device=DEV, generator=gen), z=torch.randn(n, device=DEV, generator=gen),
               con=torch.randn(n, 3, device=DEV, generator=gen), op=torch.randn(n, device=DEV, generator=gen))
    o = dict(radii=torch.empty(n, dtype=torch.int32, device=DEV), m2=torch.empty(n, 2, device=DEV), z=torch.empty(n, device=DEV),
             con=torch.empty(n, 3, device=DEV), tiles=torch.empty(n, dtype=torch.int32, device=DEV), op=torch.empty(n, device=DEV),
             comp=torch.empty(n, device=DEV))
    g = dict(means=torch.empty(n, 3, device=DEV), quats=torch.empty(n, 4, device=DEV), scales=torch.empty(n, 3, device=DEV),
             logit=torch.empty(n, device=DEV), vm=torch.empty(4, 4, device=DEV), K=torch.empty(9, device=DEV),
             coeffs=torch.empty(4, device=DEV))
    partials = torch.empty(lib.gags_project_calib_partials(n), _lib.GAGS_CALIB_PARTIAL_FLOATS, device=DEV)
    RAW, AA, POSE, KB = _lib.GAGS_PROJ_RAW, _lib.GAGS_PROJ_AA, _lib.GAGS_PROJ_POSE, _lib.GAGS_PROJ_KB
    row = {"tool": "intrinsics_bench", "unit": "ms", "n": n, "width": W, "height": H, "reps": args.reps, "flags": "RAW|AA",
           "models": {}}
    paths, radii, keep = {}, {}, []
    for name in ("pinhole", "ortho", "fisheye", "fisheye_kb"):
        model = name.split("_")[0]
        cam, kb = _lib.CAMERA_MODELS[model], KB if name.endswith("_kb") else 0
        means, K = scene(model, n, gen)
        if kb:
            K = torch.cat([K.reshape(9), torch.tensor(COEFFS, device=DEV)])
        check(lib.gags_project_fwd_cam(cam, RAW | AA | kb, n, ptr(means), ptr(rot), ptr(slog), ptr(logit), 1.0, ptr(vm), ptr(K), W, H,
                                       0.3, 0.01, 1e10, 0.0, ptr(o["radii"]), ptr(o["m2"]), ptr(o["z"]), ptr(o["con"]),
                                       ptr(o["tiles"]), ptr(o["op"]), None, None, None, ptr(o["comp"]), stream), "gags_project_fwd_cam")
        radii[name] = o["radii"].clone()
        keep.append((means, K))
        row["models"][name] = {"visible": int((radii[name] > 0).sum())}
        head = (n, ptr(means), ptr(rot), ptr(slog), ptr(logit), 1.0, ptr(vm), ptr(K), W, H, 0.3, ptr(radii[name]), ptr(cot["m2"]),
                ptr(cot["z"]), ptr(cot["con"]), ptr(cot["op"]), None)
        outs = (ptr(g["means"]), ptr(g["quats"]), ptr(g["scales"]), ptr(g["logit"]))

        def bwd(flags, cam=cam, kb=kb, head=head, outs=outs):
            check(lib.gags_project_bwd_cam(cam, RAW | AA | kb | flags, *head, *outs, ptr(g["vm"]), ptr(partials), partials.numel() * 4,
                                           stream), "gags_project_bwd_cam")

        def calib(outs, cam=cam, kb=kb, head=head):
            check(lib.gags_project_bwd_calib(cam, RAW | AA | kb | POSE, *head, *outs, ptr(g["vm"]), ptr(g["K"]), ptr(g["coeffs"]),
                                             ptr(partials), partials.numel() * 4, stream), "gags_project_bwd_calib")
        paths[name] = {"bwd": lambda b=bwd: b(0), "pose": lambda b=bwd: b(POSE), "calib": lambda c=calib, o_=outs: c(o_),
                       "calib_frozen": lambda c=calib: c((None, None, None, None))}
    ts = {m: {k: [] for k in p} for m, p in paths.items()}
    for rep in range(args.reps + 1):
        for m, p in paths.items():
            for k, fn in p.items():
                t = timed(fn)
                if rep:
                    ts[m][k].append(t)
    for m in ts:
        row["models"][m].update({k: stats(v) for k, v in ts[m].items()})
        row["models"][m]["calib_over_pose"] = round(row["models"][m]["calib"]["median"] / row["models"][m]["pose"]["median"], 3)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
