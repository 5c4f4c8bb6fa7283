#!/usr/bin/env python
"""Stage times of depth_SAM's point-to-pixel min-depth mapping (gags_amd/depthsample.py, include/gags_next.h N6) on
synthetic Gaussians (gags_amd.synthetic) seen by C cameras of 1920 x 1080 spread around the cloud (yaw +-40 degrees,
small pitch): the ED depth render of all cameras, the map pass (min depth only), the scatter pass (winner maps + finalise),
and the map pass with the dense mapping [N, C, 2] / visible [N, C] outputs.  HIP events, median of --reps runs after one
warm-up.  Gathers/s = N C decisions per second.  Algorithmic bytes: map = xyz (12 N) + one 4-byte depth read per inside
decision + min_depth (4 N); scatter = xyz per camera (12 N C) + one 4-byte depth read per inside decision + the winner
maps' memset, atomics and finalise reads (8 C H W) + samples (4 C H W) + the winners' min_depth gather; dense adds 9 N C.
Also the float32 restatement's host time per camera (tests/depthsample_ref.py, numpy) on --host-cams cameras, labelled
as such and not extrapolated.  Prints one JSON line.

--camera-model (N22) gives every camera that model through gags_rig_depth_map / _scatter, the entries the package calls for
every rig: "pinhole" (the default: the N6 kernels), "ortho" (137 px per unit), "fisheye" (0.9 W px per radian) or "kb" (that
fisheye with the distortion coefficients of set A of tests/fisheye_kb_ref.py).

    python tools/depthsample_bench.py [--n 1500000,4000000] [--cams 100,300] [--reps 5] [--host-cams 2]
                                      [--camera-model {pinhole,ortho,fisheye,kb}]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gags_amd import depthsample as DS  # noqa: E402
from gags_amd import synthetic as syn  # noqa: E402
from gags_amd.scene import Camera  # noqa: E402


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
    return round(ts[len(ts) // 2], 3)


KB_A = (-0.0290, -0.0049, 0.0012, -0.0004)


def cameras(c, w=1920, h=1080, model="pinhole"):
    """c cameras at the origin looking into the synthetic frustum, yaw in [-40, 40] degrees, pitch in [-10, 10]."""
    base = syn.make_camera(w, h)
    kw = {}
    if model == "ortho":
        kw = dict(camera_model="ortho", K=np.array([[137.0, 0, w / 2], [0, 137.0, h / 2], [0, 0, 1]], np.float32))
    elif model in ("fisheye", "kb"):
        kw = dict(camera_model="fisheye", K=np.array([[0.9 * w, 0, w / 2], [0, 0.9 * w, h / 2], [0, 0, 1]], np.float32))
        if model == "kb":
            kw["radial_coeffs"] = KB_A
    out = []
    for k in range(c):
        yaw = math.radians(-40 + 80 * k / max(c - 1, 1))
        pitch = math.radians(10 * math.sin(0.7 * k))
        cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
        Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
        out.append(Camera(Ry @ Rx, np.zeros(3), base.FoVx, base.FoVy, w, h, uid=k, **kw))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1500000,4000000")
    ap.add_argument("--cams", default="100,300")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-cams", type=int, default=2)
    ap.add_argument("--camera-model", default="pinhole", choices=("pinhole", "ortho", "fisheye", "kb"))
    args = ap.parse_args()
    res = {"tool": "depthsample_bench", "unit": "ms", "reps": args.reps, "width": 1920, "height": 1080,
           "camera_model": args.camera_model, "runs": []}
    bg = torch.zeros(3, device="cuda")
    for n in [int(v) for v in args.n.split(",")]:
        model = syn.make_model(n, 0, 1920, 1080, seed=0, device="cuda", gen_device="cuda")
        xyz = model.get_xyz.contiguous()
        for c in [int(v) for v in args.cams.split(",")]:
            cams = cameras(c, model=args.camera_model)
            vm, K, models, coeffs, (h, w) = DS.camera_rig(cams)
            rig = {} if args.camera_model == "pinhole" else dict(camera_models=models, radial_coeffs=coeffs)
            ids, _ = DS._rig(rig.get("camera_models"), coeffs if rig else None, depths=None)
            t_render = timed(lambda: DS.render_depths(model, cams, bg), max(1, min(args.reps, 3)))
            depths = DS.render_depths(model, cams, bg)
            t_map = timed(lambda: DS.point_min_depth(xyz, vm, K, depths, **rig), args.reps)
            md = DS.point_min_depth(xyz, vm, K, depths, **rig)
            lib = DS._lib.load()
            samples = torch.empty(c, h, w, device="cuda")
            scratch, nb = DS._scratch(lib, n, c, h, w, xyz.device)

            def scatter():
                DS.check(lib.gags_rig_depth_scatter(n, c, h, w, DS.ptr(xyz), DS.ptr(vm), DS.ptr(K), ids,
                                                    DS.ptr(coeffs if rig else None), DS.ptr(depths), 0.25, 0, DS.ptr(md),
                                                    DS.ptr(samples), DS.ptr(scratch), nb, DS._lib.stream()),
                         "scatter")
            t_scatter = timed(scatter, args.reps)
            row = {"n": n, "cams": c, "render_ms": t_render, "map_ms": t_map, "scatter_ms": t_scatter}
            dense_bytes = 9 * n * c
            if dense_bytes < 24 << 30:
                t_dense = timed(lambda: DS.point_pixel_mapping(xyz, vm, K, depths, **rig), args.reps)
                mapping, visible = DS.point_pixel_mapping(xyz, vm, K, depths, **rig)
                inside_vis = int(visible.sum())
                del mapping
                row["dense_ms"] = t_dense
                row["visible_frac"] = round(inside_vis / (n * c), 4)
                del visible
            torch.cuda.empty_cache()
            dec = n * c
            row["map_gathers_per_s"] = round(dec / (t_map * 1e-3) / 1e9, 2)
            row["scatter_gathers_per_s"] = round(dec / (t_scatter * 1e-3) / 1e9, 2)
            row["unit_gathers"] = "1e9/s"
            # algorithmic bytes (inside decisions bounded above by all decisions: upper bound of the depth reads)
            map_bytes = 12 * n + 4 * dec + 4 * n
            scat_bytes = 12 * dec + 4 * dec + 16 * c * h * w + 4 * c * h * w
            row["map_GBps_alg_upper"] = round(map_bytes / (t_map * 1e-3) / 1e9, 1)
            row["scatter_GBps_alg_upper"] = round(scat_bytes / (t_scatter * 1e-3) / 1e9, 1)
            if "dense_ms" in row:
                row["dense_GBps_alg_upper"] = round((map_bytes + 9 * dec) / (row["dense_ms"] * 1e-3) / 1e9, 1)
            res["runs"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del depths, samples, scratch, md
            torch.cuda.empty_cache()
        # the float32 restatement on the host, per camera, on a few cameras (not extrapolated)
        if args.host_cams > 0 and args.camera_model == "pinhole":
            import depthsample_ref as R
            cams = cameras(args.host_cams)
            vm, K, _, _, _ = DS.camera_rig(cams)
            depths = DS.render_depths(model, cams, bg).cpu().numpy()
            X, VM, KK = xyz.cpu().numpy(), vm.cpu().numpy(), K.cpu().numpy()
            t0 = time.perf_counter()
            R.depth_sample(X, VM, KK, depths)
            res.setdefault("host_restatement_ms_per_cam", {})[str(n)] = round((time.perf_counter() - t0) * 1e3 / args.host_cams, 1)
        del model, xyz
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
