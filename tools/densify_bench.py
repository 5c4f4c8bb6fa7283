#!/usr/bin/env python
"""Adaptive density control (gags_amd/densify.py, include/gags_next.h N8) against the torch composition of the same rule,
tests/densify_ref.py run on the device -- the only baseline there is -- in one process, alternating, one warm-up round of each,
then the median and minimum of --reps (>= 20) rounds, HIP events around each call.

Two workloads per size (N = 1.5 M and 4 M, sh_degree 3, D = 16; --wide adds N = 4 M, D = 512 with a single round):
  * stats:   the per-step statistics of one view (accum, denom, max_radii2D), about 60 % of the Gaussians visible;
  * densify: a whole densify_and_prune with about 5 % cloned, 5 % split and 2 % pruned, all seven tensors with both Adam moments.
Reported for each path: time, kernel launches and host synchronisations of one round (torch profiler; torch's sync debug mode:
it sees torch's own waits, which is where both paths have theirs), torch.cuda.max_memory_allocated of one round, and for the
fused densify the GB/s against the bytes the gather has to move: every output row written once for the tensor and both
moments, every copied row read once (moments: kept rows only), computed from the shapes.  Prints one JSON line.

    python tools/densify_bench.py [--sizes 1500000,4000000] [--reps 20] [--wide] [--no-count]"""
import argparse
import json
import os
import sys
import types
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import densify_ref as R  # noqa: E402
from gags_amd import densify  # noqa: E402
from gags_amd.scene import GaussianModel  # noqa: E402

DEV = "cuda"
ATTR = dict(densify.GROUPS)
ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016,
                             position_lr_delay_mult=0.01, position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05,
                             scaling_lr=0.005, rotation_lr=0.001, semantic_feature_lr=0.001)
MAX_GRAD, MIN_OPACITY, EXTENT, MSS = 0.0002, 0.005, 10.0, 20


def make_scene(n, d, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    u = torch.rand(n, device=DEV, generator=g)
    moving = u < 0.10                                           # 5 % small (cloned) + 5 % medium (split)
    medium = torch.rand(n, device=DEV, generator=g) < 0.5
    scale = torch.where(medium, 0.3, 0.03)
    t = {"xyz": torch.randn(n, 3, device=DEV, generator=g), "f_dc": torch.randn(n, 1, 3, device=DEV, generator=g),
         "f_rest": torch.randn(n, 15, 3, device=DEV, generator=g),
         "opacity": torch.where(torch.rand(n, 1, device=DEV, generator=g) < 0.02, -7.0, 1.0),
         "scaling": (scale.log()[:, None] + torch.log(0.3 + 0.7 * torch.rand(n, 3, device=DEV, generator=g))).contiguous(),
         "rotation": torch.randn(n, 4, device=DEV, generator=g), "semantic_feature": torch.randn(n, d, device=DEV, generator=g)}
    mom = {k: (torch.randn_like(v), torch.rand_like(v)) for k, v in t.items()}
    accum = torch.where(moving, 5 * MAX_GRAD, 0.2 * MAX_GRAD)[:, None].contiguous()
    denom = torch.ones(n, 1, device=DEV)
    view = {"grad": 1e-3 * torch.randn(1, n, 2, device=DEV, generator=g),
            "radii": torch.where(torch.rand(n, device=DEV, generator=g) < 0.6, torch.randint(1, 40, (n,), device=DEV, generator=g), 0).int()}
    return t, mom, accum, denom, view


def fresh_model(t, mom, accum, denom):
    """A model over the SHARED tensors (the gather reads them and replaces the model's attributes; nothing is written)."""
    m = GaussianModel.from_tensors(t["xyz"], t["scaling"], t["rotation"], t["opacity"], t["f_dc"], t["f_rest"],
                                   t["semantic_feature"], sh_degree=3)
    m.training_setup_rgb(ARGS)
    for grp in m.optimizer.param_groups:
        m.optimizer.state[grp["params"][0]] = {"step": torch.tensor(3.0), "exp_avg": mom[grp["name"]][0],
                                               "exp_avg_sq": mom[grp["name"]][1]}
    m.xyz_gradient_accum, m.denom = accum, denom
    return m


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def count(fn):
    """(kernel launches, host synchronisations torch reports, peak bytes) of one call."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode(1)
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                out = fn()
                torch.cuda.set_sync_debug_mode(0)
                torch.cuda.synchronize()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    peak = torch.cuda.max_memory_allocated() - base
    del out
    launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                   and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    return launches, sum(1 for x in w if "synchroniz" in str(x.message).lower()), peak


def stats(ts):
    ts = sorted(ts)
    return round(ts[len(ts) // 2], 4), round(ts[0], 4)


def gather_bytes(t, n_out, n_keep):
    b = 0
    for v in t.values():
        row = v[0].numel() * 4
        b += 2 * n_out * row                  # the tensor: one read and one write per output row
        b += 2 * (n_out * row + n_keep * row)  # both moments: written in full, read for kept rows
    return b


def bench(n, d, reps, counting):
    t, mom, accum, denom, view = make_scene(n, d)
    row = {"n": n, "d": d, "reps": reps}
    # ---- the per-step statistics -------------------------------------------------------------------------------------
    vis = view["radii"] > 0
    holder = types.SimpleNamespace(_xyz=t["xyz"], xyz_gradient_accum=torch.zeros(n, 1, device=DEV),
                                   denom=torch.zeros(n, 1, device=DEV), max_radii2D=torch.zeros(n, device=DEV))
    ref_state = [torch.zeros(n, 1, device=DEV), torch.zeros(n, 1, device=DEV), torch.zeros(n, device=DEV)]

    def fused_stats():
        densify.stats(holder, view["grad"], view["radii"], None, None, 1920, 1080)

    def torch_stats():
        ref_state[:] = R.add_stats(ref_state[0], ref_state[1], ref_state[2], view["grad"][0], view["radii"], vis, vis, 1920, 1080)

    paths = {"fused": fused_stats, "torch": torch_stats}
    ts = {k: [] for k in paths}
    for fn in paths.values():
        fn()
    for _ in range(reps):
        for k, fn in paths.items():
            ts[k].append(timed(fn)[0])
    for k in paths:
        row[f"stats_{k}_ms_median"], row[f"stats_{k}_ms_min"] = stats(ts[k])
        if counting:
            row[f"stats_{k}_launches"], row[f"stats_{k}_syncs"], row[f"stats_{k}_peak_MB"] = count(paths[k])
            row[f"stats_{k}_peak_MB"] = round(row[f"stats_{k}_peak_MB"] / 2 ** 20, 1)
    assert torch.equal(holder.denom, ref_state[1]) and torch.equal(holder.max_radii2D, ref_state[2])
    # ---- a whole densify_and_prune -----------------------------------------------------------------------------------
    flags = R.decide(accum, denom, t["scaling"], t["opacity"], 0.01, MAX_GRAD, MIN_OPACITY, EXTENT, MSS)
    n_split = int(flags[2].sum())
    zs = torch.randn(2 * n_split, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    row.update(clone_pct=round(100 * int(flags[1].sum()) / n, 2), split_pct=round(100 * n_split / n, 2),
               pruned_pct=round(100 * (n - int(flags[0].sum()) - n_split) / n, 2))
    models = []

    def fused_densify():
        m = models.pop()
        return m, densify.densify_and_prune(m, MAX_GRAD, MIN_OPACITY, EXTENT, MSS, samples=zs)

    def torch_densify():
        return R.densify_and_prune(t, accum, denom, 0.01, MAX_GRAD, MIN_OPACITY, EXTENT, MSS, zs, moments=mom)

    paths = {"fused": fused_densify, "torch": torch_densify}
    ts = {k: [] for k in paths}
    out = {}
    for r in range(reps + 1):  # round 0 warms up
        for k, fn in paths.items():
            models.append(fresh_model(t, mom, accum, denom))
            ms, out[k] = timed(fn)
            if r:
                ts[k].append(ms)
            if r < reps:
                out[k] = None
    m, plan = out["fused"]
    ref = out["torch"]
    assert torch.equal(plan.src.long(), ref["src"]) and all(torch.equal(getattr(m, a).detach()[:plan.first_child],
                                                                        ref[k][:plan.first_child]) for k, a in ATTR.items())
    nbytes = gather_bytes(t, plan.n_out, plan.n_keep)
    row.update(n_out=plan.n_out, gather_GB=round(nbytes / 1e9, 3))
    del out, m, ref
    for k in paths:
        row[f"densify_{k}_ms_median"], row[f"densify_{k}_ms_min"] = stats(ts[k])
        if counting:
            models.append(fresh_model(t, mom, accum, denom))
            la, sy, pk = count(paths[k])
            row[f"densify_{k}_launches"], row[f"densify_{k}_syncs"], row[f"densify_{k}_peak_GB"] = la, sy, round(pk / 1e9, 3)
    row["densify_fused_GBps"] = round(nbytes / (row["densify_fused_ms_median"] * 1e-3) / 1e9, 1)
    row["densify_speedup_median"] = round(row["densify_torch_ms_median"] / row["densify_fused_ms_median"], 2)
    row["stats_speedup_median"] = round(row["stats_torch_ms_median"] / row["stats_fused_ms_median"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1500000,4000000")
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--wide", action="store_true", help="also N = 4 M, D = 512, one round")
    ap.add_argument("--no-count", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("densify_bench: needs a GPU (no time is reported without one)")
    if args.reps < 20:
        raise SystemExit("densify_bench: at least 20 rounds")
    res = {"tool": "densify_bench", "unit": "ms", "runs": []}
    jobs = [(int(s), args.d, args.reps) for s in args.sizes.split(",") if s] + ([(4_000_000, 512, 1)] if args.wide else [])
    for n, d, reps in jobs:
        row = bench(n, d, reps, not args.no_count)
        res["runs"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
