#!/usr/bin/env python
"""MCMC density control (gags_amd/mcmc.py, include/gags_next.h N18) against the torch composition of the same rules -- the only
baseline there is -- in one process, alternating, one warm-up round of each, then the median, minimum and maximum of --reps
rounds, HIP events around each call.

Two workloads at N = 1.5 M (C3's N), sh_degree 3, D = 16, all seven tensors with both Adam moments:
  * noise:      the per-step position noise (R5) with given normal draws: one launch against about twenty element-wise passes and
                two batched matrix products.  GB/s against the 68 bytes per Gaussian the rule has to move.
  * refinement: relocate (about 5 % dead) then sample_add (5 % growth) with given uniforms.  The composition samples with
                cumsum / searchsorted / bincount, evaluates the relocation rule in float64 through a [52, 51] coefficient table
                (one gather and one row sum per source), copies rows by index assignment and grows by torch.cat.
Both paths see the same inputs; the draws must agree exactly and the values to float32 rounding, or the tool stops.
Prints one JSON line.

    python tools/mcmc_bench.py [--n 1500000] [--reps 20] [--refine-reps 10]"""
import argparse
import json
import math
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gags_amd import densify, mcmc  # noqa: E402
from gags_amd.scene import GaussianModel  # noqa: E402

DEV = "cuda"
ATTR = dict(densify.GROUPS)
ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016,
                             position_lr_delay_mult=0.01, position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05,
                             scaling_lr=0.005, rotation_lr=0.001, semantic_feature_lr=0.001)
MIN_OPACITY, TOP = 0.005, 1.0 - 2.0 ** -23


def make_scene(n, d, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    op = torch.where(torch.rand(n, 1, device=DEV, generator=g) < 0.05, -7.0, 0.0) + torch.randn(n, 1, device=DEV, generator=g).clamp(-2, 4)
    t = {"xyz": torch.randn(n, 3, device=DEV, generator=g), "f_dc": torch.randn(n, 1, 3, device=DEV, generator=g),
         "f_rest": torch.randn(n, 15, 3, device=DEV, generator=g), "opacity": op.contiguous(),
         "scaling": (math.log(0.03) + 0.5 * torch.randn(n, 3, device=DEV, generator=g)).contiguous(),
         "rotation": torch.randn(n, 4, device=DEV, generator=g), "semantic_feature": torch.randn(n, d, device=DEV, generator=g)}
    mom = {k: (torch.randn_like(v), torch.rand_like(v)) for k, v in t.items()}
    return t, mom


def fresh_model(t, mom):
    """A model over COPIES of the tensors (a relocation writes in place)."""
    c = {k: v.clone() for k, v in t.items()}
    m = GaussianModel.from_tensors(c["xyz"], c["scaling"], c["rotation"], c["opacity"], c["f_dc"], c["f_rest"],
                                   c["semantic_feature"], sh_degree=3)
    m.training_setup_rgb(ARGS)
    for grp in m.optimizer.param_groups:
        m.optimizer.state[grp["params"][0]] = {"step": torch.tensor(3.0), "exp_avg": mom[grp["name"]][0].clone(),
                                               "exp_avg_sq": mom[grp["name"]][1].clone()}
    return m


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4)}


# ---- the torch composition ------------------------------------------------------------------------------------------------
def torch_noise(xyz, op, sc, rot, z, scaler):
    o = torch.sigmoid(op).reshape(-1)
    gate = 1.0 / (1.0 + torch.exp(-100.0 * ((1.0 - o) - 0.995)))
    q = torch.nn.functional.normalize(rot)
    r, x, y, zq = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + zq * zq), 2 * (x * y - r * zq), 2 * (x * zq + r * y),
                     2 * (x * y + r * zq), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - r * x),
                     2 * (x * zq - r * y), 2 * (y * zq + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * torch.exp(sc)[:, None, :]
    cov = torch.bmm(M, M.transpose(1, 2))
    xyz.add_(torch.bmm(cov, (z * gate[:, None] * scaler)[:, :, None]).squeeze(-1))


def coefficient_table():
    """A[r, k] = sum_{i = 1..r} C(i-1, k) (-1)^k / sqrt(k + 1): denom = sum_k A[r, k] o_new^(k+1)."""
    A = torch.zeros(52, 51, dtype=torch.float64)
    for r in range(1, 52):
        A[r] = A[r - 1]
        for k in range(r):
            A[r, k] += math.comb(r - 1, k) * (-1.0) ** k / math.sqrt(k + 1)
    return A.to(DEV)


def torch_values(op, sc, rows, ratio, A):
    x = op[rows, 0].double()
    o = torch.sigmoid(x).clamp(max=TOP)
    r = ratio.clamp(1, 51)
    o_new = -torch.expm1(torch.log1p(-o) / r)
    den = (A[r] * o_new[:, None] ** torch.arange(1, 52, device=DEV)).sum(1)
    c = o_new.clamp(MIN_OPACITY, TOP)
    op[rows, 0] = torch.log(c / (1 - c)).float()
    sc[rows] = (sc[rows].double() + torch.log(o / den)[:, None]).float()


def torch_sample(w, u):
    cdf = torch.cumsum(w, 0)
    draws = torch.searchsorted(cdf, u * cdf[-1], right=True).clamp(max=w.numel() - 1)
    return draws, torch.bincount(draws, minlength=w.numel())


def torch_refinement(t, mom, u_dead, u_add, cap_max, A):
    t = {k: v.clone() for k, v in t.items()}
    mom = {k: (a.clone(), b.clone()) for k, (a, b) in mom.items()}

    def run():
        op, sc = t["opacity"], t["scaling"]
        dead = torch.sigmoid(op).reshape(-1) <= MIN_OPACITY
        dead_rows = torch.nonzero(dead).reshape(-1)
        draws, counts = torch_sample(torch.sigmoid(op.reshape(-1).double()).masked_fill(dead, 0.0), u_dead[:dead_rows.numel()])
        src = torch.nonzero(counts).reshape(-1)
        torch_values(op, sc, src, counts[src] + 1, A)
        for k in t:
            t[k][dead_rows] = t[k][draws]
            mom[k][0][src] = 0
            mom[k][1][src] = 0
        n = op.shape[0]
        n_add = max(0, min(cap_max, int(1.05 * n)) - n)
        draws2, counts2 = torch_sample(torch.sigmoid(op.reshape(-1).double()), u_add[:n_add])
        src = torch.nonzero(counts2).reshape(-1)
        torch_values(op, sc, src, counts2[src] + 1, A)
        for k in t:
            t[k] = torch.cat([t[k], t[k][draws2]])
            mom[k] = tuple(torch.cat([a, torch.zeros_like(a[:n_add])]) for a in mom[k])
        return t, draws, draws2
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_500_000)
    ap.add_argument("--d", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--refine-reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mcmc_bench: needs a GPU (no time is reported without one)")
    n = args.n
    t, mom = make_scene(n, args.d)
    row = {"tool": "mcmc_bench", "unit": "ms", "n": n, "d": args.d, "reps": args.reps, "refine_reps": args.refine_reps}
    # ---- the position noise ----------------------------------------------------------------------------------------------
    z = torch.randn(n, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    scaler = 1.6e-4 * 5e5
    holder = types.SimpleNamespace(_xyz=t["xyz"].clone(), _opacity=t["opacity"], _scaling=t["scaling"], _rotation=t["rotation"],
                                   invalidate_activations=lambda: None)
    xyz_t = t["xyz"].clone()
    paths = {"fused": lambda: mcmc.inject_noise(holder, scaler, noise=z),
             "torch": lambda: torch_noise(xyz_t, t["opacity"], t["scaling"], t["rotation"], z, scaler)}
    for fn in paths.values():
        fn()
    err = float((holder._xyz - xyz_t).abs().max())
    row["noise_max_abs_difference"] = err
    assert err <= 1e-3 * float(xyz_t.abs().max()), err
    ts = {k: [] for k in paths}
    for _ in range(args.reps):
        for k, fn in paths.items():
            ts[k].append(timed(fn)[0])
    for k in paths:
        row[f"noise_{k}_ms"] = stats(ts[k])
    row["noise_fused_GBps"] = round(68 * n / (row["noise_fused_ms"]["median"] * 1e-3) / 1e9, 1)
    row["noise_speedup_median"] = round(row["noise_torch_ms"]["median"] / row["noise_fused_ms"]["median"], 2)
    del holder, xyz_t
    # ---- one refinement --------------------------------------------------------------------------------------------------
    g = torch.Generator(device=DEV).manual_seed(2)
    u_dead = torch.rand(n, dtype=torch.float64, device=DEV, generator=g)
    u_add = torch.rand(n, dtype=torch.float64, device=DEV, generator=g)
    cap_max = 10 * n
    A = coefficient_table()
    n_dead = int((torch.sigmoid(t["opacity"]) <= MIN_OPACITY).sum())
    n_add = int(1.05 * n) - n

    def fused(m):
        def run():
            a = mcmc.relocate(m, None, MIN_OPACITY, uniforms=u_dead[:n_dead])
            b = mcmc.sample_add(m, cap_max, MIN_OPACITY, uniforms=u_add[:n_add])
            return a, b
        return run

    ts = {"fused": [], "torch": []}
    out = {}
    for r in range(args.refine_reps + 1):  # round 0 warms up
        for k in ts:
            fn = fused(fresh_model(t, mom)) if k == "fused" else torch_refinement(t, mom, u_dead, u_add, cap_max, A)
            torch.cuda.synchronize()
            ms, res = timed(fn)
            if r:
                ts[k].append(ms)
            if r == args.refine_reps:
                out[k] = res
            del fn, res
    assert out["fused"] == (n_dead, n_add), out["fused"]
    assert out["torch"][0]["xyz"].shape[0] == n + n_add
    row.update(n_dead=n_dead, n_added=n_add)
    for k in ts:
        row[f"refinement_{k}_ms"] = stats(ts[k])
    row["refinement_speedup_median"] = round(row["refinement_torch_ms"]["median"] / row["refinement_fused_ms"]["median"], 2)
    del out
    # ---- the two paths agree: one more pair, compared ----------------------------------------------------------------------
    m = fresh_model(t, mom)
    fused(m)()
    tt, _, _ = torch_refinement(t, mom, u_dead, u_add, cap_max, A)()
    same_rows = all(torch.equal(getattr(m, ATTR[k]).detach(), tt[k]) for k in ("xyz", "f_dc", "f_rest", "rotation", "semantic_feature"))
    row["copied_rows_equal"] = bool(same_rows)
    row["values_max_abs_difference"] = max(float((m._opacity.detach() - tt["opacity"]).abs().max()),
                                           float((m._scaling.detach() - tt["scaling"]).abs().max()))
    assert same_rows and row["values_max_abs_difference"] <= 1e-5, row
    print(json.dumps(row))


if __name__ == "__main__":
    main()
