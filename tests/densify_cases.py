"""Inputs of the adaptive-density-control tests (N8): the case builder tests/golden/make_golden_densify.py feeds the reference
with, and the margin condition on those inputs -- every decision quantity that is not a built tie lies at least MARGIN
(relative, float64) from its threshold, so a last-bit difference between two exp / sigmoid implementations cannot flip a
decision.  Plain numpy; shared by the fixture generator and tests/test_densify_gpu.py (random scenes at sizes the fixture does
not hold)."""
import numpy as np

MARGIN = 1e-3


def logit(p):
    return np.log(p / (1 - p))


def build_case(rng, n, sh_degree, d, extent, max_grad, mss, kind):
    """float32 inputs of one case.  kind: mixed | none | allpruned | allsplit | tie_dense | tie_world."""
    pd, min_op = 0.01, 0.005
    dense_thr, world_thr = pd * extent, 0.1 * extent
    pick = lambda *v: rng.choice(np.array(v), n)  # noqa: E731
    # world size m = max exp(s): small (clone side), medium (split side), parent above / children below 0.1 extent, huge
    cls = {"mixed": pick(0, 0, 1, 1, 2, 3), "none": pick(0, 1), "allpruned": pick(0, 1), "allsplit": np.ones(n, int),
           "tie_dense": pick(0, 1), "tie_world": pick(0, 1, 2, 3)}[kind]
    lo = np.array([0.1 * dense_thr, 1.5 * dense_thr, 1.05 * world_thr, 1.8 * world_thr])[cls]
    hi = np.array([0.8 * dense_thr, 6.0 * dense_thr, 1.50 * world_thr, 3.0 * world_thr])[cls]
    m = rng.uniform(lo, hi)
    s = np.log(m)[:, None] + np.log(rng.uniform(0.2, 1.0, (n, 3)))
    s[np.arange(n), rng.integers(0, 3, n)] = np.log(m)
    # gradient average: far below or above the threshold; 0/0, x/0, negative accum
    denom = rng.integers(1, 6, n).astype(np.float64)
    g = np.where(rng.random(n) < 0.5, rng.uniform(0.05, 0.5, n), rng.uniform(2.0, 9.0, n)) * max_grad
    if kind == "none":
        g = rng.uniform(0.05, 0.5, n) * max_grad
    if kind == "allsplit":
        g = rng.uniform(2.0, 9.0, n) * max_grad
    accum = g * denom
    op = np.where(rng.random(n) < 0.15, rng.uniform(0.0005, 0.004, n), rng.uniform(0.01, 0.95, n))
    if kind in ("none", "allsplit"):
        op = rng.uniform(0.01, 0.95, n)
    if kind == "allpruned":
        op = rng.uniform(0.0005, 0.004, n)
    if kind == "mixed":
        accum[3], denom[3] = 0.0, 0.0          # 0 / 0 -> NaN -> 0
        accum[4], denom[4] = 2.0 * max_grad, 0.0  # x / 0 = inf: selected
        accum[5] = -7.0 * max_grad * denom[5]  # negative: clones (|g|), never splits
        accum[6] = -7.0 * max_grad * denom[6]
        s[5] = np.log(0.3 * dense_thr)          # ... on the clone side
        s[6] = np.log(3.0 * dense_thr)          # ... on the split side: nothing happens
        op[3:7] = 0.5
    if kind == "tie_dense":  # exp(0) = 1 against 0.01 * 100; accum / denom == max_grad
        assert pd * extent == 1.0 and max_grad == 0.25
        s[:12] = 0.0
        accum[:12] = rng.uniform(2.0, 9.0, 12) * max_grad * denom[:12]
        accum[12:24], denom[12:24] = 0.5, 2.0
        op[:24] = 0.5
    if kind == "tie_world":  # exp(0) = 1 against 0.1 * 10
        assert 0.1 * extent == 1.0
        s[:12] = 0.0
        op[:12] = 0.5
    quat = rng.standard_normal((n, 4))
    quat *= (rng.choice(np.array([0.3, 1.0, 7.0]), n) / np.linalg.norm(quat, axis=1))[:, None]
    k = (sh_degree + 1) ** 2 - 1
    t = {"xyz": rng.uniform(-3, 3, (n, 3)), "f_dc": rng.standard_normal((n, 1, 3)), "f_rest": rng.standard_normal((n, k, 3)),
         "opacity": logit(op)[:, None], "scaling": s, "rotation": quat, "semantic_feature": rng.standard_normal((n, d))}
    t = {k_: v.astype(np.float32) for k_, v in t.items()}
    max_radii = rng.uniform(0, 80, n).astype(np.float32)  # large stored radii: zeroed before they are read
    par = dict(percent_dense=pd, max_grad=max_grad, min_opacity=min_op, extent=extent, mss=mss, sh_degree=sh_degree)
    return t, accum.astype(np.float32)[:, None], denom.astype(np.float32)[:, None], max_radii, par


def check_margin(t, accum, denom, par, ties_allowed):
    """Every decision quantity at least MARGIN (relative) from its threshold in float64, or exactly on it (built ties)."""
    with np.errstate(all="ignore"):
        g = accum.astype(np.float64).ravel() / denom.astype(np.float64).ravel()
    g = np.where(np.isnan(g), 0.0, g)
    m = np.exp(t["scaling"].astype(np.float64)).max(1)
    o = 1 / (1 + np.exp(-t["opacity"].astype(np.float64).ravel()))
    ties = 0
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    for q, thr in ((np.abs(g), par["max_grad"]), (g, par["max_grad"]), (m, par["percent_dense"] * par["extent"]),
                   (m, 0.1 * par["extent"]), (m / 1.6, 0.1 * par["extent"]), (o, par["min_opacity"])):
        for th in (thr, f32(thr)):
            dist = np.abs(q - th) / abs(th)
            on = (q == th)
            ties += int(on.sum())
            assert np.all((dist >= MARGIN) | on | ~np.isfinite(q)), (thr, np.sort(dist)[:3])
    assert ties_allowed or ties == 0, ties
    return ties
