"""N18 on the GPU: MCMC density control (gags_amd/mcmc.py, csrc/mcmc.hip) against the numpy restatement tests/mcmc_ref.py.

EXACT (bit for bit): draws and counts (against the restatement run on the device's own cdf), every copied row, the moments, `step`,
the untouched rows, the statistics, determinism.  BY TOLERANCE, each printed next to its bound: the cdf (1e-12 relative of
numpy's), the relocation values (one float32 ulp of the float64 restatement), the noise and the regularisers (max(4 x the float32
numpy run's own distance from the float64 run, one float32 ulp of the array's largest magnitude): both terms come from the
reference runs).  DESIGN.md section 7 "N18" records the printed values.
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mcmc_ref as R  # noqa: E402

DEV = torch.device("cuda", 0)
ATTR = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling",
            rotation="_rotation", semantic_feature="_semantic_feature")
ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016,
                             position_lr_delay_mult=0.01, position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05,
                             scaling_lr=0.005, rotation_lr=0.001, semantic_feature_lr=0.001)
MIN_OPACITY = 0.005


def _logit(o):
    return float(np.log(o / (1.0 - o)))


def _ulp32(a):
    return np.spacing(np.abs(np.asarray(a, np.float64)).astype(np.float32)).astype(np.float64)


def _within_one_ulp(label, got, ref64):
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, label
    worst = float((np.abs(got - ref64) / _ulp32(ref64)).max()) if got.size else 0.0
    print(f"\n{label}: worst error {worst:.3f} float32 ulps of the float64 restatement, bound 1")
    assert worst <= 1.0, (label, worst)


def _close(label, got, ref32, ref64):
    """max(4 x the float32 run's own distance from the float64 run, one float32 ulp of the largest magnitude)."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, label
    own = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    tol = max(4.0 * own, float(np.spacing(np.float32(np.abs(ref64).max()))))
    err = float(np.abs(got - ref64).max())
    print(f"\n{label}: max error {err:.3e} of float64, bound {tol:.3e}")
    assert err <= tol, (label, err, tol)


def _tensors(n, seed, dead=None, d=5, shd=1):
    """Stored tensors of n Gaussians; `dead` rows get a logit of -8 (opacity 3e-4), the others logits in [-2, 4]."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.asarray(a, np.float32)  # noqa: E731
    t = {"xyz": f(rng.standard_normal((n, 3)) * 3), "f_dc": f(rng.standard_normal((n, 1, 3))),
         "f_rest": f(rng.standard_normal((n, (shd + 1) ** 2 - 1, 3))), "opacity": f(rng.uniform(-2.0, 4.0, (n, 1))),
         "scaling": f(rng.uniform(-4.0, 0.0, (n, 3))), "rotation": f(rng.standard_normal((n, 4)) * 2),
         "semantic_feature": f(rng.standard_normal((n, d)))}
    if dead is not None:
        t["opacity"][np.asarray(dead)] = -8.0
    return t


def _model(t, shd=1, seed=1, step=3.0, rgb=True):
    """A GaussianModel on the device, as tests/test_densify_gpu.py builds its models: the seven-group optimizer with random
    moments and `step`."""
    from gags_amd.scene import GaussianModel
    g = {k: torch.as_tensor(v).to(DEV).float().contiguous() for k, v in t.items()}
    m = GaussianModel.from_tensors(g["xyz"], g["scaling"], g["rotation"], g["opacity"], g["f_dc"], g["f_rest"],
                                   g["semantic_feature"], sh_degree=shd)
    if rgb:
        m.training_setup_rgb(ARGS)
        rng = np.random.default_rng(seed)
        for grp in m.optimizer.param_groups:
            p = grp["params"][0]
            m.optimizer.state[p] = {"step": torch.tensor(step),
                                    "exp_avg": torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)).to(DEV),
                                    "exp_avg_sq": torch.from_numpy(rng.random(tuple(p.shape)).astype(np.float32)).to(DEV)}
    return m


def _snapshot(m):
    out = {k: getattr(m, a).detach().clone() for k, a in ATTR.items()}
    if m.optimizer is not None:
        for k, a in ATTR.items():
            st = m.optimizer.state[getattr(m, a)]
            out["m1_" + k], out["m2_" + k] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    return out


def _check_groups(m, step):
    seen = set()
    for grp in m.optimizer.param_groups:
        p = grp["params"][0]
        seen.add(grp["name"])
        assert p is getattr(m, ATTR[grp["name"]]) and isinstance(p, torch.nn.Parameter) and p.requires_grad, grp["name"]
        st = m.optimizer.state[p]
        assert float(st["step"]) == step and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
    assert seen == set(ATTR) and len(m.optimizer.state) == 7


def _steps_on(m, step):
    for a in ATTR.values():
        getattr(m, a).grad = torch.ones_like(getattr(m, a))
    before = m._xyz.detach().clone()
    m.optimizer.step()
    _check_groups(m, step + 1)
    assert not torch.equal(before, m._xyz.detach())


# ----------------------------------------------------------------------------------------------------------------------
# R2: sampling
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 64, 65, 4097])
@pytest.mark.parametrize("n", [1, 63, 1000])
def test_sampling_equals_the_restatement_on_the_devices_own_cdf(rows, n):
    from gags_amd import mcmc
    rng = np.random.default_rng(rows * 7 + n)
    w = rng.random(rows) * (rng.random(rows) < 0.7)
    if rows > 1:
        w[-1] = 0.0          # a zero last row: t >= cdf[N - 2] must not land on it
        w[0] = 0.0
        w[rows // 2] = 0.5
    else:
        w[0] = 0.25
    u = rng.random(n)
    u[0] = 0.0
    if n > 2:
        u[1] = np.nextafter(1.0, 0.0)
    draws, counts, cdf = mcmc.sample(torch.from_numpy(w).to(DEV), n, uniforms=torch.from_numpy(u).to(DEV))
    assert draws.dtype == torch.int32 and counts.dtype == torch.int32 and cdf.dtype == torch.float64
    cdf_h = cdf.cpu().numpy()
    want_cdf = np.cumsum(w)
    rel = float(np.max(np.abs(cdf_h - want_cdf) / np.where(want_cdf > 0, want_cdf, 1.0)))
    print(f"\nN={rows} n={n}: cdf within {rel:.2e} relative of numpy's, bound 1e-12")
    assert rel <= 1e-12 and np.array_equal(cdf_h[want_cdf == 0], want_cdf[want_cdf == 0])
    ref_draws, ref_counts = R.sample(cdf_h, u)
    assert np.array_equal(draws.cpu().numpy(), ref_draws)
    assert np.array_equal(counts.cpu().numpy(), ref_counts)
    assert int(counts.sum()) == n and not bool((counts.cpu().numpy()[w == 0] != 0).any())
    # the generator path: seeded draws are reproducible and land on positive rows only
    g = torch.Generator(device=DEV).manual_seed(5)
    d1, c1, _ = mcmc.sample(torch.from_numpy(w).to(DEV), n, generator=g)
    d2, _, _ = mcmc.sample(torch.from_numpy(w).to(DEV), n, generator=torch.Generator(device=DEV).manual_seed(5))
    assert torch.equal(d1, d2) and int(c1.sum()) == n and bool((torch.from_numpy(w).to(DEV)[d1.long()] > 0).all())


# ----------------------------------------------------------------------------------------------------------------------
# R1: relocation values
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000])
def test_relocation_values_within_one_ulp_of_float64(rows):
    from gags_amd import mcmc
    rng = np.random.default_rng(rows)
    logit = np.linspace(_logit(MIN_OPACITY), 20.0, rows).astype(np.float32) if rows > 1 else np.array([1.5], np.float32)
    rng.shuffle(logit)
    ratios = (np.arange(rows) % 56) + 1            # 1 .. 56: 52 .. 56 are clamped to 51
    if rows == 1:
        ratios[:] = 7
    if rows > 60:
        ratios[-3:] = (1000, 2 ** 31 - 1, 51)
    rng.shuffle(ratios)
    if rows > 1:
        logit[np.nonzero(ratios == 1)[0][0]] = 0.3                         # an unclamped opacity at r = 1
    scaling = rng.uniform(-6.0, 1.0, (rows, 3)).astype(np.float32)
    new_op, new_sc = mcmc.relocation_values(torch.from_numpy(logit).to(DEV).reshape(rows, 1), torch.from_numpy(scaling).to(DEV),
                                            torch.from_numpy(ratios).to(DEV), MIN_OPACITY)
    assert tuple(new_op.shape) == (rows, 1) and tuple(new_sc.shape) == (rows, 3)
    ref_op, ref_sc = R.relocation_values(logit, scaling, ratios, MIN_OPACITY)
    _within_one_ulp(f"rows={rows} new logits", new_op.cpu().numpy().reshape(-1), ref_op)
    _within_one_ulp(f"rows={rows} new log-scales", new_sc.cpu().numpy(), ref_sc)
    one = (ratios == 1) & (logit < 15.0)
    assert np.array_equal(new_sc.cpu().numpy()[one], scaling[one])          # r = 1: coeff = 1, the log-scales keep their bits
    assert rows == 1 or one.any()
    # deviation 1: a saturated float32 sigmoid (logit 20) still gives finite values
    assert bool(torch.isfinite(new_op).all()) and bool(torch.isfinite(new_sc).all())


# ----------------------------------------------------------------------------------------------------------------------
# R3: relocate
# ----------------------------------------------------------------------------------------------------------------------
def _expected_sources(before, w, n_draws, u):
    """draws / counts of the module's own sampling and the out-of-place relocation values of the drawn rows (each is tested on
    its own above)."""
    from gags_amd import mcmc
    draws, counts, _ = mcmc.sample(w, n_draws, uniforms=u)
    new_op, new_sc = mcmc.relocation_values(before["opacity"], before["scaling"], counts + 1, MIN_OPACITY)
    src = counts > 0
    op, sc = before["opacity"].clone(), before["scaling"].clone()
    op[src], sc[src] = new_op[src], new_sc[src]
    return draws.long(), counts, src, op, sc


@pytest.mark.parametrize("n", [5, 257])
@pytest.mark.parametrize("dead_kind", ["none", "third", "all_but_one"])
def test_relocate_through_a_model(n, dead_kind):
    rng = np.random.default_rng(n + len(dead_kind))
    dead = np.zeros(n, bool)
    if dead_kind == "third":
        dead[rng.permutation(n)[:max(1, int(0.3 * n))]] = True
    elif dead_kind == "all_but_one":
        dead[:] = True
        dead[n // 2] = False
    m = _model(_tensors(n, seed=n, dead=dead))
    m.cache_activations(True)
    before = _snapshot(m)
    params = {k: getattr(m, a) for k, a in ATTR.items()}
    n_dead = int(dead.sum())
    u = torch.from_numpy(rng.random(n_dead)).to(DEV)
    got = m.relocate_gs(uniforms=u, min_opacity=MIN_OPACITY)
    assert got == n_dead and m._xyz.shape[0] == n
    for k, a in ATTR.items():
        assert getattr(m, a) is params[k], k        # in place: the parameters are the same objects
    _check_groups(m, 3.0)
    after = _snapshot(m)
    if n_dead == 0:
        for k in before:
            assert torch.equal(before[k], after[k]), k
        return
    assert m.__dict__["_act_cache"] == {}
    dead_t = torch.from_numpy(dead).to(DEV)
    w = torch.sigmoid(before["opacity"].reshape(-1).double()).masked_fill(dead_t, 0.0)
    draws, counts, src, op, sc = _expected_sources(before, w, n_dead, u)
    assert not bool((src & dead_t).any()) and int(counts.sum()) == n_dead
    expect = {k: before[k].clone() for k in ATTR}
    expect["opacity"], expect["scaling"] = op, sc                              # R1 on every drawn source, once
    dead_rows = torch.nonzero(dead_t).reshape(-1)                               # ascending: the k-th dead row takes the k-th draw
    for k in ATTR:
        expect[k][dead_rows] = expect[k][draws]
        assert torch.equal(after[k], expect[k]), k
        for mom in ("m1_", "m2_"):
            want = before[mom + k].clone()
            want[src] = 0.0                                                      # zero at the sources only; dead rows keep theirs
            assert torch.equal(after[mom + k], want), (mom, k)
    # the rewritten sources against the float64 restatement, with ratio = count + 1
    rows = src.cpu().numpy()
    ref_op, ref_sc = R.relocation_values(before["opacity"].cpu().numpy()[rows], before["scaling"].cpu().numpy()[rows],
                                         counts.cpu().numpy()[rows] + 1, MIN_OPACITY)
    _within_one_ulp(f"N={n} {dead_kind} source logits", after["opacity"].cpu().numpy()[rows].reshape(-1), ref_op)
    _within_one_ulp(f"N={n} {dead_kind} source log-scales", after["scaling"].cpu().numpy()[rows], ref_sc)
    if dead_kind == "all_but_one":
        assert counts.cpu().tolist() == [n - 1 if j == n // 2 else 0 for j in range(n)]   # one source, drawn n - 1 times, written once
    _steps_on(m, 3.0)


def test_relocate_with_nothing_alive_or_a_given_mask():
    n = 40
    m = _model(_tensors(n, seed=2, dead=np.ones(n, bool)))
    before = _snapshot(m)
    assert m.relocate_gs() == 0
    for k, v in _snapshot(m).items():
        assert torch.equal(before[k], v), k
    # a caller's mask instead of the opacity rule: rows 3 and 17 of a model whose Gaussians are all opaque enough
    m = _model(_tensors(n, seed=3))
    before = _snapshot(m)
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[[3, 17]] = True
    u = torch.tensor([0.25, 0.75], dtype=torch.float64, device=DEV)
    assert m.relocate_gs(mask, uniforms=u) == 2
    w = torch.sigmoid(before["opacity"].reshape(-1).double()).masked_fill(mask, 0.0)
    draws, counts, src, op, sc = _expected_sources(before, w, 2, u)
    after = _snapshot(m)
    assert torch.equal(after["xyz"][[3, 17]], before["xyz"][draws]) and torch.equal(after["opacity"][[3, 17]], op[draws])
    keep = ~(mask | src)
    for k in ATTR:
        assert torch.equal(after[k][keep], before[k][keep]), k


# ----------------------------------------------------------------------------------------------------------------------
# R4: sample_add
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap_max,n_new", [(1000, 210), (205, 205), (200, 200)])
def test_sample_add_grows_to_the_target(cap_max, n_new):
    n = 200
    m = _model(_tensors(n, seed=cap_max))
    m.xyz_gradient_accum += 1.0
    m.cache_activations(True)
    before = _snapshot(m)
    objects = {a: getattr(m, a) for a in ATTR.values()}
    stats = (m.xyz_gradient_accum, m.denom, m.max_radii2D)
    n_add = n_new - n
    u = torch.from_numpy(np.random.default_rng(cap_max).random(n_add)).to(DEV)
    assert m.add_new_gs(cap_max, uniforms=u if n_add else None) == n_add
    assert m._xyz.shape[0] == n_new
    if n_add == 0:                                                               # a no-op: every tensor is the same object
        for a, p in objects.items():
            assert getattr(m, a) is p, a
        assert all(x is y for x, y in zip((m.xyz_gradient_accum, m.denom, m.max_radii2D), stats))
        for k, v in _snapshot(m).items():
            assert torch.equal(before[k], v), k
        return
    assert m.__dict__["_act_cache"] == {}
    w = torch.sigmoid(before["opacity"].reshape(-1).double())
    draws, counts, src, op, sc = _expected_sources(before, w, n_add, u)
    expect = {k: before[k].clone() for k in ATTR}
    expect["opacity"], expect["scaling"] = op, sc
    after = _snapshot(m)
    for k in ATTR:
        assert torch.equal(after[k][:n], expect[k]), k                           # existing rows: only the sources' R1 values moved
        assert torch.equal(after[k][n:], expect[k][draws]), k                    # one copy of the UPDATED source per draw, in draw order
        for mom in ("m1_", "m2_"):
            assert torch.equal(after[mom + k][:n], before[mom + k]), (mom, k)    # kept, drawn rows included
            assert not bool(after[mom + k][n:].any()), (mom, k)
    _check_groups(m, 3.0)
    for s, shape in (("xyz_gradient_accum", (n_new, 1)), ("denom", (n_new, 1)), ("max_radii2D", (n_new,))):
        t = getattr(m, s)
        assert tuple(t.shape) == shape and t.dtype == torch.float32 and not bool(t.any()), s
    _steps_on(m, 3.0)


# ----------------------------------------------------------------------------------------------------------------------
# R5: position noise
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 70_001])
def test_noise_against_float64(n):
    from gags_amd import mcmc
    rng = np.random.default_rng(n)
    t = _tensors(n, seed=n)
    t["opacity"] = np.array([_logit(o) for o in (0.001, 0.005, 0.5, 0.999)], np.float32)[np.arange(n) % 4].reshape(n, 1)
    t["scaling"] = np.log(10.0 ** rng.uniform(-3.0, 1.0, (n, 3))).astype(np.float32)      # four decades
    t["rotation"] = (rng.standard_normal((n, 4)) * rng.uniform(0.1, 10.0, (n, 1))).astype(np.float32)   # un-normalised
    z = rng.standard_normal((n, 3)).astype(np.float32)
    scaler = 1.6e-4 * 5e5
    m = _model(t, rgb=False)
    m.cache_activations(True)
    m.get_scaling                                                                                   # (a cached activation)
    xyz_object = m._xyz
    version = m._xyz._version
    mcmc.inject_noise(m, scaler, noise=torch.from_numpy(z).to(DEV))
    assert m._xyz is xyz_object and m._xyz._version > version and m.__dict__["_act_cache"] == {}
    args = (t["xyz"], t["opacity"], t["scaling"], t["rotation"], z, np.float32(scaler))
    ref64, ref32 = R.noise(*args, dtype=np.float64), R.noise(*args, dtype=np.float32)
    _close(f"N={n} xyz after the noise", m._xyz.detach().cpu().numpy(), ref32, ref64)
    moved = np.abs(ref64 - t["xyz"]).max(1)
    gate_open = (np.arange(n) % 4 == 0)
    assert moved[gate_open].max() > 0 and (n < 4 or moved[np.arange(n) % 4 == 2].max() < 1e-12)   # gate ~0.6 at o = 0.001, ~0 at 0.5
    # scaler = 0 leaves the positions bit-identical
    m2 = _model(t, rgb=False)
    mcmc.inject_noise(m2, 0.0, noise=torch.from_numpy(z).to(DEV))
    assert np.array_equal(m2._xyz.detach().cpu().numpy(), t["xyz"])
    # drawn on the device: seeded, reproducible
    a, b = _model(t, rgb=False), _model(t, rgb=False)
    mcmc.inject_noise(a, scaler, generator=torch.Generator(device=DEV).manual_seed(3))
    mcmc.inject_noise(b, scaler, generator=torch.Generator(device=DEV).manual_seed(3))
    assert torch.equal(a._xyz, b._xyz) and not np.array_equal(a._xyz.detach().cpu().numpy(), t["xyz"])


# ----------------------------------------------------------------------------------------------------------------------
# R6: regularisers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 70_001])
def test_regularisers_value_and_gradients_against_float64(n):
    from gags_amd import mcmc
    t = _tensors(n, seed=n + 1)
    regs = (0.01, 0.03)
    outs = []
    for _ in range(2):
        m = _model(t, rgb=False)
        m._opacity.requires_grad_(True)
        m._scaling.requires_grad_(True)
        loss = mcmc.regularisation(m, *regs)
        assert loss.shape == () and loss.dtype == torch.float32
        (loss * 2.5).backward()
        outs.append((loss.detach().clone(), m._opacity.grad.clone(), m._scaling.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)                                                # deterministic: two calls, identical bits
    v64, go64, gs64 = R.regularisation(t["opacity"], t["scaling"], *regs, dtype=np.float64)
    v32, go32, gs32 = R.regularisation(t["opacity"], t["scaling"], *regs, dtype=np.float32)
    value, g_op, g_sc = outs[0]
    _close(f"N={n} regulariser value", np.array([float(value)]), np.array([v32]), np.array([v64]))
    _close(f"N={n} d / d logit", g_op.cpu().numpy().reshape(-1), np.float32(2.5) * go32, 2.5 * go64)
    _close(f"N={n} d / d log-scale", g_sc.cpu().numpy(), np.float32(2.5) * gs32, 2.5 * gs64)


# ----------------------------------------------------------------------------------------------------------------------
# R7: the strategy, and a render across a relocation
# ----------------------------------------------------------------------------------------------------------------------
def test_strategy_three_steps_around_a_refinement():
    from gags_amd import mcmc
    n, n_dead = 300, 20
    dead = np.zeros(n, bool)
    dead[np.random.default_rng(0).permutation(n)[:n_dead]] = True
    finals = []
    for _ in range(2):
        m = _model(_tensors(n, seed=9, dead=dead))
        s = mcmc.MCMCStrategy(cap_max=1000, refine_start_iter=0, refine_every=2, refine_stop_iter=100)
        gen = torch.Generator(device=DEV).manual_seed(17)
        got = [s.step_post_backward(m, step, 1.6e-4, generator=gen) for step in (1, 2, 3)]
        assert got == [(0, 0), (n_dead, int(1.05 * n) - n), (0, 0)], got
        assert m._xyz.shape[0] == 315
        _check_groups(m, 3.0)
        assert float(torch.sigmoid(m._opacity.detach()).min()) >= MIN_OPACITY * (1 - 1e-6)   # nothing dead is left
        finals.append(_snapshot(m))
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k                       # same seed: bit-identical
    # at the cap nothing is added, and outside the window nothing is refined
    s = mcmc.MCMCStrategy(cap_max=315, refine_start_iter=0, refine_every=2, refine_stop_iter=4)
    assert s.step_post_backward(m, 2, 1.6e-4, generator=gen)[1] == 0
    assert s.step_post_backward(m, 4, 1.6e-4, generator=gen) == (0, 0) and m._xyz.shape[0] == 315


def test_an_empty_model_is_accepted_everywhere():
    from gags_amd import mcmc
    m = _model(_tensors(0, seed=0), rgb=False)
    assert m.relocate_gs() == 0 and m.add_new_gs(100) == 0 and m._xyz.shape[0] == 0
    mcmc.inject_noise(m, 80.0)
    m._opacity.requires_grad_(True)
    m._scaling.requires_grad_(True)
    loss = mcmc.regularisation(m, 0.01, 0.01)
    loss.backward()
    assert float(loss.detach()) == 0.0 and tuple(m._opacity.grad.shape) == (0, 1) and tuple(m._scaling.grad.shape) == (0, 3)
    assert mcmc.MCMCStrategy(refine_start_iter=0, refine_every=1).step_post_backward(m, 1, 1.6e-4) == (0, 0)
    d, c, cdf = mcmc.sample(torch.ones(3, dtype=torch.float64, device=DEV), 0)
    assert d.numel() == 0 and c.tolist() == [0, 0, 0] and cdf.tolist() == [1.0, 2.0, 3.0]


def test_render_before_and_after_relocating_one_dead_gaussian():
    from gags_amd import synthetic as syn
    from gags_amd.gaussian_renderer import render
    w = h = 32
    pc = syn.make_model(300, 16, w, h, seed=3, device=DEV, scale0=syn.SCALE0 * 24)
    cam = syn.make_camera(w, h, view=3, device=DEV)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        pc._opacity.clamp_(min=-3.0)
        pc._opacity[7] = -10.0
        first = render(cam, pc, None, bg, feature_mode=False)["render"]
        assert tuple(first.shape) == (3, h, w) and bool(torch.isfinite(first).all())
        assert pc.relocate_gs(generator=torch.Generator(device=DEV).manual_seed(1)) == 1
        assert float(torch.sigmoid(pc._opacity[7])) >= MIN_OPACITY * (1 - 1e-6)
        second = render(cam, pc, None, bg, feature_mode=False)["render"]
    assert tuple(second.shape) == (3, h, w) and bool(torch.isfinite(second).all())
