"""N8 on the GPU: adaptive density control through the public methods of scene.GaussianModel (gags_amd/densify.py,
csrc/densify.hip) against the reference's own results (tests/golden/densify_vectors.npz) and, at sizes the fixture does not
hold, against the restatement tests/densify_ref.py run on the device.

What is compared how.  EXACT (bit for bit): the output length, the order, every copied tensor, both Adam moments, `step`, denom,
max_radii2D and the zeroed statistics.  BY TOLERANCE: the arrays the kernels compute -- child xyz, child scaling, reset logits,
accum -- each within max(4 x the float32 reference run's own distance from the float64 run on that array, one fp32 ulp of the
array's largest magnitude) of the float64 run; both terms come from the reference runs, never from the kernel's result.
Every such comparison prints the achieved error next to its bound; DESIGN.md section 7 "N8" is where they are recorded.
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
import densify_ref as R  # noqa: E402

DEV = torch.device("cuda", 0)
Z = np.load(os.path.join(HERE, "golden", "densify_vectors.npz"))
CASES = [str(c) for c in Z["cases"]]
ATTR = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling",
            rotation="_rotation", semantic_feature="_semantic_feature")
ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016,
                             position_lr_delay_mult=0.01, position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05,
                             scaling_lr=0.005, rotation_lr=0.001, semantic_feature_lr=0.001)


def _tol(ref32, ref64):
    """The bound of this file's docstring for one computed array (numpy, any shape)."""
    ref64 = np.asarray(ref64, np.float64)
    if ref64.size == 0:
        return 0.0
    own = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    return max(4.0 * own, float(np.spacing(np.float32(np.abs(ref64).max()))))


def _close(label, got, ref32, ref64):
    got = np.asarray(got, np.float64)
    assert got.shape == np.asarray(ref64).shape, label
    err = float(np.abs(got - np.asarray(ref64, np.float64)).max()) if got.size else 0.0
    tol = _tol(ref32, ref64)
    print(f"\n{label}: max error {err:.3e} of float64, bound {tol:.3e}")
    assert err <= tol, (label, err, tol)


def _par(name):
    pd, max_grad, min_op, extent, mss, shd, step = (float(v) for v in Z[name + "_par"])
    return pd, max_grad, min_op, extent, (mss or None), int(shd), step


def _model(t, sh_degree, moments=None, step=3.0, accum=None, denom=None, max_radii=None, rgb=True):
    """A GaussianModel on the device from numpy / torch inputs; rgb: the seven-group optimizer with the given moments."""
    from gags_amd.scene import GaussianModel
    g = {k: torch.as_tensor(v).to(DEV).float().contiguous() for k, v in t.items()}
    m = GaussianModel.from_tensors(g["xyz"], g["scaling"], g["rotation"], g["opacity"], g["f_dc"], g["f_rest"],
                                   g["semantic_feature"], sh_degree=sh_degree)
    if rgb:
        m.training_setup_rgb(ARGS)
        if moments is not None:
            for grp in m.optimizer.param_groups:
                m1, m2 = moments[grp["name"]]
                m.optimizer.state[grp["params"][0]] = {"step": torch.tensor(step),
                                                       "exp_avg": torch.as_tensor(m1).to(DEV).float().contiguous(),
                                                       "exp_avg_sq": torch.as_tensor(m2).to(DEV).float().contiguous()}
    n = g["xyz"].shape[0]
    m.percent_dense = 0.01
    m.xyz_gradient_accum = torch.as_tensor(accum).to(DEV).float().reshape(n, 1).contiguous() if accum is not None else torch.zeros(n, 1, device=DEV)
    m.denom = torch.as_tensor(denom).to(DEV).float().reshape(n, 1).contiguous() if denom is not None else torch.zeros(n, 1, device=DEV)
    m.max_radii2D = torch.as_tensor(max_radii).to(DEV).float().contiguous() if max_radii is not None else torch.zeros(n, device=DEV)
    return m


def _check_model(label, m, kind, ref32, ref64, mom32=None, step=3.0, groups=tuple(ATTR)):
    """m after densify_and_prune against a reference result: ref32 / ref64 name -> array, mom32 name -> (m1, m2)."""
    kind = np.asarray(kind)
    n_out = len(kind)
    child = kind >= R.CHILD_A
    for name, attr in ATTR.items():
        got = getattr(m, attr).detach().cpu().numpy()
        want = np.asarray(ref32[name])
        assert got.shape == want.shape and got.shape[0] == n_out, (label, name, got.shape, want.shape)
        if name in ("xyz", "scaling"):
            assert np.array_equal(got[~child], want[~child]), (label, name)
            _close(f"{label} child {name}", got[child], want[child], np.asarray(ref64[name])[child])
        else:
            assert np.array_equal(got, want), (label, name)
    for s, shape in (("xyz_gradient_accum", (n_out, 1)), ("denom", (n_out, 1)), ("max_radii2D", (n_out,))):
        t = getattr(m, s)
        assert tuple(t.shape) == shape and t.dtype == torch.float32 and not bool(t.any()), (label, s)
    if m.optimizer is not None:
        seen = set()
        for grp in m.optimizer.param_groups:
            name = grp["name"]
            seen.add(name)
            p = grp["params"][0]
            assert p is getattr(m, ATTR[name]) and isinstance(p, torch.nn.Parameter) and p.requires_grad, (label, name)
            st = m.optimizer.state[p]
            assert float(st["step"]) == step, (label, name)
            if mom32 is not None:
                assert np.array_equal(st["exp_avg"].cpu().numpy(), np.asarray(mom32[name][0])), (label, name, "exp_avg")
                assert np.array_equal(st["exp_avg_sq"].cpu().numpy(), np.asarray(mom32[name][1])), (label, name, "exp_avg_sq")
            assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert seen == set(groups) and len(m.optimizer.state) == len(seen), (label, "stale optimizer state")


# ----------------------------------------------------------------------------------------------------------------------
# the fixture through the public methods
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fixture_case_through_the_public_methods(name):
    pd, max_grad, min_op, extent, mss, shd, step = _par(name)
    t = {k: Z[f"{name}_{k}"] for k in R.NAMES}
    mom = {k: (Z[f"{name}_m1_{k}"], Z[f"{name}_m2_{k}"]) for k in R.NAMES}
    m = _model(t, shd, mom, step, Z[name + "_accum"], Z[name + "_denom"], Z[name + "_max_radii"])
    m.cache_activations(True)
    m.densify_and_prune(max_grad, min_op, extent, mss, samples=torch.from_numpy(Z[name + "_Z"]).to(DEV))
    assert m.__dict__["_act_cache"] == {}
    ref32 = {k: Z[f"{name}_f32_{k}"] for k in R.NAMES}
    ref64 = {k: Z[f"{name}_f64_{k}"] for k in R.NAMES}
    mom32 = {k: (Z[f"{name}_f32_m1_{k}"], Z[f"{name}_f32_m2_{k}"]) for k in R.NAMES}
    _check_model(name, m, Z[name + "_kind"], ref32, ref64, mom32, step)


def test_fixture_statistics_over_three_views():
    n = Z["st_grad"].shape[1]
    t = {k: Z[f"none_{k}"] for k in R.NAMES}
    rep = lambda a: np.concatenate([a] * 4)[:n]  # noqa: E731  (any model of n Gaussians: the statistics read none of it)
    m = _model({k: rep(v) for k, v in t.items()}, 1)
    fused = _model({k: rep(v) for k, v in t.items()}, 1)
    from gags_amd import densify
    for v in range(3):
        w, h = int(Z["st_wh"][v, 0]), int(Z["st_wh"][v, 1])
        grad = torch.from_numpy(Z["st_grad"][v:v + 1]).to(DEV)
        vp = types.SimpleNamespace(grad=grad.clone())
        radii = torch.from_numpy(Z["st_radii"][v]).to(DEV)
        m.update_max_radii(radii, torch.from_numpy(Z["st_visible"][v]).to(DEV))
        m.add_densification_stats(vp, torch.from_numpy(Z["st_update"][v]).to(DEV), w, h)
        assert torch.equal(vp.grad, grad)  # (documented deviation: the gradient is not scaled in place)
        densify.accumulate(fused, {"viewspace_points": vp, "radii": radii, "render": torch.empty(3, h, w, device=DEV)})
    assert np.array_equal(m.denom.cpu().numpy(), Z["st_f32_denom"])
    assert np.array_equal(m.max_radii2D.cpu().numpy(), Z["st_f32_max_radii"])
    _close("accum", m.xyz_gradient_accum.cpu().numpy(), Z["st_f32_accum"], Z["st_f64_accum"])
    # the fused launch = the two methods with `radii > 0` for both filters
    two = _model({k: rep(v) for k, v in t.items()}, 1)
    for v in range(3):
        vp = types.SimpleNamespace(grad=torch.from_numpy(Z["st_grad"][v:v + 1]).to(DEV))
        radii = torch.from_numpy(Z["st_radii"][v]).to(DEV)
        two.update_max_radii(radii, radii > 0)
        two.add_densification_stats(vp, radii > 0, int(Z["st_wh"][v, 0]), int(Z["st_wh"][v, 1]))
    for s in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(getattr(fused, s), getattr(two, s)), s
    assert np.array_equal(fused.max_radii2D.cpu().numpy(), Z["st_f32_max_radii"])


def test_the_training_loops_calls_run_as_written():
    """What train.py:206-218 does, call for call, on this project's tensors: the boolean-mask assignment of line 209 into
    max_radii2D with the rasterizer's int32 radii (torch promotes them), add_densification_stats with the visibility filter for
    both roles, densify_and_prune with a size threshold of None and of 20, reset_opacity.  The statistics equal the fused
    accumulate() bit for bit."""
    from gags_amd import densify
    name = "mixed_nomss"
    pd, max_grad, min_op, extent, _, shd, _ = _par(name)
    t = {k: Z[f"{name}_{k}"] for k in R.NAMES}
    n = t["xyz"].shape[0]
    gaussians, fused = _model(t, shd), _model(t, shd)
    g = torch.Generator(device=DEV).manual_seed(2)
    for it in range(2):
        radii = torch.randint(0, 50, (n,), device=DEV, generator=g).int() * (torch.rand(n, device=DEV, generator=g) < 0.7)
        radii = radii.int()
        visibility_filter = radii > 0
        viewspace_point_tensor = types.SimpleNamespace(grad=1e-3 * torch.randn(1, n, 2, device=DEV, generator=g))
        gaussians.max_radii2D[visibility_filter] = torch.max(gaussians.max_radii2D[visibility_filter], radii[visibility_filter])
        gaussians.add_densification_stats(viewspace_point_tensor, visibility_filter, 64, 48)
        densify.accumulate(fused, {"viewspace_points": viewspace_point_tensor, "radii": radii,
                                   "render": torch.empty(3, 48, 64, device=DEV)})
    assert radii.dtype == torch.int32 and gaussians.max_radii2D.dtype == torch.float32 and float(gaussians.max_radii2D.max()) > 0
    for s in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(getattr(gaussians, s), getattr(fused, s)), s
    gaussians.xyz_gradient_accum = torch.from_numpy(Z[name + "_accum"]).to(DEV)
    gaussians.denom = torch.from_numpy(Z[name + "_denom"]).to(DEV)
    for size_threshold in (None, 20):
        before = gaussians._xyz.shape[0]
        gaussians.densify_and_prune(max_grad, 0.005, extent, size_threshold)
        assert gaussians.max_radii2D.shape == (gaussians._xyz.shape[0],) and not bool(gaussians.denom.any())
        if size_threshold is None:
            assert gaussians._xyz.shape[0] == len(Z[name + "_kind"]) != before
    gaussians.reset_opacity()
    assert float(torch.sigmoid(gaussians._opacity.detach()).max()) <= 0.01 * (1 + 1e-5)  # (a few fp32 ulps of the logit, 4.6)


def test_fixture_reset_opacity():
    n = Z["ro_opacity"].shape[0]
    t = {k: np.concatenate([Z[f"none_{k}"]] * 2)[:n] for k in R.NAMES}
    t["opacity"] = Z["ro_opacity"]
    mom = {k: (np.ones_like(t[k]), np.ones_like(t[k])) for k in R.NAMES}
    mom["opacity"] = (Z["ro_m1"], Z["ro_m2"])
    m = _model(t, 1, mom, step=1.0)
    m.cache_activations(True)
    others = {k: getattr(m, a) for k, a in ATTR.items() if k != "opacity"}
    m.reset_opacity()
    assert m.__dict__["_act_cache"] == {}
    _close("reset logits", m._opacity.detach().cpu().numpy(), Z["ro_f32"], Z["ro_f64"])
    grp = [g for g in m.optimizer.param_groups if g["name"] == "opacity"][0]
    st = m.optimizer.state[grp["params"][0]]
    assert grp["params"][0] is m._opacity and m._opacity.requires_grad and float(st["step"]) == 1.0
    assert not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any()) and len(m.optimizer.state) == 7
    for k, p in others.items():  # nothing else moved
        assert getattr(m, ATTR[k]) is p and bool((m.optimizer.state[p]["exp_avg"] == 1).all())


# ----------------------------------------------------------------------------------------------------------------------
# random scenes against the restatement on the device
# ----------------------------------------------------------------------------------------------------------------------
def _random_scene(n, d, shd, seed, mss):
    import densify_cases as G
    rng = np.random.default_rng(seed)
    t, accum, denom, max_radii, par = G.build_case(rng, n, shd, d, 10.0, 0.0002, mss, "mixed")
    assert G.check_margin(t, accum, denom, par, False) == 0
    mom = {k: (rng.standard_normal(v.shape).astype(np.float32), rng.random(v.shape).astype(np.float32)) for k, v in t.items()}
    return t, accum, denom, max_radii, par, mom


def _reference_on_device(t, accum, denom, par, mom, zs):
    out = {}
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        tt = {k: torch.from_numpy(v).to(DEV).to(dtype) for k, v in t.items()}
        mm = {k: (torch.from_numpy(a).to(DEV).to(dtype), torch.from_numpy(b).to(DEV).to(dtype)) for k, (a, b) in mom.items()}
        out[tag] = R.densify_and_prune(tt, torch.from_numpy(accum).to(DEV).to(dtype), torch.from_numpy(denom).to(DEV).to(dtype),
                                       par["percent_dense"], par["max_grad"], par["min_opacity"], par["extent"], par["mss"],
                                       zs.to(dtype), moments=mm if tag == "f32" else None)
    return out["f32"], out["f64"]


@pytest.mark.parametrize("n,d,shd", [(5000, 16, 3), (5000, 7, 1), (150000, 16, 3), (150000, 7, 1)])
def test_random_scene_equals_the_restatement_on_the_device(n, d, shd):
    """5 000 crosses the scan's 2048-entry workgroup, 150 000 takes its multi-level path; D = 16 rows ride the 16-byte lanes,
    sh_degree 1 / D = 7 gives rows of 9 and 7 floats (the scalar path at an odd pitch)."""
    t, accum, denom, max_radii, par, mom = _random_scene(n, d, shd, seed=n + d, mss=20 if d == 16 else None)
    keep, clone_ok, split, child_ok = R.decide(torch.from_numpy(accum), torch.from_numpy(denom), torch.from_numpy(t["scaling"]),
                                               torch.from_numpy(t["opacity"]), par["percent_dense"], par["max_grad"],
                                               par["min_opacity"], par["extent"], par["mss"])
    n_split = int(split.sum())
    assert min(int(keep.sum()), int(clone_ok.sum()), int(child_ok.sum())) > n // 50 and n_split > int(child_ok.sum())
    zs = torch.randn((2 * n_split, 3), generator=torch.Generator().manual_seed(5)).to(DEV)
    r32, r64 = _reference_on_device(t, accum, denom, par, mom, zs)
    assert r32["n_split"] == n_split and torch.equal(r32["kind"], r64["kind"]) and torch.equal(r32["src"], r64["src"])
    m = _model(t, shd, mom, 3.0, accum, denom, max_radii)
    m.densify_and_prune(par["max_grad"], par["min_opacity"], par["extent"], par["mss"], samples=zs)
    ref32 = {k: r32[k].cpu().numpy() for k in R.NAMES}
    ref64 = {k: r64[k].cpu().numpy() for k in R.NAMES}
    mom32 = {k: (a.cpu().numpy(), b.cpu().numpy()) for k, (a, b) in r32["moments"].items()}
    _check_model(f"N={n} D={d}", m, r32["kind"].cpu().numpy(), ref32, ref64, mom32, 3.0)


def test_plan_equals_the_restatements_row_for_row():
    from gags_amd import densify
    t, accum, denom, max_radii, par, _ = _random_scene(5000, 7, 1, seed=77, mss=20)
    m = _model(t, 1, None, 3.0, accum, denom, max_radii)
    flags = R.decide(m.xyz_gradient_accum, m.denom, m._scaling.detach(), m._opacity.detach(), 0.01, par["max_grad"],
                     par["min_opacity"], par["extent"], par["mss"])
    src, kind, zrow, n_split = R.plan(*flags)
    plan = densify.densify_and_prune(m, par["max_grad"], par["min_opacity"], par["extent"], par["mss"],
                                     generator=torch.Generator(device=DEV).manual_seed(1))
    assert plan.n_split == n_split and plan.n_out == len(src)
    assert torch.equal(plan.src.long(), src) and torch.equal(plan.kind.long(), kind) and torch.equal(plan.zrow.long(), zrow)


# ----------------------------------------------------------------------------------------------------------------------
# edges
# ----------------------------------------------------------------------------------------------------------------------
def _one(scale, opacity, g):
    t = {"xyz": np.array([[0.5, -1.0, 2.0]], np.float32), "f_dc": np.ones((1, 1, 3), np.float32), "f_rest": np.ones((1, 3, 3), np.float32),
         "opacity": np.array([[opacity]], np.float32), "scaling": np.full((1, 3), np.log(scale), np.float32),
         "rotation": np.array([[2.0, 0.0, 0.0, 0.0]], np.float32), "semantic_feature": np.ones((1, 5), np.float32)}
    mom = {k: (np.full_like(v, 0.5), np.full_like(v, 0.25)) for k, v in t.items()}
    return _model(t, 1, mom, 3.0, np.array([g], np.float32), np.array([1.0], np.float32)), t


def test_a_single_gaussian_is_kept_cloned_split_or_pruned():
    m, t = _one(0.3, 2.0, 0.0)                                     # nothing happens
    m.densify_and_prune(0.0002, 0.005, 10.0, 20)
    assert m._xyz.shape[0] == 1 and np.array_equal(m._xyz.detach().cpu().numpy(), t["xyz"])
    m, t = _one(0.03, 2.0, 1.0)                                    # small and moving: itself and a clone
    m.densify_and_prune(0.0002, 0.005, 10.0, 20)
    assert m._xyz.shape[0] == 2 and np.array_equal(m._xyz.detach().cpu().numpy(), np.concatenate([t["xyz"]] * 2))
    st = m.optimizer.state[m._xyz]
    assert st["exp_avg"].cpu().tolist() == [[0.5] * 3, [0.0] * 3] and st["exp_avg_sq"].cpu().tolist() == [[0.25] * 3, [0.0] * 3]
    m, t = _one(0.3, 2.0, 1.0)                                     # large and moving: two children; identity rotation (2, 0, 0, 0)
    z = torch.tensor([[1.0, -2.0, 0.5], [0.0, 0.25, -1.0]], device=DEV)
    m.densify_and_prune(0.0002, 0.005, 10.0, 20, samples=z)
    e = float(np.exp(np.float32(np.log(np.float32(0.3)))))
    want = t["xyz"].astype(np.float64) + e * z.cpu().numpy().astype(np.float64)
    assert m._xyz.shape[0] == 2 and np.abs(m._xyz.detach().cpu().numpy() - want).max() <= 2 * np.spacing(np.float32(2.0))
    assert np.abs(m._scaling.detach().cpu().numpy() - np.log(e / 1.6)).max() <= 2 * np.spacing(np.float32(2.0))
    assert not bool(m.optimizer.state[m._xyz]["exp_avg"].any())
    m, t = _one(0.3, -9.0, 1.0)                                    # transparent: parent and children go
    m.densify_and_prune(0.0002, 0.005, 10.0, 20, samples=z)
    assert m._xyz.shape[0] == 0


def test_no_split_draws_no_samples_and_an_empty_model_stays_usable():
    name = "none"
    pd, max_grad, min_op, extent, mss, shd, step = _par(name)
    t = {k: Z[f"{name}_{k}"] for k in R.NAMES}
    m = _model(t, shd, None, 3.0, Z[name + "_accum"], Z[name + "_denom"])
    gen = torch.Generator(device=DEV).manual_seed(9)
    before = gen.get_state().clone()
    m.densify_and_prune(max_grad, min_op, extent, mss, generator=gen)
    assert torch.equal(gen.get_state(), before) and m._xyz.shape[0] == t["xyz"].shape[0]
    for k, a in ATTR.items():
        assert np.array_equal(getattr(m, a).detach().cpu().numpy(), t[k]), k
    # output length 0, then every entry on the empty model
    m.prune_points(torch.ones(m._xyz.shape[0], dtype=torch.bool, device=DEV))
    for k, a in ATTR.items():
        assert tuple(getattr(m, a).shape) == (0,) + t[k].shape[1:], k
    assert m.denom.shape == (0, 1) and m.max_radii2D.shape == (0,)
    m.densify_and_prune(max_grad, min_op, extent, 20)
    m.reset_opacity()
    m.update_max_radii(torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.bool, device=DEV))
    assert m._xyz.shape[0] == 0 and m._opacity.shape == (0, 1)


def test_prune_points_keeps_rows_moments_and_statistics():
    name = "mixed_nomss"
    t = {k: Z[f"{name}_{k}"] for k in R.NAMES}
    mom = {k: (Z[f"{name}_m1_{k}"], Z[f"{name}_m2_{k}"]) for k in R.NAMES}
    m = _model(t, _par(name)[5], mom, 3.0, Z[name + "_accum"], Z[name + "_denom"], Z[name + "_max_radii"])
    mask = np.random.default_rng(1).random(t["xyz"].shape[0]) < 0.4
    m.prune_points(torch.from_numpy(mask).to(DEV))
    for k, a in ATTR.items():
        assert np.array_equal(getattr(m, a).detach().cpu().numpy(), t[k][~mask]), k
        st = m.optimizer.state[getattr(m, a)]
        assert np.array_equal(st["exp_avg"].cpu().numpy(), mom[k][0][~mask]) and float(st["step"]) == 3.0
        assert np.array_equal(st["exp_avg_sq"].cpu().numpy(), mom[k][1][~mask])
    assert np.array_equal(m.xyz_gradient_accum.cpu().numpy(), Z[name + "_accum"][~mask], equal_nan=True)
    assert np.array_equal(m.denom.cpu().numpy(), Z[name + "_denom"][~mask])
    assert np.array_equal(m.max_radii2D.cpu().numpy(), Z[name + "_max_radii"][~mask])


def test_feature_only_optimizer_gathers_the_geometry_as_plain_tensors():
    name = "mixed"
    pd, max_grad, min_op, extent, mss, shd, _ = _par(name)
    t = {k: Z[f"{name}_{k}"] for k in R.NAMES}
    m = _model(t, shd, None, 3.0, Z[name + "_accum"], Z[name + "_denom"], Z[name + "_max_radii"], rgb=False)
    opt = m.training_setup()
    m._semantic_feature.grad = torch.ones_like(m._semantic_feature)
    opt.step()
    m1 = opt.state[m._semantic_feature]["exp_avg"].cpu().numpy().copy()
    m2 = opt.state[m._semantic_feature]["exp_avg_sq"].cpu().numpy().copy()
    feat = m._semantic_feature.detach().cpu().numpy().copy()
    m.densify_and_prune(max_grad, min_op, extent, mss, samples=torch.from_numpy(Z[name + "_Z"]).to(DEV))
    src, kind = Z[name + "_src"], Z[name + "_kind"]
    ref32 = {k: Z[f"{name}_f32_{k}"] for k in R.NAMES}
    ref32["semantic_feature"] = feat[src]
    ref64 = {k: Z[f"{name}_f64_{k}"] for k in R.NAMES}
    keep = (kind == R.KEEP)[:, None]
    _check_model("feature-only", m, kind, ref32, ref64, {"semantic_feature": (np.where(keep, m1[src], 0), np.where(keep, m2[src], 0))},
                 1.0, groups=("semantic_feature",))
    for k, a in ATTR.items():
        assert getattr(m, a).requires_grad == (k == "semantic_feature") and isinstance(getattr(m, a), torch.nn.Parameter), k
    m._semantic_feature.grad = torch.ones_like(m._semantic_feature)
    opt.step()  # the re-keyed state steps on
    assert float(opt.state[m._semantic_feature]["step"]) == 2.0


# ----------------------------------------------------------------------------------------------------------------------
# the gather alone, past 2^31 elements
# ----------------------------------------------------------------------------------------------------------------------
def test_gather_alone_past_two_to_the_31_elements():
    """[4 200 000, 512] fp32: element offsets of the source pass 2^31 (row 4 194 304 on).  The plan drops every 97th row and
    appends 1000 clones; compared with index_select in chunks.  (csrc/densify.hip: the flat index, the row and the source
    offset are int64; the row / column pair is carried along the grid stride.)"""
    from gags_amd import densify
    n, d = 4_200_000, 512
    assert n * d > 2 ** 31
    x = torch.empty((n, d), device=DEV)
    for a in range(0, n, 600_000):
        x[a:a + 600_000] = torch.randn((min(600_000, n - a), d), device=DEV, generator=torch.Generator(device=DEV).manual_seed(a))
    rows = torch.arange(n, device=DEV, dtype=torch.int32)
    kept = rows[rows % 97 != 0]
    clones = kept[torch.linspace(0, kept.numel() - 1, 1000, device=DEV).long()]
    src = torch.cat([kept, clones]).contiguous()
    kind = torch.cat([torch.zeros_like(kept, dtype=torch.uint8), torch.ones_like(clones, dtype=torch.uint8)]).contiguous()
    assert int(src.max()) * d > 2 ** 31 and int(clones.max()) * d > 2 ** 31
    (out,) = densify.gather(src.numel(), src, kind, [(x, False)])
    assert tuple(out.shape) == (src.numel(), d)
    for a in range(0, src.numel(), 500_000):
        want = x.index_select(0, src[a:a + 500_000].long())
        assert torch.equal(out[a:a + 500_000], want), a
    del out, want
    # a moment through the same plan, on the tail that sits past 2^31: kept rows copied, clones zero
    tail = src.numel() - 2000
    (mo,) = densify.gather(src.numel(), src, kind, [(x, True)])
    assert torch.equal(mo[tail:-1000], x.index_select(0, src[tail:-1000].long())) and not bool(mo[-1000:].any())


# ----------------------------------------------------------------------------------------------------------------------
# determinism
# ----------------------------------------------------------------------------------------------------------------------
def test_two_runs_of_one_call_are_bit_identical():
    t, accum, denom, max_radii, par, mom = _random_scene(20000, 16, 3, seed=3, mss=20)
    outs = []
    for _ in range(2):
        m = _model(t, 3, mom, 3.0, accum, denom, max_radii)
        m.densify_and_prune(par["max_grad"], par["min_opacity"], par["extent"], par["mss"],
                            generator=torch.Generator(device=DEV).manual_seed(123))
        st = m.optimizer.state
        outs.append([getattr(m, a).detach() for a in ATTR.values()] + [st[getattr(m, a)]["exp_avg"] for a in ATTR.values()]
                    + [st[getattr(m, a)]["exp_avg_sq"] for a in ATTR.values()])
    assert outs[0][0].shape[0] != 20000
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------------------
# across a densify within one RasterContext; a toy training loop
# ----------------------------------------------------------------------------------------------------------------------
W, H, N0 = 64, 48, 500
STORED = tuple(ATTR.values())


def atomic_reorder_rel(terms):
    """Bound, relative to a tensor's largest magnitude, between two runs of a sum of `terms` fp32 terms added with atomics in
    whatever order they arrive: twice the worst-case reordering error, terms * 2^-23 (also used by tests/test_streams_gpu.py)."""
    return terms * 2.0 ** -23


def _scene(seed=3):
    from gags_amd import synthetic as syn
    pc = syn.make_model(N0, 16, W, H, seed=seed, device=DEV, scale0=syn.SCALE0 * 24)
    cam = syn.make_camera(W, H, view=3, device=DEV)
    return pc, cam, torch.zeros(3, device=DEV)


def _target(pc, cam, bg):
    from gags_amd.gaussian_renderer import render
    g = torch.Generator(device=DEV).manual_seed(11)
    dc = pc._features_dc.detach().clone()
    with torch.no_grad():
        pc._features_dc += 0.5 * torch.randn(dc.shape, device=DEV, generator=g)
        gt = render(cam, pc, None, bg, feature_mode=False)["render"].detach().clamp(0.0, 1.0).contiguous()
        pc._features_dc.copy_(dc)
    return gt


def _forward_backward(pc, cam, bg, gt, ctx):
    from gags_amd import losses
    from gags_amd.gaussian_renderer import render
    pkg = render(cam, pc, None, bg, feature_mode=False, context=ctx)
    loss = losses.photometric_loss(pkg["render"], gt)
    loss.backward()
    return pkg, loss.detach()


def _snapshot_model(pc):
    from gags_amd.scene import GaussianModel
    m = GaussianModel.from_tensors(pc._xyz.detach().clone(), pc._scaling.detach().clone(), pc._rotation.detach().clone(),
                                   pc._opacity.detach().clone(), pc._features_dc.detach().clone(),
                                   pc._features_rest.detach().clone(), pc._semantic_feature.detach().clone(),
                                   sh_degree=pc.max_sh_degree)
    for a in STORED[:-1]:
        getattr(m, a).requires_grad_(True)
    return m


def _stateless_context():
    from gags_amd.rasterization import RasterContext
    ctx = RasterContext(capacity_mode=False)
    ctx.keep_grad_buffer = False
    ctx.early_rowmap = False
    return ctx


def test_steps_across_a_densify_equal_the_stateless_step():
    """render 64 x 48 -> photometric_loss -> backward -> accumulate -> FeatureAdam.step in ONE RasterContext: three steps,
    densify_and_prune, two steps, reset_opacity, one step.  Every step -- in particular the first after N changed and the first
    after the opacity parameter was replaced -- is recomputed from a snapshot of its inputs with new tensors, a fresh context
    and nothing carried.  The render, the loss, the radii, denom and max_radii2D are equal bit for bit.  The RGB backward adds
    with fp32 atomics, so two runs of the SAME step differ in the order of each gradient's <= 64 * 48 terms: gradients and
    accum are compared to 3072 * 2^-23 of the tensor's largest magnitude (twice the worst-case reordering error of a sum of
    3072 terms of that magnitude).  A stale row, a buffer of the old N or a stale activation is an error of the order of the
    gradient itself."""
    from gags_amd import densify
    from gags_amd.rasterization import RasterContext
    pc, cam, bg = _scene()
    gt = _target(pc, cam, bg)
    opt = pc.training_setup_rgb(ARGS)
    pc.cache_activations(True)
    ctx = RasterContext()
    rel = atomic_reorder_rel(W * H)
    assert rel == 3072 * 2.0 ** -23
    sizes = []
    for step in range(6):
        if step == 3:
            pc.densify_and_prune(0.0002, 0.005, 5.0, None, generator=torch.Generator(device=DEV).manual_seed(4))
            assert pc._xyz.shape[0] != N0
        if step == 5:
            pc.reset_opacity()
        snap = _snapshot_model(pc)
        stats0 = (pc.xyz_gradient_accum.clone(), pc.denom.clone(), pc.max_radii2D.clone())
        opt.zero_grad(set_to_none=True)
        pkg, loss = _forward_backward(pc, cam, bg, gt, ctx)
        densify.accumulate(pc, pkg)
        spkg, sloss = _forward_backward(snap, cam, bg, gt, _stateless_context())
        snap.xyz_gradient_accum, snap.denom, snap.max_radii2D = stats0
        densify.accumulate(snap, spkg)
        assert torch.equal(pkg["render"], spkg["render"]) and torch.equal(loss, sloss) and torch.equal(pkg["radii"], spkg["radii"])
        assert torch.equal(pc.denom, snap.denom) and torch.equal(pc.max_radii2D, snap.max_radii2D)
        pairs = [(a, getattr(pc, a).grad, getattr(snap, a).grad) for a in STORED[:-1]]
        pairs.append(("accum", pc.xyz_gradient_accum, snap.xyz_gradient_accum))
        for a, got, want in pairs:
            assert got is not None and got.shape == want.shape and got.shape[0] == pc._xyz.shape[0], (step, a)
            scale = float(want.abs().max())
            assert scale > 0 and float((got - want).abs().max()) <= rel * scale, (step, a, float((got - want).abs().max()), scale)
        opt.step()
        sizes.append(pc._xyz.shape[0])
    assert sizes[0] == sizes[2] == N0 and sizes[3] == sizes[5] != N0 and int(pc.denom.max()) == 3


def _psnr(a, b):
    return float(10 * torch.log10(1.0 / ((a - b) ** 2).mean()))


def test_thirty_step_toy_training_with_and_without_densification():
    """Thirty steps on a 64 x 48 synthetic target, densifying every ten.  Asserted: the point count changed, and every tensor,
    moment and statistic of the model has the same first dimension.  The two final PSNRs are printed (DESIGN section 7 "N8")."""
    from gags_amd import densify
    from gags_amd.gaussian_renderer import render
    from gags_amd.rasterization import RasterContext
    final = {}
    for dens in (False, True):
        pc, cam, bg = _scene()
        gt = _target(pc, cam, bg)
        opt = pc.training_setup_rgb(ARGS)
        ctx = RasterContext()
        for it in range(1, 31):
            pc.update_learning_rate(it)
            opt.zero_grad(set_to_none=True)
            pkg, _ = _forward_backward(pc, cam, bg, gt, ctx)
            densify.accumulate(pc, pkg)
            if dens and it % 10 == 0:
                pc.densify_and_prune(0.0002, 0.005, 5.0, None, generator=torch.Generator(device=DEV).manual_seed(it))
            opt.step()
        with torch.no_grad():
            final[dens] = (_psnr(render(cam, pc, None, bg, feature_mode=False, context=ctx)["render"], gt), pc._xyz.shape[0])
        if dens:
            n = pc._xyz.shape[0]
            assert n != N0
            for a in STORED:
                p = getattr(pc, a)
                assert p.shape[0] == n, a
                st = opt.state.get(p, {})
                assert all(st[k].shape == p.shape for k in ("exp_avg", "exp_avg_sq") if k in st), a
            assert pc.xyz_gradient_accum.shape == (n, 1) and pc.denom.shape == (n, 1) and pc.max_radii2D.shape == (n,)
            assert len(opt.state) <= 7
    print(f"\nPSNR after 30 steps: {final[False][0]:.2f} dB at N = {final[False][1]} without densification, "
          f"{final[True][0]:.2f} dB at N = {final[True][1]} with")
