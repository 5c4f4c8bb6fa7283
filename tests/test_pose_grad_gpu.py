"""N17 on the GPU: viewmats.grad from the projection kernel to render(), against the float64 reference of tests/pose_ref.py.

Bounds (tests 1-3): error = ||got - ref64|| / ||ref64|| over the entries of the pose gradient; yardstick = the same error of
pose_ref run in float32 on the CPU with the float64 run's decisions; a single 12-number quantity makes a per-case ratio noisy,
so the yardstick is POOLED -- the maximum over the cases of the same test -- and the bound is min(F64_CAP, F64_MARGIN x pooled
yardstick) with the project's constants of tests/test_general_camera_gpu.py.  Every case prints HIP error, its own yardstick,
the pooled one and the ratio before it asserts.

Two backward passes of one call are bit-identical on the staged / geometry routes and NOT on the VALU route (final width below 16
or no multiple of 8: D = 3, SH), whose kernels add up over tiles with float atomics.  Where a test says "torch.equal to the same
call without a pose gradient" and the case is on that route, the comparison is made inside one backward pass instead (_seam): the
projection backward is re-run on the pass's own cotangents the other way, and every shared output must be the same bits."""
import contextlib
import copy
import functools
import types

import numpy as np
import pytest
import torch

import pose_ref
from helpers import clamp_census, general_camera, general_scene, rel_l2, to_dev
from test_general_camera_gpu import F64_CAP, F64_MARGIN, FULL_CASES, _cotangents
from test_pose_grad_cpu import REFINE_LR, REFINE_STEPS, refinement_case, translation_error

pytestmark = pytest.mark.gpu

MULT = 30.0      # classic cases: the splat size of tests/test_general_camera_gpu.py (>= 20 Gaussians beyond the clamp in x and y)
MULT_AA = 10.0   # antialiased cases: the splat size of tests/test_antialias_absgrad_gpu.py (compensations spread over (0, 1))
BG = 0.25


def _bound(pooled):
    return min(F64_CAP, F64_MARGIN * pooled)


def _report(label, e, y, pooled):
    print(f"{label}: HIP {e:.3e}, float32 CPU {y:.3e}, pooled {pooled:.3e}, ratio to pooled {e / pooled:.2f}, "
          f"bound {_bound(pooled):.3e}")


# -- 1. the kernel directly --------------------------------------------------------------------------------------------------------

# 70 001 Gaussians are 274 partial rows: more than the 256 threads of the one workgroup that sums them (colsum_kernel in
# csrc/project.hip walks rows t, t + 256, ...), so its second trip is taken; 255 / 256 / 257 straddle one projection workgroup,
# 63 / 64 / 65 one wave.
KERNEL_NS = (1, 63, 64, 65, 255, 256, 257, 700, 70001)
KW, KH = 97, 61


@functools.lru_cache(maxsize=None)
def _kernel_scene(n):
    s = general_scene(n, 3, KW, KH, 303 + n, scale_mult=MULT, **general_camera("pitch_roll", KW, KH))   # (n = 1: on screen)
    rng = np.random.default_rng(n)
    cot = dict(means2d=rng.standard_normal((n, 2)).astype(np.float32), depths=rng.standard_normal(n).astype(np.float32),
               conics=rng.standard_normal((n, 3)).astype(np.float32), opac=rng.standard_normal(n).astype(np.float32))
    # the compensation's cotangent as the RAW kernel forms it, so that all four variants share one reference
    cot["comp"] = cot["opac"] * s["opacities"]
    return s, cot


def _forward_radii(s, vm=None):
    from gags_amd.rasterization import _Project
    with torch.no_grad():
        radii = _Project.apply(to_dev(s["means"]), to_dev(s["quats"]), to_dev(s["scales"]), to_dev(s["viewmat"] if vm is None else vm),
                               to_dev(s["K"]), KW, KH, 0.3, 0.01, 1e10, 0.0)[0]
    return radii


@functools.lru_cache(maxsize=None)
def _kernel_refs():
    """float64 (on the device) and float32 (CPU) autograd of aa_ref.project for every (n, antialiased) of test 1, the loss masked
    to the HIP forward's radii > 0: computed once, never modified.  Returns ({(n, aa): (ref64 [4,4], yardstick)}, pooled)."""
    refs = {}
    for n in KERNEL_NS:
        s, cot = _kernel_scene(n)
        radii = _forward_radii(s).cpu().numpy()
        for aa in (False, True):
            r64 = pose_ref.project_grads(s, KW, KH, radii, cot, antialiased=aa, dev="cuda")["viewmat"]
            r32 = pose_ref.project_grads(s, KW, KH, radii, cot, antialiased=aa, dtype=torch.float32)["viewmat"]
            refs[(n, aa)] = (r64, pose_ref.rel_err(r32, r64) if np.linalg.norm(r64) > 0 else 0.0, radii)
    return refs, max(v[1] for v in refs.values())


def _kernel_inputs(s, cot, raw):
    if raw:
        p = s["raw"]
        geo = [p[k].cuda().contiguous() for k in ("xyz", "rotation", "scaling_log")] + [p["opacity_logit"].reshape(-1).cuda().contiguous()]
    else:
        geo = [to_dev(s[k]) for k in ("means", "quats", "scales")] + [None]
    return geo, {k: to_dev(v) for k, v in cot.items()}


def _pose_entry(lib, n, geo, c, vm, K, radii, raw, aa, outputs=True, fill=7.0):
    """gags_project_bwd_pose on pre-filled outputs: (v_means, v_quats, v_scales, v_logit, v_viewmat)."""
    from gags_amd import _lib
    P = _lib.ptr
    dev = vm.device
    outs = [torch.full((n, k), fill, device=dev) if outputs else None for k in (3, 4, 3)]
    outs.append(torch.full((n,), fill, device=dev) if (outputs and raw) else None)
    v_viewmat = torch.full((4, 4), fill, device=dev)
    rows = lib.gags_project_pose_partials(n)
    partials = torch.full((rows, 12), fill, device=dev)
    flags = (_lib.GAGS_POSE_RAW if raw else 0) | (_lib.GAGS_POSE_AA if aa else 0)
    _lib.check(lib.gags_project_bwd_pose(flags, n, P(geo[0]), P(geo[1]), P(geo[2]), P(geo[3]), 1.0, P(vm), P(K), KW, KH, 0.3,
                                         P(radii), P(c["means2d"]), P(c["depths"]), P(c["conics"]), P(c["opac"]) if raw else None,
                                         P(c["comp"]) if (aa and not raw) else None, *[P(o) for o in outs], P(v_viewmat),
                                         P(partials), rows * 48, _lib.stream()), "gags_project_bwd_pose")
    return outs + [v_viewmat]


def _existing_entry(lib, n, geo, c, vm, K, radii, raw, aa):
    """The entry of today for the variant: (v_means, v_quats, v_scales, v_logit or None)."""
    from gags_amd import _lib
    P = _lib.ptr
    dev = vm.device
    outs = [torch.full((n, k), 3.0, device=dev) for k in (3, 4, 3)]
    head = (n, P(geo[0]), P(geo[1]), P(geo[2]))
    cot = (P(radii), P(c["means2d"]), P(c["depths"]), P(c["conics"]))
    if raw:
        v_logit = torch.full((n,), 3.0, device=dev)
        entry = lib.gags_project_bwd_raw_aa if aa else lib.gags_project_bwd_raw
        _lib.check(entry(*head, P(geo[3]), 1.0, P(vm), P(K), KW, KH, 0.3, *cot, P(c["opac"]), *[P(o) for o in outs], P(v_logit),
                         _lib.stream()), "gags_project_bwd_raw*")
        return outs + [v_logit]
    if aa:
        _lib.check(lib.gags_project_bwd_aa(*head, P(vm), P(K), KW, KH, 0.3, *cot, P(c["comp"]), *[P(o) for o in outs], _lib.stream()),
                   "gags_project_bwd_aa")
    else:
        _lib.check(lib.gags_project_bwd(*head, P(vm), P(K), KW, KH, 0.3, P(radii), None, *cot[1:], *[P(o) for o in outs],
                                        _lib.stream()), "gags_project_bwd")
    return outs + [None]


@pytest.mark.parametrize("raw,aa", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("n", KERNEL_NS)
def test_pose_kernel_against_float64_and_the_existing_entries(n, raw, aa):
    """gags_project_bwd_pose after the projection forward, random cotangents, against float64 autograd of aa_ref.project on the
    device.  Per case: the scene gradients are torch.equal to the existing entry's; with them NULL v_viewmat is the same bits;
    two runs are the same bits; row 3 is exactly zero.  Measured on an MI355X: see docs/LAB_NOTES.md, "Camera pose gradients
    (N17)" (HIP error 6.5e-8 .. 3.8e-7; float32 CPU yardsticks 2.6e-8 .. 4.5e-6 per case, pooled 4.5e-6, bound 1.35e-5)."""
    from gags_amd import _lib
    lib = _lib.load()
    refs, pooled = _kernel_refs()
    r64, y, radii_np = refs[(n, aa)]
    s, cot = _kernel_scene(n)
    geo, c = _kernel_inputs(s, cot, raw)
    vm, K = to_dev(s["viewmat"]), to_dev(s["K"])
    radii = to_dev(radii_np)
    nvis = int((radii_np > 0).sum())
    assert nvis >= 1 and (n - nvis >= 1 or n == 1), (nvis, n)
    got = _pose_entry(lib, n, geo, c, vm, K, radii, raw, aa)
    old = _existing_entry(lib, n, geo, c, vm, K, radii, raw, aa)
    for a, b, name in zip(got[:4], old, ("v_means", "v_quats", "v_scales", "v_opacity_logit")):
        assert (a is None and b is None) or torch.equal(a, b), name
    v = got[4]
    assert torch.equal(v, _pose_entry(lib, n, geo, c, vm, K, radii, raw, aa, outputs=False, fill=-5.0)[4])
    assert torch.equal(v, _pose_entry(lib, n, geo, c, vm, K, radii, raw, aa, fill=11.0)[4])
    assert bool((v[3] == 0).all()) and bool(torch.isfinite(v).all())
    e = pose_ref.rel_err(v.cpu().numpy(), r64)
    print()
    _report(f"kernel n={n} raw={raw} aa={aa} ({nvis} visible)", e, y, pooled)
    assert e <= _bound(pooled)


@pytest.mark.parametrize("raw,aa", [(False, False), (False, True), (True, False), (True, True)])
def test_pose_kernel_with_everything_culled_and_with_no_gaussians(raw, aa):
    from gags_amd import _lib
    lib = _lib.load()
    n = 700
    s, cot = _kernel_scene(n)
    away = s["viewmat"].copy()
    away[:3] *= -1.0   # the camera turned away: every Gaussian behind it
    radii = _forward_radii(s, away)
    assert not bool(radii.any())
    geo, c = _kernel_inputs(s, cot, raw)
    got = _pose_entry(lib, n, geo, c, to_dev(away), to_dev(s["K"]), radii, raw, aa)
    assert not bool(got[4].any())
    assert all(g is None or not bool(g.any()) for g in got[:3])
    empty = [t[:0].contiguous() if t is not None else None for t in geo]
    c0 = {k: t[:0].contiguous() for k, t in c.items()}
    assert not bool(_pose_entry(lib, 0, empty, c0, to_dev(away), to_dev(s["K"]), radii[:0].contiguous(), raw, aa)[4].any())


# -- 2 / 3. rasterization() --------------------------------------------------------------------------------------------------------

def _case(name, cam, w, h, n, d, seed, mult=MULT, aa=False, render_mode="RGB", sh_degree=None, centred=False):
    return dict(name=name, cam=cam, w=w, h=h, n=n, d=d, seed=seed, mult=mult, aa=aa, render_mode=render_mode, sh_degree=sh_degree,
                centred=centred)


RASTER_CASES = [_case(f"{c[0]}-D{c[4]}", *c) for c in FULL_CASES] + [
    _case("pp_outside-D3", "pp_outside", 97, 61, 700, 3, 21),
    _case("pp_outside-D16-aa", "pp_outside", 97, 61, 700, 16, 21, mult=MULT_AA, aa=True),
    _case("behind-D128-aa", "behind", 104, 72, 700, 128, 122, mult=MULT_AA, aa=True),
    _case("render-scene-D16", "upside_down", 97, 61, 700, 16, 61, centred=True)]      # (test 5 runs it through render())
DEPTH_SH_CASES = [_case("behind-RGB+ED", "behind", 104, 72, 700, 15, 232, render_mode="RGB+ED"),      # (15 + 1 channels: geometry pass)
                  _case("pitch_roll-SH3", "pitch_roll", 97, 61, 700, 3, 741, sh_degree=3)]
ALL_CASES = {c["name"]: c for c in RASTER_CASES + DEPTH_SH_CASES}
SCENE = ("means", "quats", "scales", "opacities", "colors")
RAW_NAMES = dict(means="xyz", quats="rotation", scales="scaling_log", opacities="opacity_logit")


@functools.lru_cache(maxsize=None)
def _scene(name):
    c = ALL_CASES[name]
    k = general_camera(c["cam"], c["w"], c["h"])
    if c["centred"]:
        k = dict(k, cx=0.5 * c["w"], cy=0.5 * c["h"])
    s = general_scene(c["n"], c["d"], c["w"], c["h"], c["seed"], scale_mult=c["mult"], **k)
    colors = s["sh"] if c["sh_degree"] is not None else s["colors"]
    d_out = colors.shape[1] if c["sh_degree"] is None else 3
    d_out += 1 if c["render_mode"] != "RGB" else 0
    return s, colors, np.full(d_out - (1 if c["render_mode"] != "RGB" else 0), BG, np.float32), _cotangents(c["seed"], c["h"], c["w"], d_out), k


def _atomic_route(name):
    """The case's backward runs on gags_raster_bwd, the VALU kernels (final width below 16, or no multiple of 8): they add
    v_means2d / v_conics / v_opacities / v_colors up with float atomics over tiles, so two backward passes of one and the same
    call already differ in the last bits -- with or without a pose gradient, before and after N17."""
    from gags_amd import rasterization as R
    c = ALL_CASES[name]
    d = (3 if c["sh_degree"] is not None else c["d"]) + (1 if c["render_mode"] != "RGB" else 0)
    return R._route(c["n"], d, False, (True,) * 5, 0, False).bwd == "valu"


@contextlib.contextmanager
def _seam():
    """While active, every projection backward is run three ways ON THE SAME COTANGENTS: as the call asked, as a call without a
    pose gradient asks (the entries of before N17), and as a call that wants the pose and every scene gradient asks.  Yields
    the list of torch.equal results over all outputs that two of them share.  This is the comparison "the pose changes nothing
    else" / "frozen scene tensors change nothing" inside ONE backward pass: it holds bit for bit on every route, the atomic
    one included, where a comparison between two passes cannot."""
    from gags_amd import raster_project as RP
    seen = []
    origs = {cls: cls.backward for cls in (RP._Project, RP._ProjectRaw)}

    def spy_for(cls, n_scene, n_inputs):
        orig = origs[cls]

        def spy(ctx, *grads):
            real = orig(ctx, *grads)
            for pose in (False, True):
                needs = (True,) * n_scene + (pose,) + (False,) * (n_inputs - n_scene - 1)
                fake = types.SimpleNamespace(saved_tensors=ctx.saved_tensors, cfg=ctx.cfg, needs_input_grad=needs)
                other = orig(fake, *grads)
                seen.extend(torch.equal(a, b) for a, b in zip(real, other) if a is not None and b is not None)
            return real
        return staticmethod(spy)
    RP._Project.backward, RP._ProjectRaw.backward = spy_for(RP._Project, 3, 12), spy_for(RP._ProjectRaw, 4, 15)
    try:
        yield seen
    finally:
        for cls, orig in origs.items():
            cls.backward = staticmethod(orig)


def _run(name, *, pose=True, scene=True, raw=False):
    """rasterization() on a case with a background and a non-zero v_alpha: dict(out, alphas, g = scene gradients, vm = viewmats.grad)."""
    from gags_amd.rasterization import rasterization
    c = ALL_CASES[name]
    s, colors, bg, v, _ = _scene(name)
    if raw:
        L = {k: s["raw"][r].cuda() for k, r in RAW_NAMES.items()}
    else:
        L = {k: to_dev(s[k]) for k in SCENE[:4]}
    L["colors"] = to_dev(colors)
    for t in L.values():
        t.requires_grad_(scene)
    vm = to_dev(s["viewmat"])[None].requires_grad_(pose)
    out, alphas, info = rasterization(L["means"], L["quats"], L["scales"], L["opacities"], L["colors"], vm, to_dev(s["K"])[None],
                                      c["w"], c["h"], backgrounds=to_dev(bg)[None], render_mode=c["render_mode"],
                                      sh_degree=c["sh_degree"], rasterize_mode="antialiased" if c["aa"] else "classic",
                                      raw_params=raw)
    with _seam() as seam:
        ((out[0] * to_dev(v[0])).sum() + (alphas[0, ..., 0] * to_dev(v[1])).sum()).backward()
    torch.cuda.synchronize()
    return dict(out=out[0].detach(), alphas=alphas[0, ..., 0].detach(), g={k: t.grad for k, t in L.items() if t.grad is not None},
                vm=vm.grad, radii=info["radii"][0], seam=seam)


@functools.lru_cache(maxsize=None)
def _reference(oracle, name):
    """float64 on the device and float32 on the CPU (with the float64 run's blend decisions) for one case: computed once, never
    modified.  Radii and depth order are the fp32 oracle's."""
    c = ALL_CASES[name]
    s, colors, bg, v, _ = _scene(name)
    radii, _, depths, _ = oracle.project_fwd(s["means"], s["quats"], s["scales"], s["viewmat"], s["K"], c["w"], c["h"])
    kw = dict(antialiased=c["aa"], render_mode=c["render_mode"], sh_degree=c["sh_degree"])
    r64 = pose_ref.full(s, c["w"], c["h"], colors, bg, v[0], v[1], radii, depths, dev="cuda", **kw)
    r32 = pose_ref.full(s, c["w"], c["h"], colors, bg, v[0], v[1], radii, depths, dtype=torch.float32, include=r64["include"].cpu(), **kw)
    cut = None
    if c["sh_degree"] is not None:
        cut = pose_ref.full(s, c["w"], c["h"], colors, bg, v[0], v[1], radii, depths, dev="cuda", include=r64["include"],
                            detach_campos=True, **kw)["g"]["viewmat"]
    return dict(radii=radii, out=r64["out"], vm=r64["g"]["viewmat"], y=pose_ref.rel_err(r32["g"]["viewmat"], r64["g"]["viewmat"]),
                vm_cut=cut)


def _pooled(oracle, cases):
    return max(_reference(oracle, c["name"])["y"] for c in cases)


def _check_nothing_else_changed(name, r, plain):
    """`out`, `alphas` and every scene gradient of the run with a pose gradient against the same call without: torch.equal.
    On the atomic route (_atomic_route) two backward passes are not reproducible in themselves, so the gradients are compared
    where that does not enter -- inside each backward pass, on its own cotangents (_seam) -- and the difference between the two
    passes is printed."""
    assert plain["vm"] is None and torch.equal(r["out"], plain["out"]) and torch.equal(r["alphas"], plain["alphas"])
    assert set(r["g"]) == set(plain["g"]) == set(SCENE)
    for x in (r, plain):
        assert len(x["seam"]) >= 6 and all(x["seam"]), x["seam"]
    if _atomic_route(name):
        print("atomic route, pass to pass:", {k: f"{rel_l2(r['g'][k].cpu().numpy(), plain['g'][k].cpu().numpy()):.1e}" for k in SCENE})
        return
    for k in SCENE:
        assert torch.equal(r["g"][k], plain["g"][k]), k


def _check_pose_gradient(oracle, name, cases, r):
    ref = _reference(oracle, name)
    pooled = _pooled(oracle, cases)
    np.testing.assert_array_equal(r["radii"].cpu().numpy(), ref["radii"])
    assert rel_l2(r["out"].cpu().numpy(), ref["out"]) < 1e-5          # (the same render: the decisions agree)
    assert r["vm"].shape == (1, 4, 4) and r["vm"].dtype == torch.float32
    # (row 3: exactly zero from the projection; the SH view direction reaches it through torch's 4 x 4 inverse, in the reference too)
    assert bool((r["vm"][0, 3] == 0).all()) == (ALL_CASES[name]["sh_degree"] is None)
    e = pose_ref.rel_err(r["vm"][0].cpu().numpy(), ref["vm"])
    print()
    _report(f"rasterization() {name}", e, ref["y"], pooled)
    assert e <= _bound(pooled)
    return ref, pooled


@pytest.mark.parametrize("name", [c["name"] for c in RASTER_CASES])
def test_viewmats_grad_through_rasterization(oracle, name):
    """viewmats.grad [1,4,4] against pose_ref in float64 -- the four general cameras at D = 16 (VALU geometry route) and D = 128
    (matrix-core route), D = 3, two antialiased cases at scale_mult = 10 and the scene of the render() test -- and every other
    gradient, `out` and `alphas` torch.equal to the same call with viewmats not requiring grad.  Measured on an MI355X: see
    docs/LAB_NOTES.md, "Camera pose gradients (N17)" (HIP error 2.4e-6 .. 9.6e-6, each case's own float32 yardstick 2.8e-6 ..
    9.0e-6, HIP / own yardstick 0.86 .. 1.31, pooled 9.0e-6, bound 2.7e-5).  The D = 3 case runs on the atomic route: see
    _check_nothing_else_changed."""
    c = ALL_CASES[name]
    s = _scene(name)[0]
    if not c["aa"]:
        nx, ny, nvis, ncull = clamp_census(s, c["w"], c["h"], _reference(oracle, name)["radii"])
        assert nx >= 20 and ny >= 20 and nvis > 0 and ncull > 0, (nx, ny, nvis, ncull)
    r = _run(name)
    _check_pose_gradient(oracle, name, RASTER_CASES, r)
    _check_nothing_else_changed(name, r, _run(name, pose=False))


def test_viewmats_grad_with_raw_parameters(oracle):
    """raw_params=True: the same pose gradient as the activated call of the case (the stored parameters activate to the same
    bits), inside the same bound; the stored parameters' gradients unchanged by the pose."""
    name = "pp_outside-D16"
    r = _run(name, raw=True)
    _check_pose_gradient(oracle, name, RASTER_CASES, r)
    _check_nothing_else_changed(name, r, _run(name, pose=False, raw=True))


@pytest.mark.parametrize("name", [c["name"] for c in DEPTH_SH_CASES])
def test_viewmats_grad_in_depth_and_sh_modes(oracle, name):
    """RGB+ED (v_depths and the ED division reach the pose) and sh_degree = 3 with the camera far from the origin (the view
    direction reaches it through campos = inverse(viewmat)[:3, 3]).  The float64 reference with campos detached differs from
    the full one by more than ten times the bound: without _SH's v_campos the SH case cannot pass.  Measured on an MI355X: see
    docs/LAB_NOTES.md, "Camera pose gradients (N17)" (HIP 7.4e-6 / 4.4e-6, float32 yardsticks 8.5e-6 / 4.0e-6, pooled 8.5e-6, bound
    2.6e-5; with campos detached the reference moves by 0.15, 5900 x the bound).  The SH case runs on the atomic route."""
    c = ALL_CASES[name]
    r = _run(name)
    ref, pooled = _check_pose_gradient(oracle, name, DEPTH_SH_CASES, r)
    if c["sh_degree"] is not None:
        assert np.linalg.norm(np.linalg.inv(_scene(name)[0]["viewmat"].astype(np.float64))[:3, 3]) > 7.0
        share = pose_ref.rel_err(ref["vm_cut"], ref["vm"])
        print(f"campos detached: the reference moves by {share:.3e} ({share / _bound(pooled):.0f} x the bound)")
        assert share > 10 * _bound(pooled)
    _check_nothing_else_changed(name, r, _run(name, pose=False))


# -- 4. pose only ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["pitch_roll-D16", "behind-D128", "pp_outside-D3", "pp_outside-D16-aa", "behind-RGB+ED", "pitch_roll-SH3"])
def test_pose_only_with_every_scene_tensor_frozen(name):
    """Only viewmats requires grad (needs = (True, True, False, ...) through _route and _Rasterize, on the matrix-core and the
    VALU routes, in RGB, RGB+ED and SH modes): viewmats.grad is torch.equal to the all-gradients run's, and no scene tensor gets
    a gradient.  On the atomic route (_atomic_route: D = 3 and SH) the comparison is made inside the pose-only backward pass, on
    its own cotangents (_seam: the pose entry with every scene output wanted gives the same v_viewmat bits), and the pass-to-pass
    difference of viewmats.grad is printed and held to F64_CAP (1e-4, the project's bound for that route against the oracle)."""
    runs = [(False, _run(name), _run(name, scene=False))]
    if ALL_CASES[name]["render_mode"] == "RGB" and ALL_CASES[name]["sh_degree"] is None:
        runs.append((True, _run(name, raw=True), _run(name, scene=False, raw=True)))
    for raw, full, only in runs:
        assert only["g"] == {} and only["vm"] is not None and torch.equal(only["out"], full["out"])
        assert len(only["seam"]) >= 1 and all(only["seam"]) and all(full["seam"])
        if _atomic_route(name):
            e = pose_ref.rel_err(only["vm"].cpu().numpy(), full["vm"].cpu().numpy())
            print(f"\natomic route, pose only vs all gradients, pass to pass: {e:.1e}")
            assert e <= F64_CAP
        else:
            assert torch.equal(only["vm"], full["vm"]), raw


# -- 5. render() -------------------------------------------------------------------------------------------------------------------

def _model_and_camera(name):
    from gags_amd.scene import Camera, GaussianModel, focal2fov
    c = ALL_CASES[name]
    s, _, _, _, k = _scene(name)
    R, C = s["R"], s["C"]
    cam = Camera(R, -R.T @ C, focal2fov(k["fx"], c["w"]), focal2fov(k["fy"], c["h"]), c["w"], c["h"], device="cuda")
    p = {key: (v.cuda() if torch.is_tensor(v) else v) for key, v in s["raw"].items()}
    pc = GaussianModel.from_tensors(p["xyz"], p["scaling_log"], p["rotation"], p["opacity_logit"], p["features_dc"],
                                    p["features_rest"], p["semantic_feature"])
    return pc, cam


@pytest.mark.parametrize("raw_path", [True, False])
def test_render_gives_a_trainable_camera_its_gradient(oracle, monkeypatch, raw_path):
    """A GaussianModel and a camera whose world_view_transform requires grad, through render() on the raw-parameter path and on
    the getter path: the gradient is the transpose of rasterization()'s viewmats.grad for the same scene -- the same bits as the
    direct call with the same inputs -- and inside test 2's bound against float64."""
    from gags_amd import gaussian_renderer
    from gags_amd.rasterization import rasterization
    name = "render-scene-D16"
    c = ALL_CASES[name]
    s, colors, bg, v, _ = _scene(name)
    monkeypatch.setattr(gaussian_renderer, "RAW_PARAMS", raw_path)
    pc, cam = _model_and_camera(name)
    assert np.abs(cam.world_view_transform.T.cpu().numpy() - s["viewmat"]).max() < 1e-5
    cam.world_view_transform = cam.world_view_transform.clone().requires_grad_(True)
    pkg = gaussian_renderer.render(cam, pc, None, torch.full((3,), BG, device="cuda"), feature_mode=True)
    ((pkg["render"].permute(1, 2, 0) * to_dev(v[0])).sum() + (pkg["alphas"] * to_dev(v[1])).sum()).backward()
    g = cam.world_view_transform.grad
    assert g is not None and g.shape == (4, 4) and bool((g[:, 3] == 0).all())
    # the direct call with the same inputs
    vm = cam.world_view_transform.detach().T[None].contiguous().requires_grad_(True)
    if raw_path:
        args, kw = (pc._xyz, pc._rotation, pc._scaling, pc._opacity.squeeze(-1)), dict(raw_params=True)
    else:
        args, kw = (pc.get_xyz, pc.get_rotation, pc.get_scaling, pc.get_opacity.squeeze(-1)), {}
    with torch.no_grad():
        args = tuple(a.detach().clone() for a in args)
    out, alphas, _ = rasterization(*args, pc.get_semantic_feature.detach(), vm, gaussian_renderer._intrinsics(cam, "cuda", {})[None],
                                   c["w"], c["h"], backgrounds=to_dev(bg)[None], **kw)
    ((out[0] * to_dev(v[0])).sum() + (alphas[0, ..., 0] * to_dev(v[1])).sum()).backward()
    assert torch.equal(g, vm.grad[0].T)
    # ... and against float64 (the camera's fp32 matrix differs from the scene's in the last bits: the bound covers it)
    ref, pooled = _reference(oracle, name), _pooled(oracle, RASTER_CASES)
    e = pose_ref.rel_err(g.T.cpu().numpy(), ref["vm"])
    print()
    _report(f"render() raw path={raw_path}", e, ref["y"], pooled)
    assert e <= _bound(pooled)


# -- 6. refinement -----------------------------------------------------------------------------------------------------------------

def test_pose_refinement_through_render_and_pose_delta():
    """The float64 case of tests/test_pose_grad_cpu.py::test_pose_refinement_in_float64_recovers_the_pose on the GPU: render() of a
    frozen GaussianModel, PoseDelta.camera, L1 to the image of the true pose, Adam, 40 steps.  The loss and the translation
    error each fall at least two-fold; the reference's own reduction (26.9-fold and 16.4-fold) is the margin.
    Measured on an MI355X: loss 0.0214 -> 0.0007 (31.7-fold), translation error 0.446 -> 0.0253 (17.6-fold)."""
    from gags_amd.gaussian_renderer import render
    from gags_amd.pose import PoseDelta
    from gags_amd.scene import Camera, GaussianModel, focal2fov
    c = refinement_case()
    s, w, h, k = c["s"], c["w"], c["h"], c["k"]
    R, C = s["R"], s["C"]
    cam_true = Camera(R, -R.T @ C, focal2fov(k["fx"], w), focal2fov(k["fy"], h), w, h, device="cuda")
    p = {key: (v.cuda() if torch.is_tensor(v) else v) for key, v in s["raw"].items()}
    pc = GaussianModel.from_tensors(p["xyz"], p["scaling_log"], p["rotation"], p["opacity_logit"], p["features_dc"],
                                    p["features_rest"], p["semantic_feature"])
    bg = torch.full((3,), float(c["bg"][0]), device="cuda")
    with torch.no_grad():
        gt = render(cam_true, pc, None, bg)["render"].clone()
    cam0 = copy.copy(cam_true)
    cam0.world_view_transform = to_dev(c["vm0"].astype(np.float32)).T.contiguous()
    poses = PoseDelta(1).cuda()
    opt = torch.optim.Adam(poses.parameters(), lr=REFINE_LR)
    losses, terr = [], []
    for _ in range(REFINE_STEPS + 1):
        cam = poses.camera(cam0, 0)
        loss = (render(cam, pc, None, bg)["render"] - gt).abs().mean()
        losses.append(float(loss.detach()))
        terr.append(translation_error(cam.world_view_transform.detach().T.cpu().numpy(), c["vm_true"]))
        opt.zero_grad()
        loss.backward()
        assert poses.delta.grad is not None and bool(torch.isfinite(poses.delta.grad).all())
        opt.step()
    print(f"\nGPU refinement: loss {losses[0]:.4f} -> {losses[-1]:.4f} ({losses[0] / losses[-1]:.1f}-fold), "
          f"translation error {terr[0]:.3f} -> {terr[-1]:.4f} ({terr[0] / terr[-1]:.1f}-fold)")
    assert losses[0] / losses[-1] >= 2.0 and terr[0] / terr[-1] >= 2.0
