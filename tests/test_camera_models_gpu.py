"""Camera models (N20) on the GPU: gags_project_fwd_cam / gags_project_bwd_cam at the lane, wave and workgroup edges, through
rasterization() on both geometry routes, and through render().  Truth is the float64 restatement of tests/camera_models_ref.py
(autograd); the bound on a float is min(F64_CAP, F64_MARGIN x the error of a float32 yardstick against the same float64) -- at
kernel level the float32 CPU restatement, through rasterization() the project's pinhole path on the same scene and K.  The
orthographic forward has no transcendental function and is compared bit for bit with the kernel-order restatement.  Integers
are exact except for Gaussians float64 puts within 1e-5 of a decision boundary (at most 2 %; the CPU tests pin the seeds)."""
import functools

import numpy as np
import pytest
import torch

import aa_ref
import camera_models_ref as cm
from helpers import rel_l2, to_dev
from test_general_camera_gpu import F64_CAP, F64_MARGIN

pytestmark = pytest.mark.gpu

F64 = torch.float64
W, H = cm.KERNEL_W, cm.KERNEL_H
RAW, AA, POSE = 1, 2, 4
FLOATS = ("means2d", "depths", "conics", "comp")


def _bound(e32):
    return min(F64_CAP, F64_MARGIN * e32)


@functools.lru_cache(maxsize=None)
def _kscene(model, eps2d=0.3):
    return cm.model_scene(model, 700, 0, W, H, cm.KERNEL_SEEDS[model]), dict(cm.KERNEL_CULL, eps2d=eps2d)


def _cut(s, n, start=0):
    """n Gaussians of a scene, the first n or those from `start` on."""
    out = dict(s)
    for k in ("means", "quats", "scales", "opacities"):
        out[k] = s[k][start:start + n]
    out["raw"] = {k: (v[start:start + n] if torch.is_tensor(v) else v) for k, v in s["raw"].items()}
    return out


def _inputs(s, flags):
    if flags & RAW:
        p = s["raw"]
        return (p["xyz"].cuda().contiguous(), p["rotation"].cuda().contiguous(), p["scaling_log"].cuda().contiguous(),
                p["opacity_logit"].reshape(-1).cuda().contiguous())
    return to_dev(s["means"]), to_dev(s["quats"]), to_dev(s["scales"]), None


def _fwd_outputs(n, flags, extras):
    """The forward's outputs, pre-filled: what an entry does not write shows.  extras (RAW): quats_act, scales_act and the
    [max(n, 1), 8] record table too, else None (passed as NULL)."""
    extra = lambda *shape: torch.full(shape, 7.0, device="cuda") if (extras and flags & RAW) else None  # noqa: E731
    return dict(radii=torch.full((n,), -7, dtype=torch.int32, device="cuda"), means2d=torch.full((n, 2), 7.0, device="cuda"),
                depths=torch.full((n,), 7.0, device="cuda"), conics=torch.full((n, 3), 7.0, device="cuda"),
                tiles=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
                opac=torch.full((n,), 7.0, device="cuda") if flags & RAW else None,
                quats_act=extra(n, 4), scales_act=extra(n, 3), grec=extra(max(n, 1), 8),
                comp=torch.full((n,), 7.0, device="cuda") if flags & AA else None)


def k_fwd(model, flags, s, cull, modifier=1.0, extras=False):
    """gags_project_fwd_cam on a scene: dict of GPU tensors (radii, means2d, depths, conics, tiles, opac | None, quats_act |
    None, scales_act | None, grec | None, comp | None)."""
    from gags_amd import _lib
    from gags_amd._lib import check, ptr
    lib = _lib.load()
    means, quats, scales, logit = _inputs(s, flags)
    vm, K = to_dev(s["viewmat"]), to_dev(s["K"])      # (held here: a temporary's memory would be reused before the launch)
    n = means.shape[0]
    o = _fwd_outputs(n, flags, extras)
    check(lib.gags_project_fwd_cam(cm.MODELS[model], flags, n, ptr(means), ptr(quats), ptr(scales), ptr(logit), modifier,
                                   ptr(vm), ptr(K), W, H, cull["eps2d"], cull["near_plane"],
                                   cull["far_plane"], cull["radius_clip"], ptr(o["radii"]), ptr(o["means2d"]), ptr(o["depths"]),
                                   ptr(o["conics"]), ptr(o["tiles"]), ptr(o["opac"]), ptr(o["quats_act"]), ptr(o["scales_act"]),
                                   ptr(o["grec"]), ptr(o["comp"]), _lib.stream()), "gags_project_fwd_cam")
    torch.cuda.synchronize()
    return o


def named_fwd(flags, s, cull, modifier=1.0, extras=False):
    """k_fwd's dict from the named pinhole entry of `flags`: gags_project_fwd / _aa / _raw / _raw_aa, called directly."""
    from gags_amd import _lib
    from gags_amd._lib import check, ptr
    lib = _lib.load()
    means, quats, scales, logit = _inputs(s, flags)
    vm, K = to_dev(s["viewmat"]), to_dev(s["K"])
    n = means.shape[0]
    o = _fwd_outputs(n, flags, extras)
    name = "gags_project_fwd" + ("_raw" if flags & RAW else "") + ("_aa" if flags & AA else "")
    check(getattr(lib, name)(n, ptr(means), ptr(quats), ptr(scales), *((ptr(logit), modifier) if flags & RAW else ()), ptr(vm),
                             ptr(K), W, H, cull["eps2d"], cull["near_plane"], cull["far_plane"], cull["radius_clip"],
                             ptr(o["radii"]), ptr(o["means2d"]), ptr(o["depths"]), ptr(o["conics"]), ptr(o["tiles"]),
                             *((ptr(o["opac"]), ptr(o["quats_act"]), ptr(o["scales_act"]), ptr(o["grec"])) if flags & RAW else ()),
                             *((ptr(o["comp"]),) if flags & AA else ()), _lib.stream()), name)
    torch.cuda.synchronize()
    return o


def k_bwd(model, flags, s, cull, radii, cot, modifier=1.0, skip=(), entry="cam"):
    """gags_project_bwd_cam: dict(means, quats, scales, opacities | None, viewmat [4,4] | None) of GPU tensors.  skip: outputs
    passed as NULL (POSE only).  entry="old": the same through the entry without a camera model (pinhole) that `flags` names,
    gags_project_bwd_pose with POSE, else gags_project_bwd / _aa / _raw / _raw_aa."""
    from gags_amd import _lib
    from gags_amd._lib import check, ptr
    lib = _lib.load()
    means, quats, scales, logit = _inputs(s, flags)
    n = means.shape[0]
    raw, aa, pose = bool(flags & RAW), bool(flags & AA), bool(flags & POSE)
    g = dict(means=torch.full((n, 3), 7.0, device="cuda"), quats=torch.full((n, 4), 7.0, device="cuda"),
             scales=torch.full((n, 3), 7.0, device="cuda"), opacities=torch.full((n,), 7.0, device="cuda") if raw else None,
             viewmat=torch.full((4, 4), 7.0, device="cuda") if pose else None)
    for k in skip:
        g[k] = None
    rows = lib.gags_project_pose_partials(n)
    partials = torch.full((rows, 12), 7.0, device="cuda") if pose else None
    v_opac = to_dev(cot["opacities"][:n]) if raw else None
    v_comp = to_dev(cot["comp"][:n]) if (aa and not raw) else None
    vm, K = to_dev(s["viewmat"]), to_dev(s["K"])      # (held here: a temporary's memory would be reused before the launch)
    v_m2, v_z, v_con = to_dev(cot["means2d"][:n]), to_dev(cot["depths"][:n]), to_dev(cot["conics"][:n])
    common = (n, ptr(means), ptr(quats), ptr(scales), ptr(logit), modifier, ptr(vm), ptr(K), W, H,
              cull["eps2d"], ptr(radii), ptr(v_m2), ptr(v_z),
              ptr(v_con), ptr(v_opac), ptr(v_comp), ptr(g["means"]), ptr(g["quats"]), ptr(g["scales"]),
              ptr(g["opacities"]), ptr(g["viewmat"]), ptr(partials), 0 if partials is None else partials.numel() * 4, _lib.stream())
    if entry == "cam":
        check(lib.gags_project_bwd_cam(cm.MODELS[model], flags, *common), "gags_project_bwd_cam")
    elif pose:
        assert model == "pinhole"
        check(lib.gags_project_bwd_pose(flags & 3, *common), "gags_project_bwd_pose")
    else:  # the named pinhole entry of `flags`: gags_project_bwd / _aa / _raw / _raw_aa
        assert model == "pinhole"
        name = "gags_project_bwd" + ("_raw" if raw else "") + ("_aa" if aa else "")
        conics = torch.full((n, 3), 7.0, device="cuda")   # gags_project_bwd's ignored argument: a real tensor
        check(getattr(lib, name)(n, ptr(means), ptr(quats), ptr(scales), *((ptr(logit), modifier) if raw else ()), ptr(vm), ptr(K),
                                 W, H, cull["eps2d"], ptr(radii), *(() if (raw or aa) else (ptr(conics),)), ptr(v_m2), ptr(v_z),
                                 ptr(v_con), *((ptr(v_opac),) if raw else ()), *((ptr(v_comp),) if (aa and not raw) else ()),
                                 ptr(g["means"]), ptr(g["quats"]), ptr(g["scales"]), *((ptr(g["opacities"]),) if raw else ()),
                                 _lib.stream()), name)
    torch.cuda.synchronize()
    return g


def _truth(model, s, cull, flags, dtype, cot=None, radii=None):
    """The restatement in `dtype` on the CPU: (outputs dict, decisions, gradients dict | None)."""
    raw = bool(flags & RAW)
    pr, dec, L = cm.run(model, s, W, H, dtype, raw=raw, grad=cot is not None, **cull)
    o = cm.outputs(pr, dec)
    if raw:
        vis = dec["radii"] > 0
        op = L["opac_act"].detach().numpy()
        o["opac"] = op * np.where(vis, o["comp"], 0) if flags & AA else op
    g = None
    if cot is not None:
        n = s["means"].shape[0]
        c = {k: v[:n] for k, v in cot.items()}
        cm.project_loss(pr, radii, c, antialiased=bool(flags & AA), opac_act=L.get("opac_act")).backward()
        g = {k: (L[k].grad.numpy() if L[k].grad is not None else np.zeros(tuple(L[k].shape))) for k in L if k != "opac_act"}
    return o, dec, g


def _check_ints(got, dec, label):
    keep = ~dec["close"]
    assert (~keep).sum() <= cm.MAX_EXCLUDED * keep.size, (label, (~keep).sum())
    np.testing.assert_array_equal(got["radii"].cpu().numpy()[keep], dec["radii"][keep], err_msg=label)
    np.testing.assert_array_equal(got["tiles"].cpu().numpy()[keep], dec["tiles"][keep], err_msg=label)
    return keep


# -- kernel level: forward --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", cm.KERNEL_SIZES)
@pytest.mark.parametrize("eps2d", [0.3, 0.0])
def test_ortho_forward_is_bit_equal_to_the_kernel_order_restatement(n, eps2d):
    """RAW x AA: radii and tile counts exact, means2d, conics, depths, compensations (and the activated, compensated opacity)
    bit for bit the float32 operation-order restatement."""
    s0, cull = _kscene("ortho", eps2d)
    s = _cut(s0, n)
    for flags in (0, AA, RAW, RAW | AA):
        got = k_fwd("ortho", flags, s, cull)
        if flags & RAW:
            p = s["raw"]
            # (torch's getters as the GPU evaluates them: those are the ones the kernel reproduces bit for bit)
            q, sc = torch.nn.functional.normalize(p["rotation"].cuda()).cpu().numpy(), torch.exp(p["scaling_log"].cuda()).cpu().numpy()
        else:
            q, sc = s["quats"], s["scales"]
        want = cm.ortho_kernel_order(s["means"], q, sc, s["viewmat"], s["K"], W, H, cull["eps2d"], cull["near_plane"],
                                     cull["far_plane"], cull["radius_clip"])
        for k in ("radii", "tiles", "means2d", "depths", "conics"):
            np.testing.assert_array_equal(got[k].cpu().numpy(), want[k], err_msg=f"{k} flags={flags}")
        if flags & AA:
            np.testing.assert_array_equal(got["comp"].cpu().numpy(), want["comp"])
        if flags & RAW:
            op = torch.sigmoid(s["raw"]["opacity_logit"].reshape(-1).cuda()).cpu().numpy()
            np.testing.assert_array_equal(got["opac"].cpu().numpy(), op * want["comp"] if flags & AA else op)
    if n >= 255:
        assert (want["radii"] > 0).sum() >= 50 and (want["radii"] == 0).sum() >= 50


@pytest.mark.parametrize("n", cm.KERNEL_SIZES)
@pytest.mark.parametrize("eps2d", [0.3, 0.0])
def test_fisheye_forward_against_float64(n, eps2d):
    """RAW x AA, Gaussians up to 88 degrees off axis: floats within min(F64_CAP, F64_MARGIN x e32) of float64, e32 the float32
    CPU restatement's own error on the case; integers exact outside the Gaussians within 1e-5 of a decision boundary.
    Measured on an MI355X: see docs/LAB_NOTES.md "Camera models (N20)"."""
    s0, cull = _kscene("fisheye", eps2d)
    s = _cut(s0, n)
    for flags in (0, AA, RAW, RAW | AA):
        got = k_fwd("fisheye", flags, s, cull)
        o64, dec, _ = _truth("fisheye", s, cull, flags, F64)
        o32, d32, _ = _truth("fisheye", s, cull, flags, torch.float32)
        keep = _check_ints(got, dec, f"n={n} flags={flags}")
        both = keep & (dec["radii"] > 0) & (d32["radii"] > 0)
        culled = got["radii"].cpu().numpy() == 0
        names = [k for k in FLOATS if k != "comp" or flags & AA] + (["opac"] if flags & RAW else [])
        for k in names:
            a = got[k].cpu().numpy()
            if k != "opac":
                assert np.all(a[culled] == 0), k
            if both.sum() == 0:
                continue
            rows = both if k != "opac" or flags & AA else np.ones(n, bool)
            e, e32 = rel_l2(a[rows], o64[k][rows]), rel_l2(o32[k][rows], o64[k][rows])
            print(f"fisheye fwd n={n} eps2d={eps2d} flags={flags} {k}: HIP {e:.2e} fp32 restatement {e32:.2e} ratio {e / max(e32, 1e-30):.2f}")
            assert e <= _bound(e32), (k, flags, e, e32)
    if n == 700:
        assert cm.off_axis_deg(s)[got["radii"].cpu().numpy() > 0].max() > 80.0


def test_all_culled():
    """Every Gaussian behind the camera, n past one workgroup: zeros everywhere, forward and backward, all three models."""
    n = 300
    s0, cull = _kscene("fisheye")
    s = _cut(s0, n)
    vm = s["viewmat"].copy()
    vm[2, :] = -vm[2, :]                    # z -> -z ... and every Gaussian further back than the scene is deep
    vm[2, 3] -= 40.0
    s["viewmat"] = vm
    cot = cm.cotangents(n, 1)
    for model in ("pinhole", "ortho", "fisheye"):
        for flags in (0, RAW | AA):
            got = k_fwd(model, flags, s, cull)
            for k in ("radii", "tiles", "means2d", "depths", "conics", "comp"):
                if got[k] is not None:
                    assert not bool(got[k].any()), (model, k)
            g = k_bwd(model, flags | POSE, s, cull, got["radii"], cot)
            for k in ("means", "quats", "scales", "viewmat"):
                assert not bool(g[k].any()), (model, k)
            if flags & RAW:     # antialiased: the logit's gradient carries the compensation, 0 for a culled Gaussian
                assert not bool(g["opacities"].any())


# -- kernel level: backward -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", cm.KERNEL_SIZES)
@pytest.mark.parametrize("model", ["ortho", "fisheye"])
def test_backward_against_float64_autograd(model, n):
    """RAW x AA x POSE: every gradient and v_viewmat within min(F64_CAP, F64_MARGIN x e32) of float64 autograd through the
    restatement (e32: the same autograd in float32 on the CPU); culled rows exactly zero, row 3 of v_viewmat zero, without POSE
    the same bits as with it, outputs passed as NULL skipped.  The radii are the kernel's own, accepted by the forward rule."""
    s0, cull = _kscene(model)
    s = _cut(s0, n)
    cot = cm.cotangents(700, 2)
    for flags in (0, AA, RAW, RAW | AA):
        fwd = k_fwd(model, flags, s, cull)
        _, dec, _ = _truth(model, s, cull, flags, F64)
        _check_ints(fwd, dec, f"{model} n={n}")
        radii = fwd["radii"]
        rn = radii.cpu().numpy()
        g = k_bwd(model, flags, s, cull, radii, cot)
        gp = k_bwd(model, flags | POSE, s, cull, radii, cot)
        for k in ("means", "quats", "scales") + (("opacities",) if flags & RAW else ()):
            assert torch.equal(g[k], gp[k]), (k, flags)
            if k != "opacities" or flags & AA:
                assert not bool(g[k][radii <= 0].any()), (k, flags)
        assert bool((gp["viewmat"][3] == 0).all())
        part = k_bwd(model, flags | POSE, s, cull, radii, cot, skip=("means", "scales"))
        assert torch.equal(part["quats"], gp["quats"]) and torch.equal(part["viewmat"], gp["viewmat"])
        if n == 0:
            assert not bool(gp["viewmat"].any())
            continue
        _, _, g64 = _truth(model, s, cull, flags, F64, cot, rn)
        _, _, g32 = _truth(model, s, cull, flags, torch.float32, cot, rn)
        if not (rn > 0).any():
            continue
        for k in ("means", "quats", "scales", "viewmat") + (("opacities",) if flags & RAW else ()):
            a = gp[k].cpu().numpy()
            e, e32 = rel_l2(a, g64[k]), rel_l2(g32[k], g64[k])
            print(f"{model} bwd n={n} flags={flags} {k}: HIP {e:.2e} fp32 autograd {e32:.2e} ratio {e / max(e32, 1e-30):.2f}")
            assert e <= _bound(e32), (k, flags, e, e32)


def test_pinhole_through_the_new_entries_is_the_existing_entries():
    """GAGS_CAM_PINHOLE: torch.equal to gags_project_fwd / _aa / _raw / _raw_aa, gags_project_bwd* and gags_project_bwd_pose,
    each called directly; _Project / _ProjectRaw (which go through the flagged pair) are the third party to the same equalities."""
    from gags_amd.raster_project import _Project, _ProjectRaw
    n = 700
    s = cm.model_scene("pinhole", n, 0, W, H, 13)
    cull = dict(eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0)
    cfg = (W, H, cull["eps2d"], cull["near_plane"], cull["far_plane"], cull["radius_clip"])
    cot = cm.cotangents(n, 4)
    vm, K = to_dev(s["viewmat"]), to_dev(s["K"])
    for flags in (0, AA, RAW, RAW | AA):
        aa = bool(flags & AA)
        got = k_fwd("pinhole", flags, s, cull)
        named = named_fwd(flags, s, cull)
        for k in got:
            if got[k] is not None:
                assert torch.equal(got[k], named[k]), (k, flags)
        means, quats, scales, logit = _inputs(s, flags)
        leaves = [t.clone().requires_grad_(True) for t in (means, quats, scales) + ((logit,) if flags & RAW else ())]
        if flags & RAW:
            old = _ProjectRaw.apply(*leaves, vm, K, *cfg, 1.0, False, aa)
            names = ("radii", "means2d", "depths", "conics", "tiles", "opac", None, "comp")
        else:
            old = _Project.apply(*leaves, vm, K, *cfg, aa)
            names = ("radii", "means2d", "depths", "conics", "tiles", "comp")
        assert int((got["radii"] > 0).sum()) >= 100
        for t, k in zip(old, names):
            if k is not None:
                assert torch.equal(t, got[k]) and torch.equal(t, named[k]), (k, flags)
        # the backward without the pose: the flagged entry, the named entry, and autograd through the python wrapper
        o = dict(zip(names, old))
        loss = (o["means2d"] * to_dev(cot["means2d"])).sum() + (o["depths"] * to_dev(cot["depths"])).sum() + \
            (o["conics"] * to_dev(cot["conics"])).sum()
        if flags & RAW:
            loss = loss + (o["opac"] * to_dev(cot["opacities"])).sum()
        elif aa:
            loss = loss + (o["comp"] * to_dev(cot["comp"])).sum()
        loss.backward()
        g = k_bwd("pinhole", flags, s, cull, got["radii"], cot)
        g_named = k_bwd("pinhole", flags, s, cull, got["radii"], cot, entry="old")
        for t, k in zip(leaves, ("means", "quats", "scales", "opacities")):
            assert torch.equal(g[k], g_named[k]), (k, flags)
            assert torch.equal(t.grad, g[k]) and torch.equal(t.grad, g_named[k]), (k, flags)
        gp_new = k_bwd("pinhole", flags | POSE, s, cull, got["radii"], cot)
        gp_old = k_bwd("pinhole", flags | POSE, s, cull, got["radii"], cot, entry="old")
        for k in gp_new:
            if gp_new[k] is not None:
                assert torch.equal(gp_new[k], gp_old[k]), (k, flags)
        assert bool(gp_new["viewmat"][:3].any())


@pytest.mark.parametrize("n", (1, 257))   # one lane of one wave; two workgroups with a one-lane tail
def test_named_entries_forward_to_the_flagged_pair(n):
    """Each named forward, each named backward and gags_project_bwd_pose against the flagged entry with GAGS_CAM_PINHOLE: the same
    inputs and cotangents, every output pre-filled on both sides (an output a forward fails to pass through keeps its fill on
    one side only), torch.equal on all of them -- RAW with quats_act, scales_act and the record table non-NULL."""
    full = cm.model_scene("pinhole", 700, 0, W, H, 13)
    cull = dict(eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0)
    # rows n0 .. n0 + n, n0 the first Gaussian the float32 restatement sees on screen and away from every decision boundary
    _, dec, _ = _truth("pinhole", full, cull, 0, torch.float32)
    n0 = int(np.flatnonzero((dec["radii"] > 0) & ~dec["close"])[0])
    assert n0 + n <= 700
    s = _cut(full, n, n0)
    cot = cm.cotangents(n, 5)
    for flags in (0, AA, RAW, RAW | AA):
        got, named = k_fwd("pinhole", flags, s, cull, modifier=1.25, extras=True), named_fwd(flags, s, cull, modifier=1.25, extras=True)
        assert bool((got["radii"] > 0).any()) and not bool((got["radii"] == -7).any())
        wrote = ("radii", "means2d", "depths", "conics", "tiles") + (("opac", "quats_act", "scales_act", "grec") if flags & RAW else ()) \
            + (("comp",) if flags & AA else ())
        assert sorted(wrote) == sorted(k for k in got if got[k] is not None)
        for k in wrote:
            assert torch.equal(got[k], named[k]), (k, flags)
            assert not bool((got[k][got["radii"] > 0] == 7).all()), (k, flags)   # (the flagged entry wrote it)
        for fl in (flags, flags | POSE):
            g = k_bwd("pinhole", fl, s, cull, got["radii"], cot, modifier=1.25)
            g_named = k_bwd("pinhole", fl, s, cull, got["radii"], cot, modifier=1.25, entry="old")
            wrote = ("means", "quats", "scales") + (("opacities",) if flags & RAW else ()) + (("viewmat",) if fl & POSE else ())
            assert sorted(wrote) == sorted(k for k in g if g[k] is not None)
            for k in wrote:
                assert torch.equal(g[k], g_named[k]), (k, fl)
                assert not bool((g[k] == 7).all()), (k, fl)


ON_AXIS_MEASURED = 1.84e-7   # worst relative difference below, as measured on an MI355X (v_quats; docs/LAB_NOTES.md)


def test_on_axis_fisheye_gaussian_has_the_pinhole_gradients():
    """x = y = 0 under an identity pose: every gradient finite, and equal to the pinhole entries' within 3 x the measured
    difference (at most 1e-3 relative): the two maps agree to second order on the axis."""
    n = 4
    s = dict(means=np.array([[0, 0, 3.0], [0, 0, 7.5], [0, 0, 2.0], [0, 0, 11.0]], np.float32),
             quats=np.array([[0.9, 0.1, -0.3, 0.2]] * n, np.float32), scales=np.array([[0.2, 0.1, 0.3]] * n, np.float32),
             viewmat=np.eye(4, dtype=np.float32), K=np.array([[40.0, 0, 48.0], [0, 35.0, 30.0], [0, 0, 1]], np.float32))
    cull = dict(eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0)
    cot = cm.cotangents(n, 6)
    res = {}
    for model in ("fisheye", "pinhole"):
        fwd = k_fwd(model, AA, s, cull)
        assert bool((fwd["radii"] > 0).all())
        res[model] = (fwd, k_bwd(model, AA | POSE, s, cull, fwd["radii"], cot))
    assert torch.equal(res["fisheye"][0]["radii"], res["pinhole"][0]["radii"])
    worst = 0.0
    for k in ("means2d", "depths", "conics", "comp"):
        worst = max(worst, rel_l2(res["fisheye"][0][k].cpu().numpy(), res["pinhole"][0][k].cpu().numpy()))
    for k in ("means", "quats", "scales", "viewmat"):
        a, b = res["fisheye"][1][k].cpu().numpy(), res["pinhole"][1][k].cpu().numpy()
        assert np.isfinite(a).all(), k
        d = rel_l2(a, b)
        print(f"on-axis fisheye vs pinhole, {k}: {d:.2e}")
        worst = max(worst, d)
    print(f"on-axis fisheye vs pinhole, worst: {worst:.2e}")
    assert worst <= min(1e-3, 3 * ON_AXIS_MEASURED)


# -- through rasterization() --------------------------------------------------------------------------------------------------

def _gpu_full(model, s, w, h, colors, bg, v_out, v_alpha, *, raw, aa, mode, sh, pose):
    from gags_amd.rasterization import rasterization
    if raw:
        p = s["raw"]
        L = dict(means=p["xyz"].cuda(), quats=p["rotation"].cuda(), scales=p["scaling_log"].cuda(), opacities=p["opacity_logit"].cuda())
    else:
        L = dict(means=to_dev(s["means"]), quats=to_dev(s["quats"]), scales=to_dev(s["scales"]), opacities=to_dev(s["opacities"]))
    L["colors"] = to_dev(colors)
    L["viewmat"] = to_dev(s["viewmat"])[None]
    for k, t in L.items():
        t.requires_grad_(k != "viewmat" or pose)
    out, alphas, info = rasterization(L["means"], L["quats"], L["scales"], L["opacities"], L["colors"], L["viewmat"],
                                      to_dev(s["K"])[None], w, h, backgrounds=to_dev(bg)[None], sh_degree=sh, render_mode=mode,
                                      raw_params=raw, rasterize_mode="antialiased" if aa else "classic", camera_model=model)
    info["means2d"].retain_grad()
    ((out[0] * to_dev(v_out)).sum() + (alphas[0, ..., 0] * to_dev(v_alpha)).sum()).backward()
    torch.cuda.synchronize()
    g = {k: t.grad for k, t in L.items() if t.grad is not None}
    g = {k: (t[0] if k == "viewmat" else t.reshape(-1) if k == "opacities" else t).cpu().numpy() for k, t in g.items()}
    g["means2d"] = info["means2d"].grad[0].cpu().numpy()
    return out[0].detach().cpu().numpy(), alphas[0, ..., 0].detach().cpu().numpy(), info, g


def _ref_full(model, s, w, h, colors, bg, v_out, v_alpha, radii, depths, *, raw, aa, mode, sh, dev="cuda"):
    """float64: the restatement -> oracle.dense_ref's composite (tests/aa_ref.py states it with the compensation) and sh_colors,
    integer decisions from the kernel's radii and a stable depth order."""
    from oracle import dense_ref

    def tm(a, rg=False):
        return torch.tensor(np.asarray(a), dtype=F64, device=dev, requires_grad=rg)
    n = s["means"].shape[0]
    pr, _, L = cm.run(model, s, w, h, F64, raw=raw, grad=True, dev=dev)
    m2 = pr["means2d"]
    m2.retain_grad()
    vis = torch.as_tensor(np.asarray(radii) > 0, device=dev)
    O = L["opac_act"] if raw else tm(s["opacities"], True)
    op = O * torch.where(vis, pr["comp"], torch.zeros_like(pr["comp"])) if aa else O
    C = tm(colors, True)
    cols = C if sh is None else dense_ref.sh_colors(sh, C, L["means"], torch.inverse(L["viewmat"])[:3, 3])
    bgt = tm(bg)
    if mode in ("RGB+D", "RGB+ED"):
        cols = torch.cat([cols, pr["depths"][:, None]], dim=1)
        bgt = torch.cat([bgt, torch.zeros(1, dtype=F64, device=dev)])
    order = np.lexsort((np.arange(n), np.asarray(depths)))
    out, alphas, _ = aa_ref.composite(m2, pr["conics"], op, cols, bgt, w, h, radii, order)
    if mode == "RGB+ED":
        out = torch.cat([out[..., :-1], out[..., -1:] / alphas[..., None].clamp(min=1e-10)], dim=-1)
    ((out * tm(v_out)).sum() + (alphas * tm(v_alpha)).sum()).backward()
    g = dict(means=L["means"].grad, quats=L["quats"].grad, scales=L["scales"].grad, colors=C.grad, means2d=m2.grad,
             opacities=L["opacities"].grad if raw else O.grad, viewmat=L["viewmat"].grad)
    return out.detach().cpu().numpy(), {k: v.cpu().numpy() for k, v in g.items()}


# (w, h, D, raw_params, antialiased, render_mode, sh_degree, seed)
RASTER_CASES = [(97, 61, 16, False, False, "RGB", None, 31), (104, 72, 128, True, True, "RGB+ED", None, 32),
                (104, 72, 16, True, False, "RGB+ED", None, 33), (97, 61, 128, False, True, "RGB", None, 34),
                (97, 61, 3, False, False, "RGB", 3, 35)]


@functools.lru_cache(maxsize=None)
def _raster_case(model, w, h, d, raw, aa, mode, sh, seed):
    """One scene under `model` and under the pinhole camera with the same K, each against its float64 truth."""
    s = cm.model_scene(model, 700, 3 if sh is not None else d, w, h, seed, max_deg=75.0)
    colors = s["sh"] if sh is not None else s["colors"]
    d0 = colors.shape[1] if sh is None else 3
    bg = np.full(d0, 0.25, np.float32)
    rng = np.random.default_rng(seed)
    v_out = rng.standard_normal((h, w, d0 + (mode != "RGB"))).astype(np.float32)
    v_alpha = rng.standard_normal((h, w)).astype(np.float32)
    kw = dict(raw=raw, aa=aa, mode=mode, sh=sh)
    res = {}
    for m in (model, "pinhole"):
        out, alpha, info, g = _gpu_full(m, s, w, h, colors, bg, v_out, v_alpha, pose=sh is not None, **kw)
        radii, depths = info["radii"][0].cpu().numpy(), info["depths"][0].detach().cpu().numpy()
        if m == model:      # the kernel-level rule accepts the radii of the model under test before they are used
            pr, dec, _ = cm.run(m, s, w, h, F64)
            keep = ~dec["close"]
            assert (~keep).sum() <= cm.MAX_EXCLUDED * keep.size
            np.testing.assert_array_equal(radii[keep], dec["radii"][keep])
        r_out, rg = _ref_full(m, s, w, h, colors, bg, v_out, v_alpha, radii, depths, **kw)
        res[m] = dict(out=out, g=g, r_out=r_out, rg=rg, radii=radii, info=info)
    return s, res


@pytest.mark.parametrize("case", RASTER_CASES, ids=lambda c: f"{c[0]}x{c[1]}-D{c[2]}-{'raw' if c[3] else 'plain'}-{'aa' if c[4] else 'classic'}-{c[5]}-sh{c[6]}")
@pytest.mark.parametrize("model", ["fisheye", "ortho"])
def test_rasterization_against_float64(model, case):
    """~700 Gaussians, visible ones <= 75 degrees off axis, both geometry routes (D = 16: VALU, D = 128: matrix cores), plain and
    raw_params, classic and antialiased, RGB and RGB+ED, sh_degree = 3 with means and viewmats requiring grad.  Bound per
    quantity: min(F64_CAP, F64_MARGIN x e_pin), e_pin the pinhole path's error against float64 on the same scene and K through
    this harness.  Measured on an MI355X: see docs/LAB_NOTES.md "Camera models (N20)"."""
    s, res = _raster_case(model, *case)
    a, p = res[model], res["pinhole"]
    assert a["info"]["camera_model"] == model and (a["radii"] > 0).sum() >= 100 and (p["radii"] > 0).sum() >= 20
    if model == "fisheye":
        ang = cm.off_axis_deg(s)[a["radii"] > 0]
        assert 60.0 < ang.max() <= 75.5
    keys = ["out"] + [k for k in ("colors", "opacities", "means2d", "means", "quats", "scales", "viewmat") if k in a["g"]]
    assert ("viewmat" in keys) == (case[6] is not None)
    for k in keys:
        e = rel_l2(a["out"], a["r_out"]) if k == "out" else rel_l2(a["g"][k], a["rg"][k])
        e_pin = rel_l2(p["out"], p["r_out"]) if k == "out" else rel_l2(p["g"][k], p["rg"][k])
        print(f"{model} {case} {k}: {e:.2e} pinhole {e_pin:.2e} ratio {e / max(e_pin, 1e-30):.2f}")
        assert e <= _bound(e_pin), (k, e, e_pin)
    culled = a["radii"] == 0
    for k in ("means", "quats", "scales", "means2d"):
        assert np.all(a["g"][k][culled] == 0), k


def test_known_answers_through_rasterization():
    """A fisheye Gaussian pi/4 off axis lands at cx + fx pi/4; an orthographic camera moved along its axis changes depths only;
    camera_model="pinhole" is the call without the argument, bit for bit, outputs and gradients."""
    from gags_amd.rasterization import rasterization
    K = to_dev(np.array([[100.0, 0, 150.0], [0, 80.0, 120.0], [0, 0, 1]], np.float32))[None]
    one = lambda a: to_dev(np.array(a, np.float32))  # noqa: E731
    args = (one([[1.0, 0, 1.0], [0, 2.0, 2.0]]), one([[1.0, 0, 0, 0]] * 2), one([[0.05] * 3] * 2), one([0.5, 0.5]), one([[1.0], [1.0]]))
    _, _, info = rasterization(*args, torch.eye(4, device="cuda")[None], K, 300, 240, camera_model="fisheye")
    np.testing.assert_allclose(info["means2d"][0].cpu().numpy(), [[150 + 100 * np.pi / 4, 120], [150, 120 + 80 * np.pi / 4]], rtol=1e-6)
    assert bool((info["radii"] > 0).all())
    w, h = 97, 61
    s = cm.model_scene("ortho", 700, 16, w, h, 41)
    res = []
    for shift in (0.0, 1.5):
        vm = s["viewmat"].copy()
        vm[2, 3] += shift
        out, _, info = rasterization(to_dev(s["means"]), to_dev(s["quats"]), to_dev(s["scales"]), to_dev(s["opacities"]),
                                     to_dev(s["colors"]), to_dev(vm)[None], to_dev(s["K"])[None], w, h, camera_model="ortho",
                                     near_plane=-1e10)
        res.append((out, info))
    for k in ("radii", "means2d", "conics", "tiles_per_gauss"):
        assert torch.equal(res[0][1][k], res[1][1][k]), k
    assert int((res[0][1]["radii"] > 0).sum()) >= 100
    dz = (res[1][1]["depths"] - res[0][1]["depths"])[res[0][1]["radii"] > 0]
    assert float((dz - 1.5).abs().max()) < 1e-5
    # pinhole: the argument changes nothing
    s = cm.model_scene("pinhole", 700, 16, w, h, 42)
    v = to_dev(np.random.default_rng(0).standard_normal((h, w, 16)).astype(np.float32))
    got = []
    for kw in ({}, dict(camera_model="pinhole")):
        L = [to_dev(s[k]).requires_grad_(True) for k in ("means", "quats", "scales", "opacities", "colors")]
        vm = to_dev(s["viewmat"])[None].requires_grad_(True)
        out, alphas, info = rasterization(*L, vm, to_dev(s["K"])[None], w, h, **kw)
        (out[0] * v).sum().backward()
        got.append([out, alphas, info["radii"], info["means2d"], info["conics"], info["depths"], vm.grad] + [t.grad for t in L])
    assert got[1][2].gt(0).sum() >= 50
    for a, b in zip(*got):
        assert torch.equal(a, b)


# -- through render() -----------------------------------------------------------------------------------------------------------

def test_render_with_a_fisheye_camera():
    """scene.Camera(camera_model="fisheye", K=...) through render(): the render, the feature gradient and
    viewspace_points.grad are the rasterization() call's on the same inputs, a trainable world_view_transform receives its
    gradient, and densify.accumulate runs on the result."""
    from gags_amd import densify
    from gags_amd.gaussian_renderer import render
    from gags_amd.rasterization import rasterization
    from gags_amd.scene import Camera, GaussianModel
    w, h, n, d = 97, 61, 700, 16
    s = cm.model_scene("fisheye", n, d, w, h, 51, max_deg=75.0)
    R, C = s["R"], s["C"]
    cam = Camera(R, -R.T @ C, 1.0, 0.8, w, h, device="cuda", camera_model="fisheye", K=s["K"])
    assert np.abs(cam.world_view_transform.T.cpu().numpy() - s["viewmat"]).max() < 1e-5
    cam.world_view_transform = cam.world_view_transform.clone().requires_grad_(True)
    p = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in s["raw"].items()}
    pc = GaussianModel.from_tensors(p["xyz"], p["scaling_log"], p["rotation"], p["opacity_logit"], p["features_dc"],
                                    p["features_rest"], p["semantic_feature"])
    pc.training_setup()
    v = to_dev(np.random.default_rng(1).standard_normal((d, h, w)).astype(np.float32))
    pkg = render(cam, pc, None, torch.ones(3, device="cuda"), feature_mode=True)
    (pkg["render"] * v).sum().backward()
    assert pkg["info"]["camera_model"] == "fisheye" and int(pkg["visibility_filter"].sum()) >= 100
    # (the same leaves require grad as in the model: the feature stage trains the features alone, so the route is the same)
    L = [t.detach().clone().requires_grad_(t.requires_grad)
         for t in (pc._xyz, pc._rotation, pc._scaling, pc._opacity, pc._semantic_feature)]
    vm = cam.world_view_transform.detach().T[None].contiguous().requires_grad_(True)
    out, _, info = rasterization(L[0], L[1], L[2], L[3].squeeze(-1), L[4], vm, to_dev(s["K"])[None], w, h,
                                 backgrounds=torch.ones(1, d, device="cuda"), raw_params=True, camera_model="fisheye")
    info["means2d"].retain_grad()
    (out[0].permute(2, 0, 1) * v).sum().backward()
    assert torch.equal(pkg["render"], out[0].permute(2, 0, 1)) and torch.equal(pkg["radii"], info["radii"][0])
    assert torch.equal(pc._semantic_feature.grad, L[4].grad) and bool(L[4].grad.any())
    assert torch.equal(pkg["viewspace_points"].grad, info["means2d"].grad)
    g = cam.world_view_transform.grad
    assert g is not None and bool(g.any()) and torch.equal(g, vm.grad[0].T) and bool((g[:, 3] == 0).all())
    # ... and differs from the pinhole render of the same camera
    pin = Camera(R, -R.T @ C, 1.0, 0.8, w, h, device="cuda", K=s["K"])
    with torch.no_grad():
        assert not torch.equal(render(pin, pc, None, torch.ones(3, device="cuda"), feature_mode=True)["radii"], pkg["radii"])
    densify.accumulate(pc, pkg)
    vis = pkg["visibility_filter"]
    assert torch.equal(pc.denom.reshape(-1) > 0, vis) and bool((pc.max_radii2D[vis] > 0).all())
