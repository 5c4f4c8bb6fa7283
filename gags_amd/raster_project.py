"""The autograd functions in front of the rasterizer: projection of the activated (_Project) or the stored (_ProjectRaw)
parameters, and SH colour (_SH)."""
import torch

from . import _lib, profiler
from ._lib import check, ptr


def _c(t):
    return t if (t.is_contiguous() and t.dtype == torch.float32) else t.contiguous().float()


def _proj_flags(raw, aa, kb=False):
    return (_lib.GAGS_PROJ_RAW if raw else 0) | (_lib.GAGS_PROJ_AA if aa else 0) | (_lib.GAGS_PROJ_KB if kb else 0)


def _project_fwd(lib, cam, flags, means, quats, scales, logit, modifier, viewmat, K, width, height, eps2d, near, far, radius_clip,
                 opac, grec, comp):
    """gags_project_fwd_cam: the projection forward of every camera model (cam = _lib.GAGS_CAM_*) and variant (flags =
    _lib.GAGS_PROJ_RAW | _AA | _KB; with _KB, N21, K is the 13-float block [K, k1 .. k4]) -- the only call of that entry in the
    package.  opac / grec / comp: the outputs of RAW / RAW / AA,
    None where the variant has none.  Returns the five outputs every variant has: (radii, means2d, depths, conics, tiles)."""
    n = means.shape[0]
    dev = means.device
    radii = torch.empty(n, dtype=torch.int32, device=dev)
    means2d = torch.empty(n, 2, dtype=torch.float32, device=dev)
    depths = torch.empty(n, dtype=torch.float32, device=dev)
    conics = torch.empty(n, 3, dtype=torch.float32, device=dev)
    tiles = torch.empty(n, dtype=torch.int32, device=dev)
    with profiler.stage("project_fwd"):
        check(lib.gags_project_fwd_cam(cam, flags, n, ptr(means), ptr(quats), ptr(scales), ptr(logit), modifier, ptr(viewmat),
                                       ptr(K), width, height, eps2d, near, far, radius_clip, ptr(radii), ptr(means2d), ptr(depths),
                                       ptr(conics), ptr(tiles), ptr(opac), None, None, ptr(grec), ptr(comp), _lib.stream()),
              "gags_project_fwd_cam")
    return radii, means2d, depths, conics, tiles


def _project_bwd(lib, cam, flags, means, quats, scales, logit, modifier, viewmat, K, width, height, eps2d, radii, v_means2d,
                 v_depths, v_conics, v_opac, v_comp, want, pose):
    """gags_project_bwd_cam: the projection backward of every camera model and variant, with (pose, N17) or without the
    cotangent of viewmat -- the only call of that entry in the package.  want = which of (means, quats, scales, opacity logit)
    get a gradient: the others are neither allocated nor stored (without the pose the entry requires the first three).
    Returns (v_means, v_quats, v_scales, v_logit, v_viewmat [4,4]), None where not wanted."""
    n = means.shape[0]
    dev = means.device
    v_means, v_quats, v_scales, v_logit = (torch.empty(n, *shape, device=dev) if w else None
                                           for w, shape in zip(want, ((3,), (4,), (3,), ())))
    v_viewmat = partials = None
    if pose:
        flags |= _lib.GAGS_PROJ_POSE
        v_viewmat = torch.empty(4, 4, device=dev)
        partials = torch.empty(lib.gags_project_pose_partials(n), 12, device=dev)
    check(lib.gags_project_bwd_cam(cam, flags, n, ptr(means), ptr(quats), ptr(scales), ptr(logit), modifier, ptr(viewmat), ptr(K),
                                   width, height, eps2d, ptr(radii), ptr(v_means2d), ptr(v_depths), ptr(v_conics), ptr(v_opac),
                                   ptr(v_comp), ptr(v_means), ptr(v_quats), ptr(v_scales), ptr(v_logit), ptr(v_viewmat),
                                   ptr(partials), partials.numel() * 4 if pose else 0, _lib.stream()), "gags_project_bwd_cam")
    return v_means, v_quats, v_scales, v_logit, v_viewmat


def _project_bwd_calib(lib, cam, flags, means, quats, scales, logit, modifier, viewmat, K, width, height, eps2d, radii, v_means2d,
                       v_depths, v_conics, v_opac, v_comp, want, pose):
    """gags_project_bwd_calib (N23): _project_bwd with the cotangent of K on the way -- the only call of that entry in the
    package.  Returns _project_bwd's five and v_K, shaped like the K the projection was given: [3,3], or with GAGS_PROJ_KB the
    13-float block [v_K row-major, v_k1 .. v_k4].  Every scene gradient may be unwanted, with or without the pose."""
    n = means.shape[0]
    dev = means.device
    v_means, v_quats, v_scales, v_logit = (torch.empty(n, *shape, device=dev) if w else None
                                           for w, shape in zip(want, ((3,), (4,), (3,), ())))
    kb = bool(flags & _lib.GAGS_PROJ_KB)
    v_block = torch.empty(13 if kb else 9, device=dev)
    v_viewmat = None
    if pose:
        flags |= _lib.GAGS_PROJ_POSE
        v_viewmat = torch.empty(4, 4, device=dev)
    partials = torch.empty(lib.gags_project_calib_partials(n), _lib.GAGS_CALIB_PARTIAL_FLOATS, device=dev)
    check(lib.gags_project_bwd_calib(cam, flags, n, ptr(means), ptr(quats), ptr(scales), ptr(logit), modifier, ptr(viewmat), ptr(K),
                                     width, height, eps2d, ptr(radii), ptr(v_means2d), ptr(v_depths), ptr(v_conics), ptr(v_opac),
                                     ptr(v_comp), ptr(v_means), ptr(v_quats), ptr(v_scales), ptr(v_logit), ptr(v_viewmat),
                                     ptr(v_block), ptr(v_block[9:]) if kb else None, ptr(partials), partials.numel() * 4,
                                     _lib.stream()), "gags_project_bwd_calib")
    return v_means, v_quats, v_scales, v_logit, v_viewmat, (v_block if kb else v_block.view(3, 3))


class _Project(torch.autograd.Function):
    """K1 + K4 forward, K2 backward.  aa (rasterize_mode "antialiased"): one more output, the compensations [N], and its
    cotangent in the backward; the caller multiplies them into the opacities.  cam (N20): _lib.GAGS_CAM_*; every model, the
    pinhole (0) included, goes through _project_fwd / _project_bwd.  kb (N21, fisheye only): K is the 13-float block, the
    matrix then the distortion coefficients (GAGS_PROJ_KB).  A K that requires grad (N23) gets its gradient, shaped like it,
    from _project_bwd_calib; otherwise the backward is _project_bwd's, as before."""

    @staticmethod
    def forward(ctx, means, quats, scales, viewmat, K, width, height, eps2d, near, far, radius_clip, aa=False, cam=0, kb=False):
        lib = _lib.load()
        means, quats, scales, viewmat, K = _c(means), _c(quats), _c(scales), _c(viewmat), _c(K)
        comp = torch.empty(means.shape[0], dtype=torch.float32, device=means.device) if aa else None
        radii, means2d, depths, conics, tiles = _project_fwd(lib, cam, _proj_flags(False, aa, kb), means, quats, scales, None, 1.0,
                                                             viewmat, K, width, height, eps2d, near, far, radius_clip, None, None,
                                                             comp)
        ctx.save_for_backward(means, quats, scales, viewmat, K, radii)
        ctx.cfg = (width, height, eps2d, aa, cam, kb)
        ctx.mark_non_differentiable(radii, tiles)
        if aa:
            return radii, means2d, depths, conics, tiles, comp
        return radii, means2d, depths, conics, tiles

    @staticmethod
    def backward(ctx, _v_radii, v_means2d, v_depths, v_conics, _v_tiles, v_comp=None):
        lib = _lib.load()
        means, quats, scales, viewmat, K, radii = ctx.saved_tensors
        width, height, eps2d, aa, cam, kb = ctx.cfg
        n = means.shape[0]
        dev = means.device
        v_means2d = torch.zeros(n, 2, device=dev) if v_means2d is None else _c(v_means2d)
        v_conics = torch.zeros(n, 3, device=dev) if v_conics is None else _c(v_conics)
        v_depths = None if v_depths is None else _c(v_depths)
        v_comp = None if (not aa or v_comp is None) else _c(v_comp)
        # the pose: one more output of the same kernel, and only the scene gradients that are wanted
        pose = ctx.needs_input_grad[3]
        args = (lib, cam, _proj_flags(False, aa, kb), means, quats, scales, None, 1.0, viewmat, K, width, height, eps2d, radii,
                v_means2d, v_depths, v_conics, None, v_comp)
        v_K = None
        if ctx.needs_input_grad[4]:  # (N23: the intrinsics too; the calib entry, like the pose's, stores only what is wanted)
            v_means, v_quats, v_scales, _, v_viewmat, v_K = _project_bwd_calib(*args, tuple(ctx.needs_input_grad[:3]) + (False,), pose)
        else:
            want = tuple(ctx.needs_input_grad[:3]) if pose else (True, True, True)
            v_means, v_quats, v_scales, _, v_viewmat = _project_bwd(*args, want + (False,), pose)
        return v_means, v_quats, v_scales, v_viewmat, v_K, None, None, None, None, None, None, None, None, None


class _ProjectRaw(torch.autograd.Function):
    """K1 + K4 on the STORED parameters (GAGS_PROJ_RAW): the getters of scene/gaussian_model.py:116-139 -- exp, F.normalize,
    sigmoid -- and render()'s `* scaling_modifier` run inside the projection kernel, bit for bit as torch evaluates them; the
    backward returns gradients of the stored parameters.  aa (rasterize_mode "antialiased"): the kernel folds the compensation
    into the activated opacity and the record, the compensations [N] are one more -- non-differentiable -- output, and the
    backward takes the compensation's cotangent from the opacity's.  cam (N20), kb (N21): as in _Project."""

    @staticmethod
    def forward(ctx, means, rotation, scaling_log, opacity_logit, viewmat, K, width, height, eps2d, near, far, radius_clip,
                scaling_modifier, want_records, aa=False, cam=0, kb=False):
        lib = _lib.load()
        means, rotation, scaling_log, viewmat, K = _c(means), _c(rotation), _c(scaling_log), _c(viewmat), _c(K)
        logit = _c(opacity_logit.reshape(-1))
        n = means.shape[0]
        dev = means.device
        opac = torch.empty(n, dtype=torch.float32, device=dev)
        # the per-Gaussian records of the matrix-core raster kernels (K8b), written on the way: no record kernel in the binning
        grec = torch.empty(max(n, 1), 8, dtype=torch.float32, device=dev) if want_records else torch.empty(0, device=dev)
        comp = torch.empty(n, dtype=torch.float32, device=dev) if aa else None
        radii, means2d, depths, conics, tiles = _project_fwd(lib, cam, _proj_flags(True, aa, kb), means, rotation, scaling_log, logit,
                                                             scaling_modifier, viewmat, K, width, height, eps2d, near, far,
                                                             radius_clip, opac, grec if want_records else None, comp)
        ctx.save_for_backward(means, rotation, scaling_log, logit, viewmat, K, radii)
        ctx.cfg = (width, height, eps2d, scaling_modifier, tuple(opacity_logit.shape), aa, cam, kb)
        if aa:
            ctx.mark_non_differentiable(radii, tiles, grec, comp)
            return radii, means2d, depths, conics, tiles, opac, grec, comp
        ctx.mark_non_differentiable(radii, tiles, grec)
        return radii, means2d, depths, conics, tiles, opac, grec

    @staticmethod
    def backward(ctx, _v_radii, v_means2d, v_depths, v_conics, _v_tiles, v_opac, _v_grec, _v_comp=None):
        lib = _lib.load()
        means, rotation, scaling_log, logit, viewmat, K, radii = ctx.saved_tensors
        width, height, eps2d, modifier, oshape, aa, cam, kb = ctx.cfg
        n = means.shape[0]
        dev = means.device
        v_means2d = torch.zeros(n, 2, device=dev) if v_means2d is None else _c(v_means2d)
        v_conics = torch.zeros(n, 3, device=dev) if v_conics is None else _c(v_conics)
        v_depths = None if v_depths is None else _c(v_depths)
        v_opac = None if v_opac is None else _c(v_opac)
        pose = ctx.needs_input_grad[4]  # (see _Project.backward)
        args = (lib, cam, _proj_flags(True, aa, kb), means, rotation, scaling_log, logit, modifier, viewmat, K, width, height, eps2d,
                radii, v_means2d, v_depths, v_conics, v_opac, None)
        v_K = None
        if ctx.needs_input_grad[5]:
            v_means, v_rot, v_scal, v_logit, v_viewmat, v_K = _project_bwd_calib(*args, tuple(ctx.needs_input_grad[:4]), pose)
        else:
            want = tuple(ctx.needs_input_grad[:4]) if pose else (True, True, True, ctx.needs_input_grad[3])
            v_means, v_rot, v_scal, v_logit, v_viewmat = _project_bwd(*args, want, pose)
        return (v_means, v_rot, v_scal, None if v_logit is None else v_logit.reshape(oshape), v_viewmat, v_K, None, None, None,
                None, None, None, None, None, None, None, None)


class _SH(torch.autograd.Function):
    """K3: SH colour and its backward: coefficients, and -- when positions are trainable -- the view direction
    (d colour / d means through normalize(mean - campos), as gsplat propagates it); when the camera position needs a gradient
    (a trainable pose, N17), v_campos = - the column sums of that table (gags_colsum_f32)."""

    @staticmethod
    def forward(ctx, coeffs, means, campos, radii, degree):
        lib = _lib.load()
        coeffs, means, campos = _c(coeffs), _c(means), _c(campos)
        n, kc = coeffs.shape[0], coeffs.shape[1]
        out = torch.empty(n, 3, device=coeffs.device)
        check(lib.gags_sh_fwd(n, kc, degree, ptr(means), ptr(campos), ptr(coeffs), ptr(radii), ptr(out), _lib.stream()),
              "gags_sh_fwd")
        ctx.save_for_backward(means, campos, radii, out, coeffs if (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]) else None)
        ctx.cfg = (kc, degree)
        return out

    @staticmethod
    def backward(ctx, v_out):
        lib = _lib.load()
        means, campos, radii, out, coeffs = ctx.saved_tensors
        kc, degree = ctx.cfg
        n = means.shape[0]
        v_out = _c(v_out)
        v_coeffs = v_means = None
        if ctx.needs_input_grad[0]:
            v_coeffs = torch.empty(n, kc, 3, device=means.device)
            check(lib.gags_sh_bwd(n, kc, degree, ptr(means), ptr(campos), ptr(radii), ptr(out), ptr(v_out),
                                  ptr(v_coeffs), _lib.stream()), "gags_sh_bwd")
        v_campos = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            # (the pose alone: the same table into a temporary, for its column sums)
            v_dirs = torch.empty(n, 3, device=means.device)
            check(lib.gags_sh_bwd_dirs(n, kc, degree, ptr(means), ptr(campos), ptr(coeffs), ptr(radii), ptr(out),
                                       ptr(v_out), ptr(v_dirs), _lib.stream()), "gags_sh_bwd_dirs")
            if ctx.needs_input_grad[1]:
                v_means = v_dirs
            if ctx.needs_input_grad[2]:
                # dir = normalize(mean - campos): v_campos = - sum_i v_means_i, summed in double in a fixed order (N17)
                v_campos = torch.empty(3, device=means.device)
                check(lib.gags_colsum_f32(n, 3, ptr(v_dirs), -1.0, ptr(v_campos), 3, _lib.stream()), "gags_colsum_f32")
        return v_coeffs, v_means, v_campos, None, None
