"""Host-side mirrors of the reference types that cross the render boundary.

Only what `render(...)` reads is mirrored:

* `GaussianModel` -- tensor layout and activation getters of
  /root/reference/scene/gaussian_model.py:48-61,116-139 (`_xyz [N,3]`, `_features_dc [N,1,3]`,
  `_features_rest [N,15,3]`, `_scaling [N,3]` log-space, `_rotation [N,4]` wxyz un-normalised,
  `_opacity [N,1]` logit, `_semantic_feature [N,D]` raw), and `training_setup` of :183-208
  (only `_semantic_feature` is optimised, Adam eps=1e-15, every geometry tensor frozen).
* `Camera` -- the five attributes render() touches (scene/cameras.py:17-61):
  `FoVx, FoVy, image_width, image_height` (mutable: render.py:115-116) and
  `world_view_transform` = W2C^T, built as utils/graphics_utils.py:38-49 does.

PLY / checkpoint I/O (`save_ply`, `load_ply`, `capture`, `restore`: SURVEY.md 8f N3) go through
gags_amd/io_formats.py; adaptive density control (`densify_and_prune`, `add_densification_stats`, `reset_opacity`, ...:
SURVEY.md 8f N8) through gags_amd/densify.py; a model is started from a point cloud by `create_from_pcd` (SURVEY.md 8f N9:
gags_amd/knn.py for the initial scales, io_formats.read_point_cloud for points3D.ply, `nerfpp_norm` for the cameras' extent);
the COLMAP binary and text loaders are out of scope.
"""
import math
from typing import NamedTuple

import numpy as np
import torch
from torch import nn


def getWorld2View2(R, t, translate=np.array([0.0, 0.0, 0.0]), scale=1.0):
    """World-to-view 4x4 (float32) from camera rotation R (stored transposed, as COLMAP
    readers do) and translation t; same contract as utils/graphics_utils.py:38-49."""
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = np.asarray(R).transpose()
    Rt[:3, 3] = np.asarray(t)
    Rt[3, 3] = 1.0
    C2W = np.linalg.inv(Rt)
    C2W[:3, 3] = (C2W[:3, 3] + translate) * scale
    return np.float32(np.linalg.inv(C2W))


def focal2fov(focal, pixels):
    return 2 * math.atan(pixels / (2 * focal))


def fov2focal(fov, pixels):
    return pixels / (2 * math.tan(fov / 2))


class Camera:
    """Minimal stand-in for scene.cameras.Camera / MiniCam.  camera_model / K (N20): "pinhole", "ortho" or "fisheye", and
    explicit intrinsics [3,3] that render() then uses instead of the FoV-derived ones (required for a non-pinhole camera).
    radial_coeffs (N21; fisheye only): the distortion coefficients (k1, k2, k3, k4) of OpenCV's fisheye model, kept as float32 [4]."""

    def __init__(self, R, T, FoVx, FoVy, image_width, image_height, device="cuda", uid=0, camera_model="pinhole", K=None,
                 radial_coeffs=None):
        self.uid = uid
        if camera_model not in ("pinhole", "ortho", "fisheye"):
            raise ValueError(f"unknown camera_model {camera_model!r} (\"pinhole\", \"ortho\" or \"fisheye\")")
        self.camera_model = camera_model
        self.radial_coeffs = None
        if radial_coeffs is not None:
            if camera_model != "fisheye":
                raise ValueError(f"radial_coeffs are the distortion coefficients of a \"fisheye\" camera, not of a {camera_model!r} one")
            self.radial_coeffs = np.asarray(radial_coeffs.detach().cpu() if torch.is_tensor(radial_coeffs) else radial_coeffs,
                                            dtype=np.float32).reshape(-1)
            if self.radial_coeffs.shape != (4,):
                raise ValueError("radial_coeffs must be (k1, k2, k3, k4)")
        self.K = None
        if K is not None:
            self.K = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, dtype=np.float32)
            if self.K.shape != (3, 3):
                raise ValueError("K must be [3,3]")
        self.R = np.asarray(R, dtype=np.float64)
        self.T = np.asarray(T, dtype=np.float64)
        self.FoVx = float(FoVx)
        self.FoVy = float(FoVy)
        self.image_width = int(image_width)
        self.image_height = int(image_height)
        self.zfar = 100.0
        self.znear = 0.01
        w2c = getWorld2View2(self.R, self.T)
        self.world_view_transform = torch.tensor(w2c).transpose(0, 1).contiguous().to(device)
        self.camera_center = torch.tensor(np.linalg.inv(w2c.astype(np.float64))[:3, 3], dtype=torch.float32).to(device)

    @classmethod
    def from_opencv_fisheye(cls, params, R, T, width, height, device="cuda", uid=0):
        """A fisheye camera from a calibration in COLMAP's OPENCV_FISHEYE order: params = (fx, fy, cx, cy, k1, k2, k3, k4).
        FoVx / FoVy (which render() does not read for this model) are the angles the equidistant map puts at the image's edges."""
        params = [float(v) for v in np.asarray(params, dtype=np.float64).reshape(-1)]
        if len(params) != 8:
            raise ValueError("params must be (fx, fy, cx, cy, k1, k2, k3, k4)")
        fx, fy, cx, cy = params[:4]
        if not (fx > 0 and fy > 0):
            raise ValueError("fx and fy must be positive")
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)
        return cls(R, T, width / fx, height / fy, width, height, device=device, uid=uid, camera_model="fisheye", K=K,
                   radial_coeffs=params[4:])


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


class BasicPointCloud(NamedTuple):
    """utils/graphics_utils.py:17-20: what fetchPly returns and create_from_pcd takes."""
    points: np.ndarray
    colors: np.ndarray
    normals: np.ndarray


SH_C0 = 0.28209479177387814  # utils/sh_utils.py:24


def RGB2SH(rgb):
    """utils/sh_utils.py:114-115."""
    return (rgb - 0.5) / SH_C0


def SH2RGB(sh):
    """utils/sh_utils.py:117-118."""
    return sh * SH_C0 + 0.5


def nerfpp_norm(cameras):
    """getNerfppNorm (scene/dataset_readers.py:123-147) over objects with `.R` and `.T` (this module's Camera, or the reference's
    CameraInfo): {"translate": minus the mean camera centre [3], "radius": 1.1 x the largest distance of a centre from it}.
    The radius is the `cameras_extent` that create_from_pcd takes as spatial_lr_scale and densify_and_prune as extent.
    Host numpy, in the reference's order of operations."""
    centers = []
    for cam in cameras:
        c2w = np.linalg.inv(getWorld2View2(cam.R, cam.T))
        centers.append(c2w[:3, 3:4])
    centers = np.hstack(centers)
    center = np.mean(centers, axis=1, keepdims=True)
    diagonal = np.max(np.linalg.norm(centers - center, axis=0, keepdims=True))
    return {"translate": -center.flatten(), "radius": diagonal * 1.1}


def _init_tensors(points, colors, dist2, max_sh_degree, semantic_feature_size=0, speedup=False):
    """The element-wise part of create_from_pcd (scene/gaussian_model.py:153-180) on whatever device its inputs live on:
    points [N,3] and colors [N,3] float32 tensors, dist2 [N] the 3-nearest-neighbour mean squared distances.  Returns the
    raw tensors by attribute name (semantic feature: None when semantic_feature_size == 0)."""
    n, dev = points.shape[0], points.device
    # RGB2SH with a tensor divisor: torch divides by a Python scalar on the GPU as a product with its reciprocal (2 ulp from
    # the reference's CPU result); tensor / tensor is the IEEE division on both devices
    fused_color = (colors - 0.5) / torch.tensor(SH_C0, dtype=colors.dtype, device=dev)
    features = torch.zeros((n, 3, (max_sh_degree + 1) ** 2), dtype=torch.float32, device=dev)
    features[:, :3, 0] = fused_color
    semantic = None
    if semantic_feature_size != 0:
        if speedup:
            semantic_feature_size = int(semantic_feature_size / 32)
        semantic = torch.zeros((n, semantic_feature_size), dtype=torch.float32, device=dev)
    scales = torch.log(torch.sqrt(torch.clamp_min(dist2, 0.0000001)))[..., None].repeat(1, 3)
    rots = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    rots[:, 0] = 1
    opacities = inverse_sigmoid(0.1 * torch.ones((n, 1), dtype=torch.float32, device=dev))
    return {"_xyz": points, "_features_dc": features[:, :, 0:1].transpose(1, 2).contiguous(),
            "_features_rest": features[:, :, 1:].transpose(1, 2).contiguous(), "_scaling": scales, "_rotation": rots,
            "_opacity": opacities, "_semantic_feature": semantic, "max_radii2D": torch.zeros((n,), device=dev)}


class GaussianModel:
    """Parameter container with the reference's tensor names, shapes and getters."""

    def __init__(self, sh_degree=3):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        self._xyz = torch.empty(0)
        self._features_dc = torch.empty(0)
        self._features_rest = torch.empty(0)
        self._scaling = torch.empty(0)
        self._rotation = torch.empty(0)
        self._opacity = torch.empty(0)
        self._semantic_feature = None
        self.optimizer = None

    # -- activations: scene/gaussian_model.py:36-42,116-139 -------------------------------
    def cache_activations(self, on=True):
        """Opt-in: keep the activations of FROZEN parameters (requires_grad False: the geometry during the reference's
        feature training, train.py:62-75) between renders instead of re-evaluating exp / normalize / sigmoid on every
        getter call as scene/gaussian_model.py:116-139 does (six small kernels per view).  OFF by default: a cached value
        cannot see writes that bypass autograd's version counter (`p.data.add_(...)`, `p.data.copy_(...)` -- idiomatic
        in 3DGS code for opacity resets, clamping and weight loading), so whoever turns this on promises to call
        `invalidate_activations()` after such a write.  In-place ops on the parameter itself, replacing the parameter,
        load_ply / restore, and requires_grad are noticed without help."""
        self._cache_on = bool(on)
        self.invalidate_activations()
        return self

    def invalidate_activations(self):
        self.__dict__["_act_cache"] = {}

    def _frozen(self, name, param, fn):
        """Activation of a parameter: evaluated afresh on every call (the reference's behaviour) unless
        cache_activations() was turned on and the parameter is frozen."""
        if (not getattr(self, "_cache_on", False) or param.requires_grad
                or torch.is_grad_enabled() and param.grad_fn is not None):
            return fn(param)
        cache = self.__dict__.setdefault("_act_cache", {})
        key = (id(param), param.data_ptr(), param._version, tuple(param.shape))
        hit = cache.get(name)
        if hit is None or hit[0] != key:
            with torch.no_grad():
                hit = (key, fn(param))
            cache[name] = hit
        return hit[1]

    @property
    def get_scaling(self):
        return self._frozen("scaling", self._scaling, torch.exp)

    @property
    def get_rotation(self):
        return self._frozen("rotation", self._rotation, torch.nn.functional.normalize)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_opacity(self):
        return self._frozen("opacity", self._opacity, torch.sigmoid)

    @property
    def get_semantic_feature(self):
        return self._semantic_feature

    def rewrite_semantic_feature(self, x):
        self._semantic_feature = x

    @classmethod
    def from_tensors(cls, xyz, scaling_log, rotation, opacity_logit, features_dc=None, features_rest=None,
                     semantic_feature=None, sh_degree=3, active_sh_degree=None):
        m = cls(sh_degree)
        n = xyz.shape[0]
        dev = xyz.device
        m._xyz = nn.Parameter(xyz.contiguous().float(), requires_grad=False)
        m._scaling = nn.Parameter(scaling_log.contiguous().float(), requires_grad=False)
        m._rotation = nn.Parameter(rotation.contiguous().float(), requires_grad=False)
        m._opacity = nn.Parameter(opacity_logit.reshape(n, 1).contiguous().float(), requires_grad=False)
        if features_dc is None:
            features_dc = torch.zeros(n, 1, 3, device=dev)
        if features_rest is None:
            features_rest = torch.zeros(n, (sh_degree + 1) ** 2 - 1, 3, device=dev)
        m._features_dc = nn.Parameter(features_dc.contiguous().float(), requires_grad=False)
        m._features_rest = nn.Parameter(features_rest.contiguous().float(), requires_grad=False)
        if semantic_feature is not None:
            m._semantic_feature = nn.Parameter(semantic_feature.contiguous().float(), requires_grad=True)
        m.active_sh_degree = sh_degree if active_sh_degree is None else active_sh_degree
        return m

    def create_from_pcd(self, pcd, spatial_lr_scale, semantic_feature_size=0, speedup=False, device="cuda"):
        """scene/gaussian_model.py:151-180, field by field: positions from pcd.points, SH band 0 from pcd.colors (in [0, 1]),
        the higher bands zero, isotropic log-scales from the distance to the three nearest neighbours (gags_amd/knn.py: the
        HIP kernel, no CPU path), identity rotations, opacity 0.1, a zero semantic feature of semantic_feature_size (/ 32
        with speedup) columns unless the size is 0.  Every tensor is an nn.Parameter with requires_grad=True;
        active_sh_degree is 0 and spatial_lr_scale is kept for training_setup_rgb."""
        from . import knn
        self.spatial_lr_scale = spatial_lr_scale
        points = torch.tensor(np.asarray(pcd.points)).float().to(device)
        colors = torch.tensor(np.asarray(pcd.colors)).float().to(device)
        t = _init_tensors(points, colors, knn.dist2(points), self.max_sh_degree, semantic_feature_size, speedup)
        self.max_radii2D = t.pop("max_radii2D")
        for attr, v in t.items():
            setattr(self, attr, None if v is None else nn.Parameter(v.contiguous().requires_grad_(True)))
        self.active_sh_degree = 0
        self.invalidate_activations()
        return self

    # -- on-disk formats: scene/gaussian_model.py:63-113,240-318 (gags_amd/io_formats.py) ----------------------
    def save_ply(self, path):
        from . import io_formats
        io_formats.write_ply(path, self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling,
                             self._rotation, self._semantic_feature)

    def load_ply(self, path, device="cuda"):
        self.invalidate_activations()
        from . import io_formats
        t = {k: (None if v is None else torch.from_numpy(np.array(v)).to(device)) for k, v in
             io_formats.read_ply(path, self.max_sh_degree).items()}
        new = GaussianModel.from_tensors(t["xyz"], t["scaling"], t["rotation"], t["opacity"], t["features_dc"],
                                         t["features_rest"], t["semantic_feature"], sh_degree=self.max_sh_degree)
        self.__dict__.update(new.__dict__)
        self.active_sh_degree = self.max_sh_degree
        return self

    def capture(self):
        """The reference's 13-tuple (scene/gaussian_model.py:63-78).  The densification statistics it carries are the
        model's own once training_setup_rgb / the densification methods created them, zeros of the right shapes before
        (the feature flow never densifies)."""
        dev = self._xyz.device
        n = self._xyz.shape[0]
        return (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
                self._opacity, getattr(self, "max_radii2D", torch.zeros(n, device=dev)),
                getattr(self, "xyz_gradient_accum", torch.zeros(n, 1, device=dev)),
                getattr(self, "denom", torch.zeros(n, 1, device=dev)),
                self.optimizer.state_dict() if self.optimizer is not None else {},
                getattr(self, "spatial_lr_scale", 1.0), self._semantic_feature)

    def restore(self, model_args, semantic_feature_lr=0.001, semantic_dim=16):
        """12-tuple (RGB field: features start from zeros, train.py:82-94) or 13-tuple (feature field: features and
        optimizer state are taken over), as scene/gaussian_model.py:80-113."""
        self.invalidate_activations()
        if len(model_args) not in (12, 13):
            raise ValueError("checkpoint tuple must have 12 or 13 entries")
        (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
         self._opacity, self.max_radii2D, xyz_gradient_accum, denom, opt_dict, self.spatial_lr_scale) = model_args[:12]
        self._semantic_feature = model_args[12] if len(model_args) == 13 else None
        self.training_setup(semantic_feature_lr, semantic_dim)
        if len(model_args) == 13 and opt_dict:
            self.optimizer.load_state_dict(opt_dict)
        self.xyz_gradient_accum, self.denom = xyz_gradient_accum, denom
        return self

    def training_setup(self, semantic_feature_lr=0.001, semantic_dim=16, optimizer_type="default"):
        """Feature-only optimisation, as scene/gaussian_model.py:183-208.  optimizer_type="sparse_adam": the same group in
        optim.SelectiveAdam(skip_zero_rows=True) -- the rows the backward left at zero keep parameter and moments."""
        if optimizer_type not in ("default", "sparse_adam"):
            raise ValueError(f"optimizer_type must be 'default' or 'sparse_adam', not {optimizer_type!r}")
        n = self._xyz.shape[0]
        if self._semantic_feature is None or self._semantic_feature.shape[0] != n:
            self._semantic_feature = nn.Parameter(
                torch.zeros((n, semantic_dim), device=self._xyz.device).contiguous().requires_grad_(True))
        for p in (self._xyz, self._features_dc, self._features_rest, self._opacity, self._scaling, self._rotation):
            p.requires_grad_(False)
        # same constructor call as the reference; on the GPU the step is the single-pass HIP kernel
        groups = [{"params": [self._semantic_feature], "lr": semantic_feature_lr, "name": "semantic_feature"}]
        if optimizer_type == "sparse_adam":
            from .optim import SelectiveAdam
            self.optimizer = SelectiveAdam(groups, lr=0.0, eps=1e-15, skip_zero_rows=True)
        elif self._semantic_feature.is_cuda:
            from .optim import FeatureAdam
            self.optimizer = FeatureAdam(groups, lr=0.0, eps=1e-15)
        else:  # host-side bookkeeping only (CPU unit tests): the stock optimizer the reference uses
            self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        return self.optimizer

    # -- the RGB stage's optimizer and adaptive density control: scene/gaussian_model.py:147-149, 183-220, 261-264, 321-482
    #    (gags_amd/densify.py; train.py:206-218 runs on these unchanged) ------------------------------------------------
    def training_setup_rgb(self, training_args, semantic_dim=16, spatial_lr_scale=None, optimizer_type="default"):
        """Every tensor optimised: the seven named groups the reference's training_setup keeps as comments
        (scene/gaussian_model.py:193-199) with the rates of arguments/__init__.py:76-85, FeatureAdam(lr=0.0, eps=1e-15), the
        densification statistics, percent_dense and the position schedule.  training_setup (feature-only) is untouched.
        optimizer_type="sparse_adam": the same groups in optim.SelectiveAdam, one launch for the seven tensors; the training
        loop passes the view's mask, optimizer.step(render_pkg["visibility_filter"])."""
        from . import densify
        from .optim import FeatureAdam, SelectiveAdam
        if optimizer_type not in ("default", "sparse_adam"):
            raise ValueError(f"optimizer_type must be 'default' or 'sparse_adam', not {optimizer_type!r}")
        if not self._xyz.is_cuda:
            raise RuntimeError("gags_amd.scene.training_setup_rgb: no CPU path (the model must live on the GPU)")
        n, dev = self._xyz.shape[0], self._xyz.device
        if spatial_lr_scale is not None:
            self.spatial_lr_scale = spatial_lr_scale
        elif not hasattr(self, "spatial_lr_scale"):
            self.spatial_lr_scale = 1.0
        self.percent_dense = training_args.percent_dense
        if self._semantic_feature is None or self._semantic_feature.shape[0] != n:
            self._semantic_feature = nn.Parameter(torch.zeros((n, semantic_dim), device=dev))
        for _, attr in densify.GROUPS:
            p = getattr(self, attr)
            if not isinstance(p, nn.Parameter):
                p = nn.Parameter(p.detach().contiguous().float())
                setattr(self, attr, p)
            p.requires_grad_(True)
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        self.max_radii2D = torch.zeros((n,), device=dev)
        a = training_args
        groups = [
            {"params": [self._xyz], "lr": a.position_lr_init * self.spatial_lr_scale, "name": "xyz"},
            {"params": [self._features_dc], "lr": a.feature_lr, "name": "f_dc"},
            {"params": [self._features_rest], "lr": a.feature_lr / 20.0, "name": "f_rest"},
            {"params": [self._opacity], "lr": a.opacity_lr, "name": "opacity"},
            {"params": [self._scaling], "lr": a.scaling_lr, "name": "scaling"},
            {"params": [self._rotation], "lr": a.rotation_lr, "name": "rotation"},
            {"params": [self._semantic_feature], "lr": a.semantic_feature_lr, "name": "semantic_feature"},
        ]
        self.optimizer = (SelectiveAdam if optimizer_type == "sparse_adam" else FeatureAdam)(groups, lr=0.0, eps=1e-15)
        self.xyz_scheduler_args = dict(lr_init=a.position_lr_init * self.spatial_lr_scale,
                                       lr_final=a.position_lr_final * self.spatial_lr_scale,
                                       lr_delay_mult=a.position_lr_delay_mult, max_steps=a.position_lr_max_steps)
        self.invalidate_activations()
        return self.optimizer

    def update_learning_rate(self, iteration):
        """Learning rate of the "xyz" group at `iteration` (host arithmetic); None when there is no such group."""
        from . import densify
        for group in self.optimizer.param_groups:
            if group["name"] == "xyz":
                lr = densify.expon_lr(iteration, **self.xyz_scheduler_args)
                group["lr"] = lr
                return lr

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    def add_densification_stats(self, viewspace_point_tensor, update_filter, width, height, absgrad=False):
        """accum += |grad scaled to the [-1, 1] screen|, denom += 1 over update_filter.  The reference also scales
        viewspace_point_tensor.grad in place; nothing reads it afterwards, so it is left as it is.
        absgrad: read viewspace_point_tensor.absgrad (render(..., absgrad=True)) instead of .grad."""
        from . import densify
        grad = densify.viewspace_gradient(viewspace_point_tensor, True) if absgrad else viewspace_point_tensor.grad
        densify.stats(self, grad, None, update_filter, None, width, height)

    def update_max_radii(self, radii, visibility_filter):
        """train.py:209: max_radii2D[v] = max(max_radii2D[v], radii[v])."""
        from . import densify
        densify.stats(self, None, radii, None, visibility_filter, 0, 0)

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, *, generator=None, samples=None):
        """Clone, split and prune in one plan and one gather.  samples: the [2 n_split, 3] standard-normal draws of the split
        children (tests); otherwise torch.randn(generator=generator) on the device once the count is known."""
        from . import densify
        densify.densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, generator=generator, samples=samples)

    def prune_points(self, mask):
        from . import densify
        densify.prune_points(self, mask)

    def reset_opacity(self):
        from . import densify
        densify.reset_opacity(self)

    # -- MCMC density control (gags_amd/mcmc.py): the method names gsplat's strategy uses -------------------
    def relocate_gs(self, dead_mask=None, *, min_opacity=0.005, uniforms=None, generator=None):
        """Move the dead Gaussians (default: opacity <= min_opacity) onto live ones drawn by opacity; returns their number."""
        from . import mcmc
        return mcmc.relocate(self, dead_mask, min_opacity, uniforms=uniforms, generator=generator)

    def add_new_gs(self, cap_max, *, min_opacity=0.005, uniforms=None, generator=None):
        """Grow by 5 % up to cap_max with copies of Gaussians drawn by opacity; returns the number added."""
        from . import mcmc
        return mcmc.sample_add(self, cap_max, min_opacity, uniforms=uniforms, generator=generator)
