"""gags_amd -- MI355X-native drop-in for GAGS's feature-rasterization hot path.

Public surface (mirrors the reference's):
    gags_amd.gaussian_renderer.render(viewpoint_camera, pc, pipe, bg_color, feature_mode=True, ...)
    gags_amd.rasterization.rasterization(means, quats, scales, opacities, colors, viewmats, Ks, ...)
    gags_amd.scene.GaussianModel / Camera
    gags_amd.distCUDA2(points)                   (simple_knn._C.distCUDA2; gags_amd/knn.py)
    gags_amd.sam_masks.mask_nms / masks_update / assemble_seg_maps   (preprocess.py's mask post-processing)
    gags_amd.prompts.depth_point_grids / mindepth_point_grids / prompt_scene   (preprocess.py's and SAM_utils.py's prompt grids)
    gags_amd.tilecut.cut_tiles / level_tiles / embed_levels / language_features   (preprocess.py's CLIP tiles from SAM masks)
    gags_amd.mcmc.MCMCStrategy / relocate / sample_add / inject_noise / regularisation   (gsplat's MCMC density strategy)
    gags_amd.bilagrid.BilateralGrid / slice / total_variation_loss   (gsplat's bilateral grid; render(..., bilateral_grid=))
All device work goes through the C-ABI library gags_amd/csrc/libgags_hip.so
(include/gags_raster.h); there is no CPU or PyTorch fallback -- a missing library raises.
"""
__version__ = "0.1.0"


def __getattr__(name):
    if name == "distCUDA2":  # `from gags_amd import distCUDA2` replaces `from simple_knn._C import distCUDA2`
        from .knn import dist2
        return dist2
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
