"""Query images and loss maps on the GPU (include/gags_next.h N12): what compute_relvancy.py --image_mode writes per phrase and
view (activate_stream :100-144; the same images at evaluate_iou_loc.py:108-163, 216-221) and the three maps of --loss_mode
(:439-447).  The chain render -> decoder -> relevancy -> activate -> images runs for every phrase, and for every frame of a
video, without leaving the device.

    turbo_lut(device)                                   the 256 x 3 turbo table (a data file of this package)
    colour_maps(act, image, ...)                        the three images from activate_maps' tensors
    query_images(valid_map, image, thresh=0.4, ...)     activate_maps + colour_maps: heatmap, lerf_composited, mask_composited, mask
    query_view(feature_map, cnn_decoder, head, image)   compute_relvancy.py:265-269 for one view
    save_query_images(output_path, positives, idx, images)     the PNG files under the reference's names
    feature_loss_maps(feature_map, gt_feature_map, mask)       (l2, mean |pred|, mean |gt|) over the channels
    loss_maps_view(view, gaussians, pipe, bg, cnn_decoder, cnn_scale_decoder)   one view of compute_loss

8-bit copies follow THIS project's rule, trunc(clamp(x * 255 + 0.5, 0, 255)) (featurevis._save_image); the reference writes its
PNGs through mediapy.  GPU tensors only: there is no CPU path.  Deliberately not here: lerf_composited_whitebg and the loss
figure (matplotlib figures), the spline camera path of --video, the CLIP text encoder."""
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .losses import _pixel_major, read_sam_clip_feature
from .relevancy import activate_maps

_LUT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "turbo_lut.csv")
_lut_host = None
_luts = {}
IMAGE_KEYS = ("heatmap", "lerf_composited", "mask_composited")


def turbo_lut_host():
    """The table as a [256, 3] float32 numpy array: matplotlib.colormaps['turbo'].colors cast to float32, shipped as a text
    data file (matplotlib is not needed at run time)."""
    global _lut_host
    if _lut_host is None:
        lut = np.loadtxt(_LUT_PATH, delimiter=",", dtype=np.float64).astype(np.float32)   # (nine digits: exact float32 values)
        if lut.shape != (256, 3):
            raise RuntimeError(f"{_LUT_PATH}: expected a [256, 3] table, found {lut.shape}")
        _lut_host = lut
    return _lut_host


def turbo_lut(device):
    """The turbo table on `device` (uploaded once per device)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("gags_amd.queryvis: tensors must live on the GPU (there is no CPU path)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _luts:
        _luts[device] = torch.from_numpy(turbo_lut_host()).to(device)
    return _luts[device]


@torch.no_grad()
def colour_maps(act, image, lut=None, box=30, avg2=None, return_uint8=False):
    """The three images of activate_stream from the tensors of relevancy.activate_maps (`act`: heatmap, output, mask, stats of M
    maps [M, h, w]).  image: [h, w, 3] or [F, h, w, 3] float in [0, 1] with M % F == 0; map m uses image m // (M // F).
    avg2 = None: the box mean of `output` is computed (and returned); given: the colour kernel alone runs on it.
    Returns {heatmap, lerf_composited, mask_composited: [M, h, w, 3] float32, avg2 [M, h, w]} and, with return_uint8, the
    same three as uint8 under '<name>_u8'."""
    heat, outp, mask, stats = act["heatmap"], act["output"], act["mask"], act["stats"]
    _lib.on_gpu("queryvis", heat, outp, mask, stats, image)
    dev = heat.device
    M, h, w = heat.shape
    heat, outp, stats = heat.float().contiguous(), outp.float().contiguous(), stats.float().contiguous()
    mask = mask.to(torch.uint8).contiguous()
    img = image.float().contiguous()
    if img.dim() == 3:
        img = img[None]
    if img.dim() != 4 or tuple(img.shape[1:]) != (h, w, 3):
        raise ValueError(f"image must be [{h}, {w}, 3] or [F, {h}, {w}, 3], got {tuple(image.shape)}")
    F = img.shape[0]
    if M % F:
        raise ValueError(f"{M} maps do not divide into {F} frames")
    if tuple(outp.shape) != (M, h, w) or tuple(mask.shape) != (M, h, w) or tuple(stats.shape) != (M, 3):
        raise ValueError("output / mask / stats do not fit the heat maps")
    lut = turbo_lut(dev) if lut is None else lut.to(dev, torch.float32).contiguous()
    if tuple(lut.shape) != (256, 3):
        raise ValueError(f"lut must be [256, 3], got {tuple(lut.shape)}")
    lib = _lib.load()
    out = {k: torch.empty(M, h, w, 3, device=dev) for k in IMAGE_KEYS}
    u8 = {k: torch.empty(M, h, w, 3, dtype=torch.uint8, device=dev) if return_uint8 else None for k in IMAGE_KEYS}
    rgb = [ptr(out[k]) for k in IMAGE_KEYS] + [ptr(u8[k]) for k in IMAGE_KEYS]
    if avg2 is None:
        avg2 = torch.empty(M, h, w, device=dev)
        nb = lib.gags_query_images_scratch_bytes(M, h, w)
        scratch = _lib.scratch(nb, dev)
        check(lib.gags_query_images(M, F, h, w, ptr(heat), ptr(outp), ptr(mask), ptr(stats), ptr(img), ptr(lut), int(box),
                                    ptr(avg2), *rgb, ptr(scratch), nb, _lib.stream()), "gags_query_images")
    else:
        _lib.on_gpu("queryvis", avg2)
        avg2 = avg2.float().contiguous()
        if tuple(avg2.shape) != (M, h, w):
            raise ValueError("avg2 does not fit the heat maps")
        check(lib.gags_query_colour(M, F, h, w, ptr(heat), ptr(outp), ptr(mask), ptr(avg2), ptr(stats), ptr(img), ptr(lut),
                                    *rgb, _lib.stream()), "gags_query_colour")
    out["avg2"] = avg2
    if return_uint8:
        out.update({k + "_u8": u8[k] for k in IMAGE_KEYS})
    return out


@torch.no_grad()
def query_images(valid_map, image, thresh=0.4, lut=None, return_uint8=False):
    """activate_stream (compute_relvancy.py:100-144) for the maps valid_map [M, h, w] (frames x phrases, frame-major; for one
    view: get_max_across(sem_map).squeeze(0)) and image [h, w, 3] or [F, h, w, 3].  Returns a dict of device tensors:
    heatmap, lerf_composited, mask_composited [M, h, w, 3] float32 (what the reference writes into the folders of those names)
    and mask [M, h, w] uint8 (the final mask_pred); with return_uint8 also '<image>_u8'."""
    _lib.on_gpu("queryvis", valid_map, image)
    act = activate_maps(valid_map, thresh=thresh)
    out = colour_maps(act, image, lut=lut, return_uint8=return_uint8)
    del out["avg2"]
    out["mask"] = act["mask"]
    return out


@torch.no_grad()
def query_view(feature_map, cnn_decoder, head, image, thresh=0.4, lut=None, return_uint8=False):
    """compute_relvancy.py:265-269 for one view: the rendered [16, h, w] map through the decoder, the relevancy of every phrase
    of `head` (a relevancy.RelevancyHead) and query_images.  The stages are queued on the current stream one after the other:
    nothing is read back in between."""
    _lib.on_gpu("queryvis", feature_map, image)
    restored = cnn_decoder(feature_map)                          # [512, h, w]
    sem_map = restored.permute(1, 2, 0).unsqueeze(0)              # [1, h, w, 512]
    valid_map = head.get_max_across(sem_map).squeeze(0)           # [n_phrases, h, w]
    return query_images(valid_map, image, thresh=thresh, lut=lut, return_uint8=return_uint8)


def to_uint8(image):
    """This project's 8-bit rule in float32: trunc(clamp(x * 255 + 0.5, 0, 255))."""
    return image.detach().float().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)


def save_query_images(output_path, positives, idx, images):
    """Write query_images' result for one view under the reference's folder and file names (compute_relvancy.py:91-94,112,122,
    143): <output_path>/{heatmap,lerf_composited,mask_composited}/<phrase>_<idx:05d>.png.  Uses the '<name>_u8' tensors when
    the dict holds them, else the float images by the 8-bit rule above.  Returns {(name, phrase): path}."""
    from PIL import Image
    paths = {}
    for key in IMAGE_KEYS:
        u8 = images[key + "_u8"] if key + "_u8" in images else to_uint8(images[key])
        if u8.shape[0] != len(positives):
            raise ValueError(f"{u8.shape[0]} {key} images for {len(positives)} phrases")
        arr = u8.cpu().numpy()
        os.makedirs(os.path.join(str(output_path), key), exist_ok=True)
        for k, phrase in enumerate(positives):
            paths[key, phrase] = os.path.join(str(output_path), key, f"{phrase}_{idx:0>5}.png")
            Image.fromarray(arr[k]).save(paths[key, phrase])
    return paths


def _loss_map(x, pixel_major):
    """(tensor whose memory the kernel reads, layout, C, H, W) of a [C, H, W] map (or [H, W, C] with pixel_major)."""
    if x.dim() != 3:
        raise ValueError(f"a feature map must have three dimensions, got {tuple(x.shape)}")
    if pixel_major:
        x = x if (x.is_contiguous() and x.dtype == torch.float32) else x.float().contiguous()
        return x, 1, x.shape[2], x.shape[0], x.shape[1]
    if _pixel_major(x):
        return x, 1, x.shape[0], x.shape[1], x.shape[2]
    x = x if (x.is_contiguous() and x.dtype == torch.float32) else x.float().contiguous()
    return x, 0, x.shape[0], x.shape[1], x.shape[2]


@torch.no_grad()
def feature_loss_maps(feature_map, gt_feature_map, mask, pixel_major=False):
    """compute_relvancy.py:440-446: with both maps multiplied by the mask,
        l2 = sqrt(sum_c (gt - pred)^2),  mean_abs_pred = mean_c |pred|,  mean_abs_gt = mean_c |gt|      each [H, W] float32,
    the sums in float64, rounded once.  The maps are [C, H, W] -- channel-major memory or a permuted view of [H, W, C] memory
    (the decoders' output), each read as it lies -- or, with pixel_major=True, given as [H, W, C].  mask: [H, W] or [1, H, W], any
    dtype, used as 0 / 1 float.  Any combination of layouts gives the same bits."""
    _lib.on_gpu("queryvis", feature_map, gt_feature_map, mask)
    f, lf, C, H, W = _loss_map(feature_map, pixel_major)
    g, lg, Cg, Hg, Wg = _loss_map(gt_feature_map, pixel_major)
    if (C, H, W) != (Cg, Hg, Wg):
        raise ValueError(f"feature map {(C, H, W)} and ground truth {(Cg, Hg, Wg)} differ in shape")
    if mask.numel() != H * W:
        raise ValueError(f"mask {tuple(mask.shape)} does not fit {H} x {W} pixels")
    m = mask.reshape(H, W).float().contiguous()
    l2, mp, mg = (torch.empty(H, W, device=f.device) for _ in range(3))
    check(_lib.load().gags_feature_loss_maps(C, H * W, ptr(f), lf, ptr(g), lg, ptr(m), ptr(l2), ptr(mp), ptr(mg), _lib.stream()),
          "gags_feature_loss_maps")
    return l2, mp, mg


@torch.no_grad()
def loss_maps_view(view, gaussians, pipe, bg, cnn_decoder, cnn_scale_decoder, speedup=True):
    """One view of compute_loss (compute_relvancy.py:434-447): render, both decoders, the ground-truth assembly and the three
    loss maps (l2, mean_abs_pred, mean_abs_gt); the three-panel figure is left to the caller."""
    from .gaussian_renderer import render
    feature_map = render(view, gaussians, pipe, bg, feature_mode=True)["render"].detach()
    scale_map = cnn_scale_decoder(feature_map)
    if speedup:
        feature_map = cnn_decoder(feature_map)
    gt_feature_map, mask = read_sam_clip_feature(view.img_embed.to(scale_map.device), view.seg_map.to(scale_map.device), scale_map)
    return feature_loss_maps(feature_map, gt_feature_map, mask)
