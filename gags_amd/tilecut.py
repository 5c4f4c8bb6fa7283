"""CLIP tiles from SAM masks on the GPU (include/gags_next.h N14): what preprocess.py's mask2segmap does per kept mask with
get_seg_img, pad_img and cv2.resize(..., (224, 224)) (:356-371, :476-489), and what _embed_clip_sam_tiles does with the tiles
(:338-354, :303) -- from the image and N10's bit-packed masks, in one launch per level, without a per-mask image copy or a
host round trip.

    mask_boxes(bits, H, W)                         [M, 4] int32 (x0, y0, x1, y1), inclusive tight bounds; empty: (0, 0, -1, -1)
    sam_xywh(boxes)                                the same boxes as SAM's `bbox` (x, y, w, h)
    cut_tiles(image, bits, boxes, index=None, bgr=False, dtype=torch.float32)
                                                   [K, 3, 224, 224] fp32 in [0, 1] (or [K, 224, 224, 3] uint8)
    level_tiles(image, levels, bgr=False)          the four kept levels -> four [K_j, 3, 224, 224] tensors
    embed_levels(image, levels, encode, bgr=False) (feature [sum K, E] float16, seg_maps [4, H, W] int32, lengths [4])
    language_features(image, levels, encode, prefix=None, bgr=False)   the same, saved as <prefix>_f.npy / <prefix>_s.npy

GPU tensors only: there is no CPU path.  Limits (checked in the C entries): 1 <= H W < 2^24, K and M <= sam_masks.max_masks().
The image encoder is the caller's (`encode`); SAM and CLIP are not part of this package.

The resize is OpenCV's 8-bit INTER_LINEAR restated from memory (the arithmetic is in the header); it is pinned to cv2 itself
only where tests/golden/tilecut_cv2_vectors.npz has been written.

Deviations from the reference, all deliberate:
* Boxes.  A box that starts outside the image or cuts nothing raises ValueError; the reference's slice would wrap around a
  negative start, and cv2.resize would raise on an empty crop.  (The kernel itself writes an all-zero tile for such a box.)
* Empty levels.  A level without masks gives [0, 3, 224, 224] tiles, no feature rows and length 0; the reference raises
  KeyError there (seg_images has no such key).
* Channel order.  The reference converts the whole image once (COLOR_BGR2RGB, :465); bgr=True reads the channels in reverse
  per tap instead, which is the same values."""

import numpy as np
import torch

from . import _lib, io_formats, sam_masks
from ._lib import check, ptr

LEVELS = ("default", "s", "m", "l")   # the order of the rows of <image>_f.npy (preprocess.py:303, :344)


def side():
    """The tile side, 224 (CLIP's input size)."""
    return int(_lib.load().gags_tilecut_side())


def _check_bits(bits, H, W):
    _lib.on_gpu("tilecut", bits)
    nw = (int(H) * int(W) + 63) // 64
    if bits.dim() != 2 or bits.dtype != torch.int64 or bits.shape[1] != nw:
        raise ValueError(f"bits must be [M, {nw}] int64 for {H} x {W} pixels, got {tuple(bits.shape)} {bits.dtype}")
    return bits.contiguous()


@torch.no_grad()
def mask_boxes(bits, H, W):
    """[M, 4] int32 (x0, y0, x1, y1): the inclusive tight bounds of every mask of pack_masks' bits; (0, 0, -1, -1) for a mask
    without a set pixel.  This is what a [K, H, W] mask stack lacks next to SAM's dicts: a `bbox` (see sam_xywh)."""
    if int(H) < 1 or int(W) < 1:
        raise ValueError(f"the image must have at least one pixel, got {H} x {W}")
    bits = _check_bits(bits, H, W)
    boxes = torch.empty(bits.shape[0], 4, dtype=torch.int32, device=bits.device)
    check(_lib.load().gags_tilecut_boxes(bits.shape[0], int(H), int(W), ptr(bits), ptr(boxes), _lib.stream()), "gags_tilecut_boxes")
    return boxes


def sam_xywh(boxes):
    """(x0, y0, x1, y1) inclusive -> (x0, y0, x1 - x0, y1 - y0): the `bbox` SAM attaches to a mask.  SAM's batched_mask_to_box
    returns the inclusive extreme coordinates and box_xyxy_to_xywh subtracts them without adding one, so w and h are one less
    than the pixel extent and the reference's crop leaves out the mask's last row and column.  (Recalled from segment_anything,
    whose submodule is empty in the reference checkout: not pinned by a fixture.)  A single-pixel or empty mask has no valid
    box under this convention; cut_tiles refuses it."""
    x0, y0, x1, y1 = boxes.unbind(-1) if torch.is_tensor(boxes) else np.moveaxis(np.asarray(boxes), -1, 0)
    out = (x0, y0, x1 - x0, y1 - y0)
    return torch.stack(out, dim=-1) if torch.is_tensor(boxes) else np.stack(out, axis=-1).astype(np.int32)


def _host_boxes(boxes, H, W):
    """[K, 4] int64 on the host from a list, an array or a tensor (a GPU tensor is read back), validated as the reference's
    slice would need them."""
    b = boxes.detach().cpu().numpy() if torch.is_tensor(boxes) else np.asarray(boxes)
    if b.size == 0:
        b = b.reshape(0, 4)
    if b.ndim != 2 or b.shape[1] != 4:
        raise ValueError(f"boxes must be [K, 4] (x, y, w, h), got {b.shape}")
    b = np.int32(b).astype(np.int64)   # np.int32(mask['bbox']) is the reference's conversion
    x, y, w, h = b.T
    wc, hc = np.minimum(x + w, W) - x, np.minimum(y + h, H) - y
    bad = ~((0 <= x) & (x < W) & (0 <= y) & (y < H) & (wc >= 1) & (hc >= 1))
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f"box {k} = {tuple(int(v) for v in b[k])} does not cut a {H} x {W} image")
    return b


@torch.no_grad()
def cut_tiles(image, bits, boxes, index=None, bgr=False, dtype=torch.float32):
    """One tile per box: the crop of `image` under mask index[k], zero outside the mask, padded to a square and resized to
    224 x 224 (the contract is in include/gags_next.h N14).

    image [H, W, 3] uint8 on the GPU (HWC, as cv2.imread gives it; a view is copied), bits [M, nw] int64 from
    sam_masks.pack_masks, boxes [K, 4] (x, y, w, h) as a list, array or tensor (validated on the host: ValueError), index [K]
    mask of each tile (default: tile k cuts mask k, K == M).  bgr=True reads the channels in reverse (COLOR_BGR2RGB).
    dtype=torch.float32: [K, 3, 224, 224] in [0, 1], u8 / 255 by an IEEE division -- the bits of the reference's host-side `/ 255.0`,
    :487 -- what encode_image takes;
    dtype=torch.uint8: [K, 224, 224, 3]; dtype=None: both, as (u8, f32).  One launch."""
    if not torch.is_tensor(image) or image.dim() != 3 or image.shape[2] != 3 or image.dtype != torch.uint8:
        raise ValueError(f"image must be an [H, W, 3] uint8 tensor, got {tuple(getattr(image, 'shape', ()))} "
                         f"{getattr(image, 'dtype', type(image))}")
    H, W = int(image.shape[0]), int(image.shape[1])
    if H < 1 or W < 1:
        raise ValueError(f"the image must have at least one pixel, got {H} x {W}")
    if dtype not in (torch.float32, torch.uint8, None):
        raise ValueError(f"dtype must be torch.float32, torch.uint8 or None (both), got {dtype}")
    b = _host_boxes(boxes, H, W)
    _lib.on_gpu("tilecut", image)
    bits = _check_bits(bits, H, W)
    M, dev = bits.shape[0], image.device
    K = b.shape[0]
    if index is None:
        if K != M:
            raise ValueError(f"{K} boxes for {M} masks and no index")
        idx = torch.arange(K, dtype=torch.int32, device=dev)
    else:
        if not torch.is_tensor(index):
            index = torch.from_numpy(np.asarray(index, np.int64).reshape(-1))
        if index.dim() != 1 or index.shape[0] != K:
            raise ValueError(f"index must be [{K}], got {tuple(index.shape)}")
        if not index.is_cuda and K and (int(index.min()) < 0 or int(index.max()) >= M):
            raise ValueError(f"index names masks outside 0 .. {M - 1}")
        idx = index.to(device=dev, dtype=torch.int32).contiguous()   # (a GPU index is range-checked by the kernel: zero tile)
    s = side()
    u8 = torch.empty(K, s, s, 3, dtype=torch.uint8, device=dev) if dtype in (torch.uint8, None) else None
    f32 = torch.empty(K, 3, s, s, dtype=torch.float32, device=dev) if dtype in (torch.float32, None) else None
    if K:
        image = image.contiguous()
        dboxes = torch.from_numpy(np.ascontiguousarray(b, np.int32)).to(dev)   # (b may come in any memory order: row-major here)
        check(_lib.load().gags_tilecut(K, H, W, ptr(image), int(bool(bgr)), M, ptr(bits), ptr(idx), ptr(dboxes),
                                       ptr(u8), ptr(f32), _lib.stream()), "gags_tilecut")
    return (u8, f32) if dtype is None else (u8 if dtype == torch.uint8 else f32)


def _level(lvl, H, W, dev):
    """One kept level -> (masks [K, H, W] on the GPU or None when empty, boxes [K, 4] host / GPU)."""
    if isinstance(lvl, (tuple, list)) and len(lvl) == 2 and torch.is_tensor(lvl[0]):
        masks, boxes = lvl
        if masks.dim() != 3 or (masks.shape[0] and tuple(masks.shape[1:]) != (H, W)):
            raise ValueError(f"masks must be [K, {H}, {W}], got {tuple(masks.shape)}")
        if masks.shape[0] == 0:
            return None, None
        return masks.to(dev), boxes
    lvl = list(lvl)
    if not lvl:
        return None, None
    masks = torch.from_numpy(np.stack([np.asarray(m["segmentation"]) for m in lvl], axis=0)).to(dev)
    if tuple(masks.shape[1:]) != (H, W):
        raise ValueError(f"masks of {tuple(masks.shape[1:])} for an image of {(H, W)}")
    return masks, np.stack([np.int32(m["bbox"]) for m in lvl], axis=0)


def _levels(image, levels):
    _lib.on_gpu("tilecut", image)
    levels = list(levels)
    if len(levels) != len(LEVELS):
        raise ValueError(f"levels must be the four kept levels {LEVELS}, got {len(levels)}")
    H, W = int(image.shape[0]), int(image.shape[1])
    return [_level(lvl, H, W, image.device) for lvl in levels]


def _cut_levels(image, parsed, bgr):
    s = side()
    out = []
    for masks, boxes in parsed:
        if masks is None:
            out.append(torch.empty(0, 3, s, s, dtype=torch.float32, device=image.device))
            continue
        bits = sam_masks.pack_masks(masks)[0]
        if boxes is None:   # a mask stack carries no bbox: SAM's own rule from the masks
            boxes = sam_xywh(mask_boxes(bits, image.shape[0], image.shape[1]))
        out.append(cut_tiles(image, bits, boxes, bgr=bgr))
    return out


@torch.no_grad()
def level_tiles(image, levels, bgr=False):
    """mask2segmap's tiles for the four KEPT levels (default, s, m, l): each a list of SAM dicts (`segmentation`, `bbox`) as
    sam_masks.masks_update returns them, or a pair (masks [K, H, W] on any device, boxes [K, 4] (x, y, w, h) or None for
    sam_xywh(mask_boxes(...))).  Returns four [K_j, 3, 224, 224] fp32 tensors on the image's device; an empty level gives
    [0, 3, 224, 224]."""
    return _cut_levels(image, _levels(image, levels), bgr)


@torch.no_grad()
def embed_levels(image, levels, encode, bgr=False):
    """_embed_clip_sam_tiles and the assembly behind <image>_f.npy / <image>_s.npy (preprocess.py:338-354, :292-319).
    `encode` is any callable [K, 3, 224, 224] fp32 cuda -> [K, E] (CLIP's encode_image); every level's embedding goes through
    x / x.norm(dim=-1, keepdim=True) and .cpu().half(), and the rows are concatenated in the order default, s, m, l.  An empty
    level is not encoded.  Returns (feature [sum K, E] float16 on the host, seg_maps [4, H, W] int32 on the GPU, lengths [4]
    int64 on the host), the latter two from sam_masks.assemble_seg_maps."""
    parsed = _levels(image, levels)
    rows = []
    for tiles in _cut_levels(image, parsed, bgr):
        if tiles.shape[0] == 0:
            continue
        e = encode(tiles)
        if e.dim() != 2 or e.shape[0] != tiles.shape[0]:
            raise ValueError(f"encode returned {tuple(e.shape)} for {tiles.shape[0]} tiles")
        rows.append((e / e.norm(dim=-1, keepdim=True)).detach().cpu().half())
    feature = torch.cat(rows, dim=0) if rows else torch.empty(0, 0, dtype=torch.float16)
    stacks = [torch.empty(0, dtype=torch.bool, device=image.device) if m is None else m for m, _ in parsed]
    seg_maps, lengths = sam_masks.assemble_seg_maps(stacks, hw=tuple(image.shape[:2]), device=image.device)
    return feature, seg_maps, lengths


@torch.no_grad()
def language_features(image, levels, encode, prefix=None, bgr=False):
    """embed_levels, and with `prefix` also io_formats.save_language_features(prefix, feature, seg_maps): the two files
    io_formats.load_language_features and the distillation stage read."""
    feature, seg_maps, lengths = embed_levels(image, levels, encode, bgr=bgr)
    if prefix is not None:
        io_formats.save_language_features(prefix, feature, seg_maps)
    return feature, seg_maps, lengths
