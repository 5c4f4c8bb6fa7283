"""SAM mask post-processing of the GAS stage on the GPU (include/gags_next.h N10): what preprocess.py does between SAM's mask
generator and the CLIP tile encoder -- mask_nms (:380-447), filter (:373-378), masks_update (:449-462), the seg-map painting
of mask2segmap (:476-489) and the four-level concatenation that becomes <image>_s.npy (:307-318) -- on bit-packed masks.
The pair loop of mask_nms is a Gram matrix over bit vectors (AND + popcount, integer-exact); every float operation the
reference applies to those counts is applied here in the same order in fp32, so the selections are equal bit for bit.

    pack_masks(masks)                      masks [M, H, W] bool / uint8 -> bits [M, ceil(H W / 64)] int64, area [M] int32
    pair_intersections(bits)               inter [M, M] int32, inter[i, j] = popcount(bits[i] & bits[j])
    column_maxima(inter, area, order)      colmax [3, M] fp32 over ranks: max IoU, max upper / lower "inner" rate per column
    mask_nms(masks, scores, ...)           the reference's function: selected indices in descending-score order, int64
    nms_keep_indices(masks, scores, ...)   the same selection as ascending indices (what `filter` keeps)
    masks_update(*levels, **kwargs)        drop-in: lists of SAM dicts in, a tuple of filtered lists out
    seg_map(bits, kept, H, W, offset=0)    [H, W] int32: offset + the last kept mask covering the pixel, -1 where none
    assemble_seg_maps(levels)              the four kept levels (default, s, m, l) -> seg_maps [4, H, W] int32, lengths [4]

GPU tensors only: there is no CPU path.  Limits (checked in the C entries): 1 <= H W < 2^24, M <= MAX_MASKS.

Deviations from the reference, all deliberate:
* Top-3 fallbacks.  When no score passes score_thr the reference's fallback raises IndexError (`keep_conf[index, 0]` on a
  1-D tensor); its evident intent is implemented instead: the top 3 by score count as passing.  The same for the two
  inner-threshold fallbacks.  (With fewer than 3 masks: all of them.)
* Zero-area masks.  A mask without a set pixel raises ValueError (the reference's answer would be a chain of NaNs; SAM's
  min_mask_region_area never emits one).  The kernels themselves tolerate such a mask.
* Empty levels.  A level without masks yields no indices, a map of -1 and length 0; the reference cannot represent this.
* Score ties.  The reference's unstable sort leaves their order unspecified; here the lower index comes first."""

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr


def max_masks():
    """The cap on M (inter is [M, M] int32: 256 MiB at the cap)."""
    return int(_lib.load().gags_masks_max_count())


def pair_chunk_words():
    """Words of one mask that one block of the pair kernel reduces; longer masks are split across blocks."""
    return int(_lib.load().gags_masks_pair_chunk_words())


def _bytes(masks):
    """[M, H, W] bool / uint8 -> contiguous uint8 view (a bool tensor stores one byte per element)."""
    _lib.on_gpu("sam_masks", masks)
    if masks.dim() != 3:
        raise ValueError(f"masks must be [M, H, W], got {tuple(masks.shape)}")
    if masks.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"masks must be bool or uint8, got {masks.dtype}")
    if masks.shape[1] * masks.shape[2] < 1:
        raise ValueError(f"masks must have at least one pixel, got {tuple(masks.shape)}")
    masks = masks.contiguous()
    return masks.view(torch.uint8) if masks.dtype == torch.bool else masks


@torch.no_grad()
def pack_masks(masks):
    """(bits [M, nw] int64, area [M] int32): pixel p of the flattened row-major image is bit p & 63 of word p >> 6."""
    m8 = _bytes(masks)
    M, hw = m8.shape[0], m8.shape[1] * m8.shape[2]
    bits = torch.empty(M, (hw + 63) // 64, dtype=torch.int64, device=m8.device)
    area = torch.empty(M, dtype=torch.int32, device=m8.device)
    check(_lib.load().gags_masks_pack(M, hw, ptr(m8), ptr(bits), ptr(area), _lib.stream()), "gags_masks_pack")
    return bits, area


def _bits(bits):
    _lib.on_gpu("sam_masks", bits)
    if bits.dim() != 2 or bits.dtype != torch.int64 or bits.shape[1] < 1:
        raise ValueError(f"bits must be [M, nw] int64 with nw >= 1, got {tuple(bits.shape)} {bits.dtype}")
    return bits.contiguous()


@torch.no_grad()
def pair_intersections(bits):
    """inter [M, M] int32 from pack_masks' bits (the padding bits are zero, so only the word count matters)."""
    bits = _bits(bits)
    M, nw = bits.shape
    inter = torch.empty(M, M, dtype=torch.int32, device=bits.device)
    check(_lib.load().gags_masks_pairs(M, nw * 64 - 63, ptr(bits), ptr(inter), _lib.stream()), "gags_masks_pairs")
    return inter


@torch.no_grad()
def column_maxima(inter, area, order):
    """colmax [3, M] fp32 (include/gags_next.h N10) from inter [M, M] int32, area [M] int32 and order [M] (mask indices by
    descending score)."""
    _lib.on_gpu("sam_masks", inter, area, order)
    M = area.shape[0]
    if tuple(inter.shape) != (M, M) or tuple(order.shape) != (M,):
        raise ValueError(f"inter {tuple(inter.shape)}, area {tuple(area.shape)} and order {tuple(order.shape)} disagree")
    inter, area = inter.to(torch.int32).contiguous(), area.to(torch.int32).contiguous()
    order = order.to(torch.int32).contiguous()
    colmax = torch.empty(3, M, dtype=torch.float32, device=area.device)
    check(_lib.load().gags_masks_colmax(M, ptr(inter), ptr(area), ptr(order), ptr(colmax), _lib.stream()), "gags_masks_colmax")
    return colmax


def _nms_device(masks, scores, iou_thr, score_thr, inner_thr):
    """Everything of mask_nms that stays on the device: (idx [M] int64 by descending score, keep [M] bool over ranks,
    the four keep vectors [4, M] before the final AND, any_zero_area 0-dim bool)."""
    m8 = _bytes(masks)
    _lib.on_gpu("sam_masks", scores)
    M, hw = m8.shape[0], m8.shape[1] * m8.shape[2]
    if tuple(scores.shape) != (M,):
        raise ValueError(f"scores must be [{M}], got {tuple(scores.shape)}")
    dev = m8.device
    s_sorted, idx = torch.sort(scores, dim=0, descending=True, stable=True)
    order = idx.to(torch.int32)
    area = torch.empty(M, dtype=torch.int32, device=dev)
    colmax = torch.empty(3, M, dtype=torch.float32, device=dev)
    lib = _lib.load()
    nb = lib.gags_masks_nms_scratch_bytes(M, hw)
    scratch = _lib.scratch(nb, dev)
    check(lib.gags_masks_nms_colmax(M, hw, ptr(m8), ptr(order), ptr(area), ptr(colmax), ptr(scratch), nb, _lib.stream()),
          "gags_masks_nms_colmax")
    top3 = torch.arange(M, device=dev) < 3
    keeps = torch.stack([colmax[0] <= iou_thr, s_sorted > score_thr,
                         colmax[1] <= 1 - inner_thr, colmax[2] <= 1 - inner_thr])
    none = ~keeps.any(dim=1, keepdim=True)
    none[0] = False                       # (the reference has no fallback for the IoU test)
    keeps = torch.where(none, top3[None], keeps)
    return idx, keeps.all(dim=0), keeps, (area == 0).any()


@torch.no_grad()
def mask_nms(masks, scores, iou_thr=0.7, score_thr=0.1, inner_thr=0.2, **kwargs):
    """preprocess.py:380-447 with the reference's signature and defaults: masks [M, H, W] bool / uint8, scores [M] in
    their own dtype (SAM's are float64 and are compared as such).  Returns the selected original indices in descending-
    score order, int64, exactly like the reference's idx[keep], on the masks' device.  One readback."""
    M = masks.shape[0]
    if M == 0:
        _bytes(masks)
        return torch.empty(0, dtype=torch.int64, device=masks.device)
    idx, keep, _, zero = _nms_device(masks, scores, iou_thr, score_thr, inner_thr)
    host = torch.cat([zero.view(1).to(torch.int64), keep.to(torch.int64), idx]).cpu()
    if int(host[0]):
        raise ValueError("mask_nms: a mask without a set pixel (its overlap rates are undefined)")
    return host[1 + M:][host[1:1 + M].bool()].to(masks.device)


@torch.no_grad()
def nms_keep_indices(masks, scores, **kwargs):
    """The masks mask_nms selects as ASCENDING indices int64 (what the reference's `filter` keeps, in original order)."""
    return torch.sort(mask_nms(masks, scores, **kwargs)).values


@torch.no_grad()
def masks_update(*levels, device="cuda", **kwargs):
    """preprocess.py:449-462, drop-in: every level is a list of SAM dicts (`segmentation` [H, W] bool, `predicted_iou`,
    `stability_score`); score = stability_score * predicted_iou in float64.  Returns a tuple of the filtered lists, each
    in its original order.  An empty level stays empty."""
    out = ()
    for lvl in levels:
        lvl = list(lvl)
        if not lvl:
            out += ([],)
            continue
        seg = torch.from_numpy(np.stack([np.asarray(m["segmentation"]) for m in lvl], axis=0)).to(device)
        iou_pred = torch.from_numpy(np.stack([m["predicted_iou"] for m in lvl], axis=0))
        stability = torch.from_numpy(np.stack([m["stability_score"] for m in lvl], axis=0))
        scores = (stability * iou_pred).to(device)
        keep = nms_keep_indices(seg, scores, **kwargs).tolist()
        out += ([lvl[i] for i in keep],)
    return out


@torch.no_grad()
def seg_map(bits, kept, H, W, offset=0):
    """[H, W] int32: offset + the largest k whose mask kept[k] covers the pixel ("later paint wins", mask2segmap), -1 where
    none does.  bits [M, nw] from pack_masks, kept [K] ascending mask indices (any integer dtype; K may be 0)."""
    bits = _bits(bits)
    _lib.on_gpu("sam_masks", kept)
    M, nw = bits.shape
    hw = int(H) * int(W)
    if (hw + 63) // 64 != nw:
        raise ValueError(f"bits hold {nw} words per mask, {H} x {W} pixels need {(hw + 63) // 64}")
    if kept.dim() != 1:
        raise ValueError(f"kept must be [K], got {tuple(kept.shape)}")
    kept = kept.to(torch.int32).contiguous()
    seg = torch.empty(int(H), int(W), dtype=torch.int32, device=bits.device)
    check(_lib.load().gags_masks_paint(M, hw, ptr(bits), kept.shape[0], ptr(kept), int(offset), ptr(seg), _lib.stream()),
          "gags_masks_paint")
    return seg


@torch.no_grad()
def assemble_seg_maps(levels, hw=None, device="cuda"):
    """preprocess.py:307-318 from the four KEPT levels in the order default, s, m, l: each a list of SAM dicts (as
    masks_update returns them) or a mask tensor [K, H, W].  Returns (seg_maps [4, H, W] int32 on the GPU, lengths [4] int64
    on the host): level j is painted in list order and shifted by the kept-mask counts of the levels before it, -1 stays
    -1.  hw = (H, W) is needed only when every level is empty."""
    levels = list(levels)
    stacks = []
    for lvl in levels:
        if torch.is_tensor(lvl):
            stacks.append(lvl if lvl.shape[0] else None)
            hw = hw if lvl.dim() != 3 else tuple(lvl.shape[1:])
        else:
            lvl = list(lvl)
            stacks.append(torch.from_numpy(np.stack([np.asarray(m["segmentation"]) for m in lvl], axis=0)) if lvl else None)
    for s in stacks:
        if s is not None:
            if hw is not None and tuple(s.shape[1:]) != tuple(hw):
                raise ValueError(f"levels differ in size: {tuple(s.shape[1:])} and {tuple(hw)}")
            hw = tuple(s.shape[1:])
    if hw is None:
        raise ValueError("assemble_seg_maps: every level is empty and no hw=(H, W) was given")
    H, W = int(hw[0]), int(hw[1])
    dev = next((s.device for s in stacks if s is not None and s.is_cuda), torch.device(device))
    maps, lengths, offset = [], [], 0
    none_bits = torch.zeros(0, (H * W + 63) // 64, dtype=torch.int64, device=dev)
    for s in stacks:
        k = 0 if s is None else s.shape[0]
        bits = none_bits if s is None else pack_masks(s.to(dev))[0]
        maps.append(seg_map(bits, torch.arange(k, dtype=torch.int32, device=dev), H, W, offset))
        lengths.append(k)
        offset += k
    return torch.stack(maps), torch.tensor(lengths, dtype=torch.int64)
