"""Plain torch / numpy restatement of the GAS stage's mask post-processing (include/gags_next.h N10; preprocess.py's
mask_nms, filter, masks_update, mask2segmap's painting and the level concatenation), written from the rule and not from the
reference's text.  The pair loop is stated in matrix form: integer intersections, then the same fp32 operations element by
element -- count -> fp32, IEEE division, 1 - a b in two roundings, comparisons against 0.5 and 0.85 in fp32.  torch on the
CPU performs exactly these operations, so everything here is bit-comparable with the GPU kernels and with the reference.
tests/golden/sam_masks_vectors.npz (the reference's own functions) is pinned to this file by tests/test_sam_masks_cpu.py."""
import os

import numpy as np
import torch

# the fixture of the reference's own functions (tests/golden/make_golden_sam_masks.py) and how its cases are read
_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_masks_vectors.npz")
Z = np.load(_FIXTURE) if os.path.exists(_FIXTURE) else None   # (absent only while the generator writes it for the first time)
THRESHOLDS = {"def": {}, "call": {"iou_thr": 0.8, "score_thr": 0.7, "inner_thr": 0.5}}
LEVELS = ("default", "s", "m", "l")


def case_masks(case):
    M, H, W = (int(v) for v in Z[f"{case}_shape"])
    return np.unpackbits(Z[f"{case}_masks"])[:M * H * W].reshape(M, H, W).astype(bool)


def case_scores(case):
    return torch.from_numpy(Z[f"{case}_stab"] * Z[f"{case}_iou"])


def scene_levels(scene):
    """The four levels of a fixture scene as lists of SAM dicts (with an `id` to recognise them by)."""
    out = []
    for lname in LEVELS:
        case = f"{scene}_{lname}"
        m = case_masks(case)
        out.append([{"segmentation": m[k], "predicted_iou": Z[f"{case}_iou"][k], "stability_score": Z[f"{case}_stab"][k], "id": k}
                    for k in range(len(m))])
    return out


def pack_bits(masks):
    """[M, H, W] (nonzero = set) -> (bits [M, nw] uint64, area [M] int64): pixel p of the flattened image is bit p & 63 of
    word p >> 6 (numpy's little bit order over little-endian words), zero padded."""
    m = np.asarray(masks).reshape(len(masks), -1) != 0
    nw = (m.shape[1] + 63) // 64
    padded = np.zeros((m.shape[0], nw * 64), bool)
    padded[:, :m.shape[1]] = m
    bits = np.packbits(padded, axis=1, bitorder="little").view("<u8")
    return bits.reshape(m.shape[0], nw), m.sum(axis=1).astype(np.int64)


def intersections(masks):
    """inter [M, M] int64: common set pixels of every pair, an integer matrix product."""
    m = (np.asarray(masks).reshape(len(masks), -1) != 0).astype(np.int64)
    return m @ m.T


def column_maxima(inter, area, order, quirk=True):
    """colmax [3, M] fp32 over ranks (row / column k = mask order[k]): the largest IoU with a better-ranked mask, and the
    largest "inner" rate of the column above the diagonal and -- with the reference's quirk -- from the first
    superdiagonal downwards (quirk=False: strictly from the diagonal downwards, what the code presumably meant)."""
    order = np.asarray(order, np.int64)
    I_int = torch.from_numpy(np.asarray(inter, np.int64)[np.ix_(order, order)])
    a_int = torch.from_numpy(np.asarray(area, np.int64)[order])
    n = len(order)
    I, a = I_int.to(torch.float32), a_int.to(torch.float32)
    rate = I / a[:, None]                     # rate[x, y] = I[x, y] / a[x]
    r_i, r_j = rate, rate.t()                 # for the pair (i, j) = (row, column)
    union = (a_int[:, None] + a_int[None, :] - I_int).to(torch.float32)
    upper = torch.ones(n, n, dtype=torch.bool).triu(1)
    iou = torch.where(upper, I / union, torch.zeros(()))
    val = 1 - r_j * r_i
    zero = torch.zeros(())
    into_upper = torch.where(upper & (r_i < 0.5) & (r_j >= 0.85), val, zero)      # entry [i, j]
    into_lower = torch.where(upper & (r_i >= 0.85) & (r_j < 0.5), val, zero).t()  # entry [j, i]
    inner = into_upper + into_lower           # disjoint supports: one of the two terms is 0
    return torch.stack([iou.max(dim=0).values, inner.triu(1).max(dim=0).values,
                        inner.tril(1 if quirk else 0).max(dim=0).values])


def keep_vectors(colmax, scores_sorted, iou_thr=0.7, score_thr=0.1, inner_thr=0.2):
    """[4, M] bool over ranks: IoU, score, upper inner rate, lower inner rate; a test (other than the IoU test) that nobody
    passes is replaced by "the three best scores pass" (the evident intent of the reference's fallback, which raises)."""
    n = colmax.shape[1]
    keeps = torch.stack([colmax[0] <= iou_thr, scores_sorted > score_thr,
                         colmax[1] <= 1 - inner_thr, colmax[2] <= 1 - inner_thr])
    top3 = torch.arange(n) < 3
    for k in (1, 2, 3):
        if not keeps[k].any():
            keeps[k] = top3
    return keeps


def nms(masks, scores, iou_thr=0.7, score_thr=0.1, inner_thr=0.2, quirk=True):
    """-> dict(idx [M] by descending score (ties: lower index first), colmax [3, M], keeps [4, M], selected = idx[all four])."""
    scores = torch.as_tensor(scores)
    n = len(masks)
    if n == 0:
        e = torch.empty(0, dtype=torch.int64)
        return {"idx": e, "colmax": torch.empty(3, 0), "keeps": torch.empty(4, 0, dtype=torch.bool), "selected": e}
    inter = intersections(masks)
    area = np.diagonal(inter).copy()
    if (area == 0).any():
        raise ValueError("a mask without a set pixel")
    s_sorted, idx = torch.sort(scores, descending=True, stable=True)
    colmax = column_maxima(inter, area, idx.numpy(), quirk=quirk)
    keeps = keep_vectors(colmax, s_sorted, iou_thr, score_thr, inner_thr)
    return {"idx": idx, "colmax": colmax, "keeps": keeps, "selected": idx[keeps.all(dim=0)]}


def mask_nms(masks, scores, **kw):
    return nms(masks, scores, **kw)["selected"]


def filter_list(selected, items):
    """The items whose position is among `selected`, in their original order."""
    chosen = set(int(i) for i in selected)
    return [m for k, m in enumerate(items) if k in chosen]


def masks_update(*levels, **kw):
    out = ()
    for lvl in levels:
        lvl = list(lvl)
        if not lvl:
            out += ([],)
            continue
        seg = np.stack([m["segmentation"] for m in lvl])
        scores = torch.from_numpy(np.stack([m["stability_score"] for m in lvl]) * np.stack([m["predicted_iou"] for m in lvl]))
        out += (filter_list(mask_nms(seg, scores, **kw), lvl),)
    return out


def paint(masks, H, W, offset=0):
    """[H, W] int32: masks painted in order, a later one over an earlier one; offset + position, -1 where none."""
    seg = np.full((H, W), -1, np.int32)
    for k, m in enumerate(masks):
        seg[np.asarray(m).reshape(H, W) != 0] = k + offset
    return seg


def concat_levels(levels, H, W):
    """Four (or any number of) kept levels -> (seg_maps [L, H, W] int32, lengths [L]): level j shifted by the sizes of the
    levels before it."""
    maps, lengths, offset = [], [], 0
    for lvl in levels:
        maps.append(paint(lvl, H, W, offset))
        lengths.append(len(lvl))
        offset += len(lvl)
    return np.stack(maps), np.array(lengths, np.int64)


def rect_masks(rng, n, H, W, holes=0.1):
    """n random masks [n, H, W] bool with structure mask_nms reacts to: free rectangles, rectangles nested in an earlier
    one, and jittered near-copies of an earlier one; every mask loses `holes` of its pixels at random and keeps >= 1."""
    out = np.zeros((n, H, W), bool)
    boxes = []
    for k in range(n):
        kind = rng.random()
        if boxes and kind < 0.3:      # nested in an earlier box
            y0, y1, x0, x1 = boxes[rng.integers(len(boxes))]
            h, w = max(1, int((y1 - y0) * rng.uniform(0.2, 0.7))), max(1, int((x1 - x0) * rng.uniform(0.2, 0.7)))
            ya, xa = rng.integers(y0, y1 - h + 1), rng.integers(x0, x1 - w + 1)
            box = (ya, ya + h, xa, xa + w)
        elif boxes and kind < 0.5:    # near-copy of an earlier box
            y0, y1, x0, x1 = boxes[rng.integers(len(boxes))]
            dy, dx = rng.integers(-1, 2), rng.integers(-1, 2)
            box = (max(0, y0 + dy), min(H, max(y0 + dy + 1, y1 + dy)), max(0, x0 + dx), min(W, max(x0 + dx + 1, x1 + dx)))
        else:
            h, w = rng.integers(2, H + 1), rng.integers(2, W + 1)
            ya, xa = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
            box = (ya, ya + h, xa, xa + w)
        boxes.append(box)
        out[k, box[0]:box[1], box[2]:box[3]] = True
        out[k] &= rng.random((H, W)) >= holes
        if not out[k].any():
            out[k, box[0], box[2]] = True
    return out
