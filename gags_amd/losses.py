"""The image-space losses and ground-truth assembly of the distillation step, same function
names, arguments and results as the reference's, on HIP kernels (include/gags_next.h, csrc/seg_losses.hip, distill_l1.hip, head_distill.hip):

    utils/loss_utils.py:20-24     l1_loss, l1_loss_map
    utils/loss_utils.py:32-57     Scale_balance_loss(loss_map, seg_map, mask, mix_seg=True)
    utils/loss_utils.py:59-66     scale_regulation_loss(scale_map)
    utils/loss_utils.py:103-136   scale_region_regulation_loss(scale_map, seg_map, mix_seg=True)
    utils/loss_utils.py:138-154   get_trained_seg(seg_map, scale_map)
    scene/dataset_readers.py:54-121  read_sam_clip_feature(img_embed, seg_map, scale_map)   (default mode)
    utils/loss_utils.py:168-198   ssim(img1, img2, window_size=11, size_average=True)                      (row N7)
    utils/image_utils.py:17-19    psnr(img1, img2)                                                         (row N7)
plus photometric_loss(image, gt, lambda_dssim) = (1 - lambda) l1_loss + lambda (1 - ssim), the loss of an RGB step, as one
forward and one backward kernel (csrc/photometric.hip),
and the fusion the reference's train.py:165-166 spells as three full-size elementwise passes plus a [512,H,W]
ground-truth tensor:
    distill_l1_map(pred, img_embed, seg_map, scale_map) == l1_loss_map(pred * mask, gt * mask), mask

The reference walks the segment ids in a Python loop (one boolean-mask pass over the image per id); here one pass
over the pixels accumulates every segment's moments (gags_segment_stats) and the tiny per-segment arithmetic is done
on [n_seg]-sized tensors.  Only the variants train.py reaches are implemented (mix_seg=True; default gather mode);
anything else raises.  GPU tensors only: there is no CPU path.
"""
import ctypes
import os
import weakref

import torch

from . import _lib
from ._lib import check, ptr


def _f(t):
    _lib.on_gpu("losses", t)
    return t if (t.is_contiguous() and t.dtype == torch.float32) else t.contiguous().float()


_NSEG_CACHE = {}  # id(tensor) -> (weak reference, data_ptr, version counter, n_seg)


def _n_seg(seg_map):
    """Size of the per-segment tables: any bound above the largest id gives the same sums (rows nobody hits stay empty, ids
    outside [0, n_seg) are skipped by the kernels).  ids are small non-negative integers stored as floats; the bound costs ONE
    readback per segmentation map, not one per iteration (a host sync in the middle of an iteration drains the queue: the
    dozens of small launches behind it then run at the host's pace -- ~0.5 ms each time at 1080p): a view's SAM map does not
    change between iterations, so the answer is kept per tensor (identity, address and version counter), and
    get_trained_seg hands the bound of its source map on to the map it makes (`_gags_n_seg`).
    The version counter only sees torch's own in-place operators: a map refilled through raw pointers (a kernel, DLPack, a
    c10d collective) keeps the old bound, and ids above it are skipped.  The composed iteration does not depend on that:
    distill.distillation_loss passes the bound it knows without looking at the data (the embedding table's row count) to
    get_trained_seg(n_seg=...), no readback at all; a caller of the single losses who refills a map that way calls
    forget_n_seg()."""
    hint = getattr(seg_map, "_gags_n_seg", None)
    if hint is not None:
        return hint
    key = id(seg_map)
    hit = _NSEG_CACHE.get(key)
    if hit is not None and hit[0]() is seg_map and hit[1] == seg_map.data_ptr() and hit[2] == seg_map._version:
        return hit[3]
    n = max(int(seg_map.max().item()) + 1, 1)
    if len(_NSEG_CACHE) > 4096:
        _NSEG_CACHE.clear()
    _NSEG_CACHE[key] = (weakref.ref(seg_map), seg_map.data_ptr(), seg_map._version, n)
    return n


def forget_n_seg(seg_map=None):
    """Drop the remembered bound of `seg_map` (None: of every map): the next loss on it reads the bound back again."""
    if seg_map is None:
        _NSEG_CACHE.clear()
    else:
        _NSEG_CACHE.pop(id(seg_map), None)


def l1_loss(network_output, gt):
    return torch.abs(network_output - gt).mean()


def l1_loss_map(network_output, gt):
    return torch.abs(network_output - gt).mean(dim=0)


class _Entropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scale_map):
        s = _f(scale_map)
        acc = torch.zeros(1, dtype=torch.float64, device=s.device)
        check(_lib.load().gags_entropy_fwd(s.numel(), ptr(s), ptr(acc), _lib.stream()), "gags_entropy_fwd")
        ctx.save_for_backward(s)
        return (acc[0] / s.numel()).float()

    @staticmethod
    def backward(ctx, v):
        (s,) = ctx.saved_tensors
        vs = torch.empty_like(s)
        vd = v.detach().reshape(1).float().contiguous()  # (read on the device: no readback inside the backward pass)
        check(_lib.load().gags_entropy_bwd_dev(s.numel(), ptr(s), ptr(vd), ptr(vs), _lib.stream()), "gags_entropy_bwd_dev")
        return vs


def scale_regulation_loss(scale_map):
    """mean(-s * log(s + 1e-6)) over the [3,H,W] scale map (utils/loss_utils.py:59-66)."""
    return _Entropy.apply(scale_map)


RUNS = os.environ.get("GAGS_SEGMENT_RUNS", "1") != "0"  # 0: the wave-sum + double-atomic kernel for every shape
_STAT_COPIES = 16  # private accumulator sets of gags_segment_stats_multi (the double atomics serialize per address)


def _segment_copies(x, seg_map, n_seg, pixel_major=False):
    """Per-segment moments of x ([c, n_pix], or [n_pix, c] with pixel_major) as private copies: s1, s2 [k, n_seg, c] doubles
    and counts [k, n_seg]; the caller sums over k."""
    n_pix = seg_map.numel()
    c = x.shape[1] if pixel_major else x.shape[0]
    lib = _lib.load()
    k = lib.gags_segment_stats_runs_copies(n_pix, c, n_seg, 1 if pixel_major else 0) if RUNS else 0
    if k > 0:  # sums by runs of equal ids into one private table per workgroup: no global atomics (csrc/seg_losses.hip)
        s1 = torch.empty(k, n_seg, c, dtype=torch.float64, device=x.device)
        s2 = torch.empty_like(s1)
        cnt = torch.empty(k, n_seg, dtype=torch.int32, device=x.device)
        check(lib.gags_segment_stats_runs(n_pix, c, ptr(x), ptr(seg_map), n_seg, k, ptr(s1), ptr(s2), ptr(cnt),
                                          1 if pixel_major else 0, _lib.stream()), "gags_segment_stats_runs")
        return s1, s2, cnt
    k = _STAT_COPIES if n_seg * c * _STAT_COPIES <= (1 << 22) else 1
    s1 = torch.zeros(k, n_seg, c, dtype=torch.float64, device=x.device)
    s2 = torch.zeros_like(s1)
    cnt = torch.zeros(k, n_seg, dtype=torch.int32, device=x.device)
    check(lib.gags_segment_stats_multi(n_pix, c, ptr(x), ptr(seg_map), n_seg, k, ptr(s1), ptr(s2), ptr(cnt),
                                       1 if pixel_major else 0, _lib.stream()), "gags_segment_stats_multi")
    return s1, s2, cnt


def _segment_stats(x, seg_map, n_seg, pixel_major=False):
    """The moments summed over the copies: s1, s2 [n_seg, c], counts [n_seg]."""
    s1, s2, cnt = _segment_copies(x, seg_map, n_seg, pixel_major)
    return s1.sum(0), s2.sum(0), cnt.sum(0, dtype=torch.int32)


def _segment_loss(mode, x, seg_map, n_seg, pixel_major=False):
    """(loss [1] float, coef [n_seg] float, mean [n_seg, c] float or None) of gags_segment_loss: mode 0 = Scale_balance_loss,
    1 = scale_region_regulation_loss -- the copies' sum and all of the double-precision arithmetic on [n_seg] vectors in two
    launches."""
    s1c, s2c, cntc = _segment_copies(x, seg_map, n_seg, pixel_major)
    k, _, c = s1c.shape
    dev = x.device
    s1 = torch.empty(n_seg, c, dtype=torch.float64, device=dev)
    s2 = torch.empty_like(s1)
    cnt = torch.empty(n_seg, dtype=torch.int32, device=dev)
    loss = torch.empty(1, device=dev)
    coef = torch.empty(n_seg, device=dev)
    mean = torch.empty(n_seg, c, device=dev) if mode == 1 else None
    check(_lib.load().gags_segment_loss(mode, n_seg, c, k, seg_map.numel(), ptr(s1c), ptr(s2c), ptr(cntc), ptr(s1), ptr(s2),
                                        ptr(cnt), ptr(loss), ptr(coef), ptr(mean), _lib.stream()), "gags_segment_loss")
    return loss, coef, mean


class _ScaleBalance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, loss_map, seg_map):
        lm, seg = _f(loss_map), _f(seg_map)
        n_seg = _n_seg(seg_map)
        loss, coef, _ = _segment_loss(0, lm.reshape(1, -1), seg.reshape(-1), n_seg)
        ctx.save_for_backward(seg, coef)
        ctx.n_seg = n_seg
        return loss[0]

    @staticmethod
    def backward(ctx, v):
        seg, coef = ctx.saved_tensors
        out = torch.empty_like(seg)
        check(_lib.load().gags_gather_seg_coef(seg.numel(), ptr(seg), ctx.n_seg, ptr((coef * v).contiguous()), ptr(out), _lib.stream()),
              "gags_gather_seg_coef")
        return out, None


def Scale_balance_loss(loss_map, seg_map, mask, scale_select_idx=1, mix_seg=False):
    """Mean over the segments present in seg_map [H,W] of the segment's mean of loss_map [H,W]
    (utils/loss_utils.py:32-57 with mix_seg=True, the only form train.py:167 uses; `mask` is unused there too)."""
    if not mix_seg:
        raise NotImplementedError("Scale_balance_loss: only mix_seg=True (train.py:167) is implemented")
    return _ScaleBalance.apply(loss_map, seg_map)


class _RegionVar(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, seg_map):
        seg = _f(seg_map)
        c, hh, ww = x.shape
        # the rasterizer hands its [H,W,C] memory over as a [C,H,W] view: read it as it lies (pixel-major) instead of
        # copying 132 MB into channel-major order every iteration
        pm = x.is_cuda and x.dtype == torch.float32 and not x.is_contiguous() and x.permute(1, 2, 0).is_contiguous()
        x = x.permute(1, 2, 0) if pm else _f(x)
        n_seg = _n_seg(seg_map)
        # unbiased variances (torch.var) from moments accumulated in double about a member of each group (csrc/seg_losses.hip): the
        # subtraction is a double-precision one on accurately summed terms; segments of 0 or 1 pixels are skipped
        # (loss_utils.py:124-125); copies' sum, variances, loss and the backward's tables in two launches (gags_segment_loss)
        loss, coef, mean = _segment_loss(1, x.reshape(-1, c) if pm else x.reshape(c, -1), seg.reshape(-1), n_seg, pixel_major=pm)
        ctx.save_for_backward(x, seg, mean, coef)
        ctx.n_seg, ctx.pm, ctx.c = n_seg, pm, c
        return loss[0]

    @staticmethod
    def backward(ctx, v):
        x, seg, mean, coef = ctx.saved_tensors
        vx = torch.empty_like(x)  # (pixel-major input: [H,W,C] memory, returned as the [C,H,W] view of it)
        check(_lib.load().gags_region_var_bwd_layout(seg.numel(), ctx.c, ptr(x), ptr(seg), ctx.n_seg, ptr(mean),
                                                     ptr((coef * v).contiguous()), ptr(vx), 1 if ctx.pm else 0, _lib.stream()),
              "gags_region_var_bwd_layout")
        return (vx.permute(2, 0, 1) if ctx.pm else vx), None


class _RegionVarTee(torch.autograd.Function):
    """_RegionVar that also hands its input on: (loss, x') with x' an alias of x for the NEXT consumer of the map.  The
    backward then receives that consumer's gradient together with the loss's cotangent and adds the two in the kernel that
    forms the loss's own gradient (gags_region_var_bwd_add) -- autograd's separate sum of two 132 MB maps per 1080p iteration
    is gone.  Same values: one fp32 addition per element either way."""

    @staticmethod
    def forward(ctx, x, seg_map):
        loss = _RegionVar.forward(ctx, x, seg_map)
        return loss, x.view_as(x)

    @staticmethod
    def backward(ctx, v, g_next):
        if g_next is None:
            return _RegionVar.backward(ctx, v)
        x, seg, mean, coef = ctx.saved_tensors
        gp = g_next.permute(1, 2, 0) if ctx.pm else g_next
        if not (ctx.pm and ctx.c % 4 == 0 and gp.is_contiguous() and gp.dtype == torch.float32):
            vx, _ = _RegionVar.backward(ctx, v)
            return vx + g_next, None
        vx = torch.empty_like(x)
        check(_lib.load().gags_region_var_bwd_add(seg.numel(), ctx.c, ptr(x), ptr(seg), ctx.n_seg, ptr(mean),
                                                  ptr((coef * v).contiguous()), ptr(gp), ptr(vx), _lib.stream()), "gags_region_var_bwd_add")
        return vx.permute(2, 0, 1), None


def scale_region_regulation_loss_tee(scale_map, seg_map):
    """(scale_region_regulation_loss(scale_map, seg_map, mix_seg=True), scale_map'): use scale_map' wherever the map is
    consumed afterwards (gags_amd/distill.py feeds it to CNN_decoder) and the two gradients are summed in one kernel."""
    return _RegionVarTee.apply(scale_map, seg_map)


def scale_region_regulation_loss(scale_map, seg_map, scale_bal_idx=1, mix_seg=False):
    """sum over segments of n_seg * mean_c(var_c) / (H*W) of the map [C,H,W] under seg_map [H,W]
    (utils/loss_utils.py:103-136 with mix_seg=True; train.py:153 feeds it the rasterized feature map)."""
    if not mix_seg:
        raise NotImplementedError("scale_region_regulation_loss: only mix_seg=True (train.py:153) is implemented")
    return _RegionVar.apply(scale_map, seg_map)


def get_trained_seg(seg_map, scale_map, n_seg=None):
    """seg_map [4,H,W], scale_map [3,H,W] -> [H,W]: the segment id of the level the 5x5-smoothed scale map prefers.
    n_seg: a bound above every id of seg_map that the caller KNOWS (the ids index the view's embedding table: its row count),
    handed on to the losses that read the result; None: _n_seg's readback, remembered per tensor."""
    seg, sc = _f(seg_map), _f(scale_map.detach())
    _, h, w = seg.shape
    out = torch.empty(h, w, device=seg.device)
    check(_lib.load().gags_trained_seg(h, w, ptr(seg), ptr(sc), ptr(out), _lib.stream()), "gags_trained_seg")
    out._gags_n_seg = _n_seg(seg_map) if n_seg is None else max(int(n_seg), 1)  # (every id of the result is an id of seg_map)
    return out


class _SamFeature(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img_embed, seg_map, scale_map):
        e, seg, sc = _f(img_embed), _f(seg_map), _f(scale_map)
        c, (_, h, w), (_, H, W) = e.shape[1], seg.shape, sc.shape
        feat = torch.empty(c, H, W, device=e.device)
        mask = torch.empty(H, W, device=e.device)
        check(_lib.load().gags_sam_clip_feature(c, H, W, h, w, e.shape[0], ptr(e), ptr(seg), ptr(sc), ptr(feat), ptr(mask),
                                                _lib.stream()), "gags_sam_clip_feature")
        ctx.save_for_backward(e, seg)
        ctx.dims = (c, H, W, h, w)
        ctx.mark_non_differentiable(mask)
        return feat, mask

    @staticmethod
    def backward(ctx, v_feat, _v_mask):
        e, seg = ctx.saved_tensors
        c, H, W, h, w = ctx.dims
        vs = torch.empty(3, H, W, device=e.device)
        check(_lib.load().gags_sam_clip_feature_bwd_scale(c, H, W, h, w, e.shape[0], ptr(e), ptr(seg), ptr(_f(v_feat)), ptr(vs),
                                                          _lib.stream()), "gags_sam_clip_feature_bwd_scale")
        return None, None, vs


def read_sam_clip_feature(img_embed, seg_map, scale_map, max_mode=False, median_mode=False, show_scale_map=False):
    """(feature_map [C,H,W], mask [1,H,W] bool) as scene/dataset_readers.py:54-121 in its default mode, or with
    max_mode=True (:81-88, render.py:64,154; forward only): the arg-max level's feature where that level has a segment,
    and mask = feature_map[0:1] != 0."""
    if median_mode or show_scale_map:
        raise NotImplementedError("read_sam_clip_feature: only the default mode (train.py:162,165) and max_mode "
                                  "(render.py:64,154) are implemented")
    if max_mode:
        with torch.no_grad():
            e, seg, sc = _f(img_embed), _f(seg_map), _f(scale_map)
            c, (_, h, w), (_, H, W) = e.shape[1], seg.shape, sc.shape
            feat = torch.empty(c, H, W, device=e.device)
            mask = torch.empty(H, W, device=e.device)
            check(_lib.load().gags_sam_clip_feature_max(c, H, W, h, w, e.shape[0], ptr(e), ptr(seg), ptr(sc), ptr(feat),
                                                        ptr(mask), _lib.stream()), "gags_sam_clip_feature_max")
        return feat, (mask != 0)[None]
    feat, mask = _SamFeature.apply(img_embed, seg_map, scale_map)
    return feat, (mask != 0)[None]


def _pixel_major(t):
    """True when the [C,H,W] tensor is a permuted view of contiguous [H,W,C] fp32 memory (the decoder's and the
    rasterizer's output layout)."""
    return (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and not t.is_contiguous()
            and t.permute(1, 2, 0).is_contiguous())


class _DistillL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, img_embed, seg_map, scale_map):
        e, seg, sc = _f(img_embed), _f(seg_map), _f(scale_map)
        c, (_, h, w), (_, H, W) = e.shape[1], seg.shape, sc.shape
        if tuple(pred.shape) != (c, H, W):
            raise ValueError(f"pred {tuple(pred.shape)} vs embeddings of width {c} and a {H}x{W} scale map")
        pm = _pixel_major(pred) and c % 4 == 0
        p = pred if pm else _f(pred)  # pixel-major memory is consumed as it is (layout 1): rows in, rows out
        l1 = torch.empty(H, W, device=p.device)
        mask = torch.empty(H, W, device=p.device)
        check(_lib.load().gags_distill_l1_map_fwd(c, H, W, h, w, e.shape[0], ptr(p), ptr(e), ptr(seg), ptr(sc), ptr(l1),
                                                  ptr(mask), 1 if pm else 0, _lib.stream()), "gags_distill_l1_map_fwd")
        ctx.save_for_backward(p, e, seg, sc)
        ctx.dims = (c, H, W, h, w)
        ctx.pm = pm
        ctx.mark_non_differentiable(mask)
        return l1, mask

    @staticmethod
    def backward(ctx, v_map, _v_mask):
        p, e, seg, sc = ctx.saved_tensors
        c, H, W, h, w = ctx.dims
        # the gradient in the prediction's own layout: [H,W,c] memory behind a [c,H,W] view when it is pixel-major
        vp = torch.empty(H, W, c, device=p.device).permute(2, 0, 1) if ctx.pm else torch.empty_like(p)
        vs = torch.empty(3, H, W, device=p.device)
        check(_lib.load().gags_distill_l1_map_bwd(c, H, W, h, w, e.shape[0], ptr(p), ptr(e), ptr(seg), ptr(sc), ptr(_f(v_map)),
                                                  ptr(vp), ptr(vs), 1 if ctx.pm else 0, _lib.stream()), "gags_distill_l1_map_bwd")
        return vp, None, None, vs


def distill_l1_map(pred, img_embed, seg_map, scale_map):
    """train.py:165-166 in one pass: (l1_loss_map(pred * mask, gt * mask) [H,W], mask [1,H,W] bool) with
    gt, mask = read_sam_clip_feature(img_embed, seg_map, scale_map); gradients reach `pred` and `scale_map`."""
    l1, mask = _DistillL1.apply(pred, img_embed, seg_map, scale_map)
    return l1, (mask != 0)[None]


# ----------------------------------------------------------------------------------------------------------------------
# N7: the photometric loss of the RGB stage (include/gags_next.h, csrc/photometric.hip)

# utils/loss_utils.py:158-160 gaussian(11, 1.5): exp(-(x - 5)**2 / 4.5) in Python doubles, rounded into a float32 tensor,
# divided by its float32 sum -- the eleven float32 values, spelled out (they sum to 1 - 3.1e-8, and nothing renormalises
# them).  This tuple is what the kernels are launched with; tests/test_photometric_cpu.py compares it with the reference's.
SSIM_WINDOW = (0.001028380123898387, 0.0075987582094967365, 0.036000773310661316, 0.10936068743467331, 0.21300552785396576,
               0.26601171493530273, 0.21300552785396576, 0.10936068743467331, 0.036000773310661316, 0.0075987582094967365,
               0.001028380123898387)
_WINDOW_C = (ctypes.c_float * 11)(*SSIM_WINDOW)


def _photo_view(t):
    """(tensor, planes, images, h, w, element strides of plane / row / column) of a [C,H,W] or [B,C,H,W] float32 GPU tensor
    read where it lies: the planes must be equally spaced (a contiguous tensor, or the [C,H,W] view of the rasterizer's
    [H,W,C] memory); anything else is copied once."""
    _lib.on_gpu("losses", t)
    if t.dim() not in (3, 4):
        raise ValueError(f"expected [C,H,W] or [B,C,H,W], got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        t = t.float()
    if any(st == 0 and sz > 1 for st, sz in zip(t.stride(), t.shape)):  # (an expanded tensor: its gradient needs elements of its own)
        t = t.contiguous()
    if t.dim() == 4:
        b, c = t.shape[:2]
        if not (b == 1 or c == 1 or t.stride(0) == c * t.stride(1)):
            t = t.contiguous()
        sp = t.stride(1) if c > 1 else t.stride(0)
    else:
        b, c = 1, t.shape[0]
        sp = t.stride(0)
    h, w = t.shape[-2:]
    if b * c * h * w == 0:
        raise ValueError(f"empty image {tuple(t.shape)}")
    return t, b * c, t.shape[0], h, w, (sp, t.stride(-2), t.stride(-1))


def _photo_forward(x, y, bias, wa, wb, reduce_all, need_grad):
    """One gags_photometric_fwd: (out [1] or [images] float, sums [images, 3] double, k [2] float, dm or None, views)."""
    x, planes, images, h, w, xs = _photo_view(x)
    y, planes_y, _, hy, wy, ys = _photo_view(y)
    if (planes_y, hy, wy) != (planes, h, w) or x.dim() != y.dim():
        raise ValueError(f"image {tuple(x.shape)} vs ground truth {tuple(y.shape)}")
    lib = _lib.load()
    dev = x.device
    partials = torch.empty(lib.gags_photometric_partials(planes, h, w), 3, dtype=torch.float64, device=dev)
    sums = torch.empty(images, 3, dtype=torch.float64, device=dev)
    out = torch.empty(1 if reduce_all else images, device=dev)
    k = torch.empty(2, device=dev)
    dm = torch.empty(3, planes, h, w, device=dev) if need_grad else None
    check(lib.gags_photometric_fwd(planes, images, h, w, ptr(x), *xs, ptr(y), *ys, _WINDOW_C, bias, wa, wb, 1 if reduce_all else 0,
                                   ptr(dm), None, ptr(partials), ptr(sums), ptr(out), ptr(k), _lib.stream()), "gags_photometric_fwd")
    return out, sums, k, dm, (x, xs, y, ys, planes, images, h, w)


class _Photometric(torch.autograd.Function):
    """out = bias + wa mean|x - y| + wb mean(ssim map), over everything ([] result) or per image ([images])."""

    @staticmethod
    def forward(ctx, image, gt, bias, wa, wb, reduce_all):
        if gt.requires_grad:
            raise RuntimeError("gags_amd.losses: the ground truth of ssim / photometric_loss is not differentiated")
        need = ctx.needs_input_grad[0]
        out, _, k, dm, (x, xs, y, ys, planes, images, h, w) = _photo_forward(image, gt, bias, wa, wb, reduce_all, need)
        if need:
            ctx.save_for_backward(x, y, dm, k)
            ctx.geom = (xs, ys, planes, 1 if reduce_all else images, h, w)
        return out[0] if reduce_all else out

    @staticmethod
    def backward(ctx, v):
        x, y, dm, k = ctx.saved_tensors
        xs, ys, planes, groups, h, w = ctx.geom
        # (a, b) per image = the cotangent times (wa / n, wb / n), formed on the device: no readback inside the backward pass
        coef = (v.detach().reshape(-1, 1).float() * k).contiguous()
        vx = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=x.device)  # written in x's own layout
        check(_lib.load().gags_photometric_bwd(planes, groups, h, w, ptr(x), *xs, ptr(y), *ys, _WINDOW_C, ptr(dm), ptr(coef),
                                               ptr(vx), *xs, _lib.stream()), "gags_photometric_bwd")
        return vx, None, None, None, None, None


def _check_window(window_size):
    if window_size != 11:
        raise NotImplementedError("ssim: only window_size=11 (the reference's default, the one train.py uses) is implemented")


def ssim(img1, img2, window_size=11, size_average=True):
    """utils/loss_utils.py:168-198 on [C,H,W] or [B,C,H,W]: the mean of the SSIM map, or with size_average=False the mean per
    image ([B]; a [C,H,W] input is one image).  Differentiable in img1."""
    _check_window(window_size)
    if img1.dim() == 3 and not size_average:
        return _Photometric.apply(img1[None], img2[None], 0.0, 0.0, 1.0, False)
    return _Photometric.apply(img1, img2, 0.0, 0.0, 1.0, bool(size_average))


def photometric_loss(image, gt, lambda_dssim=0.2):
    """(1 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1 - ssim(image, gt)): 3DGS's RGB loss
    (arguments/__init__.py:88: lambda_dssim = 0.2), one forward launch plus the sum of the workgroups' partials, one backward
    launch.  `image` may be the [3,H,W] view render() returns: it is read, and its gradient written, through its strides."""
    lam = float(lambda_dssim)
    return _Photometric.apply(image, gt, lam, 1.0 - lam, -lam, True)


def psnr(img1, img2):
    """utils/image_utils.py:17-19: 20 log10(1 / sqrt(mse)) with the mean squared error per entry of the FIRST dimension (the
    reference's batch), [B, 1]; from the third partial sum of the forward kernel.  Not differentiated."""
    with torch.no_grad():
        a = img1 if img1.dim() == 4 else img1[:, None]
        b = img2 if img2.dim() == 4 else img2[:, None]
        _, sums, _, _, (_, _, _, _, planes, images, h, w) = _photo_forward(a, b, 0.0, 0.0, 0.0, False, False)
        mse = sums[:, 2:3] / float(planes // images * h * w)
        return (20.0 * torch.log10(1.0 / torch.sqrt(mse))).float()
