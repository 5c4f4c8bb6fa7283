"""A float64 restatement of the distillation step's loss functions, written from their definitions (no import of gags_amd):

    get_trained_seg                         argmax over the three levels of the 5x5 mean-smoothed scale map -> that level's id
    scale_region_regulation_loss (mix_seg)  sum over segments of >= 2 pixels of n * mean_c(unbiased var_c) / (H W)
    scale_regulation_loss                   mean(-s log(s + 1e-6))
    read_sam_clip_feature (default mode)    per level: embedding rows gathered at the seg map's resolution, bilinear
                                            (align_corners=True) to the scale map's; blended by the scale map; the mask is
                                            "all three levels have an id" at the nearest source pixel
    l1_loss_map                             mean over channels of |pred - gt|
    Scale_balance_loss (mix_seg)            mean over the segments present of the segment's mean of the loss map
    normalize                               F.normalize(dim=0): x / max(|x|, 1e-12)

Index arithmetic follows what torch does for a float32 input -- the bilinear source coordinate dst * (in - 1) / (out - 1) and
the nearest one floor(dst * (in / out)) are formed in float32 -- so the taps and the mask are exact integers that a kernel
must reproduce.  The blend and every sum are float64.  The resize is written out as an explicit gather over a band of
output rows: a whole 1080p [3, 512, H, W] float64 gather would not fit anywhere.

Tied to the reference's own outputs on the CPU by tests/test_loss_ref_cpu.py (tests/golden/next_vectors.npz); the GPU tests
(tests/test_losses_float64_gpu.py) then hold the HIP kernels to it at real sizes.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24           # unit roundoff of fp32
U64 = 2.0 ** -53         # ... of float64
EPS_LOG = float(torch.tensor(1e-6, dtype=torch.float32))  # the 1e-6 of scale_regulation_loss as a float32 tensor holds it


# ------------------------------------------------------------------------------------------------------- resize taps
def bilinear_taps(n_in, n_out, device="cpu"):
    """(i0, i1, lam) per output index for upsample_bilinear2d with align_corners=True on float32 data: the scale
    (in - 1) / (out - 1) and the source coordinate scale * dst are float32 roundings; i0 = floor(src) (at most in - 1),
    i1 = i0 + 1 unless i0 is the last row, lam = src - i0 (exact in float32).  lam is returned as float64.  Formed on the
    CPU, where float32 division is correctly rounded (a GPU's need not be: 1919 / 1919 came out below 1 there), and moved
    to `device`."""
    dst = torch.arange(n_out, dtype=torch.float32)
    if n_out > 1:
        scale = torch.tensor(float(n_in - 1), dtype=torch.float32) / float(n_out - 1)
    else:
        scale = torch.zeros((), dtype=torch.float32)
    src = scale * dst
    i0 = torch.clamp(torch.floor(src).long(), max=n_in - 1)
    lam = torch.clamp(src - i0.float(), 0.0, 1.0).double()
    i1 = torch.where(i0 < n_in - 1, i0 + 1, i0)
    return i0.to(device), i1.to(device), lam.to(device)


def nearest_index(n_in, n_out, device="cpu"):
    """Source index per output index of the nearest resize (float32 input): identity for equal sizes, else
    min(floor(dst * float32(in / out)), in - 1) with the product rounded to float32 (formed on the CPU, as above)."""
    if n_in == n_out:
        return torch.arange(n_out, device=device)
    scale = torch.tensor(float(n_in), dtype=torch.float32) / float(n_out)
    dst = torch.arange(n_out, dtype=torch.float32)
    return torch.clamp(torch.floor(dst * scale).long(), max=n_in - 1).to(device)


def bilinear_resize(img, H, W):
    """[c, h, w] -> [c, H, W] float64 through bilinear_taps (the same arithmetic the GT assembly uses)."""
    c, h, w = img.shape
    y0, y1, ly = bilinear_taps(h, H, img.device)
    x0, x1, lx = bilinear_taps(w, W, img.device)
    d = img.double()
    top = d[:, y0][:, :, x0] * (1 - lx) + d[:, y0][:, :, x1] * lx
    bot = d[:, y1][:, :, x0] * (1 - lx) + d[:, y1][:, :, x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def nearest_resize(img, H, W):
    """[c, h, w] -> [c, H, W] through nearest_index."""
    ny = nearest_index(img.shape[1], H, img.device)
    nx = nearest_index(img.shape[2], W, img.device)
    return img[:, ny][:, :, nx]


# ---------------------------------------------------------------------------------------------- ground truth (SAM + CLIP)
def sam_levels(img_embed, seg_map, H, W, rows=None):
    """The three per-level features of read_sam_clip_feature for output rows `rows` (a range; all H rows by default):
    (F [3, c, R, W] float64, A [3, c, R, W] = sum over taps of weight * |embedding| (the magnitude of the terms, for error
    bounds), mask [R, W] bool).  seg_map [4, h, w] holds ids as floats; id -1 indexes the LAST embedding row, as Python
    indexing does, and still enters the blend; the mask comes only from the nearest source pixel of levels 1..3."""
    rows = range(H) if rows is None else rows
    dev = img_embed.device
    n_emb = img_embed.shape[0]
    _, h, w = seg_map.shape
    e = img_embed.double()
    y0, y1, ly = bilinear_taps(h, H, dev)
    x0, x1, lx = bilinear_taps(w, W, dev)
    r = torch.arange(rows.start, rows.stop, device=dev)
    y0, y1, ly = y0[r], y1[r], ly[r]
    wts = [((1 - ly)[:, None] * (1 - lx)[None, :]), ((1 - ly)[:, None] * lx[None, :]),
           (ly[:, None] * (1 - lx)[None, :]), (ly[:, None] * lx[None, :])]
    taps = [(y0, x0), (y0, x1), (y1, x0), (y1, x1)]
    Fs, As = [], []
    for lev in (1, 2, 3):
        ids = seg_map[lev].long()
        ids = torch.where(ids < 0, ids + n_emb, ids)
        f = a = 0.0
        for (ty, tx), wt in zip(taps, wts):
            g = e[ids[ty][:, tx]]                               # [R, W, c]
            f = f + wt[..., None] * g
            a = a + wt[..., None] * g.abs()
        Fs.append(f.permute(2, 0, 1))
        As.append(a.permute(2, 0, 1))
    ny = nearest_index(h, H, dev)[r]
    nx = nearest_index(w, W, dev)
    near = seg_map[1:4][:, ny][:, :, nx]
    mask = (near != -1).all(dim=0)
    return torch.stack(Fs), torch.stack(As), mask


def read_sam_clip_feature(img_embed, seg_map, scale_map, rows=None):
    """(feature_map [c, R, W] float64, mask [1, R, W] bool) of the default mode; differentiable in scale_map."""
    H, W = scale_map.shape[1:]
    rows = range(H) if rows is None else rows
    Fl, _, mask = sam_levels(img_embed, seg_map, H, W, rows)
    s = scale_map[:, rows.start:rows.stop].double()
    return Fl[0] * s[0] + Fl[1] * s[1] + Fl[2] * s[2], mask[None]


def l1_loss_map(pred, gt):
    return (pred.double() - gt.double()).abs().mean(dim=0)


def l1_loss(pred, gt):
    return (pred.double() - gt.double()).abs().mean()


def normalize(x, dim=0):
    """F.normalize(x, dim): x / max(||x||_2, 1e-12)."""
    x = x.double()
    return x / x.norm(dim=dim, keepdim=True).clamp_min(1e-12)


# --------------------------------------------------------------------------------------------------------- segment losses
def _ids(seg_map):
    ids = seg_map.reshape(-1).long()
    ok = seg_map.reshape(-1) != -1
    return ids, ok


def segment_moments(x, seg_map):
    """x [c, n_pix] (any float), seg_map [n_pix]: (n [S] int64, mean [S, c] float64, centred sum of squares [S, c]) over
    the ids present (S = largest id + 1; absent rows have n = 0 and mean 0)."""
    ids, ok = _ids(seg_map)
    xd = x.double().reshape(x.shape[0], -1)[:, ok].t()          # [n_ok, c]
    idx = ids[ok]
    S = int(idx.max().item()) + 1 if idx.numel() else 1
    n = torch.bincount(idx, minlength=S)
    s1 = torch.zeros(S, xd.shape[1], dtype=torch.float64, device=x.device).index_add(0, idx, xd)
    mean = s1 / n.clamp(min=1)[:, None]
    d = xd - mean[idx]
    css = torch.zeros_like(s1).index_add(0, idx, d * d)
    return n, mean, css


def scale_region_regulation_loss(scale_map, seg_map):
    """mix_seg=True: sum over segments with at least 2 pixels of n * mean_c(var_c) / (H W), var unbiased (divisor n - 1);
    segments of 0 or 1 pixels are skipped; differentiable in scale_map."""
    c, h, w = scale_map.shape
    n, _, css = segment_moments(scale_map, seg_map)
    keep = n >= 2
    nk = n[keep].double()
    var = css[keep] / (nk - 1)[:, None]
    return (nk * var.mean(dim=1)).sum() / (h * w)


def scale_regulation_loss(scale_map):
    s = scale_map.double()
    return (-s * torch.log(s + EPS_LOG)).mean()


def Scale_balance_loss(loss_map, seg_map):
    """mix_seg=True: the mean over the segments present (id != -1, at least one pixel) of the segment's mean of loss_map.
    With no segment present the reference stacks an empty list and raises; so does this."""
    ids, ok = _ids(seg_map)
    idx = ids[ok]
    if idx.numel() == 0:
        raise ValueError("Scale_balance_loss: no segment present (the reference's torch.stack of an empty list)")
    S = int(idx.max().item()) + 1
    n = torch.bincount(idx, minlength=S)
    s1 = torch.zeros(S, dtype=torch.float64, device=loss_map.device).index_add(0, idx, loss_map.double().reshape(-1)[ok])
    present = n > 0
    return (s1[present] / n[present].double()).mean()


# --------------------------------------------------------------------------------------------------------- trained seg
def smoothed_scale(scale_map):
    """The 5x5 mean smoothing (zero padding 2) of the [3, H, W] scale map, float64."""
    k = torch.full((3, 1, 5, 5), 1.0 / 25.0, dtype=torch.float64, device=scale_map.device)
    return F.conv2d(scale_map.double()[None], k, padding=2, groups=3)[0]


def get_trained_seg(seg_map, scale_map):
    """[4, H, W] ids, [3, H, W] -> [H, W]: the id of the level (1 + argmax of the smoothed scale map; first maximum wins)."""
    arg = torch.argmax(smoothed_scale(scale_map), dim=0)
    return torch.gather(seg_map[1:].double(), 0, arg[None])[0]
