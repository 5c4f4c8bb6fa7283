"""The contract of include/gags_next.h N12 restated in float32 numpy (test infrastructure): every step is one float32 operation,
in the order the header lists them."""
import numpy as np

F = np.float32
THRESH_EDGE, LUT_EDGE = 1e-5, 2e-3


def clip01(v):
    """torch.clip(v, 0, 1) in float32 (a NaN stays a NaN)."""
    v = np.asarray(v, F)
    return np.where(v < 0, F(0), np.where(v > 1, F(1), v)).astype(F)


def lut_index(t):
    """idx(t) = (int)(t * 255.0f), a NaN taken as 0, clamped to 0..255."""
    t = np.asarray(t, F)
    t = np.where(np.isnan(t), F(0), t).astype(F)
    s = (t * F(255)).astype(F)
    return np.clip(s, 0, 255).astype(np.int64)


def lerf_q(heat, max_heat):
    """(p, pmax, q) of the lerf composite: heat [M, h, w], max_heat [M] (stats[:, 1])."""
    p = clip01(np.asarray(heat, F) - F(0.5))
    pmax = clip01(np.asarray(max_heat, F) - F(0.5))
    q = clip01((p / (pmax[:, None, None] + F(1e-6)).astype(F)).astype(F))
    return p, pmax, q


def mask_b(output, avg2):
    return clip01((F(0.5) * np.asarray(output, F)).astype(F) + (F(0.5) * np.asarray(avg2, F)).astype(F))


def frame_of(n_maps, n_frames):
    return np.arange(n_maps) // (n_maps // n_frames)


def query_images(heat, output, mask, avg2, max_heat, image, lut):
    """The three [M, h, w, 3] float32 images.  image [F, h, w, 3]; map m uses image m // (M // F)."""
    heat, output, avg2, image, lut = (np.asarray(a, F) for a in (heat, output, avg2, image, lut))
    img = image[frame_of(heat.shape[0], image.shape[0])]                     # [M, h, w, 3]
    heatmap = lut[lut_index(output)]
    _, _, q = lerf_q(heat, max_heat)
    lerf = np.where((heat < F(0.5))[..., None], (img * F(0.3)).astype(F), lut[lut_index(q)])
    b = mask_b(output, avg2)
    outside = ((img * F(0.4)).astype(F) + F(0.1)).astype(F)
    maskc = np.where(np.asarray(mask).astype(bool)[..., None], lut[lut_index(b)], outside)
    return heatmap.astype(F), lerf.astype(F), maskc.astype(F)


def to_uint8(x):
    """This project's 8-bit rule in float32: trunc(clamp(x * 255 + 0.5, 0, 255))."""
    v = ((np.asarray(x, F) * F(255)).astype(F) + F(0.5)).astype(F)
    return np.clip(v, 0, 255).astype(np.uint8)


def edge_sets(heat, output, avg2, max_heat, thresh):
    """The pixels where a result of the end-to-end path may legitimately differ from the golden one (its box means are within
    1e-6 of the exact ones, not bit-equal).  Returns a dict of [M, h, w] bool arrays:
      lut_output / lut_q / lut_b: the LUT argument times 255 lies within 2e-3 of an integer >= 1 (0 is no bin edge: the arguments
                                  are clipped to [0, 1] and all of [0, 1 / 255) has index 0);
      heat: |heat - 0.5| < 1e-5;  thresh: |output - thresh| < 1e-5;  B: the union."""
    def near_int(t):
        s = np.asarray(t, np.float64) * 255.0
        return (np.abs(s - np.rint(s)) < LUT_EDGE) & (np.rint(s) >= 1)
    _, _, q = lerf_q(heat, max_heat)
    e = {"lut_output": near_int(output), "lut_q": near_int(q), "lut_b": near_int(mask_b(output, avg2)),
         "heat": np.abs(np.asarray(heat, np.float64) - 0.5) < THRESH_EDGE,
         "thresh": np.abs(np.asarray(output, np.float64) - float(thresh)) < THRESH_EDGE}
    e["B"] = e["lut_output"] | e["lut_q"] | e["lut_b"] | e["heat"] | e["thresh"]
    return e


def feature_loss_maps(feature, gt, mask):
    """(l2, mean_abs_pred, mean_abs_gt) [H, W] float32 of [C, H, W] maps: a = fl(gt m), b = fl(f m), d = fl(a - b), the sums of
    fl(d d), |b|, |a| in float64, rounded once (numpy's float64 sum order stands in for the kernel's; the difference is far below
    the final float32 rounding)."""
    m = np.asarray(mask).reshape(1, *np.asarray(feature).shape[1:]).astype(F)
    a, b = (np.asarray(gt, F) * m).astype(F), (np.asarray(feature, F) * m).astype(F)
    d = (a - b).astype(F)
    c = a.shape[0]
    l2 = np.sqrt((d * d).astype(F).astype(np.float64).sum(0).astype(F)).astype(F)
    return l2, (np.abs(b).astype(np.float64).sum(0) / c).astype(F), (np.abs(a).astype(np.float64).sum(0) / c).astype(F)
