"""A numpy restatement of the two functions behind render.py --feature_mode, written from their definitions (no import of
gags_amd):

    max_mode_feature       read_sam_clip_feature(max_mode=True), scene/dataset_readers.py:54-88: the arg-max level's feature
                           where that level has a segment at the nearest source pixel, mask = channel 0 != 0
    feature_visualize      feature_visualize_saving, render.py:33-48: L2-normalise, 3-component PCA on every third pixel,
                           scale by the pooled 1 % / 99 % percentiles of the sample's projections, clamp

The PCA is float64 throughout and spelled out: moments of the sample, covariance, symmetric eigendecomposition, the three
largest eigenvalues in descending order, every component signed so that its entry of largest magnitude is positive (what
sklearn >= 1.5 does for these shapes: solver covariance_eigh, svd_flip(u_based_decision=False)).  Percentiles are numpy's
default linear interpolation.

The max mode is float32, because it is compared bit for bit: the resize taps are torch's float32 index arithmetic, and the
blend of the (up to four) embedding rows is the fused chain torch's CPU upsample kernel runs on the folded weights h w for
the channels-last tensor the function hands it: round(v10 q10), then fma(v11, q11, .), fma(v01, q01, .), fma(v00, q00, .) --
of the 24 tap orders, fused or not, the only one that reproduces
the reference's bits (tests/golden/make_golden_featurevis.py records them); the selection is the reference's sum of three
products.  fma32 below is an exact float32 fused multiply-add (float64 product, TwoSum, round to odd).

Tied to the reference's own outputs by tests/test_featurevis_cpu.py (tests/golden/featurevis_vectors.npz)."""
import numpy as np

NORM_EPS = 1e-12


# ------------------------------------------------------------------------------------------------------------- max mode
def _bilinear_taps(n_in, n_out):
    """(i0, i1, lam float32) of upsample_bilinear2d, align_corners=True, on float32 data."""
    dst = np.arange(n_out, dtype=np.float32)
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = (scale * dst).astype(np.float32)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    lam = (src - i0.astype(np.float32)).astype(np.float32)
    i1 = np.where(i0 < n_in - 1, i0 + 1, i0)
    return i0, i1, lam


def _nearest_index(n_in, n_out):
    """Source index of the nearest resize: min(floor(dst * float32(in / out)), in - 1)."""
    scale = np.float32(n_in) / np.float32(n_out)
    dst = np.arange(n_out, dtype=np.float32)
    return np.minimum(np.floor((dst * scale).astype(np.float32)).astype(np.int64), n_in - 1)


def fma32(a, b, c):
    """round_float32(a * b + c) with ONE rounding, elementwise on float32 arrays: the product is exact in float64, TwoSum gives
    the sum's error, and rounding the float64 sum to odd makes the final rounding to float32 the correct one."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.copy().view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0)
    away = (err > 0) == (s > 0)
    bits = np.where(fix, np.where(away, bits + 1, bits - 1), bits)
    return bits.view(np.float64).astype(np.float32)


def level_features(img_embed, seg_map, H, W):
    """(F [3, c, H, W] float32, valid [3, H, W] bool): per level the bilinearly resized gathered embeddings (id -1 reads the
    LAST row) and the level's own validity at the nearest source pixel."""
    e = np.asarray(img_embed, np.float32)
    seg = np.asarray(seg_map)
    _, h, w = seg.shape
    y0, y1, ly = _bilinear_taps(h, H)
    x0, x1, lx = _bilinear_taps(w, W)
    ny, nx = _nearest_index(h, H), _nearest_index(w, W)
    h1, w1 = ly[:, None, None], lx[None, :, None]
    h0, w0 = (np.float32(1) - ly)[:, None, None], (np.float32(1) - lx)[None, :, None]
    q00, q01, q10, q11 = h0 * w0, h0 * w1, h1 * w0, h1 * w1     # float32 products
    Fs, valid = [], []
    for lev in (1, 2, 3):
        ids = seg[lev].astype(np.int64)          # negative ids index from the end, as in Python
        g = e[ids]                                # [h, w, c]
        v00, v01, v10, v11 = g[y0][:, x0], g[y0][:, x1], g[y1][:, x0], g[y1][:, x1]
        f = fma32(v00, q00, fma32(v01, q01, fma32(v11, q11, v10 * q10)))
        Fs.append(f.transpose(2, 0, 1))
        valid.append(seg[lev][ny][:, nx] != -1)
    return np.stack(Fs), np.stack(valid)


def max_mode_feature(img_embed, seg_map, scale_map):
    """(feature_map [c, H, W] float32, mask [1, H, W] bool) of read_sam_clip_feature(max_mode=True)."""
    sc = np.asarray(scale_map, np.float32)
    _, H, W = sc.shape
    F, valid = level_features(img_embed, seg_map, H, W)
    k = np.argmax(sc, axis=0)                     # the first of equal maxima
    one_hot = (np.arange(3)[:, None, None] == k[None]).astype(np.float32)
    m = valid.astype(np.float32)
    out = F[0] * one_hot[0] * m[0] + F[1] * one_hot[1] * m[1] + F[2] * one_hot[2] * m[2]
    return out.astype(np.float32), (out[0:1] != 0)


# ------------------------------------------------------------------------------------------------------------------ PCA
def normalized_rows(feature):
    """[C, H, W] -> x^ [H W, C] float64, x / max(||x||, 1e-12) per pixel."""
    f = np.asarray(feature, np.float64)
    X = f.reshape(f.shape[0], -1).T
    return X / np.maximum(np.sqrt((X * X).sum(axis=1, keepdims=True)), NORM_EPS)


def moments(feature):
    """(sum [C], gram [C, C], S) float64 over the pixels p % 3 == 0."""
    Xs = normalized_rows(feature)[::3]
    return Xs.sum(axis=0), Xs.T @ Xs, Xs.shape[0]


def pca_from_moments(s, g, S):
    """(mean [C], components [3, C], eigenvalues descending [C])."""
    mean = s / S
    cov = (g - S * np.outer(mean, mean)) / (S - 1)
    val, vec = np.linalg.eigh(cov)
    comps = vec[:, ::-1][:, :3].T.copy()
    for k in range(3):
        if comps[k, np.argmax(np.abs(comps[k]))] < 0:
            comps[k] = -comps[k]
    return mean, comps, val[::-1].copy()


def feature_visualize(feature, gram=None):
    """dict(vis [H, W, 3] float64, mean, components, q1, q99, eigenvalues, t [H W, 3]).  gram: use this Gram matrix of the
    sample instead of the float64 one (to measure what a float32 Gram costs)."""
    C, H, W = np.asarray(feature).shape
    X = normalized_rows(feature)
    s, g, S = moments(feature)
    mean, comps, val = pca_from_moments(s, g if gram is None else np.asarray(gram, np.float64), S)
    t = (X - mean) @ comps.T
    q1, q99 = np.percentile(t[::3], [1, 99])
    vis = np.clip((t - q1) / (q99 - q1), 0.0, 1.0).reshape(H, W, 3)
    return dict(vis=vis, mean=mean, components=comps, q1=q1, q99=q99, eigenvalues=val, t=t)


def float32_gram(feature):
    """The sample's Gram matrix formed by a float32 matrix product of float32-normalised rows."""
    f = np.asarray(feature, np.float32)
    X = f.reshape(f.shape[0], -1).T
    Xs = (X / np.maximum(np.sqrt((X * X).sum(axis=1, keepdims=True, dtype=np.float32)), np.float32(NORM_EPS)))[::3]
    return (Xs.T @ Xs).astype(np.float32)


def synthetic_feature(C, H, W, seed=0):
    """The test maps: a mixture of 6 random embeddings with smooth softmax spatial weights of decreasing amplitude, plus
    0.05 noise, times 3.7 -- [C, H, W] float32 with separated leading eigenvalues."""
    rng = np.random.default_rng(seed)
    E = rng.standard_normal((6, C))
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    logits = []
    for k in range(6):
        fy, fx = rng.uniform(0.5, 2.5, 2)
        py, px = rng.uniform(0, 2 * np.pi, 2)
        logits.append(3.0 * 0.8 ** k * (np.sin(2 * np.pi * fy * yy + py) + np.cos(2 * np.pi * fx * xx + px)))
    z = np.stack(logits)
    wgt = np.exp(z - z.max(axis=0))
    wgt /= wgt.sum(axis=0)
    f = np.einsum("khw,kc->chw", wgt, E) + 0.05 * rng.standard_normal((C, H, W))
    return (3.7 * f).astype(np.float32)
