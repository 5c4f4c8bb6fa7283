"""The image query tail restated in numpy (test infrastructure): csrc/box_mean.h, the four activation kernels and
relevancy_kernel of csrc/activate.hip, and the case tables tests/test_query_tail_cpu.py and tests/test_query_tail_gpu.py share.

  box_mean_exact    the box mean from direct float64 window sums, rounded once: exact on grid-valued maps
  activate_f32      blend, min / max, normalise, clip, threshold and majority vote, one float32 operation per kernel operation
  localize_ref      max of the box mean and every (x, y) attaining it
  relevancy_f64     eval/openclip_encoder.py:42-56 in float64
  relevancy_bound   what relevancy_kernel's float32 arithmetic may differ from it by, per pixel and phrase

`mut=` selects ONE deliberate fault (MUTATIONS / REL_MUTATIONS).  The CPU tests use them to show that the case tables
below tell a wrong kernel from a right one; nothing else passes `mut`."""
import numpy as np

F = np.float32
U = 2.0 ** -24          # unit roundoff of float32
GRID = 1024             # grid-valued maps are integers / GRID: every window sum of up to 2^20 of them is exact in double

MUTATIONS = ("anchor", "symmetric", "reflect_once", "vote_last", "ge_thresh", "ge_vote", "shared_minmax", "raw_key_order")
REL_MUTATIONS = ("drop_last_channel", "next_phrase_row", "next_pixel", "last_min")


# ---- box mean ----------------------------------------------------------------------------------------------------------
def reflect101(i, n):
    """box_mean.h's loop, literally."""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def _window_sums(p, box, axis):
    return np.lib.stride_tricks.sliding_window_view(p, box, axis=axis).sum(-1)


def box_mean_exact(x, box):
    """[h, w] or [n, h, w] -> float32.  np.pad(mode="reflect") by (box // 2, box - 1 - box // 2), every window summed directly in
    float64 (row windows, then column windows of the row sums: no running sum, no summed-area table, so no cancellation),
    divided by box * box in float64 and rounded to float32 once -- the kernel's own last two operations.  On maps that are
    multiples of 2^-10 with |x| <= 4 every sum is an integer below 2^53 / 2^10 in units of 2^-10: exact in any order."""
    x = np.asarray(x)
    if x.ndim == 3:
        return np.stack([box_mean_exact(m, box) for m in x])
    a, b = box // 2, box - 1 - box // 2
    rows = _window_sums(np.pad(x.astype(np.float64), ((0, 0), (a, b)), mode="reflect"), box, 1)
    s = _window_sums(np.pad(rows, ((a, b), (0, 0)), mode="reflect"), box, 0)
    return (s / float(box * box)).astype(F)


def border_index(n, box, anchor=None, mode="reflect"):
    """Source index of each of the n + box - 1 padded positions.  mode "reflect" is reflect101; the others are faults."""
    a = box // 2 if anchor is None else anchor
    i = np.arange(-a, n + box - 1 - a)
    if n == 1:
        return np.zeros_like(i)
    if mode == "reflect":
        i = np.mod(i, 2 * (n - 1))
        return np.where(i >= n, 2 * (n - 1) - i, i)
    if mode == "symmetric":
        i = np.mod(i, 2 * n)
        return np.where(i >= n, 2 * n - 1 - i, i)
    if mode == "reflect_once":  # one reflection, then clamped: right whenever the pad is at most n - 1
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * (n - 1) - i, i)
        return np.clip(i, 0, n - 1)
    raise ValueError(mode)


def box_mean_indexed(x, box, anchor=None, mode="reflect"):
    """box_mean_exact through border_index (the form the faults are written in)."""
    x = np.asarray(x)
    if x.ndim == 3:
        return np.stack([box_mean_indexed(m, box, anchor, mode) for m in x])
    h, w = x.shape
    rows = _window_sums(x.astype(np.float64)[:, border_index(w, box, anchor, mode)], box, 1)
    s = _window_sums(rows[border_index(h, box, anchor, mode)], box, 0)
    return (s / float(box * box)).astype(F)


# ---- activation tail -----------------------------------------------------------------------------------------------------
def smooth_variant(mask, scale, vote_last=False, ge=False):
    """oracle.activate_ref.smooth with a fault: the last row / column votes, or a tie counts as a majority."""
    h, w = mask.shape
    out = mask.copy()
    eh, ew = (h, w) if vote_last else (h - 1, w - 1)
    for i in range(h):
        for j in range(w):
            sq = mask[max(0, i - scale):min(i + scale + 1, eh), max(0, j - scale):min(j + scale + 1, ew)]
            if sq.size:
                ones = 2 * int(sq.sum())
                out[i, j] = 1 if (ones >= sq.size if ge else ones > sq.size) else 0
    return out


def _raw_key_minmax(a):
    """min / max ordered by the unsigned bit pattern (what an unsigned atomic does to floats without the sign fix-up)."""
    flat = np.ascontiguousarray(a, F).reshape(-1)
    bits = flat.view(np.uint32)
    return flat[np.argmin(bits)], flat[np.argmax(bits)]


def activate_f32(valid, thresh, box, scale, avg=None, mut=None):
    """valid [n, h, w] float32 -> dict(avg, heatmap, stats [n, 3], output, mask_pred, mask), the contract of
    gags_relevancy_activate.  Every line is one float32 operation of the kernels, in their order; the build has
    -ffp-contract=off and a correctly rounded division, so this is bit-for-bit.  `avg`: use this box mean (a run's own)."""
    from oracle.activate_ref import smooth
    assert mut is None or mut in MUTATIONS, mut
    v = np.asarray(valid, F)
    assert v.ndim == 3
    if avg is None:
        if mut in ("anchor", "symmetric", "reflect_once"):
            avg = box_mean_indexed(v, box, anchor=(box - 1) // 2 if mut == "anchor" else None,
                                   mode="reflect" if mut == "anchor" else mut)
        else:
            avg = box_mean_exact(v, box)
    avg = np.asarray(avg, F)
    heat = F(0.5) * (avg + v)
    assert heat.dtype == F
    n = v.shape[0]
    stats = np.empty((n, 3), F)
    out = np.empty_like(heat)
    for k in range(n):
        src = heat if mut == "shared_minmax" else heat[k]
        mn, mx = _raw_key_minmax(src) if mut == "raw_key_order" else (src.min(), src.max())
        stats[k] = mn, mx, avg[k].max()
        o = heat[k] - mn
        o = o / ((mx - mn) + F(1e-9))
        o = o * F(2.0) + F(-1.0)
        out[k] = np.minimum(np.maximum(o, F(0)), F(1))
    assert out.dtype == F
    mask_pred = (out >= F(thresh) if mut == "ge_thresh" else out > F(thresh)).astype(np.uint8)
    if mut in ("vote_last", "ge_vote"):
        mask = np.stack([smooth_variant(m, scale, vote_last=mut == "vote_last", ge=mut == "ge_vote") for m in mask_pred])
    else:
        mask = np.stack([smooth(m, scale) for m in mask_pred])
    return dict(avg=avg, heatmap=heat, stats=stats, output=out, mask_pred=mask_pred, mask=mask)


ACT_KEYS = ("avg", "heatmap", "stats", "output", "mask_pred", "mask")


def localize_ref(avg):
    """(score, [m, 2] int64 (x, y) in row-major order) of one [h, w] box mean (evaluate_iou_loc.py:172-176)."""
    score = avg.max()
    ys, xs = np.nonzero(avg == score)
    return score, np.stack([xs, ys], 1).astype(np.int64)


# ---- the activation cases: (h, w), box, smooth_scale, thresh, value kind, n_phrases ----------------------------------------------
# Every shape with two or three values of each option (not the product).  Widths 255 / 256 / 257 and 513 sit on both sides
# of the 256-wide row segment; (1, 1), (1, 257), (257, 1), (2, 2) and (3, 5) are narrower or shorter than most boxes (box 31
# on n = 2 and box 255 on n = 3, 5 need many reflections); boxes 2, 30, 64 are even and 1, 3, 29, 31, 255 odd.
ACT_CASES = [
    # id                  h    w   box  s  thresh  kind        n
    ("1x1_b1",            1,   1,    1,  0,  0.5, "unit",      1),
    ("1x1_b30",           1,   1,   30,  3,  0.0, "straddle",  3),
    ("1x1_b64",           1,   1,   64, 40, -0.5, "negative",  7),
    ("1x257_b2",          1, 257,    2,  1,  0.5, "straddle",  3),
    ("1x257_b31",         1, 257,   31,  3,  1.0, "unit",      1),
    ("1x257_b64",         1, 257,   64,  0,  0.0, "plateau",   1),
    ("257x1_b3",        257,   1,    3,  3,  0.5, "unit",      1),
    ("257x1_b30",       257,   1,   30,  1,  0.0, "negative",  3),
    ("257x1_b29",       257,   1,   29,  0, -0.5, "constant",  1),
    ("2x2_b1",            2,   2,    1,  0,  0.5, "unit",      7),
    ("2x2_b2",            2,   2,    2,  1,  0.0, "straddle",  1),
    ("2x2_b31",           2,   2,   31,  3,  1.0, "unit",      3),
    ("3x5_b3",            3,   5,    3,  1,  0.5, "straddle",  3),
    ("3x5_b255",          3,   5,  255,  3,  0.5, "unit",      1),
    ("3x5_b30",           3,   5,   30,  0,  0.0, "plateau",   7),
    ("16x255_b29",       16, 255,   29,  3,  0.5, "unit",      3),
    ("16x255_b64",       16, 255,   64,  1, -0.5, "straddle",  1),
    ("16x256_b30",       16, 256,   30,  3,  0.5, "straddle",  1),
    ("16x256_b2",        16, 256,    2, 40,  0.0, "unit",      3),
    ("16x257_b31",       16, 257,   31,  3,  0.5, "negative",  7),
    ("16x257_b30",       16, 257,   30,  0,  1.0, "unit",      1),
    ("16x257_b1",        16, 257,    1,  1,  0.5, "straddle",  3),
    ("33x513_b64",       33, 513,   64,  3,  0.5, "unit",      3),
    ("33x513_b29",       33, 513,   29, 40,  0.5, "straddle",  1),
    ("33x513_b30",       33, 513,   30,  1,  0.0, "constant",  3),
    ("70x94_b30",        70,  94,   30,  3,  0.5, "unit",      3),
    ("70x94_b31",        70,  94,   31, 40,  1.0, "plateau",   1),
    ("70x94_b3",         70,  94,    3,  0, -0.5, "negative",  7),
    ("5x300_b1024",       5, 300, 1024,  3,  0.5, "unit",      1),
]
ACT_IDS = [c[0] for c in ACT_CASES]


def act_case(case_id):
    return ACT_CASES[ACT_IDS.index(case_id)]


def smooth_blobs(n, h, w, rng):
    """Smooth integer-valued [n, h, w] in 0 .. GRID: a few separable cosine bumps, so that thresholded regions survive a vote."""
    y = np.arange(h)[None, :, None] / max(h - 1, 1)
    x = np.arange(w)[None, None, :] / max(w - 1, 1)
    f = rng.uniform(0.5, 3.0, (4, n, 1, 1))
    ph = rng.uniform(0, 2 * np.pi, (4, n, 1, 1))
    m = 0.5 + 0.25 * np.cos(2 * np.pi * f[0] * y + ph[0]) * np.cos(2 * np.pi * f[1] * x + ph[1]) \
        + 0.25 * np.cos(2 * np.pi * f[2] * y + ph[2]) * np.cos(2 * np.pi * f[3] * x + ph[3])
    return np.rint(m * GRID).astype(np.int64)


def grid_maps(case_id):
    """The [n, h, w] float32 maps of a case: multiples of 2^-10 with |x| <= 4.  Phrase k is scaled by 1 + k % 3 and shifted by its
    own offset, so that no two neighbouring phrases share a minimum or a maximum.
      unit      [0, 1] (phrase 0): smooth bumps plus noise
      straddle  minimum below zero, maximum above
      negative  every value below zero
      constant  one value per phrase (max == min)
      plateau   [0, 0.5] noise under a rectangle of the maximum value that touches the top-left border"""
    _, h, w, _, _, _, kind, n = act_case(case_id)
    rng = np.random.default_rng(ACT_IDS.index(case_id) + 1000)
    noise = rng.integers(-128, 129, (n, h, w))
    base = np.clip(smooth_blobs(n, h, w, rng) + noise, 0, GRID)                   # 0 .. 1024
    mul = (1 + np.arange(n) % 3)[:, None, None]
    off = ((np.arange(n) * 97) % 513 - 256)[:, None, None] * (np.arange(n) > 0)[:, None, None]
    if kind == "unit":
        q = base * mul + off
    elif kind == "straddle":
        q = (2 * base - GRID) * mul + off // 2                                     # about [-1, 1] * mul
    elif kind == "negative":
        q = -(base + 256) * mul - np.abs(off)
    elif kind == "constant":
        q = np.broadcast_to(off + 37 * mul - 100, (n, h, w)).copy()
    elif kind == "plateau":
        q = (base // 2) * mul + off
        top = q.reshape(n, -1).max(1)[:, None, None] + 64
        q[:, :max(1, (2 * h) // 3), :max(1, (2 * w) // 3)] = np.broadcast_to(top, (n, max(1, (2 * h) // 3), max(1, (2 * w) // 3)))
    else:
        raise ValueError(kind)
    assert np.abs(q).max() <= 4 * GRID
    return (q.astype(np.float64) / GRID).astype(F)


# ---- relevancy -----------------------------------------------------------------------------------------------------------
def relevancy_f64(embed, pos, neg, mut=None):
    """[n_pix, c], [n_pos, c], [n_neg, c] -> [n_pos, n_pix, 2] float64: for positive j and every negative k the pair softmax of
    10 * (sim_pos_j, sim_neg_k); the pair with the FIRST minimal positive probability (torch.argmin) is returned."""
    assert mut is None or mut in REL_MUTATIONS, mut
    e, p, n = (np.asarray(a, np.float64) for a in (embed, pos, neg))
    if mut == "drop_last_channel":
        e, p, n = e[:, :-1], p[:, :-1], n[:, :-1]
    if mut == "next_pixel":
        e = np.roll(e, -1, 0)
    table = np.concatenate([p, n])
    if mut == "next_phrase_row":
        p = table[1:p.shape[0] + 1]
    a = 10.0 * (e @ p.T).T[:, :, None]          # [n_pos, n_pix, 1]
    b = 10.0 * (e @ n.T)[None, :, :]            # [1, n_pix, n_neg]
    m = np.maximum(a, b)
    ea, eb = np.exp(a - m), np.exp(b - m)
    p0, p1 = ea / (ea + eb), eb / (ea + eb)
    if mut == "last_min":
        k = p0.shape[2] - 1 - np.argmin(p0[:, :, ::-1], 2)
    else:
        k = np.argmin(p0, 2)
    k = k[:, :, None]
    return np.stack([np.take_along_axis(p0, k, 2)[..., 0], np.take_along_axis(p1, k, 2)[..., 0]], -1)


EXPF_ULP = 1  # the documented bound of HIP's expf (HIP math API, single precision: 1 ulp)


def relevancy_bound(embed, pos, neg):
    """[n_pos, n_pix, 2]: how far relevancy_kernel's float32 result may lie from relevancy_f64, with u = 2^-24.

    sim    A lane sums its ceil(c / 64) products in an fma chain (one rounding per term) and its partial sum then passes
           through the 6 adds of the shuffle tree: every product carries at most ceil(c / 64) + 6 roundings, so
               |d sim| <= gamma(ceil(c / 64) + 6) * sum_i |e_i| |p_i|,      gamma(n) = n u / (1 - n u).
    logit  a = fl(10 sim'):  |da| <= 10 |d sim| (1 + u) + u |10 sim|;  the same for the negative's b.
    x      After the subtraction of the larger logit one exponent is exactly 0 and the other is x = fl(a' - b') (or its
           negative):  |dx| <= (|da| + |db|) (1 + u) + u |a - b|.
    p      p0 = sigmoid(x) and p1 = sigmoid(-x), Lipschitz 1 / 4:  |dp| <= dx / 4 (= 2.5 (|d sim_pos| + |d sim_neg|) plus the
           two logit roundings).  exp(0) = 1 is exact; the other expf is within EXPF_ULP ulp = 2 EXPF_ULP u relative, the add
           and the correctly rounded division one u each: (2 EXPF_ULP + 2) u relative to p, to first order gamma(2 EXPF_ULP +
           2) p; an expf result below the normal range may be flushed: 2^-126 absolute.
    min    b_k is that bound for the pair with negative k.  |min_k p0'_k - min_k p0_k| <= max_k b_k =: B, which bounds
           [..., 0].  If rounding moves the arg-min from k* to k', p1 is taken from pair k': |p1'_k' - p1_k*| <= b_k' +
           |p0_k' - p0_k*| <= b_k' + (b_k' + b_k*), so [..., 1] is bounded by 3 B.
    Nothing here is fitted to a measurement."""
    e, p, n = (np.asarray(a, np.float64) for a in (embed, pos, neg))
    c = e.shape[1]
    terms = -(-c // 64) + 6
    g = terms * U / (1 - terms * U)
    ds_p = g * (np.abs(e) @ np.abs(p).T).T[:, :, None]
    ds_n = g * (np.abs(e) @ np.abs(n).T)[None, :, :]
    a = 10.0 * (e @ p.T).T[:, :, None]
    b = 10.0 * (e @ n.T)[None, :, :]
    da = 10.0 * ds_p * (1 + U) + U * np.abs(a)
    db = 10.0 * ds_n * (1 + U) + U * np.abs(b)
    dx = (da + db) * (1 + U) + U * np.abs(a - b)
    r = 2 * EXPF_ULP + 2
    rel = r * U / (1 - r * U)
    bk = 0.25 * dx + rel + 2.0 ** -126          # (p <= 1)
    big = bk.max(2)
    return np.stack([big, 3.0 * big], -1)


# (c, n_pix, n_pos, n_neg, kind).  c on both sides of the 64 lanes and at the 16-register limit; n_pix on both sides of the 4
# waves of a workgroup; the phrase-count limit 32 both ways; (10, 4) at c = 1024 is 57344 bytes of phrases, the most
# that passes the 60000-byte check.
#   unit   unit-norm embeddings and phrases
#   big    embeddings along pos[0] - neg[0] on a ramp that takes 10 sim to +-200: probabilities of exactly 0 and 1, no NaN
#   dup    unit, negative 1 is a copy of negative 0
#   zero   unit phrases, every embedding all zero: exactly (0.5, 0.5)
REL_CASES = [
    (1, 1, 1, 1, "unit"),
    (1, 5, 3, 4, "unit"),
    (16, 3, 3, 4, "unit"),
    (63, 4, 1, 1, "unit"),
    (64, 257, 28, 4, "unit"),
    (64, 5, 1, 31, "unit"),
    (64, 257, 3, 4, "big"),
    (65, 5, 3, 4, "unit"),
    (65, 257, 3, 4, "big"),
    (512, 257, 3, 4, "unit"),
    (512, 4, 3, 4, "dup"),
    (512, 3, 3, 4, "zero"),
    (1000, 5, 3, 4, "unit"),
    (1000, 257, 1, 1, "big"),
    (1024, 257, 10, 4, "unit"),
    (1024, 1, 3, 4, "dup"),
]


def rel_id(case):
    return "c{}_pix{}_{}x{}_{}".format(*case)


def rel_inputs(case):
    c, n_pix, n_pos, n_neg, kind = case
    rng = np.random.default_rng(REL_CASES.index(case) + 2000)

    def unit(m):
        v = rng.standard_normal((m, c))
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    pos, neg, e = unit(n_pos), unit(n_neg), unit(n_pix)
    if c == 1:
        neg[0] = -pos[0]  # (of two signs, so that not every pair is a tie)
    if kind == "dup":
        neg[1] = neg[0]
    elif kind == "zero":
        e[:] = 0.0
    elif kind == "big":
        d = pos[0] - neg[0]
        d /= np.linalg.norm(d)
        d = d[None] + 0.05 * e
        top = np.abs(d @ np.concatenate([pos, neg]).T).max(1, keepdims=True)    # pixel i: max |sim| = |ramp_i|
        e = d * (np.linspace(-20.0, 20.0, n_pix)[:, None] / top)
    return e.astype(F), pos.astype(F), neg.astype(F)
