"""The image query tail without a GPU: the numpy restatement (tests/query_tail_ref.py) against what the suite already pins, the
proof that the case tables of tests/test_query_tail_gpu.py tell a wrong kernel from a right one, and the argument checks
of the three C entries."""
import ctypes
import os

import numpy as np
import pytest

import query_tail_ref as Q

HERE = os.path.dirname(os.path.abspath(__file__))
ZA = np.load(os.path.join(HERE, "golden", "activate_vectors.npz"))
ZN = np.load(os.path.join(HERE, "golden", "next_vectors.npz"))
F = np.float32


# ---- the restatement against what is already pinned ----------------------------------------------------------------------------
def test_np_pad_reflect_is_the_kernels_reflect101():
    """Also beyond one reflection (pad > n - 1) and for n == 1, where the kernel has a branch of its own."""
    for n in (1, 2, 3, 5, 29, 31):
        for box in (1, 2, 7, 30, 31, 64):
            a = box // 2
            want = [Q.reflect101(i, n) for i in range(-a, n + box - 1 - a)]
            assert list(np.pad(np.arange(n), (a, box - 1 - a), mode="reflect")) == want, (n, box)
            assert list(Q.border_index(n, box)) == want, (n, box)


@pytest.mark.parametrize("case_id", ["2x2_b31", "3x5_b255", "16x257_b30", "1x257_b2"])
def test_both_forms_of_the_box_mean_agree(case_id):
    v = Q.grid_maps(case_id)
    box = Q.act_case(case_id)[3]
    want = Q.box_mean_exact(v, box)
    np.testing.assert_array_equal(Q.box_mean_indexed(v, box), want)
    # the literal definition: every window of the padded map summed on its own
    a, b = box // 2, box - 1 - box // 2
    p = np.pad(v[0].astype(np.float64), ((a, b), (a, b)), mode="reflect")
    h, w = v.shape[1:]
    lit = np.array([[p[y:y + box, x:x + box].sum() for x in range(w)] for y in range(h)]) / float(box * box)
    np.testing.assert_array_equal(lit.astype(F), want[0])


def test_restatement_on_the_reference_functions_outputs():
    """activate_vectors.npz holds what the reference's own activate_stream, smooth and lerf_localization returned (its box mean
    is cv2's float32 one: the heat map agrees to 1e-6, not bit for bit)."""
    valid, th = ZA["act_valid_map"], float(ZA["act_thresh"])
    r = Q.activate_f32(valid, th, 30, 3)
    assert np.abs(r["heatmap"] - ZA["act_heatmap"]).max() <= 1e-6
    np.testing.assert_array_equal(r["mask"], ZA["act_mask"])
    for k in range(valid.shape[0]):
        score, coords = Q.localize_ref(r["avg"][k])
        assert score == r["stats"][k, 2]
        np.testing.assert_array_equal(coords, ZA[f"act_loc_coords{k}"])
    one = Q.activate_f32(ZA["act_smooth_in"][None].astype(F), 0.5, 1, 3)
    np.testing.assert_array_equal(one["mask_pred"][0], ZA["act_smooth_in"])
    np.testing.assert_array_equal(one["mask"][0], ZA["act_smooth_out"])


def test_relevancy_f64_on_the_reference_outputs():
    got = Q.relevancy_f64(ZN["rel_embed"], ZN["rel_pos"], ZN["rel_neg"])
    for j in range(3):
        np.testing.assert_allclose(got[j], ZN[f"rel_probs{j}"], rtol=2e-5, atol=1e-7)
    sem = ZN["rel_sem_map"]
    n_levels, h, w, c = sem.shape
    across = Q.relevancy_f64(sem.reshape(-1, c), ZN["rel_pos"], ZN["rel_neg"])[..., 0].reshape(3, n_levels, h, w).transpose(1, 0, 2, 3)
    np.testing.assert_allclose(across, ZN["rel_max_across"], rtol=2e-5, atol=1e-7)


@pytest.mark.parametrize("h,w,box,seed", [(37, 41, 30, 0), (20, 300, 7, 1)])
def test_restatement_against_the_oracle_on_random_maps(h, w, box, seed):
    """On grid-valued maps the oracle's summed-area box mean is exact as well, so the two agree bit for bit."""
    from oracle import activate_ref as A
    v = (np.random.default_rng(seed).integers(0, Q.GRID + 1, (1, h, w)) / Q.GRID).astype(F)
    r, o = Q.activate_f32(v, 0.5, box, 3), A.activate(v[0], thresh=0.5, box=box, scale=3)
    for key in ("avg", "heatmap", "output", "mask_pred", "mask"):
        np.testing.assert_array_equal(r[key][0], o[key], err_msg=key)


# ---- the activation cases tell a wrong kernel from a right one ---------------------------------------------------------------
def test_the_case_table_covers_what_it_claims():
    hw = {(c[1], c[2]) for c in Q.ACT_CASES}
    assert hw >= {(1, 1), (1, 257), (257, 1), (2, 2), (3, 5), (16, 255), (16, 256), (16, 257), (33, 513), (70, 94), (5, 300)}
    assert {c[3] for c in Q.ACT_CASES} == {1, 2, 3, 29, 30, 31, 64, 255, 1024}
    assert {c[4] for c in Q.ACT_CASES} == {0, 1, 3, 40} and {c[5] for c in Q.ACT_CASES} == {0.5, 0.0, 1.0, -0.5}
    assert {c[6] for c in Q.ACT_CASES} == {"unit", "straddle", "negative", "constant", "plateau"}
    assert {c[7] for c in Q.ACT_CASES} == {1, 3, 7}
    for shape in hw - {(5, 300)}:
        mine = [c for c in Q.ACT_CASES if (c[1], c[2]) == shape]
        assert 2 <= len(mine) <= 3
    for cid in Q.ACT_IDS:
        v, kind = Q.grid_maps(cid), Q.act_case(cid)[6]
        q = v.astype(np.float64) * Q.GRID
        assert np.array_equal(q, np.rint(q)) and np.abs(v).max() <= 4, cid
        if v[0].size > 1:
            lo, hi = v.reshape(v.shape[0], -1).min(1), v.reshape(v.shape[0], -1).max(1)
            if kind == "straddle":
                assert (lo < 0).all() and (hi > 0).all(), cid
            if kind == "negative":
                assert (hi < 0).all(), cid
            if kind == "constant":
                assert (lo == hi).all(), cid
            if kind == "unit":
                assert lo[0] >= 0 and hi[0] <= 1, cid
            if v.shape[0] > 1:  # a phrase's range is not its neighbour's
                assert (np.diff(lo) != 0).all() and (np.diff(hi) != 0).all(), cid


# mutation -> the case that catches it (others do too; one is named so that a change of the table cannot lose it unnoticed)
CAUGHT_BY = {
    "anchor": "16x256_b30",          # an even box: box // 2 = 15, (box - 1) // 2 = 14
    "symmetric": "16x255_b29",
    "reflect_once": "3x5_b255",      # 127 pixels of border on maps 3 and 5 wide
    "vote_last": "70x94_b30",
    "ge_thresh": "16x257_b30",       # thresh 1.0: the maximum normalises to exactly 1
    "ge_vote": "16x256_b30",         # border windows of 4 x 7 pixels have an even count: ties exist
    "shared_minmax": "33x513_b64",   # three phrases with three ranges
    "raw_key_order": "16x256_b30",   # min < 0 < max
}


@pytest.mark.parametrize("mut", Q.MUTATIONS)
def test_every_fault_changes_an_output_of_its_case(mut):
    _, _, _, box, scale, thresh, _, _ = Q.act_case(CAUGHT_BY[mut])
    v = Q.grid_maps(CAUGHT_BY[mut])
    good, bad = Q.activate_f32(v, thresh, box, scale), Q.activate_f32(v, thresh, box, scale, mut=mut)
    differ = [k for k in Q.ACT_KEYS if not np.array_equal(good[k], bad[k])]
    print(f"{mut} on {CAUGHT_BY[mut]}: changes {differ}")
    assert differ
    expect = {"anchor": "avg", "symmetric": "avg", "reflect_once": "avg", "vote_last": "mask", "ge_thresh": "mask_pred",
              "ge_vote": "mask", "shared_minmax": "stats", "raw_key_order": "stats"}[mut]
    assert expect in differ


def test_a_constant_map_normalises_to_zero():
    for cid in ("257x1_b29", "33x513_b30", "1x1_b1"):
        _, _, _, box, scale, thresh, _, _ = Q.act_case(cid)
        r = Q.activate_f32(Q.grid_maps(cid), thresh, box, scale)
        assert not r["output"].any() and np.array_equal(r["stats"][:, 0], r["stats"][:, 1]), cid
        assert (r["mask_pred"] == (0 > thresh)).all(), cid


# ---- the relevancy bound is discriminating ----------------------------------------------------------------------------------------
def _applies(mut, case):
    c, n_pix, n_pos, n_neg, kind = case
    if kind == "zero":
        return False           # every sim is 0 whatever is read
    if mut == "next_pixel":
        return n_pix > 1
    if mut == "next_phrase_row" and c == 1:
        return False           # a phrase is +-1: the neighbouring row may be the same number
    return True


MISREADS = [(m, c) for m in ("drop_last_channel", "next_phrase_row", "next_pixel") for c in Q.REL_CASES if _applies(m, c)]


@pytest.mark.parametrize("mut,case", MISREADS, ids=[f"{m}-{Q.rel_id(c)}" for m, c in MISREADS])
def test_a_misread_operand_lies_outside_the_relevancy_bound(mut, case):
    """A kernel that drops the ragged last channel, reads the next phrase's row or the next pixel's embedding is further from
    float64 than float32 arithmetic can be: the bound would catch it on every case the fault can touch."""
    e, p, n = Q.rel_inputs(case)
    want, bad, bound = Q.relevancy_f64(e, p, n), Q.relevancy_f64(e, p, n, mut=mut), Q.relevancy_bound(e, p, n)
    ratio = (np.abs(bad - want)[..., 0] / bound[..., 0]).max()
    print(f"{mut} on {Q.rel_id(case)}: worst err / bound {ratio:.3g}")
    assert ratio > 1


def test_the_tie_rule_cannot_show_in_the_probabilities():
    """First against last minimum over the negatives.  p0 = sigmoid(a - b_k) is strictly monotone in b_k, so two pairs tie in
    p0 only if b_k ties too (the duplicated negative: both pairs hold the same two numbers) or if both p0 have saturated to
    exactly 1, where the p1 differ by less than 2^-53.  Either way the rule leaves the returned pair unchanged to within
    2^-53, far inside any rounding bound: no case can put a last-minimum kernel outside relevancy_bound, and none is claimed
    to.  What the cases do pin is that a tie is handled at all: the duplicated negative and the saturated pixels must return
    one of the tied pairs, not a mixture or a NaN."""
    for case in Q.REL_CASES:
        e, p, n = Q.rel_inputs(case)
        want, other = Q.relevancy_f64(e, p, n), Q.relevancy_f64(e, p, n, mut="last_min")
        assert np.abs(other - want).max() <= 2.0 ** -53, case
        assert not np.isnan(want).any()
        np.testing.assert_allclose(want.sum(-1), 1.0, rtol=0, atol=2.0 ** -51)  # (three roundings of numbers <= 1)


def test_the_relevancy_cases_cover_what_they_claim():
    assert {c[0] for c in Q.REL_CASES} == {1, 16, 63, 64, 65, 512, 1000, 1024}
    assert {c[1] for c in Q.REL_CASES} == {1, 3, 4, 5, 257}
    assert {(c[2], c[3]) for c in Q.REL_CASES} == {(1, 1), (3, 4), (28, 4), (1, 31), (10, 4)}
    for case in Q.REL_CASES:
        c, n_pix, n_pos, n_neg, kind = case
        assert (n_pos + n_neg) * c * 4 <= 60000 and n_pos + n_neg <= 32
        e, p, n = Q.rel_inputs(case)
        want = Q.relevancy_f64(e, p, n)
        if kind == "big":
            logits = 10.0 * e.astype(np.float64) @ np.concatenate([p, n]).astype(np.float64).T
            assert 199 <= np.abs(logits).max() <= 201
            assert (want[..., 0] == 1.0).any() and (want[..., 0] < 1e-80).any()
        if kind == "zero":
            assert (want == 0.5).all() and not Q.relevancy_bound(e, p, n)[..., 0].max() > 5 * Q.U
        if kind == "dup":
            assert np.array_equal(n[0], n[1])
    assert max((c[2] + c[3]) * c[0] * 4 for c in Q.REL_CASES) == 57344  # one more phrase of 1024 would be 61440 > 60000


# ---- C ABI refusals: every one returns before a launch ---------------------------------------------------------------------------
EINVAL, ESCRATCH = -1, -3


@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def P():
    buf = ctypes.create_string_buffer(256)
    return ctypes.cast(buf, ctypes.c_void_p)


def test_relevancy_refusals(lib, P):
    def rel(n_pix=8, c=64, n_pos=3, n_neg=4, embed=P, pos=P, neg=P, probs=P):
        return lib.gags_relevancy(n_pix, c, n_pos, n_neg, embed, pos, neg, probs, None)
    assert rel(c=16, n_pos=29, n_neg=4) == EINVAL and rel(c=16, n_pos=1, n_neg=32) == EINVAL     # 33 phrases
    assert rel(c=1025, n_pos=1, n_neg=1) == EINVAL
    assert rel(c=1024, n_pos=11, n_neg=4) == EINVAL                                                 # 61440 bytes of phrases
    assert rel(c=1000, n_pos=12, n_neg=4) == EINVAL                                                 # 64000
    assert rel(n_pos=0) == EINVAL and rel(n_neg=0) == EINVAL
    assert rel(c=0) == EINVAL and rel(n_pix=-1) == EINVAL
    assert rel(pos=None) == EINVAL and rel(neg=None) == EINVAL and rel(embed=None) == EINVAL and rel(probs=None) == EINVAL
    assert rel(n_pix=0) == 0 and rel(n_pix=0, embed=None, probs=None) == 0                          # no pixels: a no-op
    assert rel(n_pix=0, c=1024, n_pos=10, n_neg=4) == 0 and rel(n_pix=0, c=16, n_pos=28, n_neg=4) == 0  # the accepted maxima


def test_relevancy_activate_refusals(lib, P):
    nb = lib.gags_relevancy_activate_scratch_bytes(3, 8, 9)
    assert nb >= 3 * 8 * 9 * 8 + 3 * 3 * 4
    assert lib.gags_relevancy_activate_scratch_bytes(0, 8, 9) == 0 and lib.gags_relevancy_activate_scratch_bytes(3, 0, 9) == 0

    def act(n=3, h=8, w=9, thresh=0.5, box=30, scale=3, scratch_bytes=nb - 1, **null):
        a = dict(valid=P, avg=P, heat=P, output=P, mask_pred=P, mask=P, stats=P, scratch=P)
        a.update(null)
        return lib.gags_relevancy_activate(n, h, w, a["valid"], thresh, box, scale, a["avg"], a["heat"], a["output"],
                                           a["mask_pred"], a["mask"], a["stats"], a["scratch"], scratch_bytes, None)
    assert act() == ESCRATCH                                   # valid arguments, scratch one byte short: nothing is launched
    assert act(box=1) == ESCRATCH and act(box=1024) == ESCRATCH and act(scale=0) == ESCRATCH
    assert act(box=0) == EINVAL and act(box=1025) == EINVAL and act(box=-1) == EINVAL
    assert act(scale=-1) == EINVAL
    assert act(h=65536) == EINVAL and act(n=65536) == EINVAL and act(n=0) == EINVAL and act(h=0) == EINVAL and act(w=0) == EINVAL
    for name in ("valid", "avg", "heat", "output", "mask_pred", "mask", "stats", "scratch"):
        assert act(**{name: None}) == EINVAL, name
    assert act(h=65535, w=1, n=1, scratch_bytes=0) == ESCRATCH  # the accepted maximum


def test_query_images_refusals(lib, P):
    nb = lib.gags_query_images_scratch_bytes(6, 8, 9)
    assert nb >= 6 * 8 * 9 * 8

    def images(m=6, f=2, h=8, w=9, box=30, scratch_bytes=nb - 1, u=(None, None, None)):
        return lib.gags_query_images(m, f, h, w, P, P, P, P, P, P, box, P, P, P, P, u[0], u[1], u[2], P, scratch_bytes, None)
    assert images() == ESCRATCH and images(u=(P, P, P)) == ESCRATCH
    assert images(f=4) == EINVAL and images(f=5) == EINVAL
    for u in ((P, None, None), (None, P, None), (None, None, P), (P, P, None), (P, None, P), (None, P, P)):
        assert images(u=u) == EINVAL, u

    def colour(m=6, f=2, u=(None, None, None)):
        return lib.gags_query_colour(m, f, 8, 9, P, P, P, P, P, P, P, P, P, P, u[0], u[1], u[2], None)
    assert colour(f=4) == EINVAL
    for u in ((P, None, None), (None, P, None), (None, None, P)):
        assert colour(u=u) == EINVAL, u
