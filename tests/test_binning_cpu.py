"""The references of the binning tests, proven without a GPU: every restatement of tests/binning_ref.py against the CPU
twins of oracle/libgags_oracle.so (bound with the ctypes signatures of the GPU entries) and against oracle.tile_bin; the
comparison helpers against minimal perturbations of a correct result (each must raise); and the two documented call chains
composed from the restatements against each other.  Exact equality throughout."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import binning_ref as R  # noqa: E402


def P(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def cpu(oracle):
    from gags_amd import _lib
    lib = ctypes.CDLL(os.path.join(HERE, "..", "oracle", "libgags_oracle.so"))
    fn = {}
    for name in ("gags_cumsum_i32", "gags_tile_emit", "gags_sort_pairs", "gags_tile_offsets"):
        f = getattr(lib, name.replace("gags_", "gags_cpu_"))
        f.restype, f.argtypes = _lib.SIGNATURES[name]
        fn[name] = f
    return fn


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2049, 100_003])
def test_cumsum_matches_the_cpu_twin(cpu, n):
    a = R.counts(n, seed=n)
    cum, total = np.zeros(n, np.int32), np.zeros(1, np.int32)
    assert cpu["gags_cumsum_i32"](n, P(a), P(cum), P(total), None, 0, None) == 0
    want, wt = R.cumsum(a)
    R.assert_same(cum, want, "cum")
    R.assert_total_equal(total[0], wt)
    perm = np.random.default_rng(n).permutation(n).astype(np.int32)
    g = np.ascontiguousarray(a[perm])
    assert cpu["gags_cumsum_i32"](n, P(g), P(cum), P(total), None, 0, None) == 0
    want, wt = R.cumsum(a, perm)
    R.assert_same(cum, want, "cum over idx")
    R.assert_total_equal(total[0], wt)


def test_cumsum_overflow_and_the_largest_sum_that_fits(cpu):
    for a, want_total in ((np.full(300_000, 8160, np.int32), -1),
                          (R.counts_exact_sum(1_048_594, R.INT32_MAX), R.INT32_MAX),
                          (R.counts_exact_sum(1_048_594, R.INT32_MAX + 1), -1)):
        cum, total = np.zeros(a.size, np.int32), np.zeros(1, np.int32)
        assert cpu["gags_cumsum_i32"](a.size, P(a), P(cum), P(total), None, 0, None) == 0
        want, wt = R.cumsum(a)
        assert wt == want_total
        R.assert_total_equal(total[0], wt)
        fits = np.cumsum(a.astype(np.int64)) <= R.INT32_MAX
        R.assert_same(cum[fits], want[fits], "cum")
    assert R.cumsum(np.zeros(0, np.int32)) [1] == 0


def test_depth_order_sorts_bit_patterns_stably():
    d = R.depths_mixed(5000, seed=1)
    order = R.depth_order(d)
    bits = d.view(np.uint32).astype(np.int64)
    assert sorted(order.tolist()) == list(range(d.size))
    key = bits[order] * d.size + order  # (bits, index) strictly increasing <=> sorted by bits, ties by index
    assert (np.diff(key) > 0).all()
    assert np.isnan(d).any() and (d < 0).any() and (bits == 0x80000000).any()  # the specials are really in there


@pytest.mark.parametrize("grid,n,gen", [((4, 3), 300, "grid"), ((13, 8), 1500, "grid"), ((120, 68), 3000, "grid"),
                                        ((13, 8), 1500, "float"), ((120, 68), 2001, "float")])
def test_emit_matches_the_cpu_twin(cpu, oracle, grid, n, gen):
    tw, th = grid
    m, r = (R.gaussians_grid(n, tw, th, seed=n, full_cover_run=3) if gen == "grid" else R.gaussians_float(n, tw, th, seed=n))
    d = R.depths_mixed(n, seed=n + 1)
    tiles = R.tile_aabb(m, r, tw, th)[4]
    tpg = np.zeros(n, np.int32)
    oracle.lib().orc_tile_count(ctypes.c_int(n), P(m), P(r), ctypes.c_int(tw), ctypes.c_int(th), P(tpg))
    R.assert_same(tiles, tpg, "tiles_per_gauss")
    assert (tiles[r <= 0] == 0).all() and (tiles > 0).any()
    for order in (None, np.random.default_rng(n).permutation(n).astype(np.int32), R.depth_order(d)):
        cum, total = R.cumsum(tiles, order)
        ids, flat = np.full(total, -7, np.int64), np.full(total, -7, np.int32)
        assert cpu["gags_tile_emit"](n, P(m), P(r), P(d), P(cum), P(order), tw, th, P(ids), P(flat), None) == 0
        w_ids, w_flat = R.tile_emit(m, r, d, order, tw, th)
        R.assert_pairs_equal(ids, flat, w_ids, w_flat, "emit")
        c_ids, c_flat = R.tile_emit(m, r, d, order, tw, th, cap=total // 2)
        R.assert_pairs_equal(c_ids, c_flat, w_ids[:total // 2], w_flat[:total // 2], "emit, cap below the count")
        t_ids, t_flat = R.tile_emit(m, r, d, order, tw, th, cap=total + 9, with_tail=True)
        R.assert_pairs_equal(t_ids[:total], t_flat[:total], w_ids, w_flat, "emit, cap above the count")
        assert (t_ids[total:] == (tw * th) << 32).all() and (t_flat[total:] == 0).all() and t_ids.size == total + 9


@pytest.mark.parametrize("dist", R.KEY_DISTS)
@pytest.mark.parametrize("n,tile_bits", [(1, 1), (2, 9), (2047, 8), (2049, 13), (6143, 16), (6143, 17), (20_011, 24), (5000, 31)])
def test_sort_matches_the_cpu_twin(cpu, dist, n, tile_bits):
    keys = R.sort_keys(n, tile_bits, dist, seed=n + tile_bits)
    vals = np.random.default_rng(n).permutation(n).astype(np.int32)
    ko, vo = np.zeros_like(keys), np.zeros_like(vals)
    assert cpu["gags_sort_pairs"](n, tile_bits, 0, P(keys), P(vals), P(ko), P(vo), None, 0, None) == 0
    R.assert_pairs_equal(ko, vo, *R.sort_pairs(keys, vals, *R.sort_args(tile_bits, 0)), "full sort")
    # the tile-bits-only sort of the same pairs: the twin sorts all bits, so hand it keys whose low words are zeroed and
    # put the low words back through the values' permutation
    hi = (keys.view(np.uint64) & np.uint64(0xffffffff00000000)).view(np.int64)
    idx = np.arange(n, dtype=np.int32)
    io = np.zeros_like(idx)
    assert cpu["gags_sort_pairs"](n, tile_bits, 1, P(hi), P(idx), P(ko), P(io), None, 0, None) == 0
    R.assert_pairs_equal(keys[io], vals[io], *R.sort_pairs(keys, vals, *R.sort_args(tile_bits, 1)), "tile sort")


@pytest.mark.parametrize("case", ["tile0", "last", "first_last", "every", "sparse", "one_tile"])
def test_offsets_match_the_cpu_twin(cpu, case):
    g = np.random.default_rng(5)
    n_tiles, tiles = {"tile0": (500, np.zeros(3000, np.int64)), "last": (500, np.full(3000, 499)),
                      "first_last": (65_537, np.repeat([0, 65_536], [700, 900])), "every": (3001, np.arange(3001)),
                      "sparse": (8160, g.choice(g.choice(8160, 816, replace=False), 20_000)),
                      "one_tile": (1, np.zeros(77, np.int64))}[case]
    ids = R.sorted_tile_keys(tiles, seed=2)
    for k in (0, 41):
        full = R.with_sentinels(ids, n_tiles, k)
        off = np.full(n_tiles + 1, -9, np.int32)
        assert cpu["gags_tile_offsets"](full.size, P(full), n_tiles, P(off), None) == 0
        want = R.tile_offsets(full, n_tiles)
        R.assert_offsets_equal(off, want)
        assert want[-1] == ids.size and want[0] == 0
    off = np.full(n_tiles + 1, -9, np.int32)
    assert cpu["gags_tile_offsets"](0, None, n_tiles, P(off), None) == 0
    R.assert_offsets_equal(off, R.tile_offsets(np.zeros(0, np.int64), n_tiles))


def test_trim_restatements_against_a_loop():
    n_tiles, w, h = 7 * 4, 97, 61
    off = R.random_offsets(n_tiles, seed=3)
    g = np.random.default_rng(3)
    ln = np.diff(off)
    need = g.integers(0, ln + 1).astype(np.int32)
    flat = g.integers(0, 1000, off[-1]).astype(np.int32)
    off_new, flat_new = R.trim_lists(off, need, flat)
    want = [flat[off[t]:off[t] + need[t]] for t in range(n_tiles)]
    R.assert_same(flat_new, np.concatenate(want), "trimmed list")
    R.assert_same(off_new, np.concatenate([[0], np.cumsum(need)]).astype(np.int32), "trimmed offsets")
    alphas = g.random((h, w)).astype(np.float32)
    alphas[g.random((h, w)) < 0.3] = 0
    last = g.integers(0, 100, (h, w)).astype(np.int32)
    got = R.trim_last_ids(w, h, off, off_new, alphas, last)
    for i in range(h):
        for j in range(w):
            t = (i // 16) * 7 + j // 16
            assert got[i, j] == (last[i, j] + off[t] - off_new[t] if alphas[i, j] > 0 else last[i, j])


def _scene(n=1500, w=96, h=64):
    from helpers import scene_arrays
    return scene_arrays(n, 16, w, h, seed=3, view=2, scale_mult=6.0), w, h


def test_chains_match_oracle_tile_bin(oracle):
    s, w, h = _scene()
    radii, m2d, depths, _ = oracle.project_fwd(s["means"], s["quats"], s["scales"], s["viewmat"], s["K"], w, h)
    o = oracle.tile_bin(m2d, radii, depths, w, h)
    tw, th = o["tile_width"], o["tile_height"]
    R.assert_same(R.tile_aabb(m2d, radii, tw, th)[4], o["tiles_per_gauss"], "tiles_per_gauss")
    ids, flat = R.tile_emit(m2d, radii, depths, None, tw, th)
    R.assert_pairs_equal(ids, flat, o["isect_ids_unsorted"], o["flatten_ids_unsorted"], "emit")
    assert o["n_isects"] > 1000
    for chain in (R.chain_depth_sorted, R.chain_full_sort):
        ids_s, flat_s, off = chain(m2d, radii, depths, tw, th)
        R.assert_pairs_equal(ids_s, flat_s, o["isect_ids"], o["flatten_ids"], chain.__name__)
        R.assert_offsets_equal(off[:-1].reshape(th, tw), o["isect_offsets"], chain.__name__)
        assert off[-1] == o["n_isects"]


@pytest.mark.parametrize("grid,n", [((4, 3), 700), ((13, 8), 5000), ((120, 68), 20_000), ((256, 256), 20_000)])
def test_the_two_documented_chains_agree(grid, n):
    tw, th = grid
    m, r = R.gaussians_grid(n, tw, th, seed=n, full_cover_run=2)
    m, d = R.twin_neighbours(m, R.depths_positive(n, seed=n), seed=n)
    a, b = R.chain_depth_sorted(m, r, d, tw, th), R.chain_full_sort(m, r, d, tw, th)
    R.assert_binning_equal(a, b, "chain A against chain B")
    assert a[0].size > n and (np.diff(a[0].view(np.uint64)) == 0).any()  # equal (tile, depth) keys really occur


# ---- the checkers bite ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def result():
    tw, th, n = 13, 8, 4000
    m, r = R.gaussians_grid(n, tw, th, seed=11)
    m, d = R.twin_neighbours(m, R.depths_positive(n, seed=11), seed=11)
    ids_s, flat_s, off = R.chain_depth_sorted(m, r, d, tw, th)
    return ids_s, flat_s, off, tw * th


def _raises(fn, *a):
    with pytest.raises(AssertionError, match="first at index|got .* expected|expected"):
        fn(*a)


def test_checker_sees_two_equal_key_neighbours_swapped(result):
    ids_s, flat_s, off, _ = result
    i = int(np.flatnonzero((ids_s[1:] == ids_s[:-1]) & (flat_s[1:] != flat_s[:-1]))[0])
    bad = flat_s.copy()
    bad[[i, i + 1]] = bad[[i + 1, i]]
    R.assert_pairs_equal(ids_s, flat_s, ids_s, flat_s)  # (the unperturbed result passes)
    _raises(R.assert_pairs_equal, ids_s, bad, ids_s, flat_s)
    _raises(R.assert_binning_equal, (ids_s, bad, off), (ids_s, flat_s, off))
    with pytest.raises(AssertionError, match=f"first at index {i} "):
        R.assert_pairs_equal(ids_s, bad, ids_s, flat_s)


def test_checker_sees_an_entry_moved_across_a_tile_boundary(result):
    ids_s, flat_s, off, n_tiles = result
    t = int(np.flatnonzero(np.diff(off) > 0)[3])
    i = int(off[t + 1]) - 1                        # last entry of tile t joins the next non-empty tile
    bad = ids_s.copy()
    bad[i] = (int(ids_s[i + 1]) >> 32 << 32) | (int(ids_s[i]) & 0xffffffff)
    _raises(R.assert_pairs_equal, bad, flat_s, ids_s, flat_s)
    _raises(R.assert_offsets_equal, R.tile_offsets(np.sort(bad), n_tiles), off)
    _raises(R.assert_binning_equal, (bad, flat_s, off), (ids_s, flat_s, off))


def test_checker_sees_one_offset_shifted_by_one(result):
    ids_s, flat_s, off, n_tiles = result
    for t in (0, n_tiles // 2, n_tiles):
        for delta in (1, -1):
            bad = off.copy()
            bad[t] += delta
            _raises(R.assert_offsets_equal, bad, off)
            _raises(R.assert_binning_equal, (ids_s, flat_s, bad), (ids_s, flat_s, off))


def test_checker_sees_a_dropped_sentinel_tail(result):
    ids_s, flat_s, off, n_tiles = result
    k = 17
    ids_t, flat_t = R.with_sentinels(ids_s, n_tiles, k), np.concatenate([flat_s, np.zeros(k, np.int32)])
    R.assert_offsets_equal(R.tile_offsets(ids_t, n_tiles), off)  # (the tail does not move the count)
    _raises(R.assert_pairs_equal, ids_s, flat_s, ids_t, flat_t)                         # tail missing altogether
    junk = ids_t.copy()
    junk[-k:] = 12345                                                                   # tail left as the prefill
    _raises(R.assert_pairs_equal, junk, flat_t, ids_t, flat_t)
    one = ids_t.copy()
    one[-1] = (n_tiles - 1) << 32                                                       # one sentinel with a real tile's id
    _raises(R.assert_pairs_equal, one, flat_t, ids_t, flat_t)


def test_checker_sees_a_total_off_by_one():
    a = R.counts(5000, seed=1)
    cum, total = R.cumsum(a)
    R.assert_total_equal(total, total)
    for bad in (total + 1, total - 1, -1):
        _raises(R.assert_total_equal, bad, total)
    _raises(R.assert_total_equal, R.INT32_MAX, -1)
    bad = cum.copy()
    bad[-1] += 1
    _raises(R.assert_same, bad, cum)
    _raises(R.assert_same, cum.astype(np.int64), cum)   # a dtype is part of the result
    _raises(R.assert_same, cum[:-1], cum)


def test_checker_sees_a_touched_guard_word():
    buf = np.full(100, 12345, np.int32)
    buf[10:90] = 1
    R.assert_guards(buf, 10, 90, 12345)
    for i in (9, 90, 0, 99):
        bad = buf.copy()
        bad[i] = 0
        with pytest.raises(AssertionError, match=f"buffer index {i} "):
            R.assert_guards(bad, 10, 90, 12345)
