"""The binning primitives (K5-K8 and the list trimming) driven directly through the C ABI on the GPU: gags_cumsum_i32 /
_gather_i32, gags_depth_order, gags_tile_emit / _cap, gags_sort_pairs, gags_tile_offsets, gags_trim_lists / _last_ids
against the numpy restatements of tests/binning_ref.py (proven against the CPU twins in tests/test_binning_cpu.py).

Every output and scratch buffer is a slice of a larger tensor whose guard words on both sides are prefilled and must be
unchanged afterwards; const inputs must be bit-identical after the call; scratch is exactly what *_scratch_bytes(n) asks
for, and one byte less must be refused with GAGS_ESCRATCH before anything is written.  Every output is an integer: every
comparison is exact.  No input leaves the documented contracts (a `cum` that disagrees with the rectangles, a key bit at or
above 32 + tile_bits could write out of bounds and is not what is tested)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import binning_ref as R  # noqa: E402

SENT = 12345      # prefill of every output element and guard word
SENT_BYTE = 0x5a  # ... of scratch bytes
GUARD = 64        # guard elements on each side (scratch: 256 bytes, which keeps the payload's alignment)
ESCRATCH = -3


@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    return _lib.load()


def ptr(t):
    from gags_amd import _lib
    return _lib.ptr(t)


def ok(code, what):
    from gags_amd import _lib
    _lib.check(code, what)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Out:
    """n payload elements between two runs of guard words, everything prefilled with the sentinel."""

    def __init__(self, n, dtype, what):
        self.n, self.what = int(n), what
        self.g = 256 if dtype == torch.uint8 else GUARD
        self.fill = SENT_BYTE if dtype == torch.uint8 else SENT
        self.buf = torch.full((self.n + 2 * self.g,), self.fill, dtype=dtype, device="cuda")
        self.t = self.buf[self.g:self.g + self.n]
        self.nbytes = self.n * self.buf.element_size()

    @property
    def p(self):   # (not through the slice: an empty slice has no data pointer, the payload's position still exists)
        return ctypes.c_void_p(self.buf.data_ptr() + self.g * self.buf.element_size())

    def get(self):
        """The payload as numpy, after checking both guards."""
        torch.cuda.synchronize()
        a = self.buf.cpu().numpy()
        R.assert_guards(a, self.g, self.g + self.n, self.fill, self.what)
        return a[self.g:self.g + self.n].copy()

    def untouched(self):
        torch.cuda.synchronize()
        a = self.buf.cpu().numpy()
        bad = np.flatnonzero(a != self.fill)
        assert bad.size == 0, f"{self.what}: written at buffer index {int(bad[0])} by a call that must not write"


class Const:
    """A const input: uploaded once, compared bit for bit with what was uploaded after the calls."""

    def __init__(self, a, what):
        self.what = what
        self.t = dev(a)
        self.ref = self.t.clone()

    @property
    def p(self):
        return ptr(self.t)

    def check(self):
        torch.cuda.synchronize()
        assert torch.equal(self.t.view(torch.uint8), self.ref.view(torch.uint8)), f"{self.what}: a const input was modified"


def scratch(nbytes, what="scratch"):
    return Out(nbytes, torch.uint8, what)


# ---- K5: prefix sum -------------------------------------------------------------------------------------------------------
def _scan(lib, a, idx=None, in_place=False, with_total=True):
    """One gags_cumsum_i32 / _gather_i32 call under guards; returns (cum, total or None)."""
    n = a.size
    sb = lib.gags_scan_scratch_bytes(n)
    sc = scratch(sb)
    total = Out(1, torch.int32, "total")
    cum = Out(n, torch.int32, "cum")
    src = None
    if in_place:
        cum.t.copy_(dev(a))
        in_p = cum.p
    else:
        src = Const(a if n else np.zeros(1, np.int32), "in")
        in_p = src.p
    tp = total.p if with_total else None
    if idx is None:
        ok(lib.gags_cumsum_i32(n, in_p, cum.p, tp, sc.p, sb, None), "gags_cumsum_i32")
    else:
        ix = Const(idx if n else np.zeros(1, np.int32), "idx")
        ok(lib.gags_cumsum_gather_i32(n, in_p, ix.p, cum.p, tp, sc.p, sb, None), "gags_cumsum_gather_i32")
        ix.check()
    if src is not None:
        src.check()
    sc.get()
    t = total.get()
    if not with_total:
        total.untouched()
    return cum.get(), (int(t[0]) if with_total else None)


@pytest.mark.parametrize("n", R.LADDER)
def test_cumsum(lib, n):
    a = R.counts(n, seed=n)
    want, wt = R.cumsum(a)
    for in_place in (False, True):
        for with_total in (True, False):
            if n == 0 and in_place:
                continue
            cum, total = _scan(lib, a, in_place=in_place, with_total=with_total)
            what = f"cumsum n={n} in_place={in_place}"
            R.assert_same(cum, want, what)
            if with_total:
                R.assert_total_equal(total, wt, what)
    perm = np.random.default_rng(n + 1).permutation(n).astype(np.int32)
    want, wt = R.cumsum(a, perm)
    for with_total in (True, False):
        cum, total = _scan(lib, a, idx=perm, with_total=with_total)
        R.assert_same(cum, want, f"cumsum_gather n={n}")
        if with_total:
            R.assert_total_equal(total, wt, f"cumsum_gather n={n}")


def test_cumsum_refusals_write_nothing(lib):
    n = 5000
    a = Const(R.counts(n, seed=1), "in")
    idx = Const(np.arange(n, dtype=np.int32), "idx")
    sb = lib.gags_scan_scratch_bytes(n)
    assert sb == 4 * ((n + R.BLOCK - 1) // R.BLOCK)
    sc, cum, total = scratch(sb), Out(n, torch.int32, "cum"), Out(1, torch.int32, "total")
    assert lib.gags_cumsum_i32(n, a.p, cum.p, total.p, sc.p, sb - 1, None) == ESCRATCH
    assert lib.gags_cumsum_gather_i32(n, a.p, idx.p, cum.p, total.p, sc.p, sb - 1, None) == ESCRATCH
    assert lib.gags_cumsum_gather_i32(n, cum.p, idx.p, cum.p, total.p, sc.p, sb, None) == -1   # a permuted read cannot run in place
    for o in (sc, cum, total):
        o.untouched()
    a.check()
    idx.check()


def test_cumsum_total_past_int32_is_minus_one(lib):
    """Entries stay below the documented per-entry bound (2^20, include/gags_raster.h): 300 000 Gaussians that each cover
    the 1080p grid sum to 2.448e9 -> -1; the largest sum that fits comes back as itself, one more is -1 again."""
    for a, want_total in ((np.full(300_000, 8160, np.int32), -1),
                          (R.counts_exact_sum(1_048_594, R.INT32_MAX), R.INT32_MAX),
                          (R.counts_exact_sum(1_048_594, R.INT32_MAX + 1), -1)):
        want, wt = R.cumsum(a)
        assert wt == want_total
        perm = np.random.default_rng(3).permutation(a.size).astype(np.int32)
        for idx in (None, perm):
            cum, total = _scan(lib, a, idx=idx)
            # (behind a wrapped sum the entries of cum are nobody's contract: the caller refuses the view)
            fits = np.cumsum((a if idx is None else a[idx]).astype(np.int64)) <= R.INT32_MAX
            R.assert_total_equal(total, wt, "total")
            R.assert_same(cum[fits], R.cumsum(a, idx)[0][fits], "cum before the overflow")


# ---- K7a: depth order -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.LADDER + (4_194_304 + 5,))
def test_depth_order(lib, n):
    d = R.depths_mixed(n, seed=n)
    tiles = R.counts(n, seed=n + 1)
    want = R.depth_order(d)
    sb = lib.gags_depth_order_scratch_bytes(n)
    dd, tt = Const(d if n else np.zeros(1, np.float32), "depths"), Const(tiles if n else np.zeros(1, np.int32), "tiles")
    for with_tiles in (True, False):
        sc, order, tord = scratch(sb), Out(n, torch.int32, "order"), Out(n, torch.int32, "tiles_ordered")
        ok(lib.gags_depth_order(n, dd.p, tt.p if with_tiles else None, order.p, tord.p if with_tiles else None, sc.p, sb, None),
           "gags_depth_order")
        R.assert_same(order.get(), want, f"order n={n}")
        if with_tiles:
            R.assert_same(tord.get(), tiles[want], f"tiles_ordered n={n}")
        else:
            tord.untouched()
        sc.get()
    dd.check()
    tt.check()
    if n:
        sc, order = scratch(sb), Out(n, torch.int32, "order")
        assert lib.gags_depth_order(n, dd.p, None, order.p, None, sc.p, sb - 1, None) == ESCRATCH
        sc.untouched()
        order.untouched()


# ---- K7: pair sort --------------------------------------------------------------------------------------------------------
def _sort(lib, keys, vals, tile_bits, depth_sorted, what):
    n = keys.size
    sb = lib.gags_sort_scratch_bytes(n)
    k_in, v_in = Const(keys, "keys_in"), Const(vals, "vals_in")
    sc, ko, vo = scratch(sb), Out(n, torch.int64, "keys_out"), Out(n, torch.int32, "vals_out")
    assert lib.gags_sort_pairs(n, tile_bits, depth_sorted, k_in.p, v_in.p, ko.p, vo.p, sc.p, sb - 1, None) == ESCRATCH
    for o in (sc, ko, vo):
        o.untouched()
    ok(lib.gags_sort_pairs(n, tile_bits, depth_sorted, k_in.p, v_in.p, ko.p, vo.p, sc.p, sb, None), "gags_sort_pairs")
    got_k, got_v = ko.get(), vo.get()
    sc.get()
    k_in.check()
    v_in.check()
    wk, wv = R.sort_pairs(keys, vals, *R.sort_args(tile_bits, depth_sorted))
    R.assert_pairs_equal(got_k, got_v, wk, wv, what)


SMALL_N = (1, 2, 64, 2047, 2048, 2049, 6143, 100_003)
BIG_N = (4_194_304 + 5, 8_388_608 + 2049)   # rs_rowscan: 2 and 3 trips over the blocks, with a carry


@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("tile_bits", [1, 8, 9, 13, 16, 17, 24, 31])
def test_sort_by_tile_is_the_stable_grouping(lib, n, tile_bits):
    """depth_sorted = 1: only the tile bits are sorted, 1 to 4 passes.  The low words are random, not sorted: keys of one
    tile must keep their input order."""
    keys = R.sort_keys(n, tile_bits, "uniform", seed=n + tile_bits)
    _sort(lib, keys, np.arange(n, dtype=np.int32), tile_bits, 1, f"tile sort n={n} tile_bits={tile_bits}")


@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("tile_bits", [1, 9, 13, 17, 31])
@pytest.mark.parametrize("dist", R.KEY_DISTS)
def test_full_sort(lib, n, tile_bits, dist):
    """depth_sorted = 0: all of bits [0, 32 + tile_bits), 5 to 8 passes; equal keys keep their input order."""
    keys = R.sort_keys(n, tile_bits, dist, seed=n + tile_bits)
    _sort(lib, keys, np.arange(n, dtype=np.int32), tile_bits, 0, f"full sort {dist} n={n} tile_bits={tile_bits}")


@pytest.mark.parametrize("dist", [d for d in R.KEY_DISTS if d != "uniform"])
@pytest.mark.parametrize("tile_bits", [9, 17])
def test_sort_by_tile_of_every_distribution(lib, dist, tile_bits):
    keys = R.sort_keys(6143, tile_bits, dist, seed=tile_bits)
    _sort(lib, keys, np.arange(6143, dtype=np.int32), tile_bits, 1, f"tile sort {dist} tile_bits={tile_bits}")


@pytest.mark.parametrize("n", BIG_N)
@pytest.mark.parametrize("dist", ["uniform", "equal"])
@pytest.mark.parametrize("tile_bits,depth_sorted", [(13, 1), (17, 1), (13, 0), (31, 0)])
def test_sort_past_one_trip_of_the_block_scan(lib, n, dist, tile_bits, depth_sorted):
    keys = R.sort_keys(n, tile_bits, dist, seed=tile_bits)
    _sort(lib, keys, np.arange(n, dtype=np.int32), tile_bits, depth_sorted,
          f"sort {dist} n={n} tile_bits={tile_bits} depth_sorted={depth_sorted}")


@pytest.mark.parametrize("depth_sorted", [0, 1])
def test_sort_carries_arbitrary_values(lib, depth_sorted):
    n = 100_003
    keys = R.sort_keys(n, 13, "dupes", seed=9)
    vals = np.random.default_rng(9).permutation(n).astype(np.int32) - 50_000
    _sort(lib, keys, vals, 13, depth_sorted, "sort with permuted values")


@pytest.mark.parametrize("n_tiles", [255, 256])
@pytest.mark.parametrize("depth_sorted", [0, 1])
def test_sort_with_the_sentinel_tile_at_the_pass_count_boundary(lib, n_tiles, depth_sorted):
    """Capacity mode: the sentinel tile id n_tiles needs tile_bits = n_tiles.bit_length() (8 at 255, 9 at 256: one more pass)."""
    tile_bits = n_tiles.bit_length()
    n = 30_011
    keys = R.sort_keys(n, tile_bits, "uniform", seed=n_tiles, max_tile=n_tiles - 1)
    keys[np.random.default_rng(1).random(n) < 0.2] = n_tiles << 32
    _sort(lib, keys, np.arange(n, dtype=np.int32), tile_bits, depth_sorted, f"sentinel tile {n_tiles}")


def test_sort_of_nothing_writes_nothing(lib):
    sc, ko, vo = scratch(64), Out(4, torch.int64, "keys_out"), Out(4, torch.int32, "vals_out")
    ok(lib.gags_sort_pairs(0, 13, 1, ko.p, vo.p, ko.p, vo.p, sc.p, 0, None), "gags_sort_pairs")
    for o in (sc, ko, vo):
        o.untouched()


# ---- K6: emit ---------------------------------------------------------------------------------------------------------------
GRIDS = [((4, 3), 333), ((13, 8), 3001), ((120, 68), 20_011), ((256, 256), 50_003)]


def _emit_inputs(grid, n, gen="grid", full_cover_run=0):
    tw, th = grid
    m, r = (R.gaussians_grid(n, tw, th, seed=n, full_cover_run=full_cover_run) if gen == "grid"
            else R.gaussians_float(n, tw, th, seed=n))
    d = R.depths_mixed(n, seed=n + 1)
    return m, r, d, R.tile_aabb(m, r, tw, th)[4]


@pytest.mark.parametrize("grid,n,gen,run", [(g, n, "grid", 0) for g, n in GRIDS] + [((120, 68), 4001, "grid", 70),
                                                                                    ((13, 8), 3001, "float", 0),
                                                                                    ((120, 68), 20_011, "float", 0)])
@pytest.mark.parametrize("ordered", [False, True])
def test_tile_emit(lib, grid, n, gen, run, ordered):
    tw, th = grid
    m, r, d, tiles = _emit_inputs(grid, n, gen, run)
    assert n % 64 and n % 256 and (r <= 0).any() and (tiles[r > 0] == 0).any()
    if run:
        assert (tiles == tw * th).sum() >= run
    order = np.random.default_rng(n).permutation(n).astype(np.int32) if ordered else None
    cum, count = R.cumsum(tiles, order)
    w_ids, w_flat = R.tile_emit(m, r, d, order, tw, th)
    assert count == w_ids.size > n
    ins = [Const(m, "means2d"), Const(r, "radii"), Const(d, "depths"), Const(cum, "cum")]
    o = Const(order, "order") if ordered else None
    ids, flat = Out(count, torch.int64, "isect_ids"), Out(count, torch.int32, "flatten_ids")
    ok(lib.gags_tile_emit(n, *(c.p for c in ins), o.p if o else None, tw, th, ids.p, flat.p, None), "gags_tile_emit")
    R.assert_pairs_equal(ids.get(), flat.get(), w_ids, w_flat, f"emit {grid} n={n} {gen} ordered={ordered}")
    for c in ins + ([o] if o else []):
        c.check()


@pytest.mark.parametrize("grid,n", [((13, 8), 3001), ((120, 68), 20_011)])
@pytest.mark.parametrize("which", ["above", "exact", "half"])
@pytest.mark.parametrize("with_total", [True, False])
def test_tile_emit_cap(lib, grid, n, which, with_total):
    """At most `cap` pairs are written (guard words behind the capacity), the entries below min(cap, count) are those of
    the full emission, and with `total` the entries [count, cap) are sentinels of tile n_tiles."""
    tw, th = grid
    m, r, d, tiles = _emit_inputs(grid, n)
    order = R.depth_order(d)
    cum, count = R.cumsum(tiles, order)
    cap = {"above": count + 1000, "exact": count, "half": count // 2}[which]
    ins = [Const(m, "means2d"), Const(r, "radii"), Const(d, "depths"), Const(cum, "cum"), Const(order, "order")]
    total = Const(np.array([count], np.int32), "total")
    ids, flat = Out(cap, torch.int64, "isect_ids"), Out(cap, torch.int32, "flatten_ids")
    ok(lib.gags_tile_emit_cap(n, *(c.p for c in ins), tw, th, ids.p, flat.p, cap, total.p if with_total else None, None),
       "gags_tile_emit_cap")
    w_ids, w_flat = R.tile_emit(m, r, d, order, tw, th, cap=cap, with_tail=with_total)
    if not with_total and cap > count:   # nobody asked for a tail: those entries stay as they were
        w_ids = np.concatenate([w_ids, np.full(cap - count, SENT, np.int64)])
        w_flat = np.concatenate([w_flat, np.full(cap - count, SENT, np.int32)])
    R.assert_pairs_equal(ids.get(), flat.get(), w_ids, w_flat, f"emit_cap {which} total={with_total}")
    for c in ins + [total]:
        c.check()


def test_tile_emit_of_nothing(lib):
    ids, flat = Out(0, torch.int64, "isect_ids"), Out(0, torch.int32, "flatten_ids")
    total = Const(np.zeros(1, np.int32), "total")
    ok(lib.gags_tile_emit_cap(0, None, None, None, None, None, 13, 8, ids.p, flat.p, 0, total.p, None), "gags_tile_emit_cap")
    ok(lib.gags_tile_emit(0, None, None, None, None, None, 13, 8, ids.p, flat.p, None), "gags_tile_emit")
    ids.untouched()
    flat.untouched()
    # no Gaussians but a capacity: all sentinels
    ids, flat = Out(777, torch.int64, "isect_ids"), Out(777, torch.int32, "flatten_ids")
    ok(lib.gags_tile_emit_cap(0, None, None, None, None, None, 13, 8, ids.p, flat.p, 777, total.p, None), "gags_tile_emit_cap")
    R.assert_pairs_equal(ids.get(), flat.get(), np.full(777, 104 << 32, np.int64), np.zeros(777, np.int32), "empty view")


# ---- K8: offsets ------------------------------------------------------------------------------------------------------------
def _offset_case(case):
    g = np.random.default_rng(5)
    return {"tile0": (500, np.zeros(30_000, np.int64)), "last": (500, np.full(30_000, 499)),
            "first_last": (65_537, np.repeat([0, 65_536], [7000, 9000])), "every": (30_001, np.arange(30_001)),
            "sparse": (8160, g.choice(g.choice(8160, 816, replace=False), 200_000)),
            "middle": (8160, g.integers(3000, 3100, 50_000)),
            "one_tile": (1, np.zeros(777, np.int64)), "one_entry": (8160, np.array([4000]))}[case]


@pytest.mark.parametrize("case", ["tile0", "last", "first_last", "every", "sparse", "middle", "one_tile", "one_entry"])
@pytest.mark.parametrize("tail", [0, 1, 3000])
def test_tile_offsets(lib, case, tail):
    n_tiles, tiles = _offset_case(case)
    ids = R.with_sentinels(R.sorted_tile_keys(tiles, seed=2), n_tiles, tail)
    want = R.tile_offsets(ids, n_tiles)
    assert want[-1] == ids.size - tail and want.size == n_tiles + 1
    src, off = Const(ids, "sorted_ids"), Out(n_tiles + 1, torch.int32, "isect_offsets")
    ok(lib.gags_tile_offsets(ids.size, src.p, n_tiles, off.p, None), "gags_tile_offsets")
    R.assert_offsets_equal(off.get(), want, f"offsets {case} tail={tail}")
    src.check()


@pytest.mark.parametrize("n_tiles", [1, 255, 256, 257, 8160])
def test_tile_offsets_of_nothing(lib, n_tiles):
    off = Out(n_tiles + 1, torch.int32, "isect_offsets")
    ok(lib.gags_tile_offsets(0, None, n_tiles, off.p, None), "gags_tile_offsets")
    R.assert_offsets_equal(off.get(), np.zeros(n_tiles + 1, np.int32))
    # only sentinels (a capacity, no intersections)
    ids = Const(R.with_sentinels(np.zeros(0, np.int64), n_tiles, 500), "sorted_ids")
    off = Out(n_tiles + 1, torch.int32, "isect_offsets")
    ok(lib.gags_tile_offsets(500, ids.p, n_tiles, off.p, None), "gags_tile_offsets")
    R.assert_offsets_equal(off.get(), np.zeros(n_tiles + 1, np.int32))


# ---- list trimming ------------------------------------------------------------------------------------------------------------
def _need(kind, ln, g):
    if kind == "zero":
        return np.zeros_like(ln)
    if kind == "full":
        return ln.copy()
    need = g.integers(0, ln + 1)
    if kind == "some_zero":
        need[g.random(ln.size) < 0.5] = 0
    return need


@pytest.mark.parametrize("size", [(97, 61), (1920, 1080)])
@pytest.mark.parametrize("kind", ["zero", "full", "random", "some_zero"])
def test_trim_lists_and_last_ids(lib, size, kind):
    w, h = size
    tw, th = (w + 15) // 16, (h + 15) // 16
    n_tiles = tw * th
    g = np.random.default_rng(w)
    off = R.random_offsets(n_tiles, seed=w, max_len=600)   # (lists longer than one workgroup's 256 threads)
    ln = np.diff(off).astype(np.int64)
    need = _need(kind, ln, g).astype(np.int32)
    assert (ln == 0).any() and ln.max() > 256
    assert kind != "some_zero" or (((need == 0) & (ln > 0)).any() and (need > 256).any())
    flat = g.integers(0, 1 << 20, off[-1]).astype(np.int32)
    need_cum, total = R.cumsum(need)
    w_off, w_flat = R.trim_lists(off, need, flat)
    assert w_flat.size == total
    ins = [Const(off, "isect_offsets"), Const(need_cum, "need_cum"), Const(flat, "flatten_ids")]
    o_off, o_flat = Out(n_tiles + 1, torch.int32, "offsets_out"), Out(total, torch.int32, "flatten_out")
    ok(lib.gags_trim_lists(w, h, ins[0].p, ins[1].p, ins[2].p, o_off.p, o_flat.p, None), "gags_trim_lists")
    R.assert_offsets_equal(o_off.get(), w_off, f"trimmed offsets {kind}")
    R.assert_same(o_flat.get(), w_flat, f"trimmed list {kind}")
    o_off2 = Out(n_tiles + 1, torch.int32, "offsets_out")
    ok(lib.gags_trim_lists(w, h, ins[0].p, ins[1].p, None, o_off2.p, None, None), "gags_trim_lists")   # the offsets only
    R.assert_offsets_equal(o_off2.get(), w_off, f"trimmed offsets {kind}, no list")
    # last_ids: indices into the trimmed lists (anything inside the pixel's tile), exact zeros among the alphas
    alphas = g.random((h, w)).astype(np.float32)
    alphas[g.random((h, w)) < 0.3] = 0
    alphas[0, 0], alphas[-1, -1] = 0.5, 1e-30
    i, j = np.divmod(np.arange(w * h), w)
    t = (i // 16) * tw + j // 16
    last = (w_off[t] + g.integers(0, np.maximum(need[t], 1))).astype(np.int32).reshape(h, w)
    last[alphas == 0] = 0
    want = R.trim_last_ids(w, h, off, w_off, alphas, last)
    a, o_new = Const(alphas, "alphas"), Const(w_off, "offsets_trimmed")
    o_last = Out(w * h, torch.int32, "last_ids")
    o_last.t.copy_(dev(last.ravel()))
    ok(lib.gags_trim_last_ids(w, h, ins[0].p, o_new.p, a.p, o_last.p, None), "gags_trim_last_ids")
    R.assert_same(o_last.get().reshape(h, w), want, f"last_ids {kind}")
    for c in ins + [a, o_new]:
        c.check()


# ---- the two documented chains ------------------------------------------------------------------------------------------------
def _gpu_chain(lib, m, r, d, tiles, tw, th, depth_sorted):
    """INTEGRATION.md's call order composed from the entries: (ids_s, flat_s, offsets[n_tiles + 1])."""
    n, n_tiles = r.size, tw * th
    tile_bits = max(1, n_tiles.bit_length())
    ins = [Const(m, "means2d"), Const(r, "radii"), Const(d, "depths")]
    tl = Const(tiles, "tiles_per_gauss")
    sb = lib.gags_scan_scratch_bytes(n)
    sc, cum, total = scratch(sb), Out(n, torch.int32, "cum"), Out(1, torch.int32, "total")
    order = None
    if depth_sorted:
        dsb = lib.gags_depth_order_scratch_bytes(n)
        dsc, order = scratch(dsb), Out(n, torch.int32, "order")
        ok(lib.gags_depth_order(n, ins[2].p, None, order.p, None, dsc.p, dsb, None), "gags_depth_order")
        ok(lib.gags_cumsum_gather_i32(n, tl.p, order.p, cum.p, total.p, sc.p, sb, None), "gags_cumsum_gather_i32")
        dsc.get()
    else:
        ok(lib.gags_cumsum_i32(n, tl.p, cum.p, total.p, sc.p, sb, None), "gags_cumsum_i32")
    count = int(total.get()[0])
    assert count == int(tiles.astype(np.int64).sum())
    ids, flat = Out(count, torch.int64, "isect_ids"), Out(count, torch.int32, "flatten_ids")
    ok(lib.gags_tile_emit(n, ins[0].p, ins[1].p, ins[2].p, cum.p, order.p if order else None, tw, th, ids.p, flat.p, None),
       "gags_tile_emit")
    ssb = lib.gags_sort_scratch_bytes(count)
    ssc, ids_s, flat_s = scratch(ssb), Out(count, torch.int64, "ids sorted"), Out(count, torch.int32, "flat sorted")
    ok(lib.gags_sort_pairs(count, tile_bits, depth_sorted, ids.p, flat.p, ids_s.p, flat_s.p, ssc.p, ssb, None), "gags_sort_pairs")
    off = Out(n_tiles + 1, torch.int32, "isect_offsets")
    ok(lib.gags_tile_offsets(count, ids_s.p, n_tiles, off.p, None), "gags_tile_offsets")
    for o in (sc, ssc, cum, ids, flat) + ((order,) if order else ()):
        o.get()
    for c in ins + [tl]:
        c.check()
    return ids_s.get(), flat_s.get(), off.get()


@pytest.mark.parametrize("grid,n,max_radius", [((13, 8), 5003, 40), ((120, 68), 300_007, 40), ((256, 256), 200_003, 40)])
def test_the_two_documented_chains_agree(lib, grid, n, max_radius):
    from gags_amd import rasterization as rz
    tw, th = grid
    n_tiles = tw * th
    m, r = R.gaussians_grid(n, tw, th, seed=n, max_radius=max_radius, full_cover_run=2)
    m, d = R.twin_neighbours(m, R.depths_positive(n, seed=n), seed=n)
    tiles = R.tile_aabb(m, r, tw, th)[4]
    want = R.chain_full_sort(m, r, d, tw, th)
    count = want[0].size
    assert (np.diff(want[0].view(np.uint64)) == 0).any() and count > 2 * n   # fully equal (tile, depth) keys occur
    a = _gpu_chain(lib, m, r, d, tiles, tw, th, 1)
    R.assert_binning_equal(a, want, "chain A (depth order, sort by tile) against the restatement")
    b = _gpu_chain(lib, m, r, d, tiles, tw, th, 0)
    R.assert_binning_equal(b, want, "chain B (index order, full sort) against the restatement")
    R.assert_binning_equal(a, b, "chain A against chain B")
    # the product's own front-end on the same inputs
    w, h = tw * 16 - 3, th * 16 - 5   # (ragged image, same tile grid)
    args = (dev(m), dev(r), dev(d), dev(tiles), w, h)
    ids_s, flat_s, off_view, cnt, _, offsets = rz.tile_binning(*args)
    torch.cuda.synchronize()
    assert cnt == count and tuple(off_view.shape) == (th, tw)
    R.assert_binning_equal((ids_s.cpu().numpy(), flat_s.cpu().numpy(), offsets.cpu().numpy()), want, "tile_binning")
    cap = count + 4099
    ids_c, flat_c, _, cnt_c, _, offsets_c = rz.tile_binning(*args, cap=cap)
    assert cnt_c.get() == count
    torch.cuda.synchronize()
    ids_c, flat_c = ids_c.cpu().numpy(), flat_c.cpu().numpy()
    assert ids_c.size == cap
    R.assert_binning_equal((ids_c[:count], flat_c[:count], offsets_c.cpu().numpy()), want, "tile_binning with a capacity")
    R.assert_pairs_equal(ids_c[count:], flat_c[count:], np.full(cap - count, n_tiles << 32, np.int64),
                         np.zeros(cap - count, np.int32), "tile_binning with a capacity: the tail")
