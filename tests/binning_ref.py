"""Plain numpy restatements of the binning chain (K5-K8 and the list trimming): prefix sum, depth order, tile rectangle,
intersection emit, stable pair sort, per-tile offsets, trimmed lists.  int64 / uint64 arithmetic, no GPU, no ctypes: the
references tests/test_binning_gpu.py holds the HIP kernels to, themselves proven against the CPU twins and the oracle in
tests/test_binning_cpu.py.  Also the seeded input generators both files share and the comparison helpers, which report
the first differing index.  Every output of this chain is an integer: every comparison is exact."""
import numpy as np

TILE = 16
INT32_MAX = (1 << 31) - 1
BLOCK = 2048  # pairs per scan / sort workgroup (csrc/scan.h SCAN_TILE, csrc/sort.hip RS_TILE)


# ---- restatements ------------------------------------------------------------------------------------------------------
def cumsum(a, idx=None):
    """K5: (cum int32, total): inclusive sums of a[idx] in int64; total = -1 when the sum does not fit an int32 (cum is
    then only meaningful up to the last entry that still fits)."""
    a = np.asarray(a, np.int32)
    v = a if idx is None else a[np.asarray(idx, np.int64)]
    c = np.cumsum(v.astype(np.int64))
    total = int(c[-1]) if c.size else 0
    return c.astype(np.int32), (-1 if total > INT32_MAX else total)


def depth_order(depths):
    """K7a: stable argsort of the depths' BIT PATTERNS (negative, NaN and -0.0 depths are fully determined too)."""
    return np.argsort(np.ascontiguousarray(depths, np.float32).view(np.uint32), kind="stable").astype(np.int32)


def tile_aabb(means2d, radii, tile_w, tile_h):
    """gags_tile_aabb (csrc/common.h) in float32: (x0, x1, y0, y1, tiles_per_gauss); radius <= 0 covers nothing."""
    m = np.asarray(means2d, np.float32).reshape(-1, 2)
    r = np.asarray(radii, np.int32)
    tr = r.astype(np.float32) / np.float32(TILE)
    tx, ty = m[:, 0] / np.float32(TILE), m[:, 1] / np.float32(TILE)

    def clamp(v, hi):  # fminf(fmaxf(v, 0), hi): a NaN gives 0
        return np.fmin(np.fmax(v, np.float32(0)), np.float32(hi)).astype(np.int64)
    x0, x1 = clamp(np.floor(tx - tr), tile_w), clamp(np.ceil(tx + tr), tile_w)
    y0, y1 = clamp(np.floor(ty - tr), tile_h), clamp(np.ceil(ty + tr), tile_h)
    live = r > 0
    x0, x1, y0, y1 = (np.where(live, v, 0) for v in (x0, x1, y0, y1))
    return x0, x1, y0, y1, ((x1 - x0) * (y1 - y0)).astype(np.int32)


def tile_emit(means2d, radii, depths, order, tile_w, tile_h, cap=None, with_tail=False):
    """K6: (ids int64, flat int32).  Gaussians in `order` (None: by index), each emits its rectangle row-major,
    key = tile << 32 | bits(depth).  cap: only the first `cap` entries; with_tail: entries [count, cap) are the sentinel
    (n_tiles << 32, 0)."""
    n = np.asarray(radii).shape[0]
    order = np.arange(n, dtype=np.int64) if order is None else np.asarray(order, np.int64)
    x0, x1, y0, y1, tiles = tile_aabb(means2d, radii, tile_w, tile_h)
    cnt = tiles.astype(np.int64)[order]
    start = np.cumsum(cnt) - cnt
    count = int(cnt.sum())
    gid = np.repeat(order, cnt)
    r = np.arange(count, dtype=np.int64) - np.repeat(start, cnt)
    w = np.maximum(x1 - x0, 1)[gid]
    dy = r // w
    tile = (y0[gid] + dy) * tile_w + x0[gid] + (r - dy * w)
    bits = np.ascontiguousarray(depths, np.float32).view(np.uint32).astype(np.int64)
    ids, flat = (tile << 32) | bits[gid], gid.astype(np.int32)
    if cap is not None:
        ids, flat = ids[:cap], flat[:cap]
        if with_tail and cap > count:
            ids = np.concatenate([ids, np.full(cap - count, (tile_w * tile_h) << 32, np.int64)])
            flat = np.concatenate([flat, np.zeros(cap - count, np.int32)])
    return ids, flat


def sort_pairs(keys, vals, first_bit, nbits):
    """K7: stable sort on (keys >> first_bit) & (2^nbits - 1).  gags_sort_pairs(tile_bits, depth_sorted) is
    (32, max(tile_bits, 1)) when depth_sorted else (0, 32 + tile_bits); the kernel sorts whole 8-bit digits, which is the
    same thing as long as no key bit at or above 32 + tile_bits is set (the ABI's own assumption)."""
    k = np.ascontiguousarray(keys, np.int64).view(np.uint64)
    d = k >> np.uint64(first_bit)
    if nbits < 64:
        d = d & np.uint64((1 << nbits) - 1)
    p = np.argsort(d, kind="stable")
    return k[p].view(np.int64), np.asarray(vals, np.int32)[p]


def sort_args(tile_bits, depth_sorted):
    return (32, max(tile_bits, 1)) if depth_sorted else (0, 32 + tile_bits)


def tile_offsets(sorted_ids, n_tiles):
    """K8: n_tiles + 1 entries: first sorted index of each tile; the last one = the count (where sentinel keys begin)."""
    t = np.ascontiguousarray(sorted_ids, np.int64).view(np.uint64) >> np.uint64(32)
    return np.searchsorted(t, np.arange(n_tiles + 1, dtype=np.uint64), "left").astype(np.int32)


def trim_lists(offsets, need, flat):
    """(offsets_out [n_tiles + 1], flat_out): every tile's list cut to its first need[t] entries."""
    offsets, need = np.asarray(offsets, np.int64), np.asarray(need, np.int64)
    off_new = np.concatenate([[0], np.cumsum(need)])
    src = np.repeat(offsets[:-1] - off_new[:-1], need) + np.arange(int(off_new[-1]), dtype=np.int64)
    return off_new.astype(np.int32), np.asarray(flat, np.int32)[src]


def trim_last_ids(width, height, offsets, offsets_trimmed, alphas, last_ids):
    """last_ids of the trimmed lists as indices of the full lists; pixels with alpha == 0 keep their value."""
    tile_w = (width + TILE - 1) // TILE
    i, j = np.divmod(np.arange(width * height, dtype=np.int64), width)
    t = (i // TILE) * tile_w + j // TILE
    shift = (np.asarray(offsets, np.int64) - np.asarray(offsets_trimmed, np.int64))[t].reshape(height, width)
    last = np.asarray(last_ids, np.int64).reshape(height, width)
    return np.where(np.asarray(alphas, np.float32).reshape(height, width) > 0, last + shift, last).astype(np.int32)


def chain_depth_sorted(means2d, radii, depths, tile_w, tile_h):
    """Chain A of INTEGRATION.md: depth_order -> cumsum over order -> emit(order) -> sort on the tile bits -> offsets."""
    n_tiles = tile_w * tile_h
    tile_bits = max(1, n_tiles.bit_length())
    order = depth_order(depths)
    ids, flat = tile_emit(means2d, radii, depths, order, tile_w, tile_h)
    ids_s, flat_s = sort_pairs(ids, flat, *sort_args(tile_bits, 1))
    return ids_s, flat_s, tile_offsets(ids_s, n_tiles)


def chain_full_sort(means2d, radii, depths, tile_w, tile_h):
    """Chain B: cumsum -> emit(order = NULL) -> full sort -> offsets."""
    n_tiles = tile_w * tile_h
    tile_bits = max(1, n_tiles.bit_length())
    ids, flat = tile_emit(means2d, radii, depths, None, tile_w, tile_h)
    ids_s, flat_s = sort_pairs(ids, flat, *sort_args(tile_bits, 0))
    return ids_s, flat_s, tile_offsets(ids_s, n_tiles)


# ---- input generators (seeded) -----------------------------------------------------------------------------------------
LADDER = (0, 1, 63, 64, 65, 2047, 2048, 2049, 4097, 524_288, 524_289, 1_048_577 + 17)
KEY_DISTS = ("uniform", "equal", "alternating", "sorted", "reversed", "ff00", "straddle", "dupes")


def counts(n, seed=0):
    """Tile counts: uniform in [0, 40), ~30 % zeros."""
    g = np.random.default_rng(seed)
    v = g.integers(1, 40, n).astype(np.int32)
    v[g.random(n) < 0.3] = 0
    return v


def counts_exact_sum(n, total):
    """n entries that sum to `total` exactly, as evenly as possible."""
    q, r = divmod(total, n)
    v = np.full(n, q, np.int32)
    v[:r] += 1
    return v


def depths_mixed(n, seed=0):
    """Uniform positives with ~10 % exact duplicates, and +0.0, -0.0, denormals, +inf, negatives and NaN mixed in."""
    g = np.random.default_rng(seed)
    d = g.uniform(0.01, 100.0, n).astype(np.float32)
    if n > 1:
        dup = g.random(n) < 0.1
        d[dup] = d[g.integers(0, n, int(dup.sum()))]
        special = np.array([0.0, -0.0, 1e-45, 1e-39, -1e-40, np.inf, -np.inf, -1.5, -1e30, np.nan, -np.nan], np.float32)
        k = max(1, n // 50)
        d[g.integers(0, n, k)] = special[g.integers(0, special.size, k)]
    return d


def depths_positive(n, seed=0):
    """Depths of visible Gaussians: positive, ~10 % exact duplicates."""
    g = np.random.default_rng(seed)
    d = g.uniform(0.2, 50.0, n).astype(np.float32)
    dup = g.random(n) < 0.1
    d[dup] = d[g.integers(0, max(n, 1), int(dup.sum()))]
    return d


def sort_keys(n, tile_bits, dist, seed=0, max_tile=None):
    """int64 keys tile << 32 | random low word, no bit at or above 32 + tile_bits set.  The low words are random (NOT in
    depth order), so a tile-bits-only sort must come out as the stable grouping by tile."""
    g = np.random.default_rng(seed)
    top = (1 << tile_bits) if max_tile is None else max_tile + 1
    mask = np.uint64((1 << (32 + tile_bits)) - 1)

    def uni(m):
        return (g.integers(0, top, m, dtype=np.uint64) << np.uint64(32)) | g.integers(0, 1 << 32, m, dtype=np.uint64)
    if dist == "uniform":
        k = uni(n)
    elif dist == "equal":
        k = np.full(n, uni(1)[0], np.uint64)
    elif dist == "alternating":
        k = uni(2)[np.arange(n) & 1]
    elif dist == "sorted":
        k = np.sort(uni(n))
    elif dist == "reversed":
        k = np.sort(uni(n))[::-1].copy()
    elif dist == "ff00":  # every 8-bit digit 0x00 or 0xff (the topmost one cut to the key's width)
        bits = g.integers(0, 2, (n, 8), dtype=np.uint64)
        k = np.zeros(n, np.uint64)
        for b in range(8):
            k |= (bits[:, b] * np.uint64(0xff)) << np.uint64(8 * b)
        k &= mask
    elif dist == "straddle":  # one run of a single key across the first 2048-pair boundary (and every later one it reaches)
        k = uni(n)
        lo, hi = min(n, BLOCK - 600), min(n, BLOCK + 700)
        k[lo:hi] = uni(1)[0]
    elif dist == "dupes":  # few distinct keys: long runs of fully equal keys everywhere
        k = uni(7)[g.integers(0, 7, n)]
    else:
        raise ValueError(dist)
    assert not (k & ~mask).any()
    return k.view(np.int64)


def gaussians_grid(n, tile_w, tile_h, seed=0, max_radius=40, full_cover_run=0):
    """(means2d on a 0.25-pixel grid, integer radii): the tile rectangle is exact in any precision.  Culled Gaussians
    (radius <= 0) at wave lanes 0 and 63 and as whole waves, rectangles clipped to nothing on each side of the screen,
    and (full_cover_run) a run of neighbours that each cover the whole grid."""
    g = np.random.default_rng(seed)
    W, H = tile_w * TILE, tile_h * TILE
    m = np.stack([g.integers(-8 * TILE, 4 * (W + 2 * TILE), n), g.integers(-8 * TILE, 4 * (H + 2 * TILE), n)], 1)
    m = (m.astype(np.float32) * np.float32(0.25))
    r = g.integers(1, max_radius + 1, n).astype(np.int32)
    r[g.random(n) < 0.15] = 0
    r[g.random(n) < 0.02] = -3
    i = np.arange(n)
    r[(i % 64 == 0) & (i % 128 == 0)] = 0          # lane 0 of every other wave
    r[(i % 64 == 63) & (i % 192 >= 128)] = 0       # lane 63 of every third wave
    if n >= 320:
        r[256:320] = 0                              # a whole wave
    if n >= 1100:
        r[1024:1088] = -1
    far = [(-1000.0, H / 2), (W + 1000.0, H / 2), (W / 2, -1000.0), (W / 2, H + 1000.0)]   # radius > 0, nothing on screen
    for k, (x, y) in enumerate(far):
        if n > 8 + k:
            m[5 + k], r[5 + k] = (x, y), 7
    if full_cover_run and n > 100 + full_cover_run:
        m[70:70 + full_cover_run] = (W / 2, H / 2)
        r[70:70 + full_cover_run] = max(W, H)
    return np.ascontiguousarray(m, np.float32), r


def gaussians_float(n, tile_w, tile_h, seed=0, max_radius=40):
    """Random float32 means (not on a grid) and integer radii."""
    g = np.random.default_rng(seed)
    W, H = tile_w * TILE, tile_h * TILE
    m = np.stack([g.uniform(-40, W + 40, n), g.uniform(-40, H + 40, n)], 1).astype(np.float32)
    r = g.integers(0, max_radius + 1, n).astype(np.int32)
    return m, r


def twin_neighbours(means2d, depths, seed=0, share=0.05):
    """~5 % of the Gaussians take their predecessor's centre and depth (in place): wherever both are on screen the two emit
    fully equal (tile, depth) keys, whose order only a stable sort decides."""
    g = np.random.default_rng(seed)
    i = np.flatnonzero(g.random(depths.size) < share)
    i = i[i > 0]
    means2d[i], depths[i] = means2d[i - 1], depths[i - 1]
    return means2d, depths


def sorted_tile_keys(tiles, seed=0):
    """Sorted keys for the given (non-decreasing) tile ids with random low words."""
    g = np.random.default_rng(seed)
    t = np.sort(np.asarray(tiles, np.uint64))
    return np.sort((t << np.uint64(32)) | g.integers(0, 1 << 32, t.size, dtype=np.uint64)).view(np.int64)


def with_sentinels(sorted_ids, n_tiles, k):
    return np.concatenate([sorted_ids, np.full(k, n_tiles << 32, np.int64)])


def random_offsets(n_tiles, seed=0, empty=0.4, max_len=50):
    """offsets [n_tiles + 1] with a share of empty tiles."""
    g = np.random.default_rng(seed)
    ln = g.integers(1, max_len + 1, n_tiles)
    ln[g.random(n_tiles) < empty] = 0
    return np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)


# ---- comparison helpers ------------------------------------------------------------------------------------------------
def assert_same(got, want, what="array"):
    """Exact equality of dtype, shape and every element (bit patterns for floats); reports the first differing index."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype}, expected {want.dtype}"
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    if got.dtype.kind == "f":
        got, want = got.view(f"u{got.dtype.itemsize}"), want.view(f"u{want.dtype.itemsize}")
    bad = np.flatnonzero(got.ravel() != want.ravel())
    if bad.size:
        i = int(bad[0])
        lo, hi = max(i - 2, 0), i + 3
        raise AssertionError(f"{what}: {bad.size} of {got.size} entries differ, first at index {i} (block {i // BLOCK}, "
                             f"offset {i % BLOCK}): got {got.ravel()[lo:hi].tolist()}, expected {want.ravel()[lo:hi].tolist()} "
                             f"(entries {lo}..{hi - 1})")


def assert_pairs_equal(got_keys, got_vals, want_keys, want_vals, what="pairs"):
    """Keys AND values, position by position: equal keys must carry their values in input order (stability)."""
    assert_same(got_keys, want_keys, what + ": keys")
    assert_same(got_vals, want_vals, what + ": values")


def assert_offsets_equal(got, want, what="offsets"):
    assert_same(got, want, what)


def assert_total_equal(got, want, what="total"):
    assert int(got) == int(want), f"{what}: got {int(got)}, expected {int(want)}"


def assert_binning_equal(got, want, what="binning"):
    """(ids_s, flat_s, offsets[n_tiles + 1]) of a whole chain."""
    assert_pairs_equal(got[0], got[1], want[0], want[1], what)
    assert_offsets_equal(got[2], want[2], what + ": offsets")


def assert_guards(buf, lo, hi, sentinel, what="buffer"):
    """buf[:lo] and buf[hi:] (numpy) still hold the prefill."""
    for name, part, base in (("front", buf[:lo], 0), ("back", buf[hi:], hi)):
        bad = np.flatnonzero(part != sentinel)
        assert bad.size == 0, (f"{what}: {name} guard overwritten at buffer index {base + int(bad[0])} "
                               f"(payload is [{lo}, {hi})): {part[bad[0]]}")
