"""Restatement of the N9 contract (include/gags_next.h: gags_knn3_dist2) and the builders of the clouds its tests run on.

    dist2_f32(x)   brute force with the contract's exact float32 expression: d2 = (dx*dx + dy*dy) + dz*dz, dx = x_j - x_i,
                   the three smallest values over j != i, ((b0 + b1) + b2) / 3 -- numpy never contracts into an FMA
    dist2_f64(x)   the same from the same float32 coordinates in float64
    CASES / cloud(name)   seeded inputs, shared by tests/test_knn_cpu.py and tests/test_knn_gpu.py; never touches the reference

The clouds are the smallest at which the traversal of csrc/knn.hip can still go wrong (see CASES); B is its box size."""
import functools

import numpy as np

from gags_amd.knn import BOX as B  # the box size of csrc/knn.hip: the sizes around it are where the traversal changes path


def _three_smallest(d2):
    """rows of d2 [m, n] -> the three smallest values of each row, ascending."""
    return np.sort(np.partition(d2, 2, axis=1)[:, :3], axis=1)


def _brute(x, dtype, chunk=512):
    x = np.ascontiguousarray(np.asarray(x, np.float32)).astype(dtype)
    n = x.shape[0]
    assert x.ndim == 2 and x.shape[1] == 3 and n >= 4
    out = np.empty(n, dtype)
    three = dtype(3.0)
    for s in range(0, n, chunk):
        q = x[s:s + chunk]
        dx = x[None, :, 0] - q[:, None, 0]
        dy = x[None, :, 1] - q[:, None, 1]
        dz = x[None, :, 2] - q[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == dtype
        d2[np.arange(q.shape[0]), s + np.arange(q.shape[0])] = np.inf  # j != i, by index
        b = _three_smallest(d2)
        out[s:s + chunk] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / three
    return out


def dist2_f32(x):
    return _brute(x, np.float32)


def dist2_f64(x):
    return _brute(x, np.float64)


def _uniform(n, seed):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


def _lattice():
    g = np.arange(7, dtype=np.float32) * np.float32(0.25)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def _two_clusters(n_each=500, seed=21):
    rng = np.random.default_rng(seed)
    tight = rng.normal(0.0, 1e-3, (n_each, 3))
    loose = 50.0 + rng.normal(0.0, 1.0, (n_each, 3))
    outlier = np.array([[1e3, -1e3, 5e2]])
    triple = 20.0 + np.array([[0.0, 0.0, 0.0], [1e-4, 0.0, 0.0], [0.0, 1e-4, 0.0]])
    return np.concatenate([tight, loose, outlier, triple]).astype(np.float32)


def two_clusters_scaled(n, seed=21):
    """The two_clusters recipe at about n points (tools/knn_bench.py): half tight, half loose, the outlier and the triple."""
    return _two_clusters((n - 4) // 2, seed)


def _offset():
    return (1e4 + 1e-2 * np.random.default_rng(31).random((300, 3))).astype(np.float32)


def _plane():
    x = _uniform(200, 41)
    x[:, 1] = np.float32(0.75)
    return x


def _line():
    x = _uniform(100, 43)
    x[:, 0] = np.float32(-2.0)
    x[:, 2] = np.float32(3.5)
    return x


def _duplicates():
    x = np.repeat(_uniform(64, 51), 4, axis=0)
    return x[np.random.default_rng(52).permutation(x.shape[0])]


def _presorted():
    x = _uniform(1025, 7)
    return np.ascontiguousarray(x[np.argsort(x[:, 0], kind="stable")])


# name -> builder.  What each catches:
_BUILDERS = {
    "min4": lambda: _uniform(4, 1),                # fewer candidates than the seed window
    "min5": lambda: _uniform(5, 2),
    "wave63": lambda: _uniform(63, 3),             # a partial last wave
    "wave64": lambda: _uniform(64, 4),
    "wave65": lambda: _uniform(65, 5),
    "box_m1": lambda: _uniform(B - 1, 11),         # a partial last box, box boundaries
    "box": lambda: _uniform(B, 12),
    "box_p1": lambda: _uniform(B + 1, 13),
    "box_4p1": lambda: _uniform(4 * B + 1, 14),
    "uniform": lambda: _uniform(1025, 7),          # the general case
    "lattice": _lattice,                           # 7^3 at pitch 0.25: many exact ties at the third-best
    "two_clusters": _two_clusters,                 # the triple's third neighbour is across a gap; the outlier scans everything
    "offset": _offset,                             # cancellation; Morton quantisation with a tiny extent
    "plane": _plane,                               # zero extent on one axis
    "line": _line,                                 # ... on two
    "duplicates": _duplicates,                     # dist2 exactly 0; identical Morton keys
    "presorted": _presorted,                       # the scatter to input order
    "reversed": lambda: np.ascontiguousarray(_presorted()[::-1]),
}
CASES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def _case(name):
    x = np.ascontiguousarray(_BUILDERS[name](), np.float32)
    r32, r64 = dist2_f32(x), dist2_f64(x)
    for a in (x, r32, r64):
        a.setflags(write=False)
    return x, r32, r64


def cloud(name):
    """[N, 3] float32, read-only."""
    return _case(name)[0]


def expected(name):
    """(float32 restatement, float64 restatement) of the case, computed once per process and read-only."""
    return _case(name)[1:]
