"""N5 (include/gags_next.h): the 3-D query's C ABI without a GPU -- the entry points are declared, exported and typed, and
every argument check returns its code before anything is launched -- and the fixture tests/golden/pcd_query_vectors.npz
(the reference's own smooth_pcd_mask / pcd_relvancy, tests/golden/make_golden_pcd.py) pinned to the float64 rule the GPU
kernel implements."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "pcd_query_vectors.npz"))
PARAMS = [(0.05, 20), (0.1, 10), (0.0625, 4)]  # make_golden_pcd.PARAMS
CLOUDS = ("lattice", "blobs", "dups")
N5 = {"gags_point_relevancy_mask_scratch_bytes", "gags_point_relevancy_mask", "gags_point_mask_smooth_scratch_bytes",
      "gags_point_mask_smooth"}
EINVAL, ESCRATCH = -1, -3


@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_n5_entries_are_declared_exported_and_typed(lib):
    from gags_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gags_next.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gags_point_\w+)\s*\(", src))
    assert declared == N5
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in N5:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    # radius crosses the ABI as a double (r*r is formed in float64, as scipy does), rel_thresh as a float
    assert _lib.SIGNATURES["gags_point_mask_smooth"][1][4] is ctypes.c_double
    assert _lib.SIGNATURES["gags_point_relevancy_mask"][1][3] is ctypes.c_float


def test_relevancy_mask_argument_checks(lib):
    P = ctypes.c_void_p(256)  # never dereferenced: every call below returns before a launch
    nb = lib.gags_point_relevancy_mask_scratch_bytes(3, 1000)
    assert nb >= 3 * 2 * 4
    assert lib.gags_point_relevancy_mask_scratch_bytes(0, 1000) == 0 and lib.gags_point_relevancy_mask_scratch_bytes(3, 0) == 0
    f = lib.gags_point_relevancy_mask
    assert f(3, -1, P, 0.4, P, P, P, nb, None) == EINVAL
    assert f(-1, 10, P, 0.4, P, P, P, nb, None) == EINVAL
    assert f(65536, 10, P, 0.4, P, P, P, 1 << 40, None) == EINVAL
    for i in (2, 4, 5, 6):
        args = [3, 1000, P, 0.4, P, P, P, nb, None]
        args[i] = None
        assert f(*args) == EINVAL, i
    assert f(3, 1000, P, 0.4, P, P, P, nb - 1, None) == ESCRATCH
    assert f(3, 0, None, 0.4, None, None, None, 0, None) == 0  # n == 0: a no-op
    assert f(0, 1000, None, 0.4, None, None, None, 0, None) == 0


def test_mask_smooth_argument_checks(lib):
    P = ctypes.c_void_p(256)
    nb = lib.gags_point_mask_smooth_scratch_bytes(2, 1000)
    assert nb >= 2 * 1000 * (8 + 8 + 4 + 12)  # keys in / sorted, sources, gathered coordinates
    assert lib.gags_point_mask_smooth_scratch_bytes(2, 0) == 0 and lib.gags_point_mask_smooth_scratch_bytes(0, 10) == 0
    assert lib.gags_point_mask_smooth_scratch_bytes(2, 1 << 30) == 0  # K n >= 2^31: not served
    f = lib.gags_point_mask_smooth
    ok = [2, 1000, P, P, 0.05, 20, P, None, P, nb, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    assert call(a1=-1) == EINVAL                                   # negative n
    assert call(a0=-1) == EINVAL and call(a0=65535) == EINVAL      # mask count
    for r in (0.0, -0.05, float("nan"), float("inf")):            # radius must be finite and positive
        assert call(a4=r) == EINVAL, r
    assert call(a5=-1) == EINVAL                                   # negative threshold
    for i in (2, 3, 6, 8):                                         # null xyz, mask, out, scratch with n > 0
        assert call(**{f"a{i}": None}) == EINVAL, i
    assert call(a9=nb - 1) == ESCRATCH
    assert call(a0=2, a1=1 << 30, a9=1 << 62) == EINVAL            # K n = 2^31: past the radix sort's range
    assert f(2, 0, None, None, 0.05, 20, None, None, None, 0, None) == 0  # n == 0: a no-op
    assert f(0, 10, None, None, 0.05, 20, None, None, None, 0, None) == 0


def test_cpu_tensors_are_rejected_not_rerouted():
    from gags_amd import pointquery as PQ
    with pytest.raises(RuntimeError, match="no CPU path"):
        PQ.smooth_point_mask(torch.zeros(4, dtype=torch.bool), torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        PQ.recolor_dc(torch.zeros(4, 3), torch.zeros(4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU path"):
        PQ.query_points(torch.zeros(4, 16), torch.zeros(4, 3), None, None)
    with pytest.raises(NotImplementedError, match="colormap"):
        PQ.recolor_dc(torch.zeros(4, 3), torch.zeros(4, dtype=torch.bool), mask_color="rel")
    with pytest.raises(ValueError):
        PQ.recolor_dc(torch.zeros(4, 3), torch.zeros(4, dtype=torch.bool), bg_color="white")


def brute_counts(xyz, masks, r):
    x = xyz.astype(np.float64)
    d = x[:, None, :] - x[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    within = d2 <= r * r
    return np.stack([within[:, m].sum(1) for m in masks])


@pytest.mark.parametrize("cloud", CLOUDS)
def test_fixture_follows_the_float64_rule(cloud):
    """Guard on the fixture: the reference's KD-tree smoothing equals c > threshold or (mask and c >= 10) with the float64
    brute-force count, on every cloud and parameter set (the generator asserts the same when it runs)."""
    xyz, masks = Z[f"{cloud}_xyz"], Z[f"{cloud}_mask"]
    for p, (r, thr) in enumerate(PARAMS):
        c = brute_counts(xyz, masks, r)
        assert np.array_equal(c, Z[f"{cloud}_p{p}_count"])
        assert np.array_equal((c > thr) | (masks & (c >= 10)), Z[f"{cloud}_p{p}_out"])


def test_fixture_end_to_end_case_is_well_separated():
    rel, nrm, raw, sm = Z["e2e_relevancy"], Z["e2e_normalized"], Z["e2e_mask_raw"], Z["e2e_mask"]
    thr = float(Z["e2e_rel_thresh"])
    assert np.array_equal(raw, nrm > np.float32(thr))
    assert (np.abs(nrm - thr).min(1) > 5e-3).all()
    assert ((rel.max(1) - rel.min(1)) >= 0.4).all()
    c = brute_counts(Z["e2e_xyz"], raw, 0.05)
    assert np.array_equal(sm, (c > 20) | (raw & (c >= 10)))
    assert (sm & ~raw).any() and (raw & ~sm).any()  # the vote both adds and removes points
