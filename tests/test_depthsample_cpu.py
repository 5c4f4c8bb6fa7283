"""N6 (include/gags_next.h): depth_SAM's point-to-pixel min-depth mapping without a GPU -- the entry points are declared,
exported and typed, every argument check returns its code before anything is launched -- and the fixture
tests/golden/depthsample_vectors.npz (the reference's own depth_SAM.main, make_golden_depthsample.py) pinned to the float32
restatement tests/depthsample_ref.py that the GPU kernels implement."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import depthsample_ref as R  # noqa: E402

Z = np.load(os.path.join(ROOT, "golden", "depthsample_vectors.npz"))
SCENES = ("even", "odd")
N6 = {"gags_depthsample_scratch_bytes", "gags_depthsample_map", "gags_depthsample_scatter"}
EINVAL, ESCRATCH = -1, -3


@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_n6_entries_are_declared_exported_and_typed(lib):
    from gags_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(ROOT), "include", "gags_next.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(gags_depthsample_\w+)\s*\(", src)) == N6
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in N6:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    # vis_thresh crosses as a float (the reference rounds it to fp32), cut_bound as an int, n as 64 bits
    for name in ("gags_depthsample_map", "gags_depthsample_scatter"):
        args = _lib.SIGNATURES[name][1]
        assert args[0] is ctypes.c_int64 and args[8] is ctypes.c_float and args[9] is ctypes.c_int, name


def test_scratch_bytes(lib):
    nb = lib.gags_depthsample_scratch_bytes(1000, 300, 1080, 1920)
    assert nb >= 16 * 1080 * 1920 * 4 + 300 * 64           # winner maps of one 16-camera chunk + camera constants
    assert nb <= (128 << 20) + 300 * 64 + 512                # a chunk's maps stay within the cache budget
    assert lib.gags_depthsample_scratch_bytes(1000, 2, 32, 32) >= 2 * 32 * 32 * 4
    assert lib.gags_depthsample_scratch_bytes(0, 2, 32, 32) == 0
    for bad in ((-1, 2, 32, 32), (10, 0, 32, 32), (10, 2, 0, 32), (10, 2, 32, -1), (10, 2, 1 << 16, 1 << 15), ((1 << 31) - 1, 2, 8, 8)):
        assert lib.gags_depthsample_scratch_bytes(*bad) == 0, bad


def test_map_and_scatter_argument_checks(lib):
    P = ctypes.c_void_p(256)  # never dereferenced: every call below returns before a launch
    nb = lib.gags_depthsample_scratch_bytes(1000, 3, 32, 40)
    fm, fs = lib.gags_depthsample_map, lib.gags_depthsample_scatter
    ok_m = [1000, 3, 32, 40, P, P, P, P, 0.25, 0, P, None, None, P, nb, None]
    ok_s = [1000, 3, 32, 40, P, P, P, P, 0.25, 0, P, P, P, nb, None]

    def call(f, ok, **kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    for f, ok in ((fm, ok_m), (fs, ok_s)):
        assert call(f, ok, a0=-1) == EINVAL                       # negative n
        assert call(f, ok, a0=(1 << 31) - 1) == EINVAL            # point indices are int32
        assert call(f, ok, a1=0) == EINVAL and call(f, ok, a1=-2) == EINVAL
        assert call(f, ok, a2=0) == EINVAL and call(f, ok, a3=0) == EINVAL
        assert call(f, ok, a2=1 << 16, a3=1 << 15) == EINVAL     # h w >= 2^31
        assert call(f, ok, a9=-1) == EINVAL                       # negative cut_bound
    for i in (4, 5, 6, 7, 10, 13):                               # xyz, viewmats, Ks, depths, min_depth, scratch
        assert call(fm, ok_m, **{f"a{i}": None}) == EINVAL, i
    for i in (4, 5, 6, 7, 10, 11, 12):                           # ... min_depth, samples, scratch
        assert call(fs, ok_s, **{f"a{i}": None}) == EINVAL, i
    assert call(fm, ok_m, a14=nb - 1) == ESCRATCH
    assert call(fs, ok_s, a13=nb - 1) == ESCRATCH
    assert fm(0, 3, 32, 40, None, None, None, None, 0.25, 0, None, None, None, None, 0, None) == 0  # n == 0: a no-op


def test_restatement_equals_the_reference():
    """The reference's own depth_SAM.main (single-threaded torch) == the float32 restatement, bit for bit."""
    for s in SCENES:
        ref = R.depth_sample(Z[f"{s}_xyz"], Z[f"{s}_viewmats"], Z[f"{s}_Ks"], Z[f"{s}_depths"])
        assert np.array_equal(ref["mapping"], Z[f"{s}_mapping"]), s
        assert np.array_equal(ref["visible"], Z[f"{s}_visible"]), s
        assert np.array_equal(ref["min_depth"], Z[f"{s}_min_depth"]), s
        assert np.array_equal(ref["samples"], Z[f"{s}_samples"]), s
        assert np.isinf(Z[f"{s}_min_depth"]).any() and np.isfinite(Z[f"{s}_min_depth"]).any()


def test_fixture_margin_property():
    """Under the random-pose cameras no point lies in the band where the reference's BLAS summation order could change a
    decision; the axis-aligned cameras hold exact ties instead (u = k + 0.5, |d - zc| = 0.25 d)."""
    ties = 0
    for s in SCENES:
        xyz, vm, K, D = Z[f"{s}_xyz"], Z[f"{s}_viewmats"], Z[f"{s}_Ks"], Z[f"{s}_depths"]
        for c in range(D.shape[0]):
            vis64, _, _, band = R.decide64(xyz, vm[c], K[c], D[c])
            if Z[f"{s}_exact"][c]:
                assert np.array_equal(vm[c][:3, :3], np.eye(3, dtype=np.float32)) and K[c][0, 0] == 32.0
                ties += int(band.sum())
            else:
                assert not band.any(), (s, c)
                assert np.array_equal(vis64, Z[f"{s}_visible"][:, c]), (s, c)
    assert ties > 50
    assert Z["odd_depths"].shape[1] % 2 == 1 and Z["odd_depths"].shape[2] % 2 == 1


def test_cpu_tensors_and_mismatches_raise():
    from gags_amd import depthsample as DS
    x, vm, K, D = torch.zeros(4, 3), torch.eye(4)[None], torch.eye(3)[None], torch.ones(1, 8, 8)
    for fn in (DS.point_pixel_mapping, DS.point_min_depth, DS.depth_samples):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(x, vm, K, D)
    if torch.cuda.is_available():  # shape checks run after the device check
        x, vm, K, D = x.cuda(), vm.cuda(), K.cuda(), D.cuda()
        for bad in ((x[:, :2], vm, K, D), (x, vm.repeat(2, 1, 1), K, D), (x, vm, K[:, :2], D), (x, vm, K, D[0])):
            with pytest.raises(ValueError):
                DS.point_min_depth(*bad)

    class Cam:
        def __init__(self, w, h):
            self.FoVx = self.FoVy = 1.0
            self.image_width, self.image_height = w, h
            self.world_view_transform = torch.eye(4)
    with pytest.raises(ValueError, match="differ in size"):
        DS.camera_matrices([Cam(32, 24), Cam(32, 25)], device="cpu")
    vm, K, hw = DS.camera_matrices([Cam(33, 24), Cam(33, 24)], device="cpu")
    assert hw == (24, 33) and K[0, 0, 2] == 16.5 and K[0, 1, 2] == 12.0 and vm.shape == (2, 4, 4)
    with pytest.raises(ValueError):
        DS.camera_matrices([])


def test_depth_files_pair_by_name(tmp_path):
    """img1 / img10: the sorted file list (img10_depth.npy < img1_depth.npy) and the sorted names (img1 < img10) disagree;
    load_rendered_depths pairs by name, and save_depth_samples writes <name>_depth_sample.npy."""
    from gags_amd import depthsample as DS
    names = ["img1", "img10", "img2"]
    for k, nm in enumerate(names):
        np.save(tmp_path / f"{nm}_depth.npy", np.full((3, 4), k, np.float32))
    assert sorted(os.listdir(tmp_path))[0] == "img10_depth.npy"
    d = DS.load_rendered_depths(str(tmp_path), names, device="cpu")
    assert [float(d[k, 0, 0]) for k in range(3)] == [0.0, 1.0, 2.0]
    with pytest.raises(FileNotFoundError):
        DS.load_rendered_depths(str(tmp_path), ["img3"], device="cpu")
    np.save(tmp_path / "odd_depth.npy", np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError):
        DS.load_rendered_depths(str(tmp_path), ["img1", "odd"], device="cpu")
    out = tmp_path / "samples"
    paths = DS.save_depth_samples(str(out), names, d, min_depth=torch.arange(3.0))
    assert [os.path.basename(p) for p in paths] == [f"{nm}_depth_sample.npy" for nm in names] + ["pcd_depth.npy"]
    for k, nm in enumerate(names):
        a = np.load(out / f"{nm}_depth_sample.npy")
        assert a.dtype == np.float32 and a.shape == (3, 4) and (a == k).all()
    with pytest.raises(ValueError):
        DS.save_depth_samples(str(out), names[:2], d)
