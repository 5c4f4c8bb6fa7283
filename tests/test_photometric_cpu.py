"""N7 (include/gags_next.h): the photometric loss of the RGB stage without a GPU -- the float64 restatement
tests/photometric_ref.py against the reference's own results (tests/golden/photometric_vectors.npz, written by
make_golden_photometric.py), the window table, what the fixture stores, the entry points' declarations and argument checks,
the workgroup count, and the Python layer's refusals."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import photometric_ref as R  # noqa: E402

Z = np.load(os.path.join(ROOT, "golden", "photometric_vectors.npz"))
SHAPES = [(3, 5, 7), (3, 16, 16), (3, 33, 17), (3, 47, 63), (1, 64, 48), (2, 3, 20, 24)]
KINDS = ("near", "rand", "flat")
CASES = [k + "_" + "x".join(map(str, s)) for k in KINDS for s in SHAPES]
N7 = {"gags_photometric_partials", "gags_photometric_fwd", "gags_photometric_bwd"}
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_fixture_holds_every_case():
    assert {k[:-2] for k in Z.files if k.endswith("_x")} == set(CASES)
    assert os.path.getsize(os.path.join(ROOT, "golden", "photometric_vectors.npz")) <= 1 << 20
    for name in CASES:
        assert Z[name + "_x"].dtype == np.float32 and Z[name + "_y"].dtype == np.float32
        assert Z[name + "_grad64"].dtype == np.float64 and Z[name + "_grad32"].dtype == np.float32
        if name.startswith("near"):  # pixels exactly on the target: sign(0)
            assert int((Z[name + "_x"] == Z[name + "_y"]).sum()) >= 3


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference_in_float64(name):
    x, y = torch.from_numpy(Z[name + "_x"]), torch.from_numpy(Z[name + "_y"])
    loss, grad = R.value_and_grad(R.photometric_loss, x, y, 0.2)
    assert abs(float(loss) - float(Z[name + "_loss64"])) <= 1e-12
    assert float(np.abs(grad.numpy() - Z[name + "_grad64"]).max()) <= 1e-12
    assert abs(float(R.ssim(x, y)) - float(Z[name + "_ssim64"])) <= 1e-12
    assert abs(float(R.l1_loss(x, y)) - float(Z[name + "_l164"])) <= 1e-12
    p = R.psnr(x, y).numpy()
    assert p.shape == Z[name + "_psnr64"].shape == (x.shape[0], 1)
    assert float(np.abs(p - Z[name + "_psnr64"]).max()) <= 1e-12
    if x.dim() == 4:
        assert float(np.abs(R.ssim(x, y, size_average=False).numpy() - Z[name + "_ssimb64"]).max()) <= 1e-12


def test_window_table_is_the_references_bit_for_bit():
    from gags_amd import losses
    assert Z["window"].dtype == np.float32 and Z["window"].shape == (11,)
    assert len(losses.SSIM_WINDOW) == 11
    mine = np.array(losses.SSIM_WINDOW, dtype=np.float64)
    assert np.array_equal(mine.astype(np.float32).astype(np.float64), mine)   # every entry IS a float32 value
    assert np.array_equal(mine.astype(np.float32).view(np.uint32), Z["window"].view(np.uint32))
    assert np.array_equal(np.frombuffer(losses._WINDOW_C, dtype=np.uint32), Z["window"].view(np.uint32))  # what is launched
    assert np.array_equal(R.window_1d().numpy().view(np.uint32), Z["window"].view(np.uint32))
    assert float(Z["window"].astype(np.float64).sum()) != 1.0                 # and nothing renormalises them


def test_stored_float32_distances_and_floors():
    """What the fixture stores about the reference's own float32 run: the orders of magnitude seen when it was written (value
    up to ~1e-7 and gradient 2e-7 .. 2e-6 on near / rand; the cancellation of E[x^2] - mu^2 on `flat`: ~1e-4 on the gradient),
    and the two floors recomputed from the stored arrays."""
    fv = fg = 0.0
    for name in CASES:
        dv = max(abs(float(Z[f"{name}_{k}32"]) - float(Z[f"{name}_{k}64"])) for k in ("ssim", "l1", "loss"))
        dg = float(np.abs(Z[name + "_grad32"].astype(np.float64) - Z[name + "_grad64"]).max() / np.abs(Z[name + "_grad64"]).max())
        if name.startswith("flat"):
            assert dv < 2e-5 and dg < 1e-3, (name, dv, dg)
        else:
            assert dv < 1e-6 and 1e-8 < dg < 5e-6, (name, dv, dg)
            fv, fg = max(fv, dv), max(fg, dg)
    assert float(Z["floor_value"]) == fv and float(Z["floor_grad"]) == fg
    worst_flat = max(float(np.abs(Z[n + "_grad32"].astype(np.float64) - Z[n + "_grad64"]).max() / np.abs(Z[n + "_grad64"]).max())
                     for n in CASES if n.startswith("flat"))
    assert worst_flat > 10 * fg  # the cancellation is in the fixture


def test_n7_entries_are_declared_exported_and_typed(lib):
    from gags_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(ROOT), "include", "gags_next.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(gags_photometric_\w+)\s*\(", src)) == N7
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in N7:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    fwd, bwd = _lib.SIGNATURES["gags_photometric_fwd"][1], _lib.SIGNATURES["gags_photometric_bwd"][1]
    assert len(fwd) == 24 and len(bwd) == 20
    for args in (fwd, bwd):  # strides cross as 64-bit element counts
        assert all(args[i] is ctypes.c_int64 for i in (5, 6, 7, 9, 10, 11))
    assert fwd[13:16] == [ctypes.c_double] * 3
    assert lib.gags_abi_version() == 2


def test_partials_count(lib):
    n = lib.gags_photometric_partials
    assert n(1, 16, 32) == 1                                   # one tile (32 columns x 16 rows)
    assert n(1, 16, 33) == 2 and n(1, 17, 32) == 2 and n(1, 17, 33) == 4   # one tile plus one pixel
    assert n(3, 5, 7) == 3                                     # an image smaller than the window: one tile per plane
    assert n(3, 1080, 1920) == 3 * 68 * 60
    assert n(6, 131, 197) == 6 * 9 * 7
    for bad in ((0, 8, 8), (-1, 8, 8), (3, 0, 8), (3, 8, -2), (1 << 16, 8, 8)):
        assert n(*bad) == 0, bad


def test_argument_checks_return_einval_without_launching(lib):
    P = ctypes.c_void_p(256)  # never dereferenced: every call below returns before a launch
    W = (ctypes.c_float * 11)(*([0.0] * 11))
    ok_f = [3, 1, 8, 9, P, 72, 9, 1, P, 72, 9, 1, W, 0.2, 0.8, -0.2, 1, P, None, P, P, P, P, None]
    ok_b = [3, 1, 8, 9, P, 72, 9, 1, P, 72, 9, 1, W, P, P, P, 72, 9, 1, None]

    def call(f, ok, **kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    for f, ok in ((lib.gags_photometric_fwd, ok_f), (lib.gags_photometric_bwd, ok_b)):
        for i in (0, 1, 2, 3):
            assert call(f, ok, **{f"a{i}": 0}) == EINVAL, i           # non-positive sizes
            assert call(f, ok, **{f"a{i}": -4}) == EINVAL, i
        assert call(f, ok, a1=2) == EINVAL                             # 3 planes are not 2 images
        assert call(f, ok, a0=1 << 16) == EINVAL
        for i in (4, 8, 12):
            assert call(f, ok, **{f"a{i}": None}) == EINVAL, i         # x, y, window
        for i in (5, 6, 7, 9, 10, 11):
            assert call(f, ok, **{f"a{i}": -1}) == EINVAL, i           # negative strides
    assert call(lib.gags_photometric_fwd, ok_f, a19=None) == EINVAL    # partials
    assert call(lib.gags_photometric_fwd, ok_f, a20=None) == EINVAL    # sums
    assert call(lib.gags_photometric_bwd, ok_b, a13=None) == EINVAL    # a backward without the forward's dm maps
    assert call(lib.gags_photometric_bwd, ok_b, a14=None) == EINVAL    # coef
    assert call(lib.gags_photometric_bwd, ok_b, a15=None) == EINVAL    # v_x
    assert call(lib.gags_photometric_bwd, ok_b, a17=-9) == EINVAL


def test_python_layer_refusals():
    from gags_amd import losses
    x, y = torch.rand(3, 12, 12), torch.rand(3, 12, 12)
    with pytest.raises(NotImplementedError):
        losses.ssim(x, y, window_size=7)
    for call in (lambda: losses.ssim(x, y), lambda: losses.photometric_loss(x, y), lambda: losses.psnr(x, y),
                 lambda: losses.ssim(x, y, size_average=False)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
