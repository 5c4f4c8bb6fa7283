"""N12 without a GPU: the float32 restatement of the contract (tests/queryvis_ref.py) against the images the reference's own
activate_stream produced (tests/golden/make_golden_queryvis.py -> queryvis_vectors.npz), the identity that spares the lerf
composite a reduction, the shipped colour table, and the argument validation of the C entry points."""
import ctypes
import os

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import queryvis_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "queryvis_vectors.npz"))
F = np.float32


def max_heat(case):
    return Z[f"qv{case}_heat"].reshape(Z[f"qv{case}_heat"].shape[0], -1).max(1)


@pytest.mark.parametrize("case", [1, 2])
def test_reference_restatement_reproduces_the_golden_images_bit_for_bit(case):
    pre = f"qv{case}_"
    hm, lerf, mc = R.query_images(Z[pre + "heat"], Z[pre + "output"], Z[pre + "mask"], Z[pre + "avg2"], max_heat(case),
                                  Z[pre + "image"][None], Z["qv_lut"])
    np.testing.assert_array_equal(hm, Z[pre + "heatmap"])
    np.testing.assert_array_equal(lerf, Z[pre + "lerf_composited"])
    np.testing.assert_array_equal(mc, Z[pre + "mask_composited"])
    # every branch of the composites is exercised by the fixture
    assert 0.05 < (Z[pre + "heat"] < 0.5).mean() < 0.95 and 0.05 < Z[pre + "mask"].mean() < 0.95


@pytest.mark.parametrize("case", [1, 2])
def test_pmax_from_the_stats_is_the_reference_max_on_the_fixture(case):
    heat = Z[f"qv{case}_heat"]
    p, pmax, _ = R.lerf_q(heat, max_heat(case))
    np.testing.assert_array_equal(pmax, p.reshape(p.shape[0], -1).max(1))
    np.testing.assert_array_equal(pmax, Z[f"qv{case}_pmax"])


@settings(max_examples=200, deadline=None)
@given(st.lists(st.floats(width=32, allow_nan=False, allow_infinity=True), min_size=1, max_size=64))
def test_pmax_identity_holds_for_any_map(values):
    """x -> clip(fl(x - 0.5), 0, 1) is monotone non-decreasing in float32 (a correctly rounded subtraction of a constant is, and
    so is clip), so it commutes with max: clip(max heat - 0.5) == max clip(heat - 0.5), bit for bit."""
    heat = np.array(values, F).reshape(1, 1, -1)
    p, pmax, _ = R.lerf_q(heat, heat.reshape(1, -1).max(1))
    assert pmax[0] == p.max()


def test_fixture_keeps_the_excluded_set_small():
    for case in (1, 2):
        pre = f"qv{case}_"
        e = R.edge_sets(Z[pre + "heat"], Z[pre + "output"], Z[pre + "avg2"], max_heat(case), float(Z["qv_thresh"]))
        assert e["B"].mean() <= 0.02
        np.testing.assert_allclose(e["B"].mean(), Z["qv_edge_share"][case - 1], rtol=0, atol=1e-12)


def test_shipped_lut_is_matplotlibs_turbo():
    from gags_amd import queryvis
    lut = queryvis.turbo_lut_host()
    assert lut.shape == (256, 3) and lut.dtype == np.float32
    np.testing.assert_array_equal(lut, Z["qv_lut"])
    matplotlib = pytest.importorskip("matplotlib")
    np.testing.assert_array_equal(lut, np.asarray(matplotlib.colormaps["turbo"].colors, np.float64).astype(np.float32))


def test_uint8_rule():
    x = np.array([-1.0, 0.0, 0.6 / 255, 0.4 / 255, 0.5, 1.0, 2.0, 254.4 / 255, 254.6 / 255, np.nan], F)
    with np.errstate(invalid="ignore"):
        got = R.to_uint8(x)
    np.testing.assert_array_equal(got[:-1], np.array([0, 0, 1, 0, 128, 255, 255, 254, 255], np.uint8))


def test_loss_map_restatement_is_within_the_references_own_error():
    for case in (1, 2):
        pre = f"lm{case}_"
        got = R.feature_loss_maps(Z[pre + "feature_f16"].astype(F), Z[pre + "gt"], Z[pre + "mask"])
        for g, name in zip(got, ("l2", "mean_abs_pred", "mean_abs_gt")):
            want = Z[pre + name + "_f64"]
            bound = max(float(Z[pre + name + "_err_ref"]), float(np.spacing(F(want.max()))))
            assert np.abs(g.astype(np.float64) - want).max() <= bound, (case, name)


@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_argument_validation_returns_codes_without_launching(lib):
    buf = ctypes.create_string_buffer(256)
    P = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL, ESCRATCH = -1, -3
    assert lib.gags_strerror(ESCRATCH) not in (b"ok", b"unknown error")

    def images(m=6, f=2, h=8, w=8, box=30, nb=0, **null):
        a = dict(heat=P, output=P, mask=P, stats=P, image=P, lut=P, avg2=P, o0=P, o1=P, o2=P, u0=None, u1=None, u2=None, scratch=P)
        a.update(null)
        return lib.gags_query_images(m, f, h, w, a["heat"], a["output"], a["mask"], a["stats"], a["image"], a["lut"], box, a["avg2"],
                                     a["o0"], a["o1"], a["o2"], a["u0"], a["u1"], a["u2"], a["scratch"], nb, None)
    assert images() == ESCRATCH                      # valid arguments, scratch_bytes = 0: nothing is launched
    assert lib.gags_query_images_scratch_bytes(6, 8, 8) >= 6 * 8 * 8 * 8
    assert lib.gags_query_images_scratch_bytes(0, 8, 8) == 0
    for name in ("heat", "output", "mask", "stats", "image", "lut", "avg2", "o0", "o1", "o2", "scratch"):
        assert images(**{name: None}) == EINVAL, name
    assert images(u0=P) == EINVAL                    # the 8-bit outputs come as three or none
    assert images(u0=P, u1=P, u2=P) == ESCRATCH
    assert images(m=-1) == EINVAL and images(h=0) == EINVAL and images(w=0) == EINVAL and images(f=0) == EINVAL
    assert images(m=6, f=4) == EINVAL                # M % F != 0
    assert images(box=0) == EINVAL and images(box=1025) == EINVAL
    assert images(box=1) == ESCRATCH and images(box=1024) == ESCRATCH
    assert images(m=0) == 0                          # no maps: a no-op
    assert images(m=0, heat=None, scratch=None) == 0

    def colour(m=6, f=2, h=8, w=8, **null):
        a = dict(heat=P, output=P, mask=P, avg2=P, stats=P, image=P, lut=P, o0=P, o1=P, o2=P)
        a.update(null)
        return lib.gags_query_colour(m, f, h, w, a["heat"], a["output"], a["mask"], a["avg2"], a["stats"], a["image"], a["lut"],
                                     a["o0"], a["o1"], a["o2"], None, None, None, None)
    for name in ("heat", "output", "mask", "avg2", "stats", "image", "lut", "o0", "o1", "o2"):
        assert colour(**{name: None}) == EINVAL, name
    assert colour(m=6, f=4) == EINVAL and colour(h=-3) == EINVAL and colour(m=0) == 0

    def loss(c=16, n=64, lf=0, lg=1, **null):
        a = dict(f=P, g=P, mask=P, l2=P, mf=P, mg=P)
        a.update(null)
        return lib.gags_feature_loss_maps(c, n, a["f"], lf, a["g"], lg, a["mask"], a["l2"], a["mf"], a["mg"], None)
    for name in ("f", "g", "mask", "l2", "mf", "mg"):
        assert loss(**{name: None}) == EINVAL, name
    assert loss(c=0) == EINVAL and loss(n=-1) == EINVAL and loss(lf=2) == EINVAL and loss(lg=-1) == EINVAL
    assert loss(n=0) == 0


def test_cpu_tensors_are_rejected_not_rerouted():
    import torch
    from gags_amd import queryvis
    with pytest.raises(RuntimeError, match="no CPU path"):
        queryvis.query_images(torch.zeros(1, 8, 8), torch.zeros(8, 8, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        queryvis.feature_loss_maps(torch.zeros(16, 4, 4), torch.zeros(16, 4, 4), torch.ones(4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        queryvis.turbo_lut("cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        queryvis.query_view(torch.zeros(16, 4, 4), None, None, torch.zeros(4, 4, 3))
