"""N24 (include/gags_next.h): the bilateral grid without a GPU -- the tent form of tests/bilagrid_ref.py against
torch.nn.functional.grid_sample in float64 and against central differences, the identity grid, the TV closed forms, the
construction of the GPU test's inputs, the entry points' declarations and argument checks, and the refusals of the Python
layer and of render()."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import bilagrid_ref as R  # noqa: E402

N24 = {"gags_bilagrid_scratch_bytes", "gags_bilagrid_slice_fwd", "gags_bilagrid_slice_bwd", "gags_bilagrid_tv_partials",
       "gags_bilagrid_tv_fwd", "gags_bilagrid_tv_bwd"}
EINVAL, ESCRATCH = -1, -3
IMAGES = [(1, 1), (3, 5), (5, 7)]
GRIDS = [(2, 2, 2), (4, 3, 5), (8, 16, 16)]  # (L, Gh, Gw): 2x2x2, 5x3x4 (Gw=5, Gh=3, L=4), 16x16x8


@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _case(h, w, L, gh, gw, force=None):
    rgb = R.make_image(h, w, L, seed=7 * h + w, force=force).double()
    grid = R.make_grid(L, gh, gw, seed=L + gh + gw).double()
    v_out = R.make_cotangent(h, w, seed=h + w).double()
    return grid, rgb, v_out


@pytest.mark.parametrize("L,gh,gw", GRIDS)
@pytest.mark.parametrize("h,w", IMAGES)
def test_tent_form_equals_grid_sample_in_float64(h, w, L, gh, gw):
    forces = (None, "negative", "above", "black") if h * w < 6 else (None,)
    for force in forces:
        grid, rgb, v_out = _case(h, w, L, gh, gw, force)
        kind = R.edge_kind(rgb)
        if h * w >= 6:
            assert {1, 2, 3} <= set(kind.reshape(-1).tolist())   # gray < 0, gray > 1 and exact black are in the image
        elif force is not None:
            assert int(kind[0, 0]) > 0
        out, v_grid, v_rgb = R.value_and_grads(R.slice_grid_sample, grid, rgb, v_out)
        mine = R.slice_tent(grid, rgb)
        my_grid, my_rgb, guide = R.grads_tent(grid, rgb, v_out)
        for name, a, b in (("forward", mine, out), ("v_grid", my_grid, v_grid), ("v_rgb", my_rgb, v_rgb)):
            err = float((a - b).abs().max())
            assert err <= 1e-12, (name, force, err)
        assert bool((guide[kind > 0] == 0).all())               # no guide gradient on the clamped and black pixels ...
        if bool((kind == 0).any()):
            assert float(guide[kind == 0].abs().max()) > 0      # ... and some everywhere else
        # grid_sample agrees: what is left of v_rgb there is the affine part alone
        wx, wy, wz, _, _ = R._weights(grid, rgb)
        A = torch.einsum("clmn,ijl,im,jn->cij", grid, wz, wy, wx).reshape(3, 4, h, w)
        direct = torch.einsum("rcij,ijr->ijc", A[:, :3], v_out)
        assert float((v_rgb - direct)[kind > 0].abs().max() if bool((kind > 0).any()) else 0.0) <= 1e-12


@pytest.mark.parametrize("L,gh,gw", GRIDS)
def test_gradients_equal_central_differences(L, gh, gw):
    """On inputs whose frac(z) lies in [0.05, 0.95] (no edge pixels: the slice is smooth within 0.05 / (L - 1) of each)."""
    h, w = 3, 5
    rgb = R.make_image(h, w, L, seed=3, edges=False).double()
    assert int((R.check_inputs(rgb, L) > 0).sum()) == 0
    grid = R.make_grid(L, gh, gw, seed=11).double()
    v_out = R.make_cotangent(h, w, seed=5).double()
    v_grid, v_rgb, _ = R.grads_tent(grid, rgb, v_out)
    f = lambda g, p: float((R.slice_tent(g, p) * v_out).sum())  # noqa: E731
    eps = 1e-6
    for i in range(h):
        for j in range(w):
            for c in range(3):
                d = torch.zeros_like(rgb)
                d[i, j, c] = eps
                num = (f(grid, rgb + d) - f(grid, rgb - d)) / (2 * eps)
                assert abs(num - float(v_rgb[i, j, c])) <= 1e-7 * max(1.0, abs(num)), (i, j, c)
    gen = torch.Generator().manual_seed(1)
    hit = R.reached(grid.shape, rgb).nonzero()
    picks = [tuple(hit[k].tolist()) for k in torch.randperm(hit.shape[0], generator=gen)[:12].tolist()]
    miss = (~R.reached(grid.shape, rgb)).nonzero()
    picks += [tuple(miss[k].tolist()) for k in range(min(3, miss.shape[0]))]
    for (l, m, n) in picks:
        for ch in (0, 5, 11):
            d = torch.zeros_like(grid)
            d[ch, l, m, n] = eps
            num = (f(grid + d, rgb) - f(grid - d, rgb)) / (2 * eps)
            assert abs(num - float(v_grid[ch, l, m, n])) <= 1e-7 * max(1.0, abs(num)), (ch, l, m, n)


def test_an_identity_grid_returns_the_image():
    from gags_amd.bilagrid import BilateralGrid
    bg = BilateralGrid(2)
    assert tuple(bg.grids.shape) == (2, 12, 8, 16, 16) and bg.grids.dtype == torch.float32 and bg.grids.requires_grad
    assert torch.equal(bg.grids.detach()[1, :, 3, 2, 5].reshape(3, 4), torch.eye(4)[:3])
    assert tuple(BilateralGrid(1, grid_X=5, grid_Y=3, grid_W=4).grids.shape) == (1, 12, 4, 3, 5)
    rgb = R.make_image(5, 7, 8, seed=2).double()
    out = R.slice_tent(bg.grids.detach()[0].double(), rgb)
    assert float((out - rgb).abs().max()) <= 1e-15
    assert float((R.slice_grid_sample(bg.grids.detach()[0].double(), rgb) - rgb).abs().max()) <= 1e-14


def test_inputs_of_the_gpu_test_are_what_they_claim():
    """Every image the GPU test uses satisfies check_inputs by construction, holds the three edge pixels when it has six pixels
    or more, and leaves nodes of the 16x16x8 grid unreached when it is smaller than the grid."""
    for (h, w) in [(1, 1), (1, 2), (3, 5), (17, 33), (70, 130)]:
        for (L, gh, gw) in GRIDS:
            rgb = R.make_image(h, w, L, seed=7 * h + w)
            kind = R.check_inputs(rgb, L)
            assert rgb.dtype == torch.float32
            assert ({1, 2, 3} <= set(kind.reshape(-1).tolist())) == (h * w >= 6)
            hit = R.reached((12, L, gh, gw), rgb.double())
            if (h, w) != (70, 130) and (L, gh, gw) == (8, 16, 16):
                assert int((~hit).sum()) > 0
            if (h, w) == (70, 130):
                assert bool(hit.any(0).all())   # every xy-node is reached
    with pytest.raises(AssertionError):
        R.check_inputs(torch.tensor([[[0.5, 0.5, 0.5]]]), 3)   # gray (L - 1) = 1.0: on a node


def test_tv_closed_forms():
    const = torch.full((3, 12, 4, 5, 6), 0.7, dtype=torch.float64)
    assert float(R.tv_ref(const)) == 0.0
    for d, size in ((2, 4), (3, 5), (4, 6)):
        shape = [1, 1, 1, 1, 1]
        shape[d] = size
        ramp = torch.arange(size, dtype=torch.float64).reshape(shape).expand(3, 12, 4, 5, 6)
        assert abs(float(R.tv_ref(ramp)) - 2.0) <= 1e-14      # every difference along d is 1: (2 / B) B n_d / n_d
    g = torch.randn(2, 12, 3, 4, 5, dtype=torch.float64, requires_grad=True)
    R.tv_ref(g).backward()
    gd = g.detach()
    want = torch.zeros_like(gd)
    b = gd.shape[0]
    for d in (2, 3, 4):
        diff = gd.narrow(d, 1, gd.shape[d] - 1) - gd.narrow(d, 0, gd.shape[d] - 1)
        k = 4.0 / (b * (diff.numel() // b))
        want.narrow(d, 1, gd.shape[d] - 1).add_(k * diff)      # + (g - g[-1])
        want.narrow(d, 0, gd.shape[d] - 1).sub_(k * diff)      # - (g[+1] - g)
    assert float((g.grad - want).abs().max()) <= 1e-14


def test_n24_entries_are_declared_exported_and_typed(lib):
    from gags_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(ROOT), "include", "gags_next.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(gags_bilagrid_\w+)\s*\(", src)) == N24
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in N24:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    fwd, bwd = _lib.SIGNATURES["gags_bilagrid_slice_fwd"][1], _lib.SIGNATURES["gags_bilagrid_slice_bwd"][1]
    assert all(fwd[i] is ctypes.c_int64 for i in (7, 8, 9))                       # strides cross as 64-bit element counts
    assert all(bwd[i] is ctypes.c_int64 for i in (7, 8, 9, 11, 12, 13, 17))
    for name in N24 - {"gags_bilagrid_scratch_bytes", "gags_bilagrid_tv_partials"}:
        assert _lib.SIGNATURES[name][1][-1] is ctypes.c_void_p                      # ... and every launching entry takes a stream
    assert lib.gags_abi_version() == 2


def test_scratch_and_partial_counts(lib):
    import json
    sys.path.insert(0, os.path.join(os.path.dirname(ROOT), "tools"))
    import record_scratch_bytes as rec
    s = lib.gags_bilagrid_scratch_bytes
    assert s(8, 16, 16) == 8 * 12 * 8 * 16 * 16 * 4          # 256 nodes x 8 row chunks = 2048 workgroups
    assert s(2, 2, 2) == 64 * 12 * 2 * 2 * 2 * 4              # (never more than 64 chunks)
    assert s(16, 64, 64) == 1 * 12 * 16 * 64 * 64 * 4         # 4096 nodes: one chunk
    for bad in ((1, 16, 16), (17, 16, 16), (8, 1, 16), (8, 16, 65), (8, 0, 16), (-8, 16, 16)):
        assert s(*bad) == 0, bad
    t = lib.gags_bilagrid_tv_partials
    assert t(1, 2, 2, 2) == 1 and t(1, 8, 16, 16) == 96 and t(100, 8, 16, 16) == 1024
    for bad in ((0, 8, 16, 16), (-1, 8, 16, 16), (1, 1, 16, 16), (1, 8, 16, 65), ((1 << 16) + 1, 8, 16, 16)):
        assert t(*bad) == 0, bad
    # the function's own fixture (tools/record_scratch_bytes.py LATER): every row recorded, none drifted
    name, rows = rec.LATER["gags_bilagrid_scratch_bytes"]
    with open(os.path.join(ROOT, "golden", name)) as f:
        golden = json.load(f)
    assert {tuple(r["args"]) for r in golden} == set(rows) and all(r["fn"] == "gags_bilagrid_scratch_bytes" for r in golden)
    assert [r["value"] for r in golden] == [int(s(*r["args"])) for r in golden]
    assert any(r["value"] > 0 for r in golden) and any(r["value"] == 0 for r in golden)


def test_argument_checks_return_einval_without_launching(lib):
    P = ctypes.c_void_p(256)  # never dereferenced: every call below returns before a launch
    ok_f = [8, 16, 16, 9, 11, P, P, 1, 33, 3, P, None]
    ok_b = [8, 16, 16, 9, 11, P, P, 1, 33, 3, P, 1, 33, 3, P, P, P, 1 << 20, None]
    ok_tf = [2, 8, 16, 16, P, P, P, None]
    ok_tb = [2, 8, 16, 16, P, P, P, None]

    def call(f, ok, **kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    for f, ok in ((lib.gags_bilagrid_slice_fwd, ok_f), (lib.gags_bilagrid_slice_bwd, ok_b)):
        for i, bads in ((0, (1, 0, -8, 17)), (1, (1, 0, -2, 65)), (2, (1, 0, -2, 65)), (3, (0, -1)), (4, (0, -1))):
            for bad in bads:
                assert call(f, ok, **{f"a{i}": bad}) == EINVAL, (i, bad)    # sizes below the minima and above the maxima
        assert call(f, ok, a3=1 << 16, a4=1 << 15) == EINVAL                # more than 2^30 pixels
        for i in (5, 6, 10):
            assert call(f, ok, **{f"a{i}": None}) == EINVAL, i              # grid, rgb, out / v_out
        for i in (7, 8, 9):
            assert call(f, ok, **{f"a{i}": -1}) == EINVAL, i                # negative strides
    b = lib.gags_bilagrid_slice_bwd
    for i in (11, 12, 13):
        assert call(b, ok_b, **{f"a{i}": -3}) == EINVAL, i
    assert call(b, ok_b, a14=None, a15=None) == EINVAL                      # nothing asked for
    assert call(b, ok_b, a16=None) == EINVAL                                # v_grid without a scratch
    assert call(b, ok_b, a17=lib.gags_bilagrid_scratch_bytes(8, 16, 16) - 1) == ESCRATCH
    assert call(b, ok_b, a17=0) == ESCRATCH
    for f, ok in ((lib.gags_bilagrid_tv_fwd, ok_tf), (lib.gags_bilagrid_tv_bwd, ok_tb)):
        for i, bads in ((0, (0, -1, (1 << 16) + 1)), (1, (1, 0, 17)), (2, (1, 65)), (3, (1, 65, -4))):
            for bad in bads:
                assert call(f, ok, **{f"a{i}": bad}) == EINVAL, (i, bad)
        for i in (4, 5, 6):
            assert call(f, ok, **{f"a{i}": None}) == EINVAL, i


def test_python_layer_refusals():
    from gags_amd import bilagrid as B
    grid, rgb = torch.zeros(12, 8, 16, 16), torch.rand(3, 6, 7)
    for bad_grid in (torch.zeros(12, 8, 16), torch.zeros(11, 8, 16, 16), torch.zeros(12, 8, 16, 16, dtype=torch.float64),
                     torch.zeros(12, 1, 16, 16), torch.zeros(12, 17, 16, 16), torch.zeros(12, 8, 65, 16),
                     torch.zeros(2, 12, 8, 16, 16)):
        with pytest.raises(ValueError):
            B.slice(bad_grid, rgb)
    for bad_rgb in (torch.rand(6, 7), torch.rand(4, 6, 7), torch.rand(1, 3, 6, 7), torch.rand(3, 6, 7).double(),
                    torch.rand(3, 6, 7).half(), torch.rand(3, 0, 7)):
        with pytest.raises(ValueError):
            B.slice(grid, bad_rgb)
    for bad_grids in (torch.zeros(12, 8, 16, 16), torch.zeros(2, 11, 8, 16, 16), torch.zeros(2, 12, 8, 16, 16).double(),
                      torch.zeros(0, 12, 8, 16, 16), torch.zeros(2, 12, 1, 16, 16)):
        with pytest.raises(ValueError):
            B.total_variation_loss(bad_grids)
    # well-formed CPU tensors: there is no CPU path
    for call in (lambda: B.slice(grid, rgb), lambda: B.slice(grid, rgb.permute(1, 2, 0)),
                 lambda: B.total_variation_loss(torch.zeros(2, 12, 8, 16, 16)), lambda: B.BilateralGrid(2)(rgb, 1),
                 lambda: B.BilateralGrid(2).tv_loss()):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    bg = B.BilateralGrid(3)
    for idx in (3, -1, 100):
        with pytest.raises(IndexError):
            bg(rgb, idx)
    for kw in (dict(grid_W=1), dict(grid_W=17), dict(grid_X=65), dict(grid_Y=1)):
        with pytest.raises(ValueError):
            B.BilateralGrid(2, **kw)
    with pytest.raises(ValueError):
        B.BilateralGrid(0)


def test_render_refuses_a_grid_on_anything_but_an_rgb_render():
    """Before anything of the scene or the camera is touched: None stands in for both."""
    from gags_amd.bilagrid import BilateralGrid
    from gags_amd.gaussian_renderer import render
    bg = BilateralGrid(1)
    with pytest.raises(ValueError, match="feature_mode"):
        render(None, None, None, None, feature_mode=True, bilateral_grid=bg)
    with pytest.raises(ValueError, match="feature_mode"):
        render(None, None, None, None, bilateral_grid=bg)               # (feature_mode defaults to True)
    for mode in ("RGB+ED", "D", "ED", "RGB+D"):
        with pytest.raises(NotImplementedError):
            render(None, None, None, None, feature_mode=False, render_mode=mode, bilateral_grid=bg)
