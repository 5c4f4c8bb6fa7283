"""N16 without a GPU: the float64 restatement of the antialiased compensation and of absgrad (tests/aa_ref.py) against closed
forms, the backward's analytic partials against autograd and central differences, the route and flag words with absgrad, the
new C entries, and the argument errors of rasterization()."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import aa_ref
from gags_amd import _lib as L
from gags_amd import rasterization as R
from test_route_cpu import ALL, CASES, COL, NONE

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
F64 = torch.float64


def test_compensation_closed_form_for_an_isotropic_splat_facing_the_camera():
    """Identity pose, the mean on the optical axis, fx = fy = f: cov2d = (f sigma / z)^2 I, so comp = s2 / (s2 + eps2d)."""
    f, z, eps = 50.0, 4.0, 0.3
    sig = torch.tensor([0.002, 0.01, 0.05, 0.3, 2.0], dtype=F64)
    n = sig.shape[0]
    means = torch.tensor([[0.0, 0.0, z]], dtype=F64).repeat(n, 1)
    quats = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=F64).repeat(n, 1)
    K = torch.tensor([[f, 0, 32.0], [0, f, 24.0], [0, 0, 1]], dtype=F64)
    _, _, _, comp = aa_ref.project(means, quats, sig[:, None].repeat(1, 3), torch.eye(4, dtype=F64), K, 64, 48, eps2d=eps)
    s2 = (f * sig / z) ** 2
    assert torch.allclose(comp, s2 / (s2 + eps), rtol=1e-13, atol=0)
    assert comp[0] < 0.01 and comp[-1] > 0.999   # sub-pixel splats are dimmed, large ones are not
    culled = aa_ref.project(means, quats, sig[:, None].repeat(1, 3), torch.eye(4, dtype=F64), K, 64, 48, eps2d=eps,
                            radii=np.array([0, 3, 0, 5, 9]))[3]
    assert culled[0] == 0 and culled[2] == 0 and torch.equal(culled[[1, 3, 4]], comp[[1, 3, 4]])


def test_compensation_partials_against_autograd_and_central_differences():
    g = torch.Generator().manual_seed(5)
    A = torch.randn(64, 2, 2, generator=g, dtype=F64)
    S = A @ A.transpose(1, 2) * torch.logspace(-3, 2, 64, dtype=F64)[:, None, None]   # SPD, from sub-pixel to large
    eps = 0.3
    s = [S[:, 0, 0].clone().requires_grad_(), S[:, 0, 1].clone().requires_grad_(), S[:, 1, 1].clone().requires_grad_()]
    comp = aa_ref.compensation(*s, eps)
    v = torch.randn(64, generator=g, dtype=F64)
    (comp * v).sum().backward()
    r, d00, d11, d01 = aa_ref.compensation_partials(*[t.detach() for t in s], eps)
    assert torch.allclose(comp.detach(), r.sqrt(), rtol=1e-14)
    v_r = v / (2 * comp.detach())
    for got, part in ((s[0].grad, d00), (s[1].grad, d01), (s[2].grad, d11)):
        assert torch.allclose(got, v_r * part, rtol=1e-10, atol=1e-300)
    for i, part in ((0, d00), (1, d01), (2, d11)):   # central differences of r itself
        h = 1e-6 * S[:, 0, 0].clamp(min=S[:, 1, 1])
        hi = [t.detach().clone() for t in s]
        lo = [t.detach().clone() for t in s]
        hi[i] += h
        lo[i] -= h
        fd = (aa_ref.compensation(*hi, eps) ** 2 - aa_ref.compensation(*lo, eps) ** 2) / (2 * h)
        assert torch.allclose(fd, part, rtol=1e-6, atol=1e-9 * part.abs().max()), i


def one_gaussian(centre=(8.0, 8.0), conic=(0.05, 0.01, 0.08), opacity=0.8):
    """One Gaussian on a 16x16 image, D = 3: inputs of aa_ref.composite (float64 leaves) and a uniform cotangent."""
    m2 = torch.tensor([centre], dtype=F64, requires_grad=True)
    con = torch.tensor([conic], dtype=F64)
    op = torch.tensor([opacity], dtype=F64)
    col = torch.tensor([[0.9, 0.2, 0.5]], dtype=F64)
    bg = torch.tensor([0.1, 0.3, 0.2], dtype=F64)
    return m2, con, op, col, bg


def hand_absgrad(centre, conic, opacity, col, bg, v_out, v_alpha, w=16, h=16):
    """(signed, absolute) sums over pixels of d loss / d (dx, dy), by hand: alpha = o exp(-sigma), loss' = kappa = <v, c - bg> + v_a."""
    a, b, c = conic
    kappa = float(np.dot(v_out, np.asarray(col) - np.asarray(bg)) + v_alpha)
    sg, ab = np.zeros(2), np.zeros(2)
    for i in range(h):
        for j in range(w):
            dx, dy = centre[0] - (j + 0.5), centre[1] - (i + 0.5)
            sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
            alpha = opacity * np.exp(-sigma)
            if alpha < 1.0 / 255.0 or alpha > 0.999:
                continue
            g = np.array([-alpha * kappa * (a * dx + b * dy), -alpha * kappa * (b * dx + c * dy)])
            sg += g
            ab += np.abs(g)
    return sg, ab


def test_absgrad_restatement_against_a_hand_sum():
    m2, con, op, col, bg = one_gaussian()
    out, alphas, aux = aa_ref.composite(m2, con, op, col, bg, 16, 16, np.array([40]), np.array([0]))
    v_out, v_alpha = np.array([0.7, -0.4, 1.1]), 0.35
    ((out * torch.tensor(v_out)).sum() + (alphas * v_alpha).sum()).backward()
    got = aa_ref.absgrad_of(aux, 1)[0].numpy()
    sg, ab = hand_absgrad((8.0, 8.0), con[0].tolist(), 0.8, col[0].tolist(), bg.tolist(), v_out, v_alpha)
    assert aux["n_blend"] > 100
    np.testing.assert_allclose(got, ab, rtol=1e-12)
    np.testing.assert_allclose(m2.grad[0].numpy(), sg, rtol=0, atol=1e-12 * ab.max())
    # centred on the pixel-grid centre the signed gradient cancels; the absolute one does not
    assert np.all(np.abs(m2.grad[0].numpy()) < 1e-12 * got) and np.all(got > 0.1)


# -- the route ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,bwd", [(3, "valu"), (16, "staged+geom"), (20, "valu"), (24, "staged+geom"), (128, "staged+geom")])
def test_route_with_absgrad(d, bwd):
    off, on = R._route(300, d, False, ALL, 0, False), R._route(300, d, False, ALL, 0, False, absgrad=True)
    assert on.bwd == bwd and on.absgrad and not off.absgrad and on == off._replace(absgrad=True)
    R._check_absgrad_route(on, d)
    assert R._fwd_flags(on) == R._fwd_flags(off) and R._bwd_flags(on) == R._bwd_flags(off)
    assert R._stage_bits(on.flags, on.half) == R._stage_bits(off.flags, off.half)
    if bwd == "staged+geom":
        assert R._geom_flags(on) == R._geom_flags(off) | L.GAGS_GEOM_ABSGRAD and not (R._geom_flags(off) & L.GAGS_GEOM_ABSGRAD)
        f32 = R._route(300, d, False, ALL, L.GAGS_BWD_F32MFMA, False, absgrad=True)
        assert R._geom_flags(f32) == L.GAGS_RECS_BY_GAUSSIAN | L.GAGS_GEOM_F32MFMA | L.GAGS_GEOM_ABSGRAD


def test_route_carries_absgrad_only_where_a_geometry_gradient_is_produced():
    for needs in (NONE, COL, (False,) * 4 + (True,)):
        for d in (3, 16, 128, 513):
            assert not R._route(300, d, False, needs, 0, False, absgrad=True).absgrad
    for d in (36, 513, 1028):   # the VALU route above one channel chunk: refused
        r = R._route(300, d, False, ALL, 0, False, absgrad=True)
        assert r.bwd == "valu" and r.absgrad
        with pytest.raises(NotImplementedError, match="absgrad"):
            R._check_absgrad_route(r, d)
        R._check_absgrad_route(r._replace(absgrad=False), d)
    late = R._route(300, 128, False, ALL, 0, False, absgrad=True).without_scratch()   # the scratch-free fallback at wide D
    assert late.bwd == "valu" and late.absgrad
    with pytest.raises(NotImplementedError):
        R._check_absgrad_route(late, 128)
    R._check_absgrad_route(R._route(300, 24, False, ALL, 0, False, absgrad=True).without_scratch(), 24)


@pytest.mark.parametrize("name", list(CASES))
def test_existing_route_table_is_reproduced_with_absgrad_off(name):
    got, want, words = CASES[name]
    if words is None:
        return
    assert got == want and got.absgrad is False
    if got.bwd == "staged+geom":
        assert not (R._geom_flags(got) & L.GAGS_GEOM_ABSGRAD)
    # the same inputs with the keyword spelled out
    assert R._Route(**got._asdict()) == got and got._replace(absgrad=False) == want


# -- the ABI ----------------------------------------------------------------------------------------------------------------------

NEW_ENTRIES = ("gags_project_fwd_aa", "gags_project_bwd_aa", "gags_project_fwd_raw_aa", "gags_project_bwd_raw_aa",
               "gags_raster_bwd_abs")


def test_new_flag_is_a_distinct_single_bit_and_equals_the_header():
    src = open(os.path.join(ROOT, "include", "gags_raster.h")).read()
    m = re.findall(r"^#define\s+GAGS_GEOM_ABSGRAD\s+(0x[0-9a-fA-F]+|\d+)\b", src, flags=re.M)
    assert len(m) == 1
    v = int(m[0], 0)
    assert v == L.GAGS_GEOM_ABSGRAD and v > 0 and v & (v - 1) == 0
    assert v not in (L.GAGS_GEOM_F32MFMA, L.GAGS_RECS_BY_GAUSSIAN)


def test_new_entries_are_declared_typed_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gags_raster.h")).read(), flags=re.S)
    if not os.path.exists(L.LIB_PATH):
        L.build()
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.SIGNATURES and hasattr(raw, name), name
    assert lib.gags_abi_version() == 2
    # the old signatures are what they were (one more argument each in the new ones)
    for old, new, extra in (("gags_project_fwd", "gags_project_fwd_aa", 1), ("gags_project_fwd_raw", "gags_project_fwd_raw_aa", 1),
                            ("gags_project_bwd_raw", "gags_project_bwd_raw_aa", 0), ("gags_raster_bwd", "gags_raster_bwd_abs", 1)):
        assert len(L.SIGNATURES[new][1]) == len(L.SIGNATURES[old][1]) + extra
    # argument validation, no launch: NULLs, and absgrad above one channel chunk
    assert lib.gags_project_fwd_aa(-1, *([None] * 5), 16, 16, 0.3, 0.01, 1e10, 0.0, *([None] * 6), None) == -1
    assert lib.gags_project_fwd_aa(8, *([None] * 5), 16, 16, 0.3, 0.01, 1e10, 0.0, *([None] * 6), None) == -1
    assert lib.gags_project_fwd_raw_aa(8, *([None] * 4), 1.0, None, None, 16, 16, 0.3, 0.01, 1e10, 0.0, *([None] * 10), None) == -1
    assert lib.gags_project_bwd_aa(8, *([None] * 5), 16, 16, 0.3, *([None] * 8), None) == -1
    assert lib.gags_project_bwd_raw_aa(8, *([None] * 4), 1.0, None, None, 16, 16, 0.3, *([None] * 9), None) == -1
    assert lib.gags_project_fwd_aa(0, *([None] * 5), 16, 16, 0.3, 0.01, 1e10, 0.0, *([None] * 6), None) == 0   # n = 0: no launch
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p(ctypes.addressof(buf))
    args = lambda d, v_abs, flags=0: (d, 16, 16, *([P] * 7), 1, None, *([P] * 2), P, None, *([P] * 4), v_abs, flags, None)
    assert lib.gags_raster_bwd_abs(*args(36, P)) == -1
    assert lib.gags_raster_bwd_abs(*args(33, P)) == -1
    assert lib.gags_raster_bwd_abs(*args(16, P, L.GAGS_BWD_COLORS_ONLY)) == -1
    assert lib.gags_raster_bwd_abs(*args(16, P)[:10], 0, *args(16, P)[11:]) == 0   # no intersection: nothing to do


# -- rasterization()'s arguments ---------------------------------------------------------------------------------------------------

def _cpu_call(d=3, grad=False, **kw):
    n = 4
    t = lambda *s: torch.rand(*s).requires_grad_(grad)
    return R.rasterization(t(n, 3), t(n, 4), t(n, 3), t(n), t(n, d), torch.eye(4)[None], torch.eye(3)[None], 16, 16, **kw)


def test_argument_errors():
    with pytest.raises(ValueError, match="rasterize_mode"):
        _cpu_call(rasterize_mode="mip")
    with pytest.raises(ValueError, match="absgrad"):
        _cpu_call(absgrad=1)
    for kw in (dict(rasterize_mode="antialiased"), dict(absgrad=True), dict(rasterize_mode="antialiased", absgrad=True, grad=True)):
        with pytest.raises(RuntimeError, match="GPU"):   # accepted options; there is no CPU path
            _cpu_call(**kw)
    with pytest.raises(NotImplementedError, match="absgrad"):   # decided from plain values, before any tensor is touched
        _cpu_call(d=36, grad=True, absgrad=True)
    with pytest.raises(RuntimeError, match="GPU"):   # D = 36 without geometry gradients: nothing to refuse
        _cpu_call(d=36, absgrad=True)


def test_densify_reads_absgrad_and_says_when_it_is_missing():
    from gags_amd import densify
    vp = torch.zeros(1, 4, 2, requires_grad=True)
    with pytest.raises(RuntimeError, match="absgrad"):
        densify.viewspace_gradient(vp, absgrad=True)
    with pytest.raises(RuntimeError, match="absgrad"):
        densify.accumulate(object(), dict(viewspace_points=vp, render=torch.zeros(3, 8, 8), radii=None), absgrad=True)
    vp.absgrad = torch.ones(1, 4, 2)
    assert densify.viewspace_gradient(vp, absgrad=True) is vp.absgrad
    with pytest.raises(RuntimeError, match="no gradient"):
        densify.viewspace_gradient(vp)
