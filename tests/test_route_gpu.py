"""The route on the kernels: the named cases of tests/test_route_cpu.py through rasterization() on a six-tile view (48 x 32:
every tile and block edge present), with counting spies on the loaded library's raster entries.  Per case: the entries called,
their order relative to the end of the forward, whether `scratch` and `blk_rows` were NULL, and the flag / stage words -- all
against a hand-written expectation; then outputs and gradients against the oracle at the bounds of
test_parity_gpu.py::test_forward_and_colour_grad and ::test_full_backward."""
import warnings

import numpy as np
import pytest
import torch

from helpers import check_forward, rel_l2, scene_arrays, to_dev

pytestmark = pytest.mark.gpu

N, W, H = 300, 48, 32
GRAD_TOL, GEOM_TOL, GSPLAT_ORDER_TOL = 2e-5, 1e-4, 2e-6  # (test_parity_gpu.py)
# an fp16 table's gradient is rounded to fp16 once, on top of the fp32 sums: 2^-11 relative per element, so in rel-L2
F16_GRAD_TOL = GRAD_TOL + 2.0 ** -11
RECS, COLORS_ONLY, NO_MFMA, FEAT_F16, ONLY_W, ONLY_F, PREZEROED = 256, 1, 2, 32, 512, 1024, 128  # (include/gags_raster.h)
END = ("forward returned",)
# name -> (index of `flags` / `stage`, index of blk_rows, index of the forward's scratch) in the entry's argument list
ENTRIES = {"gags_raster_fwd": (19, 18, 16), "gags_bwd_rowmap": (None, 4, 5), "gags_raster_bwd_colors_staged": (15, 7, 10),
           "gags_raster_bwd_geom": (20, 11, 12), "gags_raster_bwd": (20, None, None)}


def _call(name, word=None, blk_rows=None, scratch=None):
    """An expected call: the flag / stage word and whether blk_rows / scratch are passed (True) or NULL (False)."""
    return (name, word, blk_rows, scratch)


def fwd(word, kept=True):
    return _call("gags_raster_fwd", word, kept, kept)


ROWMAP = _call("gags_bwd_rowmap", None, True, True)


def staged(word=0):
    return _call("gags_raster_bwd_colors_staged", word, True, True)


GEOM = _call("gags_raster_bwd_geom", RECS, True, True)


def valu(word):
    return _call("gags_raster_bwd", word)


COL, ALL = "colors", "all"
# name: (d, what requires grad, options, the expected calls)
CASES = {
    "D=3 colours only": (3, COL, {}, [fwd(RECS, False), END, valu(RECS | COLORS_ONLY)]),
    "D=16 no gradient: lean": (16, None, {}, [fwd(RECS, False), END]),
    "D=16 no gradient, profiler on: two launches": (16, None, dict(profiler=True),
                                                    [fwd(RECS | ONLY_W), fwd(RECS | ONLY_F), END]),
    "D=16 colours only: early row map, staged": (16, COL, {}, [fwd(RECS), ROWMAP, END, staged()]),
    "D=24 all gradients: staged + matrix-core geometry": (24, ALL, {}, [fwd(RECS), END, ROWMAP, staged(), GEOM]),
    "D=20 all gradients: VALU backward": (20, ALL, {}, [fwd(RECS), END, valu(RECS)]),
    "D=1028 colours only: no staged backward": (1028, COL, {}, [fwd(RECS), END, valu(RECS | COLORS_ONLY)]),
    "fp16 table D=128": (128, COL, dict(f16=True), [fwd(RECS | FEAT_F16), ROWMAP, END, staged(64)]),
    "fp16 table D=128, GAGS_FWD_NO_MFMA": (128, COL, dict(f16=True, flags="GAGS_FWD_NO_MFMA"),
                                           [fwd(RECS | NO_MFMA, False), END, valu(RECS | NO_MFMA | COLORS_ONLY)]),
    "GAGS_BWD_ATOMIC": (128, COL, dict(flags="GAGS_BWD_ATOMIC"), [fwd(RECS), END, valu(RECS | COLORS_ONLY)]),
    "GAGS_FWD_FUSED": (128, COL, dict(flags="GAGS_FWD_FUSED"), [fwd(RECS, False), END, valu(RECS | COLORS_ONLY)]),
    "capacity_mode: no early row map": (16, COL, dict(capacity_mode=True), [fwd(RECS), END, ROWMAP, staged()]),
    "overlap_zero_fill": (16, COL, dict(zero_fill=True), [fwd(RECS), ROWMAP, END, staged(PREZEROED)]),
    "grad_range_hook set: no zero-fill": (16, COL, dict(zero_fill=True, hook=True), [fwd(RECS), ROWMAP, END, staged()]),
    "n = 0": (16, COL, dict(n=0), [fwd(RECS, False), END, valu(RECS | COLORS_ONLY)]),
    "no intersection: split instead of lean": (16, None, dict(culled=True), [fwd(RECS), END]),
    "no intersection: no early row map": (16, COL, dict(culled=True), [fwd(RECS), END, ROWMAP, staged()]),
    "the scratch does not fit": (128, COL, dict(f16=True, no_scratch=True), [fwd(RECS, False), END, valu(RECS | COLORS_ONLY)]),
    "the scratch does not fit, all gradients": (24, ALL, dict(no_scratch=True), [fwd(RECS, False), END, valu(RECS)]),
}

_ORACLE = {}


def _reference(oracle, d, f16):
    """Scene and oracle results for a width, computed once (all gradients; the colours-only oracles next to them)."""
    key = (d, f16)
    if key not in _ORACLE:
        s = scene_arrays(N, d, W, H, seed=40 + d % 37, view=2, scale_mult=5.0)
        cols = s["colors"].astype(np.float16).astype(np.float32) if f16 else s["colors"]  # (the table's values, widened exactly)
        bg = np.full(d, 0.25, np.float32)
        rng = np.random.default_rng(d)
        v_out, v_alpha = rng.standard_normal((H, W, d)).astype(np.float32), rng.standard_normal((H, W)).astype(np.float32)
        o_out, o_alpha, oi = oracle.rasterization(s["means"], s["quats"], s["scales"], s["opacities"], cols, s["viewmat"], s["K"],
                                                  bg, W, H)
        geo = oracle.raster_bwd(oi["means2d"], oi["conics"], s["opacities"], cols, bg, W, H, oi["isect_offsets"],
                                oi["flatten_ids"], o_alpha, oi["last_ids"], v_out, v_alpha)
        o_vmeans, o_vq, o_vs = oracle.project_bwd(s["means"], s["quats"], s["scales"], s["viewmat"], s["K"], W, H, oi["radii"],
                                                  geo[2], None, geo[3])
        o_vc = oracle.raster_bwd(oi["means2d"], oi["conics"], s["opacities"], cols, bg, W, H, oi["isect_offsets"],
                                 oi["flatten_ids"], o_alpha, oi["last_ids"], v_out, None, colors_only=True)[0]
        o_vf = oracle.raster_bwd_colors_fwdorder(oi["means2d"], oi["conics"], s["opacities"], d, W, H, oi["isect_offsets"],
                                                 oi["flatten_ids"], v_out, N)
        _ORACLE[key] = dict(s=s, cols=cols, bg=bg, v_out=v_out, v_alpha=v_alpha, out=o_out, alpha=o_alpha, vc_all=geo[0],
                            vo=geo[1], vm2=geo[2], vmeans=o_vmeans, vq=o_vq, vs=o_vs, vc=o_vc, vf=o_vf)
    return _ORACLE[key]


@pytest.mark.parametrize("name", list(CASES))
def test_route_on_the_kernels(oracle, monkeypatch, name):
    from gags_amd import _lib, profiler, raster_tunables
    from gags_amd import rasterization as R
    d, wants, opt, expected = CASES[name]
    f16 = opt.get("f16", False)
    ref = _reference(oracle, d, f16)
    s, n = ref["s"], opt.get("n", N)
    means = s["means"].copy()
    if opt.get("culled"):
        means[:, 2] = -5.0  # everything behind the camera: zero intersections
    t = {k: to_dev(v[:n]) for k, v in dict(means=means, quats=s["quats"], scales=s["scales"], opac=s["opacities"],
                                           cols=ref["cols"]).items()}
    if f16:
        t["cols"] = t["cols"].half()
    for k in {None: (), COL: ("cols",), ALL: tuple(t)}[wants]:
        t[k].requires_grad_(True)
    ctx = R.RasterContext(capacity_mode=opt.get("capacity_mode", False), overlap_zero_fill=opt.get("zero_fill", False))
    ctx.early_rowmap, ctx.trim_lists = True, None
    hooked = []
    if opt.get("hook"):
        ctx.grad_range_hook = lambda g, c0, c1: hooked.append((c0, c1))
    if opt.get("zero_fill"):
        monkeypatch.setattr(raster_tunables, "ZERO_FILL_MIN_ELEMS", 0)  # (the fill is worth it from 2^24 elements; here: that it is routed)
    lib = _lib.load()
    if opt.get("no_scratch"):
        monkeypatch.setattr(lib, "gags_raster_fwd_scratch_bytes", lambda *a: 1 << 52)  # "does not fit"
    calls = []

    def spy(entry):
        real, (i_word, i_blk, i_scr) = getattr(lib, entry), ENTRIES[entry]

        def f(*args):
            passed = lambda i: None if i is None else bool(args[i] is not None and args[i].value)  # noqa: E731  (not NULL)
            calls.append((entry, None if i_word is None else args[i_word], passed(i_blk), passed(i_scr)))
            return real(*args)
        return f
    for entry in ENTRIES:
        monkeypatch.setattr(lib, entry, spy(entry))
    flags = getattr(_lib, opt["flags"]) if "flags" in opt else 0
    profiler.enable(bool(opt.get("profiler")))
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out, alphas, info = R.rasterization(t["means"], t["quats"], t["scales"], t["opac"], t["cols"], to_dev(s["viewmat"])[None],
                                                to_dev(s["K"])[None], W, H, backgrounds=to_dev(ref["bg"])[None], raster_flags=flags,
                                                context=ctx)
        calls.append(END)
        if wants is not None:
            if wants == ALL:
                info["means2d"].retain_grad()
            ((out[0] * to_dev(ref["v_out"])).sum() + (alphas[0, ..., 0] * to_dev(ref["v_alpha"])).sum()).backward()
        torch.cuda.synchronize()
    finally:
        profiler.enable(False)
    assert calls == expected
    said = [str(w.message) for w in caught if "gags_amd" in str(w.message)]
    assert (len(said) == 1 and "scratch-free kernels" in said[0]) if opt.get("no_scratch") else not said
    assert hooked == ([(0, d)] if opt.get("hook") else [])

    out, alpha = out[0].detach().cpu().numpy(), alphas[0, ..., 0].detach().cpu().numpy()
    if n == 0 or opt.get("culled"):
        np.testing.assert_array_equal(out, np.broadcast_to(ref["bg"], (H, W, d)))
        np.testing.assert_array_equal(alpha, np.zeros((H, W), np.float32))
        assert info["n_isects"] == 0
        assert wants is None or (t["cols"].grad.shape == (n, d) and float(t["cols"].grad.abs().sum()) == 0.0)
        return
    np.testing.assert_array_equal(alpha, ref["alpha"])
    check_forward(out, ref["out"])
    if wants is None:
        return
    assert t["cols"].grad.dtype == t["cols"].dtype
    g = t["cols"].grad.float().cpu().numpy()
    tol = F16_GRAD_TOL if f16 else GRAD_TOL
    if wants == COL:  # (the alpha cotangent does not reach the colours)
        assert min(rel_l2(g, ref["vc"]), rel_l2(g, ref["vf"])) <= tol
        assert rel_l2(g, ref["vc"]) <= (F16_GRAD_TOL if f16 else GSPLAT_ORDER_TOL)
    else:
        assert rel_l2(g, ref["vc_all"]) <= tol
        assert rel_l2(t["opac"].grad.cpu().numpy(), ref["vo"]) <= GEOM_TOL
        assert rel_l2(info["means2d"].grad[0].cpu().numpy(), ref["vm2"]) <= GEOM_TOL
        assert rel_l2(t["means"].grad.cpu().numpy(), ref["vmeans"]) <= GEOM_TOL
        assert rel_l2(t["quats"].grad.cpu().numpy(), ref["vq"]) <= GEOM_TOL
        assert rel_l2(t["scales"].grad.cpu().numpy(), ref["vs"]) <= GEOM_TOL
