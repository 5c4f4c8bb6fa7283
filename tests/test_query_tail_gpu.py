"""The image query tail on the GPU at its kernel edges: gags_relevancy_activate, gags_relevancy, gags_query_images and
gags_query_colour called through the C ABI, every output inside a sentinel-guarded buffer, every input a view at a non-zero
offset of a larger buffer, against tests/query_tail_ref.py.  Grid-valued maps (multiples of 2^-10) make the box sums exact, so
(a), (c) and (e) compare with == ; (b) allows the final rounding of avg one ulp and nothing else; (d) holds relevancy_kernel
to the bound derived from its own summation.  tests/test_query_tail_cpu.py shows that these cases catch a wrong kernel."""
import numpy as np
import pytest
import torch

import query_tail_ref as Q
import queryvis_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
GUARD = 256             # sentinel elements before and after every output
SENT32 = 0x7FDB5A5A     # a NaN: an element the kernel should have written and did not fails every comparison
SENT8 = 0xA5            # neither 0 nor 1


def _sentinel(buf):
    if buf.dtype == torch.float32:
        buf.view(torch.int32).fill_(SENT32)
    else:
        buf.fill_(SENT8)
    return buf


def _guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = _sentinel(torch.empty(GUARD + n + GUARD, dtype=dtype, device="cuda"))
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf):
    raw, sent = (buf.view(torch.int32), SENT32) if buf.dtype == torch.float32 else (buf, SENT8)
    return bool((raw[:GUARD] == sent).all()) and bool((raw[-GUARD:] == sent).all())


def _offset_view(a, off=3):
    """`a` on the device as a view `off` elements into a larger sentinel-filled buffer (12 bytes for floats: no 16-byte alignment)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = _sentinel(torch.empty(off + t.numel() + 5, dtype=t.dtype, device="cuda"))
    view = buf[off:off + t.numel()].view(*t.shape)
    view.copy_(t)
    assert view.data_ptr() != buf.data_ptr() and view.is_contiguous()
    return view


def _scratch(nbytes):
    return _sentinel(torch.empty(int(nbytes) + GUARD, dtype=torch.uint8, device="cuda"))


def _scratch_tail_intact(buf):
    return bool((buf[-GUARD:] == SENT8).all())


def run_activate(valid, thresh, box, scale):
    """One gags_relevancy_activate call -> {name: numpy}; the guards are checked here."""
    from gags_amd import _lib
    from gags_amd._lib import check, ptr
    lib = _lib.load()
    n, h, w = valid.shape
    v = _offset_view(valid)
    got = {name: _guarded((n, h, w), torch.float32) for name in ("avg", "heatmap", "output")}
    got.update({name: _guarded((n, h, w), torch.uint8) for name in ("mask_pred", "mask")})
    got["stats"] = _guarded((n, 3), torch.float32)
    nb = lib.gags_relevancy_activate_scratch_bytes(n, h, w)
    scratch = _scratch(nb)
    check(lib.gags_relevancy_activate(n, h, w, ptr(v), float(thresh), int(box), int(scale), ptr(got["avg"][1]),
                                      ptr(got["heatmap"][1]), ptr(got["output"][1]), ptr(got["mask_pred"][1]),
                                      ptr(got["mask"][1]), ptr(got["stats"][1]), ptr(scratch), nb, _lib.stream()),
          "gags_relevancy_activate")
    torch.cuda.synchronize()
    for name, (buf, _) in got.items():
        assert _guards_intact(buf), f"{name}: written outside its output"
    assert _scratch_tail_intact(scratch), "written past the scratch the library asked for"
    assert torch.equal(v.cpu(), torch.from_numpy(valid)), "the input was modified"
    return {name: view.cpu().numpy() for name, (_, view) in got.items()}


# ---- (a) exact --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", Q.ACT_IDS)
def test_activation_tail_is_exact_on_grid_valued_maps(case_id):
    _, h, w, box, scale, thresh, kind, n = Q.act_case(case_id)
    valid = Q.grid_maps(case_id)
    want = Q.activate_f32(valid, thresh, box, scale)
    got = run_activate(valid, thresh, box, scale)
    for key in Q.ACT_KEYS:
        bad = np.argwhere(got[key] != want[key])
        assert bad.size == 0, f"{case_id} {key}: {len(bad)} differ, first at {bad[0]}: {got[key][tuple(bad[0])]} != {want[key][tuple(bad[0])]}"
    if kind == "constant" or h * w == 1:
        assert not got["output"].any() and not np.isnan(got["output"]).any()


# ---- (b) general float32 maps ---------------------------------------------------------------------------------------------------
def _general_maps(kind, n, h, w):
    g = torch.Generator().manual_seed(h * 1000 + w)
    if kind == "normal":
        return torch.randn(n, h, w, generator=g).numpy()
    base = torch.nn.functional.interpolate(torch.rand(n, 1, 5, 8, generator=g), size=(h, w), mode="bicubic")[:, 0]
    return (base + 0.05 * torch.randn(n, h, w, generator=g)).clamp(0, 1).contiguous().numpy()


@pytest.mark.parametrize("kind", ["normal", "blobs"])
@pytest.mark.parametrize("h,w", [(33, 513), (70, 94)])
def test_activation_tail_on_general_maps(kind, h, w):
    """avg: the kernel's double sums differ from the exact ones by about 2^-53 relative, so only the final rounding to float32
    can fall the other way: one ulp.  Everything after avg is float32 arithmetic on the run's own avg: bit-equal, every pixel."""
    valid = _general_maps(kind, 3, h, w)
    got = run_activate(valid, 0.5, 30, 3)
    exact = Q.box_mean_exact(valid, 30)
    off = np.abs(got["avg"].astype(np.float64) - exact.astype(np.float64))
    print(f"{kind} {h}x{w}: {int((off > 0).sum())} of {off.size} box means are not the rounded exact mean, worst {off.max():.3g}")
    assert (off <= np.spacing(np.abs(exact))).all()
    want = Q.activate_f32(valid, 0.5, 30, 3, avg=got["avg"])
    for key in Q.ACT_KEYS:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert 0 < got["mask_pred"].mean() < 1


# ---- (c) localize, mask_iou --------------------------------------------------------------------------------------------------------
def test_localize_returns_every_position_of_an_exact_tie():
    """A constant plateau against the border: reflection makes neighbouring windows hold the same multiset of pixels, and every
    one of them attains the maximum."""
    from gags_amd.relevancy import localize
    for case_id, box in (("70x94_b31", 30), ("70x94_b31", 31), ("3x5_b30", 3), ("1x257_b64", 64)):
        valid = Q.grid_maps(case_id)
        scores, coords, hits = localize(torch.from_numpy(valid).cuda(), box=box)
        assert hits is None
        avg = Q.box_mean_exact(valid, box)
        for k in range(valid.shape[0]):
            score, want = Q.localize_ref(avg[k])
            assert scores[k].item() == score
            assert len(want) > 1, "the case has no tie"
            np.testing.assert_array_equal(coords[k].cpu().numpy(), want)


def test_localize_single_maximum_and_hit_test():
    from gags_amd.relevancy import localize
    q = np.zeros((2, 40, 60), np.int64)
    q[0, 10:25, 20:35] = 512
    q[0, 17, 27] = 4096       # one pixel that no other window can make up for: a 15 x 15 window centred on it wins alone
    q[1, 5, 50] = 1024
    valid = (q / Q.GRID).astype(F)
    avg = Q.box_mean_exact(valid, 15)
    want = [Q.localize_ref(a)[1] for a in avg]
    assert want[0].tolist() == [[27, 17]]
    x, y = (int(t) for t in want[0][0])
    boxes = [
        [[x + 5, y + 5, x, y]],                       # corners swapped, the coordinate on the box's corner
        [[0, 0, 3, 3]],
    ]
    scores, coords, hits = localize(torch.from_numpy(valid).cuda(), boxes, box=15)
    for k in range(2):
        np.testing.assert_array_equal(coords[k].cpu().numpy(), want[k])
    assert hits == [True, False]
    edge = [[[x - 9, y, x, y + 2]], [[0, 0, 59, 39]]]                 # on the right edge; the whole image
    assert localize(torch.from_numpy(valid).cuda(), edge, box=15)[2] == [True, True]
    miss = [[[x + 1, y, x + 5, y + 5], [x - 5, y + 1, x + 5, y + 5]], [[0, 0, 0, 0]]]   # one pixel off, twice
    assert localize(torch.from_numpy(valid).cuda(), miss, box=15)[2] == [False, False]
    later = [[[0, 0, 1, 1], [x, y, x, y]], [[0, 0, 0, 0]]]           # the second box of a phrase, a single pixel
    assert localize(torch.from_numpy(valid).cuda(), later, box=15)[2] == [True, False]


def test_mask_iou_edges():
    from gags_amd.relevancy import mask_iou
    a = torch.zeros(4, 6, 9, dtype=torch.uint8, device="cuda")
    b = torch.zeros_like(a)
    a[0, :3], b[0, 3:] = 1, 1            # disjoint
    a[1, 1:4, 2:5], b[1, 1:4, 2:5] = 1, 1  # identical
    a[3, :2], b[3, 1:3] = 1, 1           # two rows each, one shared
    iou = mask_iou(a, b).cpu().numpy()
    assert iou[0] == 0.0 and iou[1] == 1.0 and np.isnan(iou[2]) and iou[3] == 9 / 27


# ---- (d) relevancy ---------------------------------------------------------------------------------------------------------------
def run_relevancy(e, p, n):
    from gags_amd import _lib
    from gags_amd._lib import check, ptr
    n_pix, c = e.shape
    ed, pd, nd = _offset_view(e), _offset_view(p), _offset_view(n)
    buf, probs = _guarded((p.shape[0], n_pix, 2), torch.float32)
    check(_lib.load().gags_relevancy(n_pix, c, p.shape[0], n.shape[0], ptr(ed), ptr(pd), ptr(nd), ptr(probs), _lib.stream()),
          "gags_relevancy")
    torch.cuda.synchronize()
    assert _guards_intact(buf), "written outside probs"
    return probs.cpu().numpy()


@pytest.mark.parametrize("case", Q.REL_CASES, ids=Q.rel_id)
def test_relevancy_within_the_derived_bound(case):
    e, p, n = Q.rel_inputs(case)
    got = run_relevancy(e, p, n)
    want, bound = Q.relevancy_f64(e, p, n), Q.relevancy_bound(e, p, n)
    assert not np.isnan(got).any()
    ratio = np.abs(got.astype(np.float64) - want) / bound
    print(f"relevancy {Q.rel_id(case)}: worst err / bound = {ratio[..., 0].max():.3g} (p0), {ratio[..., 1].max():.3g} (p1)")
    assert ratio.max() <= 1.0
    kind = case[4]
    if kind == "zero":
        assert (got == 0.5).all()
    if kind == "big":
        assert (got[..., 0] == 1.0).any() and (got[..., 0] == 0.0).any() and (got[..., 1] == 1.0).any()
    if kind == "dup":  # negative 1 = negative 0: dropping it changes nothing, bit for bit
        np.testing.assert_array_equal(got, run_relevancy(e, p, np.delete(n, 1, 0)))


@pytest.mark.parametrize("n_levels", [1, 3])
def test_get_max_across_layout(n_levels):
    from gags_amd.relevancy import RelevancyHead
    c, h, w = 512, 5, 7
    e, p, n = Q.rel_inputs((c, 257, 3, 4, "unit"))
    sem = e[:n_levels * h * w].reshape(n_levels, h, w, c)
    got = RelevancyHead(torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda()).get_max_across(torch.from_numpy(sem).cuda())
    assert got.shape == (n_levels, 3, h, w) and got.is_contiguous()
    flat = sem.reshape(-1, c)
    want = Q.relevancy_f64(flat, p, n)[..., 0].reshape(3, n_levels, h, w).transpose(1, 0, 2, 3)
    bound = Q.relevancy_bound(flat, p, n)[..., 0].reshape(3, n_levels, h, w).transpose(1, 0, 2, 3)
    assert (np.abs(got.cpu().numpy().astype(np.float64) - want) <= bound).all()
    # and the layout is discriminating: levels and phrases of this input differ by far more than the bound
    assert (np.abs(want[:, 0] - want[:, 1]) > bound[:, 0]).any()
    if n_levels > 1:
        assert (np.abs(want[0] - want[1]) > bound[0]).any()


# ---- (e) query images ------------------------------------------------------------------------------------------------------------
def _lut():
    from gags_amd import queryvis
    return queryvis.turbo_lut_host()


def run_query(entry, heat, output, mask, stats, image, box=None, avg2=None, u8=False):
    """gags_query_images (avg2 None: computed, box given) or gags_query_colour -> dict of numpy arrays."""
    from gags_amd import _lib
    from gags_amd._lib import check, ptr
    lib = _lib.load()
    m, h, w = heat.shape
    f = image.shape[0]
    d = {k: _offset_view(v) for k, v in dict(heat=heat, output=output, mask=mask, stats=stats, image=image, lut=_lut()).items()}
    got = {name: _guarded((m, h, w, 3), torch.float32) for name in ("heatmap", "lerf", "maskc")}
    if u8:
        got.update({name + "_u8": _guarded((m, h, w, 3), torch.uint8) for name in ("heatmap", "lerf", "maskc")})
    u = [ptr(got[name + "_u8"][1]) if u8 else None for name in ("heatmap", "lerf", "maskc")]
    if entry == "images":
        got["avg2"] = _guarded((m, h, w), torch.float32)
        nb = lib.gags_query_images_scratch_bytes(m, h, w)
        scratch = _scratch(nb)
        check(lib.gags_query_images(m, f, h, w, ptr(d["heat"]), ptr(d["output"]), ptr(d["mask"]), ptr(d["stats"]), ptr(d["image"]),
                                    ptr(d["lut"]), int(box), ptr(got["avg2"][1]), ptr(got["heatmap"][1]), ptr(got["lerf"][1]),
                                    ptr(got["maskc"][1]), u[0], u[1], u[2], ptr(scratch), nb, _lib.stream()), "gags_query_images")
    else:
        a2 = _offset_view(avg2)
        check(lib.gags_query_colour(m, f, h, w, ptr(d["heat"]), ptr(d["output"]), ptr(d["mask"]), ptr(a2), ptr(d["stats"]),
                                    ptr(d["image"]), ptr(d["lut"]), ptr(got["heatmap"][1]), ptr(got["lerf"][1]),
                                    ptr(got["maskc"][1]), u[0], u[1], u[2], _lib.stream()), "gags_query_colour")
    torch.cuda.synchronize()
    for name, (buf, _) in got.items():
        assert _guards_intact(buf), f"{name}: written outside its output"
    if entry == "images":
        assert _scratch_tail_intact(scratch)
    return {name: view.cpu().numpy() for name, (_, view) in got.items()}


def _check_images(got, heat, output, mask, avg2, max_heat, image, u8):
    with np.errstate(invalid="ignore"):
        want = dict(zip(("heatmap", "lerf", "maskc"), R.query_images(heat, output, mask, avg2, max_heat, image, _lut())))
        for name, img in want.items():
            assert not np.isnan(img).any()
            np.testing.assert_array_equal(got[name], img, err_msg=name)
            if u8:
                np.testing.assert_array_equal(got[name + "_u8"], R.to_uint8(img), err_msg=name + "_u8")


@pytest.mark.parametrize("case_id,u8", [("1x257_b2", False), ("3x5_b255", True), ("16x257_b31", True), ("33x513_b64", False)])
def test_query_images_box_mean_is_exact(case_id, u8):
    _, h, w, box, _, _, _, m = Q.act_case(case_id)
    rng = np.random.default_rng(h * w + box)
    output = (np.mod(np.rint(Q.grid_maps(case_id).astype(np.float64) * Q.GRID), Q.GRID + 1) / Q.GRID).astype(F)  # on the grid, in [0, 1]
    assert 0.1 < (output > 0).mean() and len(np.unique(output)) > 3 * m
    heat = rng.random((m, h, w), F)
    mask = (rng.random((m, h, w)) < 0.5).astype(np.uint8)
    stats = np.stack([heat.reshape(m, -1).min(1), heat.reshape(m, -1).max(1), np.zeros(m, F)], 1).astype(F)
    image = rng.random((1, h, w, 3), F)
    got = run_query("images", heat, output, mask, stats, image, box=box, u8=u8)
    avg2 = Q.box_mean_exact(output, box)
    np.testing.assert_array_equal(got["avg2"], avg2)
    _check_images(got, heat, output, mask, avg2, stats[:, 1], image, u8)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("hw,n_frames", [(1, 1), (255, 2), (256, 3), (257, 6), (257, 1), (1, 6)])
def test_query_colour_edges(hw, n_frames, u8):
    """The pixel count on both sides of a workgroup, map m reading image m // (6 / n_frames), NaN in each of the three maps (LUT
    index 0, uint8 0) and a heat of exactly 0.5 (the lerf composite takes the colour, not the dimmed image)."""
    m = 6
    rng = np.random.default_rng(hw * 10 + n_frames)
    heat, output, avg2 = (rng.random((m, 1, hw), F) for _ in range(3))
    mask = (rng.random((m, 1, hw)) < 0.5).astype(np.uint8)
    image = rng.random((n_frames, 1, hw, 3), F)
    heat[0, 0, 0] = 0.5
    output[1, 0, 0], heat[2, 0, 0], avg2[3, 0, 0] = np.nan, np.nan, np.nan
    mask[1, 0, 0], mask[3, 0, 0] = 1, 1   # the NaN of output / avg2 reaches the mask composite's LUT
    if hw > 1:
        heat[:, 0, hw // 2] = 0.5
        output[4, 0, -1], heat[4, 0, -1], avg2[4, 0, -1] = np.nan, np.nan, np.nan
        mask[4, 0, -1] = 1
    max_heat = np.where(np.isnan(heat), F(0), heat).reshape(m, -1).max(1)   # (what a max that skips NaN returns; heat >= 0)
    stats = np.stack([np.zeros(m, F), max_heat, np.zeros(m, F)], 1).astype(F)
    got = run_query("colour", heat, output, mask, stats, image, avg2=avg2, u8=u8)
    _check_images(got, heat, output, mask, avg2, max_heat, image, u8)
    lut = _lut()
    np.testing.assert_array_equal(got["heatmap"][1, 0, 0], lut[0])     # NaN output -> LUT index 0
    np.testing.assert_array_equal(got["lerf"][2, 0, 0], lut[0])        # NaN heat: not < 0.5, q is NaN -> index 0
    np.testing.assert_array_equal(got["maskc"][3, 0, 0], lut[0])       # NaN avg2 inside the mask
    assert not np.array_equal(got["lerf"][0, 0, 0], (image[0, 0, 0] * F(0.3)).astype(F))  # heat == 0.5 is coloured
