"""No driver writes past the scratch it asked for.

Every binding allocates its scratch through gags_amd._lib.scratch(nbytes, device) with the library's own byte count.  Here
that helper is replaced by one that allocates TAIL more bytes, fills them with 0xA5 and hands out the first nbytes: after
a call the tail must be untouched, and the results must be those of a plain call (bit-equal where the function's own
tests assert repeatability bit for bit, else within the tolerance those tests use).  One call per function, at the smallest
shape that reaches every region of its layout.  The raster drivers run on the scene of tests/test_route_gpu.py (N = 300 on
48 x 32: six tiles, every tile and block edge), each call with a RasterContext of its own so that no kept gradient buffer
links the plain and the guarded call; their paths are asserted deterministic by
test_parity_gpu.py::test_backward_flavours_agree_and_staged_is_deterministic and
::test_wide_geometry_backward_matches_the_valu_kernel_and_is_deterministic, so everything is compared bit for bit.
"""
import pytest
import torch

from helpers import scene_arrays, to_dev

pytestmark = pytest.mark.gpu
TAIL, FILL = 4096, 0xA5


class Guard:
    """Stand-in for _lib.scratch: nbytes (floored at 1, as the helper does) + a sentinel tail; remembers every buffer."""

    def __init__(self):
        self.buffers = []

    def __call__(self, nbytes, device):
        n = max(int(nbytes), 1)
        buf = torch.empty(n + TAIL, dtype=torch.uint8, device=device)
        buf[n:] = FILL
        self.buffers.append((buf, n))
        return buf[:n]

    def tails_intact(self):
        torch.cuda.synchronize()
        return all(bool((buf[n:] == FILL).all()) for buf, n in self.buffers)


def rng(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _knn():
    from gags_amd import knn
    x = torch.randn(300, 3, device="cuda", generator=rng(1))  # two boxes of 256 sorted points
    return lambda: {"dist2": knn.dist2(x)}, {}


def _smooth():
    from gags_amd.pointquery import smooth_point_mask
    xyz = torch.rand(500, 3, device="cuda", generator=rng(2)) * 0.5
    masks = torch.rand(2, 500, device="cuda", generator=rng(3)) < 0.5

    def call():
        out, counts = smooth_point_mask(masks, xyz, radius=0.1, threshold=10, return_counts=True)
        return {"mask": out, "counts": counts}
    return call, {}


def _query_points():
    from gags_amd.decoders import CNN_decoder
    from gags_amd.pointquery import query_points
    from gags_amd.relevancy import RelevancyHead
    torch.manual_seed(4)
    dec = CNN_decoder(16, 512).cuda()
    emb = torch.nn.functional.normalize(torch.randn(6, 512, device="cuda", generator=rng(5)), dim=-1)
    head = RelevancyHead(emb[:2], emb[2:])
    sem = torch.randn(500, 16, device="cuda", generator=rng(6))
    xyz = torch.rand(500, 3, device="cuda", generator=rng(7)) * 0.3
    # tests/test_pcd_query_gpu.py: relevancy <= 1e-4, normalized <= 1e-3, both masks identical
    return lambda: query_points(sem, xyz, dec, head), {"relevancy": 1e-4, "normalized": 1e-3}


def _valid_maps(k, h, w, seed):
    return torch.rand(k, h, w, device="cuda", generator=rng(seed))


def _activate():
    from gags_amd.relevancy import activate_maps
    valid = _valid_maps(2, 9, 11, 8)
    # tests/test_next_gpu.py: avg, heat map and stats <= 1e-6, output <= 5e-6, the majority filter bit-exact
    return lambda: activate_maps(valid, thresh=0.5, box=5), {"avg": 1e-6, "heatmap": 1e-6, "stats": 1e-6, "output": 5e-6}


def _moments():
    from gags_amd import featurevis as fv
    x = torch.randn(16, 12, 13, device="cuda", generator=rng(9))

    def call():
        s, g = fv.feature_moments(x)
        return {"sum": s, "gram": g}
    return call, {}


def _select():
    from gags_amd import featurevis as fv
    v = torch.randn(12 * 13, device="cuda", generator=rng(10))
    return lambda: {"stats": fv.order_statistics(v, [0, 77, 155])}, {}


def _query_images():
    from gags_amd.queryvis import colour_maps
    from gags_amd.relevancy import activate_maps
    act = activate_maps(_valid_maps(3, 8, 9, 11), thresh=0.4, box=5)
    image = torch.rand(8, 9, 3, device="cuda", generator=rng(12))
    return lambda: colour_maps(act, image, box=5, return_uint8=True), {}


def _nms():
    from gags_amd import sam_masks as sm
    masks = torch.rand(5, 17, 19, device="cuda", generator=rng(13)) < 0.4
    scores = torch.rand(5, device="cuda", generator=rng(14))

    def call():
        idx, keep, keeps, zero = sm._nms_device(masks, scores, 0.7, 0.1, 0.2)
        return {"idx": idx, "keep": keep, "keeps": keeps, "zero": zero, "selected": sm.mask_nms(masks, scores)}
    return call, {}


def _depthsample():
    from gags_amd import depthsample as DS
    n, h, w = 1000, 32, 40
    xyz = torch.rand(n, 3, device="cuda", generator=rng(15)) * 2.0 + torch.tensor([-1.0, -1.0, 2.0], device="cuda")  # in front of both
    vm = torch.eye(4, device="cuda").repeat(2, 1, 1)
    vm[1, 0, 3] = 0.25                                         # the second camera a little to the side
    K = torch.tensor([[40.0, 0.0, 20.0], [0.0, 40.0, 16.0], [0.0, 0.0, 1.0]], device="cuda").repeat(2, 1, 1)
    depths = 2.5 + torch.rand(2, h, w, device="cuda", generator=rng(16))

    def call():
        mapping, visible = DS.point_pixel_mapping(xyz, vm, K, depths)
        samples, md = DS.depth_samples(xyz, vm, K, depths, return_min_depth=True)
        return {"mapping": mapping, "visible": visible, "samples": samples, "min_depth": md}
    return call, {}


def _prompts():
    from gags_amd import _lib, prompts as P
    c, h, w, n = 1, 270, 480, 1                                # the smallest shape whose rows are split into slabs
    assert _lib.load().gags_promptgrid_scratch_bytes(c, h, w, n, P.crop_layout(h, w, n)["crop_h"]) > 0
    depths = 1.0 + torch.rand(c, h, w, device="cuda", generator=rng(17))
    samples = depths * (torch.rand(c, h, w, device="cuda", generator=rng(18)) < 0.1)
    return lambda: P.crop_stats(depths, samples, n), {}


def _wgrad_exact():
    from gags_amd import decoders as D
    p, n, k = 777, 64, 16
    dz = torch.randn(p, n, device="cuda", generator=rng(19))
    a1 = torch.randn(p, k, device="cuda", generator=rng(20))

    def call():
        dw, db = D._xwgrad(p, dz, a1, None, n, k)
        return {"dw": dw, "db": db}
    return call, {}


def _raster(d, all_grads, trim):
    """rasterization() + backward on the scene of tests/test_route_gpu.py, a fresh RasterContext per call."""
    from gags_amd.rasterization import RasterContext, rasterization
    n, w, h = 300, 48, 32
    s = scene_arrays(n, d, w, h, seed=40 + d % 37, view=2, scale_mult=5.0)
    names = ("means", "quats", "scales", "opacities", "colors")
    viewmat, K, bg = to_dev(s["viewmat"])[None], to_dev(s["K"])[None], torch.full((1, d), 0.25, device="cuda")
    v_out = torch.randn(h, w, d, device="cuda", generator=rng(21 + d))
    v_alpha = torch.randn(h, w, device="cuda", generator=rng(22 + d))

    def call():
        t = {k: to_dev(s[k]) for k in names}
        for k in (names if all_grads else ("colors",)):
            t[k].requires_grad_(True)
        ctx = RasterContext()
        ctx.early_rowmap, ctx.trim_lists = True, (True if trim else None)
        out, alphas, info = rasterization(*(t[k] for k in names), viewmat, K, w, h, backgrounds=bg, context=ctx)
        if all_grads:
            info["means2d"].retain_grad()
        ((out[0] * v_out).sum() + (alphas[0, ..., 0] * v_alpha).sum()).backward()
        res = {"out": out.detach(), "alphas": alphas.detach(), "last_ids": info["last_ids"], "n_isects": torch.tensor(info["n_isects"])}
        res.update({"v_" + k: t[k].grad for k in names if t[k].grad is not None})
        if all_grads:
            res["v_means2d"] = info["means2d"].grad
        if trim:
            assert info["n_isects_trimmed"] is not None
        return res
    return call, {}


def _raster_colours():  # depth order, scan, sort, forward scratch, early row map, staged scratch
    return _raster(16, False, False)


def _raster_all_grads():  # ... and the geometry scratch
    return _raster(24, True, False)


def _raster_trimmed():  # ... and the trimming scan
    return _raster(16, False, True)


CASES = [_knn, _smooth, _query_points, _activate, _moments, _select, _query_images, _nms, _depthsample, _prompts, _wgrad_exact,
         _raster_colours, _raster_all_grads, _raster_trimmed]


def test_every_driver_stays_inside_the_scratch_it_asked_for(monkeypatch):
    from gags_amd import _lib
    for case in CASES:
        call, tolerance = case()
        plain = call()
        guard = Guard()
        with monkeypatch.context() as m:
            m.setattr(_lib, "scratch", guard)
            guarded = call()
            ok = guard.tails_intact()
        name = case.__name__
        assert guard.buffers, f"{name}: the scratch did not come from _lib.scratch"
        assert ok, f"{name}: bytes past scratch_bytes were written"
        assert plain.keys() == guarded.keys()
        for key, want in plain.items():
            got = guarded[key]
            if key in tolerance:
                err = float((got.double() - want.double()).abs().max())
                print(f"{name}.{key}: max |guarded - plain| = {err:.3e}")
                assert err <= tolerance[key], (name, key, err)
            else:
                assert torch.equal(got, want), (name, key)
