"""Row-selective Adam on the GPU: gags_adam_step_rows and optim.SelectiveAdam against the restatement of
tests/selective_adam_ref.py (the CPU oracle's Adam on the selected rows, the inputs elsewhere).  Every comparison is == on
the bits of parameter, exp_avg and exp_avg_sq; no tolerance anywhere."""
import ctypes
import types

import numpy as np
import pytest
import torch

from helpers import spy_entries
import selective_adam_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ARGS = types.SimpleNamespace(percent_dense=0.01, position_lr_init=0.00016, position_lr_final=0.0000016,
                             position_lr_delay_mult=0.01, position_lr_max_steps=30000, feature_lr=0.0025, opacity_lr=0.05,
                             scaling_lr=0.005, rotation_lr=0.001, semantic_feature_lr=0.001)
ATTR = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling",
            rotation="_rotation", semantic_feature="_semantic_feature")
NS = (1, 2, 63, 64, 65, 257, 1000)
WS = (1, 3, 4, 16, 45, 48, 512, 513)
MASKS = ("null", "all", "none", "alternating", "first", "last", "random")
LR, EPS = 1e-3, 1e-15


def _launch(n_rows, tensors, mask, flags, step):
    """tensors: (param, grad, exp_avg, exp_avg_sq, width, lr) of device tensors; mask: a device uint8 tensor or None."""
    from gags_amd import _lib
    lib = _lib.load()
    descs = [_lib.AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), w, lr, 0.9, 0.999, EPS)
             for p, g, m, v, w, lr in tensors]
    table = (_lib.AdamTensor * len(descs))(*descs)
    with torch.cuda.device(DEV):
        _lib.check(lib.gags_adam_step_rows(n_rows, len(descs), ctypes.cast(table, ctypes.c_void_p), _lib.ptr(mask), flags, step,
                                           _lib.stream(DEV)), "gags_adam_step_rows")


def _flags(skip, bias):
    from gags_amd import _lib
    return (_lib.GAGS_ADAM_SKIP_ZERO_ROWS if skip else 0) | (0 if bias else _lib.GAGS_ADAM_NO_BIAS_CORRECTION)


def _state(n, w, rng):
    f = lambda a: np.asarray(a, np.float32)  # noqa: E731
    return f(rng.standard_normal((n, w))), f(rng.standard_normal((n, w)) * 0.1), f(rng.random((n, w)) * 0.01)


def _mask(kind, n, step, rng):
    """uint8 [n] or None; the set bytes are not all 1 (any non-zero byte selects)."""
    if kind == "null":
        return None
    m = np.zeros(n, np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "alternating":
        m[step % 2::2] = 255
    elif kind == "first":
        m[0] = 2
    elif kind == "last":
        m[-1] = 1
    elif kind == "random":
        m[rng.random(n) < 0.27] = 128
    return m


def _grad(n, w, step, rng):
    """A new gradient: about 40 % of the rows zero, and three special rows -- all -0.0 (zero), zero but a NaN in the last
    element (non-zero), zero but one number in the last element (non-zero; at w = 513 the element past the last full sweep).
    With fewer than three rows the specials take turns over the steps."""
    g = np.asarray(rng.standard_normal((n, w)), np.float32)
    g[rng.random(n) < 0.4] = 0.0
    rows = rng.permutation(n)[:3] if n >= 3 else np.arange(n)
    for j, r in enumerate(rows):
        kind = j if n >= 3 else (step + j) % 3
        g[r] = 0.0
        if kind == 0:
            g[r] = -0.0
        elif kind == 1:
            g[r, -1] = np.nan
        else:
            g[r, -1] = 0.75
    return g


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the kernel against the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", WS)
def test_kernel_equals_the_restatement(oracle, w):
    """Every N x mask kind x zero test on / off x bias correction on / off at this width, three consecutive steps each with a
    new gradient and a new mask.  Widths: 1, 3, 45, 513 take the 4-byte path (3 and 45: lane groups with idle lanes; 513: a wave
    per row, nine sweeps, four of them kept in registers), 4, 16, 48, 512 the 16-byte path (48: 12 of 16 lanes; 512: a wave per
    row, two sweeps).  N: one row, less than / exactly / more than a wave's rows, more than one workgroup."""
    rng = np.random.default_rng(1000 + w)
    seen_skipped = seen_live = 0
    for n in NS:
        p0, m0, v0 = _state(n, w, rng)
        for kind in MASKS:
            for skip in (False, True):
                for bias in (True, False):
                    ref = (p0, m0, v0)
                    p, m, v = _dev(p0), _dev(m0), _dev(v0)
                    for step in (1, 2, 3):
                        g, mask = _grad(n, w, step, rng), _mask(kind, n, step, rng)
                        ref = R.step(oracle, ref[0], g, ref[1], ref[2], LR, mask=mask, skip_zero_rows=skip, bias_correction=bias,
                                     eps=EPS, step=step)
                        gd, md = _dev(g), _dev(mask)
                        _launch(n, [(p, gd, m, v, w, LR)], md, _flags(skip, bias), step)
                        label = f"n={n} w={w} mask={kind} skip={skip} bias={bias} step={step}"
                        for name, got, want in zip(("param", "exp_avg", "exp_avg_sq"), (p, m, v), ref):
                            R.assert_same_bits(got.cpu().numpy(), want, f"{label} {name}")
                        assert torch.equal(gd.cpu().view(torch.int32), torch.from_numpy(g).view(torch.int32)), label  # read-only
                        sel = R.selection(g, mask, skip)
                        seen_skipped += int((~sel).sum())
                        seen_live += int(sel.sum())
    assert seen_skipped > 0 and seen_live > 0


# ----------------------------------------------------------------------------------------------------------------------
# 2. alignment: views at an odd offset, row slices, and the floats around them
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [4, 512])
@pytest.mark.parametrize("skip", [False, True])
def test_views_at_a_one_float_offset_and_row_slices(oracle, w, skip):
    """All four arrays are views one float into a larger buffer (4-byte aligned only: the 4-byte path although w % 4 == 0), then
    a row slice [c0:c1] of 16-byte aligned tables (the 16-byte path on a shifted base).  The buffer's elements before and
    after the view, and the rows outside the slice, are compared on the host with what was uploaded."""
    n, pad = 131, 8
    rng = np.random.default_rng(7 + w)
    p0, m0, v0 = _state(n, w, rng)
    g0 = _grad(n, w, 1, rng)
    mask = _mask("random", n, 1, rng)
    want = R.step(oracle, p0, g0, m0, v0, LR, mask=mask, skip_zero_rows=skip, eps=EPS, step=2)
    guard = np.float32(-7.25)
    bufs, views = [], []
    for a in (p0, g0, m0, v0):
        host = np.full(pad + n * w + pad, guard, np.float32)
        host[pad + 1:pad + 1 + n * w] = a.reshape(-1)
        buf = _dev(host)
        view = buf[pad + 1:pad + 1 + n * w].view(n, w)
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
        bufs.append(buf)
        views.append(view)
    _launch(n, [(views[0], views[1], views[2], views[3], w, LR)], _dev(mask), _flags(skip, True), 2)
    for name, buf, ref in zip(("param", "grad", "exp_avg", "exp_avg_sq"), bufs, (want[0], g0, want[1], want[2])):
        host = buf.cpu().numpy()
        assert (host[:pad + 1] == guard).all() and (host[pad + 1 + n * w:] == guard).all(), f"{name}: guard floats changed"
        R.assert_same_bits(host[pad + 1:pad + 1 + n * w].reshape(n, w), ref, f"offset view, w={w} {name}")
    # a row slice: the entry sees rows c0 .. c1 only
    c0, c1 = 37, 102
    full = [_dev(a) for a in (p0, g0, m0, v0)]
    part = [t[c0:c1] for t in full]
    assert all(t.data_ptr() % 16 == 0 and t.is_contiguous() for t in part)
    _launch(c1 - c0, [(part[0], part[1], part[2], part[3], w, LR)], _dev(mask[c0:c1]), _flags(skip, True), 2)
    inside = np.zeros(n, bool)
    inside[c0:c1] = True
    for name, t, before, after in zip(("param", "exp_avg", "exp_avg_sq"), (full[0], full[2], full[3]), (p0, m0, v0), want):
        R.assert_same_bits(t.cpu().numpy(), np.where(inside[:, None], after, before), f"row slice, w={w} {name}")


# ----------------------------------------------------------------------------------------------------------------------
# 3. one launch, several tensors; 6. the version counter
# ----------------------------------------------------------------------------------------------------------------------
RGB_SHAPES = ((3,), (1, 3), (15, 3), (1,), (3,), (4,), (16,))


def _optimizer(shapes, n, rng, **kw):
    from gags_amd.optim import SelectiveAdam
    params = [torch.nn.Parameter(_dev(np.asarray(rng.standard_normal((n,) + s), np.float32))) for s in shapes]
    groups = [{"params": [p], "lr": 1e-3 * (k + 1), "name": f"t{k}"} for k, p in enumerate(params)]
    return params, SelectiveAdam(groups, lr=0.0, eps=EPS, **kw)


def _host_state(opt, p):
    st = opt.state[p]
    if len(st) == 0:
        z = np.zeros(tuple(p.shape), np.float32)
        return p.detach().cpu().numpy(), z, z.copy()
    return p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()


@pytest.mark.parametrize("count,launches", [(7, 1), (9, 2)])
def test_one_step_of_several_tensors(oracle, count, launches):
    """The seven RGB shapes at N = 1000 with seven learning rates (then nine tensors: two launches): two step(visibility) calls
    equal per-tensor restatements, the entry was called once (twice) per step, and every parameter's version counter moved."""
    n = 1000
    rng = np.random.default_rng(count)
    shapes = (RGB_SHAPES + ((2, 2), (5,)))[:count]
    params, opt = _optimizer(shapes, n, rng)
    for step in (1, 2):
        vis = rng.random(n) < 0.27
        before = [_host_state(opt, p) for p in params]
        grads = [np.asarray(rng.standard_normal(tuple(p.shape)), np.float32) for p in params]
        for p, g in zip(params, grads):
            p.grad = _dev(g)
        versions = [p._version for p in params]
        with spy_entries("gags_adam_step_rows", "gags_adam_step") as calls:
            opt.step(_dev(vis))
        assert [c[0] for c in calls] == ["gags_adam_step_rows"] * launches
        assert sorted(c[1][1] for c in calls) == sorted([min(count, 8), count - 8][:launches])
        for k, (p, g, (p0, m0, v0)) in enumerate(zip(params, grads, before)):
            assert p._version > versions[k], k
            assert int(opt.state[p]["step"].item()) == step
            want = R.step(oracle, p0, g, m0, v0, 1e-3 * (k + 1), mask=vis, eps=EPS, step=step)
            for name, got, ref in zip(("param", "exp_avg", "exp_avg_sq"), _host_state(opt, p), want):
                R.assert_same_bits(got, ref, f"tensor {k} {tuple(p.shape)} step {step} {name}")
        opt.zero_grad(set_to_none=True)


def test_first_dimensions_that_differ(oracle):
    """Without a mask, parameters of different first dimensions (a decoder's weights) are one row each: a dense step.  With a
    mask that is an error, as is a mask of another length."""
    from gags_amd.optim import SelectiveAdam
    rng = np.random.default_rng(3)
    shapes = ((10, 4), (7,), (3, 5, 2))
    params = [torch.nn.Parameter(_dev(np.asarray(rng.standard_normal(s), np.float32))) for s in shapes]
    opt = SelectiveAdam(params, lr=2e-3, eps=1e-8, bias_correction=False)
    grads = [np.asarray(rng.standard_normal(s), np.float32) for s in shapes]
    before = [p.detach().cpu().numpy() for p in params]
    for p, g in zip(params, grads):
        p.grad = _dev(g)
    with pytest.raises(RuntimeError, match="first dimensions"):
        opt.step(torch.ones(10, dtype=torch.bool, device=DEV))
    assert all(len(opt.state[p]) == 0 or int(opt.state[p]["step"].item()) == 0 for p in params)
    with spy_entries("gags_adam_step_rows") as calls:
        opt.step()
    assert len(calls) == 1 and calls[0][1][0] == 1 and calls[0][1][1] == 3
    for p, g, p0 in zip(params, grads, before):
        z = np.zeros_like(p0)
        want = R.step(oracle, p0, g, z, z, 2e-3, bias_correction=False, eps=1e-8, step=1)
        for name, got, ref in zip(("param", "exp_avg", "exp_avg_sq"), _host_state(opt, p), want):
            R.assert_same_bits(got, ref, f"{tuple(p.shape)} {name}")
    one = torch.nn.Parameter(torch.zeros(10, 4, device=DEV))
    one.grad = torch.ones(10, 4, device=DEV)
    with pytest.raises(RuntimeError, match="first dimensions"):
        SelectiveAdam([one], lr=1e-3).step(torch.ones(11, dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        SelectiveAdam([one], lr=1e-3).step(torch.ones(10, dtype=torch.bool))


# ----------------------------------------------------------------------------------------------------------------------
# 4. all rows selected == the existing dense kernel
# ----------------------------------------------------------------------------------------------------------------------
def test_all_rows_selected_equals_feature_adam():
    """W = 16, N = 70 001 (more float4s than one pass of either kernel's grid), five steps on clones.  The same bits from:
    FeatureAdam; SelectiveAdam with an all-true mask (the rows mapping); the entry itself without mask or zero test (its
    one-unit-per-lane mapping); SelectiveAdam with one tensor and nothing to select, which hands the step to the dense kernel
    (docs/LAB_NOTES.md "Selective Adam (N19)") -- and with bias_correction=False does not."""
    from gags_amd.optim import FeatureAdam, SelectiveAdam
    n, w = 70_001, 16
    gen = torch.Generator(device=DEV).manual_seed(5)
    start = torch.randn((n, w), device=DEV, generator=gen)
    ps = [torch.nn.Parameter(start.clone()) for _ in range(3)]
    opts = [FeatureAdam([{"params": [ps[0]], "lr": 1e-3}], lr=0.0, eps=EPS),
            SelectiveAdam([{"params": [ps[1]], "lr": 1e-3}], lr=0.0, eps=EPS),
            SelectiveAdam([{"params": [ps[2]], "lr": 1e-3}], lr=0.0, eps=EPS)]
    raw = [start.clone(), torch.zeros_like(start), torch.zeros_like(start)]
    everything = torch.ones(n, dtype=torch.bool, device=DEV)
    for step in range(5):
        g = torch.randn((n, w), device=DEV, generator=gen)
        for p in ps:
            p.grad = g.clone()
        opts[0].step()
        with spy_entries("gags_adam_step_rows", "gags_adam_step") as calls:
            opts[1].step()
            opts[2].step(everything)
        assert [c[0] for c in calls] == ["gags_adam_step", "gags_adam_step_rows"]
        _launch(n, [(raw[0], g, raw[1], raw[2], w, 1e-3)], None, 0, step + 1)
        for k in (1, 2):
            assert torch.equal(ps[k].detach(), ps[0].detach()), (step, k)
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(opts[k].state[ps[k]][key], opts[0].state[ps[0]][key]), (step, k, key)
        assert torch.equal(raw[0], ps[0].detach()) and torch.equal(raw[1], opts[0].state[ps[0]]["exp_avg"])
        assert torch.equal(raw[2], opts[0].state[ps[0]]["exp_avg_sq"])
    assert not torch.equal(ps[0].detach(), start)
    q = torch.nn.Parameter(start.clone())
    q.grad = torch.ones_like(start)
    with spy_entries("gags_adam_step_rows", "gags_adam_step") as calls:
        SelectiveAdam([q], lr=1e-3, bias_correction=False).step()
    assert [c[0] for c in calls] == ["gags_adam_step_rows"]


# ----------------------------------------------------------------------------------------------------------------------
# 5. model level
# ----------------------------------------------------------------------------------------------------------------------
def test_feature_training_with_sparse_adam_skips_the_rows_the_backward_left_at_zero(oracle):
    """training_setup(optimizer_type="sparse_adam"): render -> <render, G> -> backward -> optimizer.step() ->
    zero_grad(set_to_none=True), four steps over three views in ONE RasterContext with the persistent gradient buffer on.  Per
    step: the rows whose gradient row is all zero keep parameter and moments, the others equal the restatement, and the scene
    (3000 Gaussians, most of them outside any one 160 x 112 view) has rows of both kinds."""
    from gags_amd import rasterization as RZ, synthetic as syn
    from gags_amd.gaussian_renderer import render
    from gags_amd.optim import SelectiveAdam
    n, d, w, h = 3000, 16, 160, 112
    pc = syn.make_model(n, d, w, h, seed=5, device=DEV, scale0=syn.SCALE0 * 4)
    opt = pc.training_setup(optimizer_type="sparse_adam")
    assert type(opt) is SelectiveAdam and opt.skip_zero_rows
    lr = opt.param_groups[0]["lr"]
    G = syn.make_cotangent(d, h, w, seed=1).to(DEV)
    bg = torch.zeros(3, device=DEV)
    ctx = RZ.RasterContext()
    assert ctx.keep_grad_buffer
    touched = np.zeros(n, bool)
    for step, view in enumerate((3, 0, 7, 3), start=1):
        p = pc._semantic_feature
        p0, m0, v0 = _host_state(opt, p)
        cam = syn.make_camera(w, h, view=view, device=DEV)
        (render(cam, pc, None, bg, feature_mode=True, context=ctx)["render"] * G).sum().backward()
        g = p.grad.detach().cpu().numpy()
        live = R.nonzero_rows(g)
        assert 0 < int(live.sum()) < n, (step, int(live.sum()))
        version = p._version
        with spy_entries("gags_adam_step_rows", "gags_adam_step") as calls:
            opt.step()
        assert [c[0] for c in calls] == ["gags_adam_step_rows"] and p._version > version
        opt.zero_grad(set_to_none=True)
        assert p.grad is None and int(opt.state[p]["step"].item()) == step
        got = _host_state(opt, p)
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got, (p0, m0, v0)):
            R.assert_same_bits(a[~live], b[~live], f"step {step}: untouched rows, {name}")
        want = R.step(oracle, p0, g, m0, v0, lr, skip_zero_rows=True, eps=EPS, step=step)
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got, want):
            R.assert_same_bits(a, b, f"step {step}: {name}")
        assert not np.array_equal(got[0][live], p0[live])
        touched |= live
    assert ctx._kept, "the persistent gradient buffer was not in use"
    assert 0 < int(touched.sum()) < n


def _rgb_step(oracle, pc, opt, cam, bg, gt, ctx, label):
    """One RGB step with step(visibility_filter), compared with the restatement for all seven tensors.  The feature table gets
    a gradient on EVERY row (a term of the loss of its own): only the mask keeps its invisible rows still."""
    from gags_amd import densify, losses
    from gags_amd.gaussian_renderer import render
    opt.zero_grad(set_to_none=True)
    before = {k: _host_state(opt, getattr(pc, a)) for k, a in ATTR.items()}
    steps = {k: (int(opt.state[getattr(pc, a)]["step"].item()) if len(opt.state[getattr(pc, a)]) else 0) for k, a in ATTR.items()}
    pkg = render(cam, pc, None, bg, feature_mode=False, context=ctx)
    (losses.photometric_loss(pkg["render"], gt) + 1e-3 * pc._semantic_feature.sum()).backward()
    densify.accumulate(pc, pkg)
    vis = pkg["visibility_filter"]
    n = pc._xyz.shape[0]
    assert vis.dtype == torch.bool and tuple(vis.shape) == (n,)
    visible = vis.cpu().numpy()
    assert 0 < int(visible.sum()) < n, (label, int(visible.sum()), n)
    grads = {k: getattr(pc, a).grad.detach().cpu().numpy() for k, a in ATTR.items()}
    with spy_entries("gags_adam_step_rows", "gags_adam_step") as calls:
        opt.step(vis)
    assert [c[0] for c in calls] == ["gags_adam_step_rows"] and calls[0][1][1] == 7, label
    for grp in opt.param_groups:
        k = grp["name"]
        p = getattr(pc, ATTR[k])
        assert grp["params"][0] is p and tuple(opt.state[p]["exp_avg"].shape) == tuple(p.shape) and p.shape[0] == n, (label, k)
        assert int(opt.state[p]["step"].item()) == steps[k] + 1
        got = _host_state(opt, p)
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got, before[k]):
            R.assert_same_bits(a[~visible], b[~visible], f"{label} {k}: invisible rows, {name}")
        want = R.step(oracle, *[before[k][0], grads[k], before[k][1], before[k][2]], grp["lr"], mask=visible, eps=EPS,
                      step=steps[k] + 1)
        for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got, want):
            R.assert_same_bits(a, b, f"{label} {k}: {name}")
    assert not np.array_equal(_host_state(opt, pc._semantic_feature)[0][visible], before["semantic_feature"][0][visible])


def test_rgb_training_with_sparse_adam_across_densify_and_relocation(oracle):
    """training_setup_rgb(optimizer_type="sparse_adam") on the 500-Gaussian, 64 x 48 scene of tests/test_densify_gpu.py: three
    steps, densify_and_prune (N changes, the state is re-keyed), a step, an MCMC relocation of three Gaussians made dead, a
    step.  Every step is compared with the restatement from the state as it stood before it."""
    from gags_amd import synthetic as syn
    from gags_amd.gaussian_renderer import render
    from gags_amd.optim import SelectiveAdam
    from gags_amd.rasterization import RasterContext
    w, h, n0 = 64, 48, 500
    pc = syn.make_model(n0, 16, w, h, seed=3, device=DEV, scale0=syn.SCALE0 * 24)
    cam = syn.make_camera(w, h, view=3, device=DEV)
    bg = torch.zeros(3, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(11)
    with torch.no_grad():
        dc = pc._features_dc.detach().clone()
        pc._features_dc += 0.5 * torch.randn(dc.shape, device=DEV, generator=gen)
        gt = render(cam, pc, None, bg, feature_mode=False)["render"].detach().clamp(0.0, 1.0).contiguous()
        pc._features_dc.copy_(dc)
    opt = pc.training_setup_rgb(ARGS, optimizer_type="sparse_adam")
    assert type(opt) is SelectiveAdam and not opt.skip_zero_rows and [g["name"] for g in opt.param_groups] == list(ATTR)
    ctx = RasterContext()
    for step in range(3):
        _rgb_step(oracle, pc, opt, cam, bg, gt, ctx, f"step {step}")
    pc.densify_and_prune(0.0002, 0.005, 5.0, None, generator=torch.Generator(device=DEV).manual_seed(4))
    n1 = pc._xyz.shape[0]
    assert n1 != n0 and pc.optimizer is opt
    _rgb_step(oracle, pc, opt, cam, bg, gt, ctx, "after densify")
    with torch.no_grad():
        pc._opacity[torch.tensor([5, 17, 40], device=DEV)] = -10.0
    assert pc.relocate_gs(generator=torch.Generator(device=DEV).manual_seed(1)) == 3 and pc._xyz.shape[0] == n1
    _rgb_step(oracle, pc, opt, cam, bg, gt, ctx, "after relocation")
