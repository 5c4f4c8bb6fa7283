"""State carried from one training step to the next, against a recomputation that carries none.

The product is a loop of tens of thousands of steps; between two of them the Python layer keeps a persistent gradient buffer
and its flag arrays (raster_context._KeptGrad), the row map a forward enqueues for its backward (_EarlyRowmap) and its pool of
pinned words, packed 16-bit decoder weights (decoders._PACK_CACHE), a bound on the segment ids (losses._NSEG_CACHE) and the
optimizer's moments (optim.FeatureAdam) -- each trusted on identity, address, version counter or a reference count.  Every
test here runs K steps with all of that at its default, snapshots the inputs of each step, and compares what the step
produced with the same step recomputed FROM THE SNAPSHOT with nothing carried: new tensors for every input, a new
RasterContext with the buffer, the capacity mode and the early row map off, the decoder and segment caches emptied.
Re-anchoring at every step is deliberate: the reference's Adam runs with eps = 1e-15, a trajectory compared over K steps
amplifies rounding noise to +-lr per element and proves nothing.  The stateless step itself is pinned to the oracle, the
float64 restatements and the reference's fixtures by the single-step tests (test_parity_gpu.py, test_iteration_gpu.py, ...).

Stale VALUES are what is tested.  No test hands a kernel a count, capacity, index or size other than the true one.
Wall time of this file on one MI355X: 7 s of tests, 9 s with the interpreter's start (measured once, for information).
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from helpers import spy_entries

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device("cuda", 0)


# ----------------------------------------------------------------------------------------------------------------------
# helpers: a model / context / step with nothing carried over
# ----------------------------------------------------------------------------------------------------------------------
def _model_class(half):
    from gags_amd.scene import GaussianModel
    if not half:
        return GaussianModel

    class HalfTableModel(GaussianModel):
        """An fp16 feature table (BASELINE.json configs[4]) behind its fp32 master: the rasterizer reads and differentiates the
        halves, autograd's cast hands the master an fp32 gradient, FeatureAdam steps the master."""

        @property
        def get_semantic_feature(self):
            return self._semantic_feature.half()

    return HalfTableModel


def _clone_model(pc, feature=None, geometry_grads=False):
    """A model of new tensors: `pc`'s geometry cloned, `feature` (default: pc's current table) cloned."""
    feat = (pc._semantic_feature if feature is None else feature).detach().clone()
    m = type(pc).from_tensors(pc._xyz.detach().clone(), pc._scaling.detach().clone(), pc._rotation.detach().clone(),
                              pc._opacity.detach().clone(), pc._features_dc.detach().clone(),
                              pc._features_rest.detach().clone(), feat, sh_degree=pc.max_sh_degree)
    if geometry_grads:
        _geometry_grads(m, True)
    return m


def _geometry_grads(pc, on):
    for name in ("_xyz", "_scaling", "_rotation", "_opacity"):
        getattr(pc, name).requires_grad_(on)
        getattr(pc, name).grad = None


def _stateless_context():
    from gags_amd.rasterization import RasterContext
    ctx = RasterContext(capacity_mode=False)
    ctx.keep_grad_buffer = False
    ctx.early_rowmap = False
    return ctx


@contextlib.contextmanager
def _no_module_state():
    """The module-level caches (packed decoder weights, segment-id bounds) emptied for the stateless recomputation -- and put
    back afterwards exactly as they were: the stateful loop must go on with the entries IT made, or the recomputation between
    two of its steps would do the invalidation the loop is being tested for."""
    from gags_amd import decoders, losses
    saved = dict(decoders._PACK_CACHE), dict(losses._NSEG_CACHE)
    decoders.invalidate_packed()
    losses._NSEG_CACHE.clear()
    try:
        yield
    finally:
        for cache, old in zip((decoders._PACK_CACHE, losses._NSEG_CACHE), saved):
            cache.clear()
            cache.update(old)


def _make_model(n, d, w, h, seed, mult, half=False):
    from gags_amd import synthetic as syn
    pc = syn.make_model(n, d, w, h, seed=seed, device=DEV, scale0=syn.SCALE0 * mult)
    if half:
        pc.__class__ = _model_class(True)
    return pc


def _stateless_feature_grad(pc, feature, view, G, w, h, geometry_grads=False):
    """d <render(view), G> / d feature table from the snapshot `feature`, with no carried state."""
    from gags_amd import synthetic as syn
    from gags_amd.gaussian_renderer import render
    with _no_module_state():
        m = _clone_model(pc, feature, geometry_grads)
        cam = syn.make_camera(w, h, view=view, device=DEV)
        out = render(cam, m, None, torch.zeros(3, device=DEV), feature_mode=True, context=_stateless_context())["render"]
        (out * G.clone()).sum().backward()
        return m._semantic_feature.grad.detach().clone()


def _kept_ptrs(ctx):
    return {e.buf.data_ptr() for e in ctx._kept.values()}


# ----------------------------------------------------------------------------------------------------------------------
# a. rasterizer + optimizer, deterministic, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
VIEW_ORDER = (0, 7, 3, 3, 0, 7, 3, 0, 7, 0, 3, 7)  # 12 steps over 3 views, one view twice in a row once


@pytest.mark.parametrize("case,d,half,narrow", [("d16", 16, False, False), ("d256", 256, False, False),
                                                ("d513", 513, False, False), ("fp16_table", 256, True, False),
                                                ("narrow", 256, False, True)])
def test_twelve_steps_equal_the_stateless_step_bit_for_bit(oracle, monkeypatch, case, d, half, narrow):
    """render -> <render, G> -> backward -> FeatureAdam.step -> zero_grad(set_to_none=True), twelve times in one context with
    the persistent gradient buffer and the early row map on (the defaults).  Per step: the feature gradient equals the
    stateless one (torch.equal); parameter and both moments after step() equal oracle.adam_step applied to the snapshot (bit
    equality: the bound of test_adam_step_matches_oracle_and_fixture).  Widths: 16 (what the reference trains), 256, 513 (the
    extra channel rides with the float4 columns), an fp16 table behind its fp32 master, and 256 with PROW_MAX_BYTES at 0 so that
    the kept buffer is written one 128-channel range at a time (the "narrow" path of the staged backward).  The mechanism
    under test is asserted to have been on: one buffer over all steps, no step counted as a failure."""
    from gags_amd import _lib, raster_tunables as T, rasterization as R, synthetic as syn
    from gags_amd.gaussian_renderer import render
    from gags_amd.optim import FeatureAdam
    n, w, h = 6000, 200, 138
    pc = _make_model(n, d, w, h, seed=4, mult=3, half=half)
    opt = pc.training_setup()
    assert isinstance(opt, FeatureAdam)
    lr, eps = opt.param_groups[0]["lr"], opt.param_groups[0]["eps"]
    cams = {v: syn.make_camera(w, h, view=v, device=DEV) for v in set(VIEW_ORDER)}
    G = syn.make_cotangent(d, h, w, seed=2, device=DEV)
    bg = torch.zeros(3, device=DEV)
    ctx = R.RasterContext()
    assert ctx.keep_grad_buffer and ctx.early_rowmap and not ctx.capacity_mode
    ptrs, rows_seen = set(), []
    for t, view in enumerate(VIEW_ORDER, start=1):
        p = pc._semantic_feature
        feat0 = p.detach().clone()
        st = opt.state[p]
        m0 = st["exp_avg"].detach().cpu().numpy().copy() if len(st) else np.zeros((n, d), np.float32)
        v0 = st["exp_avg_sq"].detach().cpu().numpy().copy() if len(st) else np.zeros((n, d), np.float32)
        with monkeypatch.context() as mp, spy_entries("gags_raster_bwd_colors_staged") as staged:
            if narrow:
                mp.setattr(T, "PROW_MAX_BYTES", 0)
            (render(cams[view], pc, None, bg, feature_mode=True, context=ctx)["render"] * G).sum().backward()
        # (argument 15: the stage word, 17: the channel width) the range-sized scratch in every call of the narrow case, in none else
        ranged = [bool(a[15] & _lib.GAGS_STAGED_RANGE_SCRATCH) for _, a in staged]
        assert ranged and all(r == narrow for r in ranged), (case, t, ranged)
        assert not narrow or all(a[17] == 128 for _, a in staged), (case, t)
        with spy_entries("gags_raster_bwd_colors_staged") as staged:
            want = _stateless_feature_grad(pc, feat0, view, G, w, h)
        assert staged and not any(a[15] & _lib.GAGS_STAGED_RANGE_SCRATCH for _, a in staged), (case, t)
        got = p.grad
        assert got.dtype == torch.float32 and torch.equal(got, want), (case, t, view, float((got - want).abs().max()))
        rows_seen.append((want != 0).any(1))
        ptrs |= _kept_ptrs(ctx)
        if not half:  # (autograd adopted the buffer's alias; the fp16 gradient reaches its fp32 master through a cast)
            assert _kept_ptrs(ctx) == {got.data_ptr()}, (case, t)
        del got
        po = feat0.cpu().numpy().copy()
        oracle.adam_step(po, want.cpu().numpy(), m0, v0, lr, eps=eps, step=t)
        opt.step()
        opt.zero_grad(set_to_none=True)
        assert p.grad is None
        st = opt.state[p]
        assert int(st["step"].item()) == t
        np.testing.assert_array_equal(st["exp_avg"].cpu().numpy(), m0, err_msg=f"{case} step {t}")
        np.testing.assert_array_equal(st["exp_avg_sq"].cpu().numpy(), v0, err_msg=f"{case} step {t}")
        np.testing.assert_array_equal(p.detach().cpu().numpy(), po, err_msg=f"{case} step {t}")
    assert not torch.equal(rows_seen[0], rows_seen[1])  # the views touch different rows: re-zeroing had something to do
    assert len(ptrs) == 1, "the persistent buffer was not reused over the steps"
    assert ctx._kept_fails and all(v == 0 for v in ctx._kept_fails.values()), ctx._kept_fails


# ----------------------------------------------------------------------------------------------------------------------
# b. changing shapes, a forward that is never differentiated, a step with geometry gradients
# ----------------------------------------------------------------------------------------------------------------------
def test_changing_shapes_evaluation_and_geometry_steps_within_one_context(oracle):
    """One context; three (N, D) shapes in rotation (more than KEEP_GRAD_SHAPES: every step evicts a buffer), then two shapes
    (buffers reused after an eviction), then N changes for one width (densification / pruning: a second model), then a forward
    that is rendered with a graph and dropped (evaluation inside the loop: its _EarlyRowmap is released unused) between two
    trained steps, then a step with geometry gradients on (full backward) between two colours-only steps.  Same assertions as
    above per step, for the model that stepped."""
    from gags_amd import raster_tunables as T, rasterization as R, synthetic as syn
    from gags_amd.gaussian_renderer import render
    w, h = 160, 112
    shapes = {"A": (3000, 64), "B": (2500, 128), "C": (2000, 32), "A2": (3600, 64)}
    assert len(shapes) > T.KEEP_GRAD_SHAPES
    models, opts, Gs, steps = {}, {}, {}, {}
    for i, (k, (n, d)) in enumerate(shapes.items()):
        models[k] = _make_model(n, d, w, h, seed=20 + i, mult=5)
        opts[k] = models[k].training_setup()
        Gs[k] = syn.make_cotangent(d, h, w, seed=30 + i, device=DEV)
        steps[k] = 0
    cams = {v: syn.make_camera(w, h, view=v, device=DEV) for v in range(8)}
    bg = torch.zeros(3, device=DEV)
    ctx = R.RasterContext()

    def trained_step(k, view, geometry=False):
        pc, opt = models[k], opts[k]
        n, d = shapes[k]
        p = pc._semantic_feature
        feat0 = p.detach().clone()
        st = opt.state[p]
        m0 = st["exp_avg"].cpu().numpy().copy() if len(st) else np.zeros((n, d), np.float32)
        v0 = st["exp_avg_sq"].cpu().numpy().copy() if len(st) else np.zeros((n, d), np.float32)
        if geometry:
            _geometry_grads(pc, True)
        (render(cams[view], pc, None, bg, feature_mode=True, context=ctx)["render"] * Gs[k]).sum().backward()
        if geometry:
            assert pc._xyz.grad is not None and float(pc._xyz.grad.abs().max()) > 0
            _geometry_grads(pc, False)
        want = _stateless_feature_grad(pc, feat0, view, Gs[k], w, h, geometry_grads=geometry)
        assert torch.equal(p.grad, want), (k, view, geometry, float((p.grad - want).abs().max()))
        assert float(want.abs().max()) > 0
        steps[k] += 1
        po = feat0.cpu().numpy().copy()
        oracle.adam_step(po, want.cpu().numpy(), m0, v0, opt.param_groups[0]["lr"], eps=opt.param_groups[0]["eps"], step=steps[k])
        opt.step()
        opt.zero_grad(set_to_none=True)
        st = opt.state[p]
        np.testing.assert_array_equal(st["exp_avg"].cpu().numpy(), m0)
        np.testing.assert_array_equal(st["exp_avg_sq"].cpu().numpy(), v0)
        np.testing.assert_array_equal(p.detach().cpu().numpy(), po)
        assert len(ctx._kept) <= T.KEEP_GRAD_SHAPES

    for i, k in enumerate("ABCABCA"):           # rotation over three shapes
        trained_step(k, view=(3 * i + 1) % 8)
    for i, k in enumerate("ABBAAB"):            # two shapes: both buffers stay, rows change from step to step
        trained_step(k, view=(5 * i + 2) % 8)
    kept_a = {e.buf.data_ptr() for key, e in ctx._kept.items() if key[0] == shapes["A"][0]}
    for i, k in enumerate(("A", "A2", "A", "A2", "A2")):  # N changes and changes back for one width
        trained_step(k, view=(3 * i) % 8)
    trained_step("A", view=6)
    assert kept_a and kept_a == {e.buf.data_ptr() for key, e in ctx._kept.items() if key[0] == shapes["A"][0]}
    # evaluation inside the loop: rendered with a graph (the forward enqueues the backward's row map), never differentiated
    trained_step("B", view=1)
    dropped = render(cams[4], models["B"], None, bg, feature_mode=True, context=ctx)["render"]
    assert dropped.requires_grad
    del dropped
    with torch.no_grad():
        render(cams[5], models["B"], None, bg, feature_mode=True, context=ctx)
    trained_step("B", view=6)
    trained_step("B", view=6)
    # geometry gradients on for one step
    trained_step("A", view=2)
    trained_step("A", view=5, geometry=True)
    trained_step("A", view=0)
    assert all(v == 0 for v in ctx._kept_fails.values()), ctx._kept_fails


# ----------------------------------------------------------------------------------------------------------------------
# c. writers the version counter does not see
# ----------------------------------------------------------------------------------------------------------------------
class _Done:
    def wait(self):
        return True


def _blind_collectives(monkeypatch, grad, total, rank=0, world=2):
    """gags_amd.dist as rank `rank` of `world`, its collectives replaced by stand-ins that leave in `grad` what the real ones
    would -- the prepared sum over the ranks `total` -- written through `.data`, which does not move the version counter (c10d's
    all_reduce and reduce_scatter_tensor do not either).  Every stand-in records grad._version before and after its write."""
    from gags_amd import dist as gd
    seen = []
    flat_total = total.reshape(-1)
    base, esz, numel = grad.data_ptr(), grad.element_size(), grad.numel()

    def inside(t):
        off = (t.data_ptr() - base) // esz
        return off if (0 <= off and off + t.numel() <= numel and (t.data_ptr() - base) % esz == 0) else None

    def write(dst, src):
        v = grad._version
        dst.data.copy_(src)
        seen.append((v, grad._version))

    def all_reduce(t, op=None, async_op=False):
        off = inside(t)
        if off is None:  # (the out-of-place form reduces a private copy of the whole gradient)
            assert t.numel() == numel
            off = 0
        write(t, flat_total[off:off + t.numel()].view(t.shape))
        return _Done() if async_op else None

    def reduce_scatter_tensor(out, inp):
        off = inside(inp)
        assert off is not None and inp.numel() % world == 0
        k = inp.numel() // world
        write(out, flat_total[off + rank * k:off + (rank + 1) * k].view(out.shape))

    def all_gather_into_tensor(out, shard):
        off = inside(out)
        assert off is not None
        write(out, flat_total[off:off + out.numel()].view(out.shape))

    monkeypatch.setattr(gd, "world", lambda: world)
    monkeypatch.setattr(gd.dist, "get_rank", lambda *a, **k: rank)
    monkeypatch.setattr(gd.dist, "all_reduce", all_reduce)
    monkeypatch.setattr(gd.dist, "reduce_scatter_tensor", reduce_scatter_tensor)
    monkeypatch.setattr(gd.dist, "all_gather_into_tensor", all_gather_into_tensor)
    return seen


def _writer_scene():
    from gags_amd import rasterization as R, synthetic as syn
    n, d, w, h = 6000, 256, 200, 138
    pc = _make_model(n, d, w, h, seed=4, mult=3)
    pc.training_setup()
    G = syn.make_cotangent(d, h, w, seed=2, device=DEV)
    cams = {v: syn.make_camera(w, h, view=v, device=DEV) for v in (0, 7, 3)}
    feat = pc._semantic_feature.detach().clone()
    # what each view's step must give (stateless), and the "other rank's" gradient: view 7's
    want = {v: _stateless_feature_grad(pc, feat, v, G, w, h) for v in (0, 7, 3)}
    return pc, G, cams, want, R.RasterContext(), (n, d, w, h)


def _step(ctx, pc, cam, G):
    from gags_amd.gaussian_renderer import render
    (render(cam, pc, None, torch.zeros(3, device=DEV), feature_mode=True, context=ctx)["render"] * G).sum().backward()
    return pc._semantic_feature.grad


def _rows(t):
    return (t != 0).any(1)


@pytest.mark.parametrize("route", ["allreduce", "rs_ag", "rs_ag_in_place", "rs_ag_ragged_tail", "allreduce_out_of_place"])
def test_a_reduced_gradient_does_not_leak_into_the_next_step(monkeypatch, route):
    """Step 1 renders view 0; the gradient autograd adopted (the persistent buffer's alias) is summed over two "ranks" by
    dist.reduce_feature_grad -- the collectives replaced by stand-ins that write the other rank's rows (view 7's gradient)
    without moving the version counter, as c10d's do -- and released.  Step 2 renders view 3 and must give exactly the
    stateless gradient of view 3: the other rank's rows that neither step's flags cover must not survive.  Asserted on the way:
    the stand-ins really left the counter alone, and they really wrote a row that view 0 did not flag and view 3 does not
    touch (that row is the whole test).  The out-of-place form must leave its source as it was, and the buffer in use."""
    from gags_amd import dist as gd
    pc, G, cams, want, ctx, _ = _writer_scene()
    g = _step(ctx, pc, cams[0], G)
    assert torch.equal(g, want[0])
    first_ptr = g.data_ptr()
    assert _kept_ptrs(ctx) == {first_ptr}
    total = want[0] + want[7]
    stale = _rows(want[7]) & ~_rows(want[0]) & ~_rows(want[3])
    assert int(stale.sum()) > 0
    with monkeypatch.context() as mp:  # (undone before the gradient is released: the stand-ins hold a reference to it)
        seen = _blind_collectives(mp, g, total)
        if route == "allreduce_out_of_place":
            out = gd.reduce_feature_grad_oop(g, mode="allreduce")
            assert torch.equal(g, want[0]) and out.data_ptr() != g.data_ptr() and torch.equal(out, total)
            pc._semantic_feature.grad = out
            del out
        else:
            if route == "rs_ag_in_place":
                mp.setattr(gd, "_IN_PLACE", True)
            # (a bucket size that leaves 536 002 elements behind the last whole bucket: they go through the tail's all-reduce)
            kw = dict(mode="allreduce" if route == "allreduce" else "rs_ag")
            if route == "rs_ag_ragged_tail":
                kw["bucket_bytes"] = 4 * 999_998
            gd.reduce_feature_grad(g, **kw)
            assert torch.equal(g, total) and bool(_rows(g)[stale].all())
    assert seen and all(a == b for a, b in seen), "a stand-in moved the version counter: this no longer tests a blind writer"
    del g
    pc._semantic_feature.grad = None
    g2 = _step(ctx, pc, cams[3], G)
    assert torch.equal(g2, want[3]), (route, int((_rows(g2) & stale).sum()), float((g2 - want[3]).abs().max()))
    # the buffer stayed in use (wiped, not replaced), and the step did not count towards the three-strikes switch-off
    assert g2.data_ptr() == first_ptr and all(v == 0 for v in ctx._kept_fails.values()), ctx._kept_fails
    del g2
    pc._semantic_feature.grad = None
    g3 = _step(ctx, pc, cams[0], G)
    assert torch.equal(g3, want[0]) and g3.data_ptr() == first_ptr


def test_in_place_reduction_every_step_keeps_the_buffer_in_use(monkeypatch):
    """The allreduce mode of a by-view step, five steps: every step's buffer is written by the reduction and released; every
    step's local gradient is exact, on the same buffer, and the switch-off counter never moves."""
    from gags_amd import dist as gd
    pc, G, cams, want, ctx, _ = _writer_scene()
    ptrs = set()
    for t, (view, other) in enumerate(((0, 7), (3, 0), (7, 3), (7, 0), (0, 3))):
        g = _step(ctx, pc, cams[view], G)
        assert torch.equal(g, want[view]), (t, view)
        ptrs.add(g.data_ptr())
        with monkeypatch.context() as mp:
            seen = _blind_collectives(mp, g, want[view] + want[other])
            gd.reduce_feature_grad(g, mode="allreduce")
        assert seen and all(a == b for a, b in seen) and torch.equal(g, want[view] + want[other])
        del g
        pc._semantic_feature.grad = None
    assert len(ptrs) == 1 and all(v == 0 for v in ctx._kept_fails.values()), (ptrs, ctx._kept_fails)


def test_a_callers_own_writer_needs_grad_written_or_no_kept_buffer():
    """A writer this package cannot see (DDP-style dist.all_reduce(p.grad), a kernel on data_ptr()): here `.data.add_`, which
    leaves the version counter alone like those.  With the documented call rasterization.grad_written(p.grad) after the write
    the next step is exact; with keep_grad_buffer = False (GAGS_KEEP_GRAD=0) it is exact without the call."""
    from gags_amd import rasterization as R
    pc, G, cams, want, ctx, _ = _writer_scene()
    stale = _rows(want[7]) & ~_rows(want[0]) & ~_rows(want[3])
    assert int(stale.sum()) > 0
    plain = R.RasterContext()
    plain.keep_grad_buffer = False
    for c, call in ((ctx, True), (plain, False)):
        g = _step(c, pc, cams[0], G)
        v = g._version
        g.data.add_(want[7])
        assert g._version == v and bool(_rows(g)[stale].all())
        if call:
            assert R.grad_written(g) is g and g._version != v
        del g
        pc._semantic_feature.grad = None
        g2 = _step(c, pc, cams[3], G)
        assert torch.equal(g2, want[3]), (call, float((g2 - want[3]).abs().max()))
        del g2
        pc._semantic_feature.grad = None


# ----------------------------------------------------------------------------------------------------------------------
# e. the composed iteration, K steps
# ----------------------------------------------------------------------------------------------------------------------
W_IT, H_IT, N_IT = 32, 24, 1500  # the image of tests/golden/iteration_vectors.npz


def _iteration_views(n_emb_b=21, ids_b=21):
    """Two views with different segment maps and embedding tables: the fixture's (13 segments) and a seeded synthetic one
    (`n_emb_b` embeddings, ids below `ids_b`, 4 x 4 blocks, -1 = none)."""
    z = np.load(os.path.join(HERE, "golden", "iteration_vectors.npz"))
    g = torch.Generator().manual_seed(11)
    emb_b = torch.nn.functional.normalize(torch.randn(n_emb_b, 512, generator=g), dim=-1)
    seg_b = torch.randint(-1, ids_b, (4, H_IT // 4, W_IT // 4), generator=g).float()
    seg_b = seg_b.repeat_interleave(4, 1).repeat_interleave(4, 2).contiguous()
    return [dict(view=2, seg=torch.from_numpy(z["seg_map"]).to(DEV), emb=torch.from_numpy(z["img_embed"]).to(DEV)),
            dict(view=5, seg=seg_b.to(DEV), emb=emb_b.to(DEV))]


def _decoders(precision, state=None):
    from gags_amd.decoders import CNN_decoder, CNN_scale_decoder
    dec, sdec = CNN_decoder(16, 512, precision).to(DEV), CNN_scale_decoder(16, 3, precision).to(DEV)
    if state is not None:
        dec.load_state_dict({k: v.clone() for k, v in state[0].items()})
        sdec.load_state_dict({k: v.clone() for k, v in state[1].items()})
    return dec, sdec


def _iteration(pc, cam, seg, emb, dec, sdec, iteration, threshold, ctx):
    """One composed iteration up to and including backward: (loss, d loss / d feature_map, feature gradient, decoder grads)."""
    from gags_amd.distill import distillation_loss
    from gags_amd.gaussian_renderer import render
    fmap = render(cam, pc, None, torch.zeros(3, device=DEV), feature_mode=True, context=ctx)["render"]
    fmap.retain_grad()
    loss, _ = distillation_loss(fmap, seg, emb, dec, sdec, iteration, scale_regulation_iteration=threshold)
    loss.backward()
    out = {"loss": loss.detach().reshape(1).clone(), "d_fmap": fmap.grad.detach().clone(),
           "feature": pc._semantic_feature.grad.detach().clone()}
    for name, model in (("dec", dec), ("sdec", sdec)):
        for k, p in model.named_parameters():
            out[f"{name}.{k}"] = p.grad.detach().clone()
    return out


def _stateless_iteration(pc, feature, view, seg, emb, precision, state, iteration, threshold):
    from gags_amd import synthetic as syn
    with _no_module_state():
        m = _clone_model(pc, feature)
        dec, sdec = _decoders(precision, state)
        cam = syn.make_camera(W_IT, H_IT, view=view, device=DEV)
        return _iteration(m, cam, seg.clone(), emb.clone(), dec, sdec, iteration, threshold, _stateless_context())


def _ulp(x):
    return float(np.spacing(np.float32(x)))


def _compare(got, ref_a, ref_b, where, spreads):
    """Each quantity of the stateful step against the stateless recomputation: within 4 x the spread of two stateless runs from
    the same snapshot (one pair does not bound run-to-run rounding), floored at one ulp of the quantity's largest element;
    bit-equal where that spread is zero."""
    assert got.keys() == ref_a.keys() == ref_b.keys()
    for k in got:
        assert torch.isfinite(ref_a[k]).all() and float(ref_a[k].abs().max()) > 0, (where, k)
        spread = float((ref_a[k] - ref_b[k]).abs().max())
        spreads[k] = max(spreads.get(k, 0.0), spread)
        err = float((got[k] - ref_a[k]).abs().max())
        print(f"{where} {k}: stateless spread {spread:.3e}, stateful - stateless {err:.3e}")
        if spread == 0.0:
            assert torch.equal(got[k], ref_a[k]), (where, k, err)
        else:
            assert err <= max(4.0 * spread, _ulp(float(ref_a[k].abs().max()))), (where, k, err, spread)


@pytest.mark.parametrize("decoder_optimizer", ["torch_adam", "feature_adam"])
@pytest.mark.parametrize("precision", ["f16", "exact"])
def test_six_composed_iterations_equal_the_stateless_iteration(precision, decoder_optimizer):
    """render -> distill.distillation_loss -> backward -> FeatureAdam.step on the features and Adam(lr=1e-4) on both decoders
    -> zero_grad(set_to_none=True), six iterations over two views with different segment maps and embedding tables (13 and 21
    segments), crossing scale_regulation_iteration after the third (the loss weights change and the region-variance term starts
    to send gradient into the map), in the training tier "f16" (fused kernels, packed 16-bit weights, cached between uses) and
    in "exact".  decoder_optimizer "feature_adam" hands the decoders' parameters to gags_amd.optim.FeatureAdam, which writes
    them through raw pointers.  Per iteration, from the snapshot of every parameter: loss, d loss / d feature_map, the feature
    gradient and every decoder gradient within the bound of _compare.
    Measured spreads of the stateless recomputation run twice (max abs difference over the six iterations, every quantity,
    both tiers): 0 -- on these 32 x 24 maps every segment sum came out the same in both runs; the comparisons were bit-exact."""
    from gags_amd import rasterization as R, synthetic as syn
    from gags_amd.optim import FeatureAdam
    torch.manual_seed(0)
    views = _iteration_views()
    pc = _make_model(N_IT, 16, W_IT, H_IT, seed=6, mult=30)
    feat_opt = pc.training_setup()
    dec, sdec = _decoders(precision)
    if decoder_optimizer == "torch_adam":
        opts = [torch.optim.Adam(dec.parameters(), lr=1e-4), torch.optim.Adam(sdec.parameters(), lr=1e-4)]
    else:
        opts = [FeatureAdam([{"params": list(dec.parameters()) + list(sdec.parameters()), "lr": 1e-4}], lr=0.0, eps=1e-8)]
    cams = [syn.make_camera(W_IT, H_IT, view=v["view"], device=DEV) for v in views]
    ctx = R.RasterContext()
    spreads, threshold = {}, 4
    before = [p.detach().clone() for p in dec.parameters()]
    for it in range(1, 7):
        v = views[(it - 1) % 2]
        feat0 = pc._semantic_feature.detach().clone()
        state = ({k: t.detach().clone() for k, t in dec.state_dict().items()},
                 {k: t.detach().clone() for k, t in sdec.state_dict().items()})
        got = _iteration(pc, cams[(it - 1) % 2], v["seg"], v["emb"], dec, sdec, it, threshold, ctx)
        refs = [_stateless_iteration(pc, feat0, v["view"], v["seg"], v["emb"], precision, state, it, threshold) for _ in range(2)]
        _compare(got, refs[0], refs[1], f"{precision}/{decoder_optimizer} iteration {it}", spreads)
        for o in [feat_opt] + opts:
            o.step()
            o.zero_grad(set_to_none=True)
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, dec.parameters()))  # the decoders really trained
    assert all(x == 0 for x in ctx._kept_fails.values())
    print("largest stateless spreads:", {k: s for k, s in spreads.items() if s > 0} or "all zero")


@pytest.mark.parametrize("writer", ["copy_", "version_blind"])
def test_a_refilled_segment_map_gets_the_stateless_loss(writer):
    """One seg_map TENSOR refilled between iterations with larger ids (a dataloader that reuses its device buffer): once
    through copy_ (moves the version counter), once through `.data.copy_` (does not: what a kernel, DLPack or a collective
    does).  Ids stay inside the embedding table (40 rows; 15 used first, all 40 afterwards).  The loss and the map's gradient
    must be the stateless ones: no id may be skipped on a bound remembered from the first fill."""
    from gags_amd import rasterization as R, synthetic as syn
    torch.manual_seed(0)
    first = _iteration_views(n_emb_b=40, ids_b=15)[1]
    g = torch.Generator().manual_seed(12)
    refill = torch.randint(-1, 40, (4, H_IT // 4, W_IT // 4), generator=g).float()
    refill = refill.repeat_interleave(4, 1).repeat_interleave(4, 2).contiguous().to(DEV)
    assert float(refill.max()) > float(first["seg"].max()) + 10
    pc = _make_model(N_IT, 16, W_IT, H_IT, seed=6, mult=30)
    pc.training_setup()
    dec, sdec = _decoders("f16")
    cam = syn.make_camera(W_IT, H_IT, view=first["view"], device=DEV)
    ctx = R.RasterContext()
    seg, emb = first["seg"], first["emb"]
    for it in (5, 6, 7):
        if it == 6:
            v = seg._version
            seg.copy_(refill) if writer == "copy_" else seg.data.copy_(refill)
            assert (seg._version == v) == (writer == "version_blind")
        state = ({k: t.detach().clone() for k, t in dec.state_dict().items()},
                 {k: t.detach().clone() for k, t in sdec.state_dict().items()})
        got = _iteration(pc, cam, seg, emb, dec, sdec, it, 4, ctx)
        refs = [_stateless_iteration(pc, pc._semantic_feature, first["view"], seg, emb, "f16", state, it, 4) for _ in range(2)]
        _compare(got, refs[0], refs[1], f"refill {writer} iteration {it}", {})
        for m in (dec, sdec):
            m.zero_grad(set_to_none=True)
        pc._semantic_feature.grad = None


def test_the_remembered_segment_bound_follows_a_refill_through_copy():
    """losses._n_seg for a direct caller of the segment losses (no embedding table to take the bound from): the bound is
    remembered per tensor and must be read again after copy_ put larger ids into the same tensor; forget_n_seg() is the call
    for writers the version counter does not see.  Reference: the same loss on new tensors with the cache emptied."""
    from gags_amd import losses as L
    g = torch.Generator().manual_seed(5)
    h, w = 48, 64
    noise = torch.rand(h, w, generator=g).to(DEV)
    small = torch.randint(0, 6, (h // 4, w // 4), generator=g).float().repeat_interleave(4, 0).repeat_interleave(4, 1).to(DEV)
    large = torch.randint(0, 30, (h // 4, w // 4), generator=g).float().repeat_interleave(4, 0).repeat_interleave(4, 1).to(DEV)
    loss_map = noise + 0.05 * large  # (segment means that depend on the id: a skipped id shows)
    seg = small.clone()

    def fresh(ids):
        L._NSEG_CACHE.clear()
        return L.Scale_balance_loss(loss_map.clone(), ids.clone(), None, mix_seg=True)

    want_small, want_large = fresh(small), fresh(large)
    assert not torch.equal(want_small, want_large)
    L._NSEG_CACHE.clear()
    assert torch.equal(L.Scale_balance_loss(loss_map, seg, None, mix_seg=True), want_small)
    assert L._n_seg(seg) == 6
    seg.copy_(large)
    assert torch.equal(L.Scale_balance_loss(loss_map, seg, None, mix_seg=True), want_large)
    seg.copy_(small)
    L.Scale_balance_loss(loss_map, seg, None, mix_seg=True)
    seg.data.copy_(large)          # a writer the counter does not see ...
    L.forget_n_seg(seg)            # ... and the documented call
    assert torch.equal(L.Scale_balance_loss(loss_map, seg, None, mix_seg=True), want_large)
