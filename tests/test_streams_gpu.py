"""Every op family on a side stream, behind late producers (tests/stream_harness.py).

Each case of CASES runs twice: plainly on the default stream (the reference run; its values are pinned by the rest of the
suite), and on a fresh torch.cuda.Stream() under late_producers().  For the second run the device inputs are allocated and
filled with a DECOY -- a second, valid input set of the same shapes from another seed -- on the default stream; the real
inputs are copied over the decoys on the side stream, behind the first delay.  A kernel, memset or copy of the package that does
not go to the caller's stream runs ahead of that copy and computes on the decoy: a wrong number, never a wild address (no case
hands a kernel a count, index, capacity or size that is not true; tests/test_multistep_gpu.py states the same rule).

Routes documented as bit-reproducible must be torch.equal between the two runs.  Routes with float or LDS-double atomics are
compared with the reference and the bound of that route's own test, imported from there.  After each side-stream run every
recorded call that takes a `void *stream` must have received the side stream's handle (audit_streams), and the last test
requires the union of the recorded entries to cover every streamed entry the package names.
Wall time of this file on one MI355X: 21 s for its 53 tests (docs/LAB_NOTES.md, "Stream tests"); no case above 2.5 s.
"""
import contextlib
from typing import Any, Callable, NamedTuple

import numpy as np
import pytest
import torch

import stream_harness as SH
import test_multistep_gpu as MS
import test_parity_gpu as PAR
from helpers import rel_l2, scene_arrays, spy_entries

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
REAL_SEED, DECOY_SEED = 41, 97


class Case(NamedTuple):
    inputs: Callable[[int], dict]          # seed -> {name: CPU tensor}: everything the case reads from device memory
    run: Callable[[dict], dict]            # {name: device tensor} -> {name: tensor | number}, all on the current stream
    loose: Any = None                      # (oracle, real CPU inputs, got, ref): keys it checked against its own reference
    spread: bool = False                   # compare by test_multistep_gpu._compare (two reference runs bound the atomics' spread)


CASES = {}
RECORDED = {}     # case name -> names of the entries its side-stream run called
_REFERENCE = {}   # case name -> outputs of the reference run (computed once, shared, never written)


def _host(v):
    return v.detach().clone() if torch.is_tensor(v) else v


def _to_dev(host):
    return {k: v.to(DEV) for k, v in host.items()}


def _reference(name):
    if name not in _REFERENCE:
        case = CASES[name]
        runs = []
        for _ in range(2 if case.spread else 1):
            with MS._no_module_state():
                out = case.run(_to_dev(case.inputs(REAL_SEED)))
            out.pop("_own_streams", None)
            runs.append({k: _host(v) for k, v in out.items()})
        torch.cuda.synchronize()
        _REFERENCE[name] = runs
    return _REFERENCE[name]


def _side_run(case, copy_on_default=False):
    """The case on a side stream under late_producers: (outputs, recorded calls, the stream).  The real inputs reach the
    case's buffers in two hops, both behind the first delay: real -> a staging set (which holds the decoy until then), staging
    set -> the buffers.  copy_on_default issues the second hop on the default stream instead (the mutant of part 6): it runs
    at once, ahead of its producer, and copies the decoy."""
    decoy, real = _to_dev(case.inputs(DECOY_SEED)), _to_dev(case.inputs(REAL_SEED))
    assert decoy.keys() == real.keys() and all(decoy[k].shape == real[k].shape and decoy[k].dtype == real[k].dtype for k in real)
    stage = {k: v.clone() for k, v in decoy.items()}
    torch.cuda.synchronize()
    stream = SH.concurrent_stream()
    second_hop = torch.cuda.stream(torch.cuda.default_stream()) if copy_on_default else contextlib.nullcontext()
    with MS._no_module_state(), torch.cuda.stream(stream), SH.late_producers(stream) as calls:
        with torch.no_grad():
            for k in stage:
                stage[k].copy_(real[k])
            with second_hop:
                for k in decoy:
                    decoy[k].copy_(stage[k])
        out = case.run(decoy)
        out = {k: _host(v) for k, v in out.items()}
    stream.synchronize()
    torch.cuda.synchronize()
    calls = _Calls(calls)
    calls.own = tuple(out.pop("_own_streams", ()))
    return out, calls, stream


class _Calls(list):
    """The recorded calls of a side-stream run, and the handles of the streams the package itself made for that run (the
    exchange stream of dist.OverlappedGradReducer: entries it launches there, behind events, are where they belong)."""
    own = ()


def _mismatches(got, ref, skip=()):
    assert got.keys() == ref.keys(), (sorted(got), sorted(ref))
    bad = []
    for k in got:
        if k in skip:
            continue
        if torch.is_tensor(ref[k]):
            if not (got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k])):
                bad.append(k)
        elif got[k] != ref[k]:
            bad.append(k)
    return bad


# ----------------------------------------------------------------------------------------------------------------------
# rasterization(): 2000 Gaussians, 112 x 80 and 97 x 61 (ragged tiles)
# ----------------------------------------------------------------------------------------------------------------------
N_R = 2000
INDEX_KEYS = ("radii", "tiles_per_gauss", "isect_ids", "flatten_ids", "isect_offsets", "last_ids")


def _raster_inputs(d, w, h, views=(3,), sh=False):
    def make(seed):
        s = scene_arrays(N_R, d, w, h, seed=seed, view=views[0], scale_mult=5.0)
        rng = np.random.default_rng(seed + 100)
        raw = s["raw"]
        t = dict(means=raw["xyz"], quats=torch.from_numpy(s["quats"]), scales=torch.from_numpy(s["scales"]),
                 opacities=torch.from_numpy(s["opacities"]), rotation=raw["rotation"], scaling_log=raw["scaling_log"],
                 opacity_logit=raw["opacity_logit"], K=torch.from_numpy(np.ascontiguousarray(s["K"], np.float32)))
        t["colors"] = torch.from_numpy(s["sh"]) if sh else raw["semantic_feature"]
        dd = (3 if sh else d)
        t["bg"] = torch.full((dd,), 0.25)
        for i, v in enumerate(views):
            vm = scene_arrays(4, 0, w, h, seed=seed, view=v)["viewmat"]
            t[f"viewmat{i}"] = torch.from_numpy(np.ascontiguousarray(vm, np.float32))
            t[f"v_out{i}"] = torch.from_numpy(rng.standard_normal((h, w, dd + (1 if sh == "ed" else 0))).astype(np.float32))
            t[f"v_alpha{i}"] = torch.from_numpy(rng.standard_normal((h, w)).astype(np.float32))
        return {k: v.contiguous() for k, v in t.items()}
    return make


def _raster_run(w, h, views=(3,), grads=("colors",), half=False, flags=0, context=None, raw=False, tunables=None, backward=True,
                v_alpha=False, no_grad_first=False, **kw):
    """rasterization() per view in one context, <out, v_out> (+ <alpha, v_alpha>) differentiated w.r.t. `grads`: every output,
    every index tensor of `info` and every gradient."""
    def run(dev):
        from gags_amd import raster_tunables as T
        from gags_amd.rasterization import RasterContext, rasterization
        ctx = context() if context is not None else RasterContext()
        saved = {k: getattr(T, k) for k in (tunables or {})}
        for k, v in (tunables or {}).items():
            setattr(T, k, v)
        res = {}
        try:
            for i in range(len(views)):
                names = (dict(quats="rotation", scales="scaling_log", opacities="opacity_logit") if raw else {})
                leaf = {k: dev[names.get(k, k)].detach() for k in ("means", "quats", "scales", "opacities", "colors")}
                leaf["viewmat"] = dev[f"viewmat{i}"].detach()
                if half:
                    leaf["colors"] = leaf["colors"].half()
                for k in grads:
                    leaf[k].requires_grad_(True)
                args = (leaf["means"], leaf["quats"], leaf["scales"], leaf["opacities"], leaf["colors"], leaf["viewmat"][None],
                        dev["K"][None], w, h)
                opts = dict(backgrounds=dev["bg"][None], raster_flags=flags, context=ctx, raw_params=raw, **kw)
                if no_grad_first:
                    with torch.no_grad():
                        o, a, _ = rasterization(*args, **opts)
                    res.update({f"{i}.nograd.out": o, f"{i}.nograd.alpha": a})
                out, alphas, info = rasterization(*args, **opts)
                res.update({f"{i}.out": out, f"{i}.alphas": alphas, f"{i}.n_isects": int(info["n_isects"])})
                res.update({f"{i}.{k}": info[k] for k in INDEX_KEYS})
                if info.get("compensations") is not None:
                    res[f"{i}.compensations"] = info["compensations"]
                if backward and grads:
                    loss = (out[0] * dev[f"v_out{i}"]).sum()
                    if v_alpha:
                        loss = loss + (alphas[0, ..., 0] * dev[f"v_alpha{i}"]).sum()
                    geom = any(k != "colors" for k in grads)
                    if geom:
                        info["means2d"].retain_grad()
                    loss.backward()
                    res.update({f"{i}.grad.{k}": leaf[k].grad for k in grads})
                    if geom:
                        res[f"{i}.grad.means2d"] = info["means2d"].grad
                        if kw.get("absgrad"):
                            res[f"{i}.absgrad"] = info["means2d"].absgrad
                    res = {k: _host(v) for k, v in res.items()}
                    del loss, leaf
        finally:
            for k, v in saved.items():
                setattr(T, k, v)
        return res
    return run


GEOM = ("colors", "means", "quats", "scales", "opacities")


def _oracle_full_backward(w, h):
    """tests/test_parity_gpu.py::test_full_backward's comparison, with its bounds (GRAD_TOL and 1e-4), for view 0."""
    def check(oracle, t, got, ref):
        s = {k: t[k].numpy() for k in ("means", "quats", "scales", "opacities", "colors")}
        bg, vm, K = t["bg"].numpy(), t["viewmat0"].numpy(), t["K"].numpy()
        v_out, v_alpha = t["v_out0"].numpy(), t["v_alpha0"].numpy()
        o_out, o_alpha, oi = oracle.rasterization(s["means"], s["quats"], s["scales"], s["opacities"], s["colors"], vm, K, bg, w, h)
        o_vc, o_vo, o_vm2, o_vcon = oracle.raster_bwd(oi["means2d"], oi["conics"], s["opacities"], s["colors"], bg, w, h,
                                                      oi["isect_offsets"], oi["flatten_ids"], o_alpha, oi["last_ids"], v_out, v_alpha)
        o_vmeans, o_vq, o_vs = oracle.project_bwd(s["means"], s["quats"], s["scales"], vm, K, w, h, oi["radii"], o_vm2, None, o_vcon)
        want = {"colors": (o_vc, PAR.GRAD_TOL), "opacities": (o_vo, 1e-4), "means2d": (o_vm2, 1e-4), "means": (o_vmeans, 1e-4),
                "quats": (o_vq, 1e-4), "scales": (o_vs, 1e-4)}
        for k, (o, tol) in want.items():
            g = got[f"0.grad.{k}"].cpu().numpy()
            e = rel_l2(g[0] if k == "means2d" else g, o)
            print(f"{k}: rel-L2 {e:.3e} of the oracle (bound {tol:g})")
            assert e <= tol, (k, e)
        return {f"0.grad.{k}" for k in want}
    return check


def _oracle_colour_backward(w, h, d):
    """tests/test_parity_gpu.py::test_backward_flavours_agree_and_staged_is_deterministic's comparison of the float-atomic
    colours-only backward: the forward-order oracle, GRAD_TOL."""
    def check(oracle, t, got, ref):
        s = {k: t[k].numpy() for k in ("means", "quats", "scales", "opacities", "colors")}
        bg, vm, K = t["bg"].numpy(), t["viewmat0"].numpy(), t["K"].numpy()
        _, _, oi = oracle.rasterization(s["means"], s["quats"], s["scales"], s["opacities"], s["colors"], vm, K, bg, w, h)
        o_vf = oracle.raster_bwd_colors_fwdorder(oi["means2d"], oi["conics"], s["opacities"], d, w, h, oi["isect_offsets"],
                                                 oi["flatten_ids"], t["v_out0"].numpy(), N_R)
        e = rel_l2(got["0.grad.colors"].cpu().numpy(), o_vf)
        print(f"colors: rel-L2 {e:.3e} of the forward-order oracle (bound {PAR.GRAD_TOL:g})")
        assert e <= PAR.GRAD_TOL, e
        return {"0.grad.colors"}
    return check


def _atomic_sum_bound(key, terms):
    """A gradient the narrow VALU backward adds up with fp32 atomics (four channels: below the matrix-core widths), in whatever
    order the blocks arrive: two runs differ by at most twice the worst-case reordering error of a sum of `terms` terms (one
    per pixel) of the tensor's largest magnitude, terms * 2^-23 * max -- the reasoning and the bound of
    tests/test_densify_gpu.py::test_steps_across_a_densify_equal_the_stateless_step (atomic_reorder_rel there).  A gradient computed on the decoy, or on
    a stale intermediate, is off by the order of the gradient itself."""
    def check(oracle, t, got, ref):
        import test_densify_gpu as DENS
        rel = DENS.atomic_reorder_rel(terms)
        scale = float(ref[key].abs().max())
        err = float((got[key] - ref[key]).abs().max())
        print(f"{key}: max abs difference {err:.3e} between the two runs, bound {rel * scale:.3e}")
        assert scale > 0 and err <= rel * scale, (key, err, scale)
        return {key}
    return check


def _both(*checks):
    def check(oracle, t, got, ref):
        return set().union(*[c(oracle, t, got, ref) for c in checks])
    return check


def _ctx(trim_lists=None, **kw):
    def make():
        from gags_amd.rasterization import RasterContext
        ctx = RasterContext(**kw)
        if trim_lists is not None:
            ctx.trim_lists = trim_lists
        return ctx
    return make


def _register_raster():
    from gags_amd import _lib
    A, B = (112, 80), (97, 61)
    # D = 3: the narrow VALU path, forward and full backward (float atomics: against the oracle)
    CASES["raster_d3_valu_full"] = Case(_raster_inputs(3, *A), _raster_run(*A, grads=GEOM, v_alpha=True),
                                        loose=_oracle_full_backward(*A))
    CASES["raster_d3_valu_absgrad"] = Case(_raster_inputs(3, *B), _raster_run(*B, grads=GEOM, v_alpha=True, absgrad=True),
                                           loose=_both(_oracle_full_backward(*B), _atomic_sum_bound("0.absgrad", B[0] * B[1])))
    CASES["raster_d16"] = Case(_raster_inputs(16, *B), _raster_run(*B))
    CASES["raster_d16_forward"] = Case(_raster_inputs(16, *B), _raster_run(*B, grads=(), backward=False))
    CASES["raster_d128_fp32"] = Case(_raster_inputs(128, *A), _raster_run(*A))
    CASES["raster_d128_fp16"] = Case(_raster_inputs(128, *B), _raster_run(*B, half=True))
    CASES["raster_d128_atomic"] = Case(_raster_inputs(128, *A), _raster_run(*A, flags=_lib.GAGS_BWD_ATOMIC),
                                       loose=_oracle_colour_backward(*A, 128))
    CASES["raster_d128_fused"] = Case(_raster_inputs(128, *A), _raster_run(*A, grads=(), backward=False, flags=_lib.GAGS_FWD_FUSED))
    CASES["raster_d328_geom"] = Case(_raster_inputs(328, *B), _raster_run(*B, grads=GEOM, v_alpha=True))
    CASES["raster_d513"] = Case(_raster_inputs(513, *A), _raster_run(*A))
    CASES["raster_capacity_mode"] = Case(_raster_inputs(128, *A, views=(3, 5)),
                                         _raster_run(*A, views=(3, 5), context=_ctx(capacity_mode=True)))
    CASES["raster_overlap_zero_fill"] = Case(_raster_inputs(128, *B), _raster_run(*B, context=_ctx(overlap_zero_fill=True),
                                                                                  tunables=dict(ZERO_FILL_MIN_ELEMS=0)))
    CASES["raster_trim_lists"] = Case(_raster_inputs(128, *B), _raster_run(*B, context=_ctx(trim_lists=True)))
    CASES["raster_raw_aa_absgrad"] = Case(_raster_inputs(32, *A), _raster_run(*A, grads=GEOM, v_alpha=True, raw=True,
                                                                              rasterize_mode="antialiased", absgrad=True))
    CASES["raster_aa"] = Case(_raster_inputs(32, *B), _raster_run(*B, grads=GEOM, rasterize_mode="antialiased"))
    CASES["raster_raw"] = Case(_raster_inputs(32, *B), _raster_run(*B, grads=GEOM, raw=True))
    CASES["raster_pose"] = Case(_raster_inputs(32, *B), _raster_run(*B, grads=("viewmat",), v_alpha=True))
    CASES["raster_fisheye"] = Case(_raster_inputs(32, *A), _raster_run(*A, grads=GEOM, camera_model="fisheye"))
    CASES["raster_sh3_rgb_ed"] = Case(_raster_inputs(3, *A, sh="ed"), _raster_run(*A, sh_degree=3, render_mode="RGB+ED",
                                                                                  no_grad_first=True),
                                      loose=_atomic_sum_bound("0.grad.colors", A[0] * A[1]))


_register_raster()


# ----------------------------------------------------------------------------------------------------------------------
# the composed distillation iteration (tests/test_iteration_gpu.py's, at its 32 x 24 size), two in a row
# ----------------------------------------------------------------------------------------------------------------------
def _iteration_inputs(precision):
    def make(seed):
        from gags_amd import synthetic as syn
        from gags_amd.decoders import CNN_decoder, CNN_scale_decoder
        w, h, n = MS.W_IT, MS.H_IT, MS.N_IT
        g = torch.Generator().manual_seed(seed)
        p = syn.make_gaussians(n, 16, w, h, seed=seed, scale0=syn.SCALE0 * 30)
        t = {f"pc.{k}": v for k, v in p.items()}
        t["emb"] = torch.nn.functional.normalize(torch.randn(21, 512, generator=g), dim=-1)
        seg = torch.randint(-1, 21, (4, h // 4, w // 4), generator=g).float()
        t["seg"] = seg.repeat_interleave(4, 1).repeat_interleave(4, 2).contiguous()
        torch.manual_seed(seed)
        for name, m in (("dec", CNN_decoder(16, 512, precision)), ("sdec", CNN_scale_decoder(16, 3, precision))):
            t.update({f"{name}.{k}": v.detach().clone() for k, v in m.state_dict().items()})
        return t
    return make


def _model_on(dev, cls=None):
    """A GaussianModel whose parameters ARE the device tensors of `dev` (no copy)."""
    from gags_amd.scene import GaussianModel
    p = {k[3:]: v for k, v in dev.items() if k.startswith("pc.")}
    m = (cls or GaussianModel).from_tensors(p["xyz"], p["scaling_log"], p["rotation"], p["opacity_logit"], p["features_dc"],
                                            p["features_rest"], p["semantic_feature"], sh_degree=3)
    assert m._xyz.data_ptr() == p["xyz"].data_ptr() and m._semantic_feature.data_ptr() == p["semantic_feature"].data_ptr()
    return m


def _decoders_on(dev, precision):
    from gags_amd.decoders import CNN_decoder, CNN_scale_decoder
    out = []
    for name, m in (("dec", CNN_decoder(16, 512, precision)), ("sdec", CNN_scale_decoder(16, 3, precision))):
        m = m.to(DEV)
        for k, p in list(m.named_parameters()) + list(m.named_buffers()):
            p.data = dev[f"{name}.{k}"]
        out.append(m)
    return out


def _iteration_run(precision, fused_head, fused_chain=True):
    def run(dev):
        from gags_amd import decoders
        saved = decoders.FUSED
        decoders.FUSED = fused_chain  # (False: the 16-bit tiers run their chains layer by layer)
        try:
            return chain(dev)
        finally:
            decoders.FUSED = saved

    def chain(dev):
        from gags_amd import synthetic as syn
        from gags_amd.distill import distillation_loss
        from gags_amd.gaussian_renderer import render
        from gags_amd.rasterization import RasterContext
        pc = _model_on(dev)
        pc.training_setup()
        dec, sdec = _decoders_on(dev, precision)
        cam = syn.make_camera(MS.W_IT, MS.H_IT, view=2, device=DEV)
        ctx, res = RasterContext(), {}
        for it, iteration in enumerate((3, 5)):  # (scale_regulation_iteration = 4: the region-variance term joins the second)
            fmap = render(cam, pc, None, torch.zeros(3, device=DEV), feature_mode=True, context=ctx)["render"]
            fmap.retain_grad()
            loss, _ = distillation_loss(fmap, dev["seg"], dev["emb"], dec, sdec, iteration, scale_regulation_iteration=4,
                                        fused_head=fused_head)
            loss.backward()
            res[f"{it}.loss"] = loss.detach().reshape(1).clone()
            res[f"{it}.d_fmap"] = fmap.grad.detach().clone()
            res[f"{it}.feature"] = pc._semantic_feature.grad.detach().clone()
            for name, model in (("dec", dec), ("sdec", sdec)):
                for k, p in model.named_parameters():
                    res[f"{it}.{name}.{k}"] = p.grad.detach().clone()
            del fmap, loss
            for m in (dec, sdec):
                m.zero_grad(set_to_none=True)
            pc._semantic_feature.grad = None
        return res
    return run


for _prec in ("exact", "bf16x2", "f16", "bf16"):  # ("bf16": the tier behind the library's un-suffixed 16-bit entries)
    for _fused in (True, False):
        CASES[f"iteration_{_prec}_{'fused' if _fused else 'two_step'}_head"] = Case(
            _iteration_inputs(_prec), _iteration_run(_prec, _fused), spread=True)
for _prec in ("bf16", "f16"):
    CASES[f"iteration_{_prec}_layer_by_layer"] = Case(_iteration_inputs(_prec), _iteration_run(_prec, False, fused_chain=False),
                                                      spread=True)


# ----------------------------------------------------------------------------------------------------------------------
# render() on a GaussianModel: RGB training with sparse Adam across a densification and a relocation
# ----------------------------------------------------------------------------------------------------------------------
_ORACLE = {}  # the session's oracle, for the cases that check themselves against a CPU restatement while they run
W_T, H_T, N_T = 64, 48, 500  # the toy scene of tests/test_densify_gpu.py


def _model_inputs(n, d, w, h, mult, dead=0.0):
    def make(seed):
        from gags_amd import synthetic as syn
        p = syn.make_gaussians(n, d, w, h, seed=seed, scale0=syn.SCALE0 * mult)
        if dead:
            g = torch.Generator().manual_seed(seed + 5)
            p["opacity_logit"][torch.rand(n, generator=g) < dead] = -10.0
        return {f"pc.{k}": v for k, v in p.items()}
    return make


def _training_inputs(seed):
    t = _model_inputs(N_T, 16, W_T, H_T, 24)(seed)
    t["gt"] = torch.rand(3, H_T, W_T, generator=torch.Generator().manual_seed(seed + 1))
    return t


def _training_run(dev):
    """tests/test_selective_adam_gpu.py::test_rgb_training_with_sparse_adam_across_densify_and_relocation cut to three steps, a
    densify_and_prune, a step, a relocation, a step.  The RGB backward adds with fp32 atomics and Adam (eps = 1e-15) turns that
    noise into +-lr, so two runs of the loop are not comparable and every step is re-anchored instead, by the two tests this
    loop is taken from: _rgb_step compares every parameter and both moments of all seven tensors, bit for bit, with the
    restatement applied to the state as it stood and the gradients as they came out; and those gradients are compared with a
    stateless recomputation from a snapshot (new tensors, a fresh context, nothing carried) to 3072 * 2^-23 of the tensor's
    largest magnitude, the bound of test_steps_across_a_densify_equal_the_stateless_step (twice the worst-case reordering
    error of a sum of 64 * 48 terms; test_densify_gpu.atomic_reorder_rel).
    This case is judged by the asserts made inside the run, not by its return value, and those asserts read parameters and
    moments back to the host (.cpu()), which drains the side stream before and after opt.step: a mis-streamed Adam launch HERE
    is caught by the handle audit only.  Adam by value on a side stream is the case selective_adam_eight_tensors."""
    import test_densify_gpu as DENS
    import test_selective_adam_gpu as SA
    from gags_amd import losses, synthetic as syn
    from gags_amd.gaussian_renderer import render
    from gags_amd.rasterization import RasterContext
    pc = _model_on(dev)
    cam = syn.make_camera(W_T, H_T, view=3, device=DEV)
    bg, gt = torch.zeros(3, device=DEV), dev["gt"]
    opt = pc.training_setup_rgb(SA.ARGS, optimizer_type="sparse_adam")
    ctx = RasterContext()
    rel = DENS.atomic_reorder_rel(W_T * H_T)
    res = {}

    def step(label):
        snap = DENS._snapshot_model(pc)
        spkg = render(cam, snap, None, bg, feature_mode=False, context=DENS._stateless_context())
        (losses.photometric_loss(spkg["render"], gt) + 1e-3 * snap._semantic_feature.sum()).backward()
        SA._rgb_step(_ORACLE["oracle"], pc, opt, cam, bg, gt, ctx, label)
        for a in DENS.STORED:
            got, want = getattr(pc, a).grad, getattr(snap, a).grad
            scale = float(want.abs().max())
            err = float((got - want).abs().max())
            assert scale > 0 and err <= rel * scale, (label, a, err, scale)
        res[f"{label}.n"] = pc._xyz.shape[0]

    for k in range(3):
        step(f"step{k}")
    pc.densify_and_prune(0.0002, 0.005, 5.0, None, generator=torch.Generator(device=DEV).manual_seed(4))
    assert pc._xyz.shape[0] != N_T
    step("after_densify")
    with torch.no_grad():
        pc._opacity[torch.tensor([5, 17, 40], device=DEV)] = -10.0
    assert pc.relocate_gs(generator=torch.Generator(device=DEV).manual_seed(1)) >= 3
    step("after_relocation")
    return {"steps": len(res)}


CASES["model_rgb_training_sparse_adam"] = Case(_training_inputs, _training_run)


def _stored(pc):
    from gags_amd import densify
    out = {}
    for name, attr in densify.GROUPS:
        p = getattr(pc, attr, None)
        if p is not None:
            out[name] = p.detach()
            st = pc.optimizer.state.get(p, {}) if pc.optimizer is not None else {}
            for k in ("exp_avg", "exp_avg_sq"):
                if k in st:
                    out[f"{name}.{k}"] = st[k]
    return out


def _densify_inputs(seed):
    t = _model_inputs(N_T, 16, W_T, H_T, 24)(seed)
    g = torch.Generator().manual_seed(seed + 2)
    t["denom"] = torch.randint(1, 4, (N_T, 1), generator=g).float()
    t["accum"] = t["denom"] * 0.0006 * torch.rand(N_T, 1, generator=g)
    t["max_radii"] = 30.0 * torch.rand(N_T, generator=g)
    for k in ("xyz", "scaling_log", "rotation", "opacity_logit", "features_dc", "features_rest", "semantic_feature"):
        t[f"grad.{k}"] = torch.randn(t[f"pc.{k}"].shape, generator=g)
    return t


def _densify_run(dev):
    import test_selective_adam_gpu as SA
    from gags_amd import densify
    pc = _model_on(dev)
    opt = pc.training_setup_rgb(SA.ARGS)
    names = dict(xyz="xyz", scaling="scaling_log", rotation="rotation", opacity="opacity_logit", f_dc="features_dc",
                 f_rest="features_rest", semantic_feature="semantic_feature")
    for name, attr in densify.GROUPS:  # one optimizer step: the moments exist and are gathered with their rows
        p = getattr(pc, attr)
        p.grad = dev[f"grad.{names[name]}"].reshape(p.shape).clone()
    opt.step()
    opt.zero_grad(set_to_none=True)
    pc.xyz_gradient_accum, pc.denom, pc.max_radii2D = dev["accum"], dev["denom"], dev["max_radii"]
    pc.densify_and_prune(0.0002, 0.005, 5.0, 20, generator=torch.Generator(device=DEV).manual_seed(4))
    res = {"n": pc._xyz.shape[0], **{f"densified.{k}": v.clone() for k, v in _stored(pc).items()}}
    pc.reset_opacity()
    res.update({f"reset.{k}": v.clone() for k, v in _stored(pc).items()})
    res.update(accum=pc.xyz_gradient_accum, denom=pc.denom, max_radii=pc.max_radii2D)
    return res


CASES["densify_and_prune_reset_opacity"] = Case(_densify_inputs, _densify_run)


def _mcmc_run(dev):
    import test_selective_adam_gpu as SA
    from gags_amd import mcmc
    pc = _model_on(dev)
    pc.training_setup_rgb(SA.ARGS)
    gen = torch.Generator(device=DEV).manual_seed(9)
    res = {"n_relocated": pc.relocate_gs(generator=gen)}
    res.update({f"relocated.{k}": v.clone() for k, v in _stored(pc).items()})
    res["n_added"] = pc.add_new_gs(int(1.02 * N_T), generator=gen)
    mcmc.inject_noise(pc, 0.5, generator=gen)
    res.update({f"grown.{k}": v.clone() for k, v in _stored(pc).items()})
    reg = mcmc.regularisation(pc)
    reg.backward()
    res.update(reg=reg.detach().reshape(1), v_opacity=pc._opacity.grad, v_scaling=pc._scaling.grad)
    draws, counts, cdf = mcmc.sample(torch.sigmoid(pc._opacity.detach().reshape(-1).double()), 77, generator=gen)
    res.update(draws=draws, counts=counts, cdf=cdf)
    return res


CASES["mcmc_relocate_grow_noise_regularise"] = Case(_model_inputs(N_T, 16, W_T, H_T, 24, dead=0.05), _mcmc_run)


# ----------------------------------------------------------------------------------------------------------------------
# the by-view exchange as ONE process runs it (OverlappedGradReducer(loopback=...)): dist.py's single-process entries
# ----------------------------------------------------------------------------------------------------------------------
def _loopback_run(w, h, d, wire=None):
    def run(dev):
        from gags_amd.dist import OverlappedGradReducer
        from gags_amd.rasterization import RasterContext, rasterization
        ctx = RasterContext()
        cols = dev["colors"].detach().requires_grad_(True)
        red = OverlappedGradReducer(mode="rs_ag", rows="union", param=cols, loopback=(8, int(0.8 * N_R)), context=ctx, wire=wire)
        out, _, _ = rasterization(dev["means"], dev["quats"], dev["scales"], dev["opacities"], cols, dev["viewmat0"][None],
                                  dev["K"][None], w, h, backgrounds=dev["bg"][None], context=ctx)
        loss = (out[0] * dev["v_out0"]).sum()
        with red:
            loss.backward()
        red.finish(cols.grad)
        return {"out": out, "grad": cols.grad, "rows_exchanged": red.rows_exchanged, "_own_streams": [red.comm.cuda_stream]}
    return run


CASES["loopback_exchange_d256"] = Case(_raster_inputs(256, 112, 80), _loopback_run(112, 80, 256))
CASES["loopback_exchange_d256_bf16_wire"] = Case(_raster_inputs(256, 97, 61), _loopback_run(97, 61, 256, wire="bf16"))


# ----------------------------------------------------------------------------------------------------------------------
# offline families, one call each
# ----------------------------------------------------------------------------------------------------------------------
def _decoder_inputs(precision="exact", extra=None):
    def make(seed):
        from gags_amd.decoders import CNN_decoder
        torch.manual_seed(seed)
        t = {f"dec.{k}": v.detach().clone() for k, v in CNN_decoder(16, 512, precision).state_dict().items()}
        g = torch.Generator().manual_seed(seed + 3)
        t["pos"] = torch.nn.functional.normalize(torch.randn(3, 512, generator=g), dim=-1)
        t["neg"] = torch.nn.functional.normalize(torch.randn(4, 512, generator=g), dim=-1)
        t.update(extra(seed, g) if extra else {})
        return t
    return make


def _decoder_on(dev, precision):
    from gags_amd.decoders import CNN_decoder
    m = CNN_decoder(16, 512, precision).to(DEV)
    for k, p in list(m.named_parameters()) + list(m.named_buffers()):
        p.data = dev[f"dec.{k}"]
    return m


def _points_extra(seed, g, n=3000):
    return {"sem": torch.randn(n, 16, generator=g) / 4, "xyz": torch.rand(n, 3, generator=g)}


def _query_points_run(precision, fused):
    def run(dev):
        from gags_amd.pointquery import query_points, smooth_point_mask
        from gags_amd.relevancy import RelevancyHead
        dec, head = _decoder_on(dev, precision), RelevancyHead(dev["pos"], dev["neg"])
        res = query_points(dev["sem"], dev["xyz"], dec, head, rel_thresh=0.4, radius=0.1, threshold=10, chunk=1024, fused=fused)
        out, cnt = smooth_point_mask(res["mask_raw"], dev["xyz"], 0.1, 10, return_counts=True)
        return {**res, "smooth": out, "counts": cnt}
    return run


CASES["query_points_and_smooth"] = Case(_decoder_inputs("exact", _points_extra), _query_points_run("exact", False))
CASES["query_points_fused_f16"] = Case(_decoder_inputs("f16", _points_extra), _query_points_run("f16", True))


def _view_extra(seed, g, h=37, w=53):
    return {"fmap": torch.randn(h, w, 16, generator=g) / 4, "image": torch.rand(h, w, 3, generator=g),
            "gt_fmap": torch.randn(512, h, w, generator=g) / 20, "mask": (torch.rand(h, w, generator=g) < 0.7).float()}


def _query_view_run(precision):
    def run(dev):
        from gags_amd import queryvis as Q
        from gags_amd.relevancy import RelevancyHead, activate_maps
        dec, head = _decoder_on(dev, precision), RelevancyHead(dev["pos"], dev["neg"])
        fmap = dev["fmap"].permute(2, 0, 1)  # (what render() hands over: [H,W,C] memory behind a [C,H,W] view)
        res = {}
        for call in (0, 1):  # (the second call hits queryvis' cache of the colour table)
            r = Q.query_view(fmap, dec, head, dev["image"], return_uint8=True)
            res.update({f"{call}.{k}": v for k, v in r.items()})
        valid = dec.query(fmap, head)
        act = activate_maps(valid, thresh=0.4)
        res.update({f"act.{k}": v for k, v in act.items()})
        res["valid"] = valid
        cm = Q.colour_maps(act, dev["image"])
        again = Q.colour_maps(act, dev["image"], avg2=cm["avg2"])  # (the colour kernel alone)
        res.update({f"colour.{k}": v for k, v in again.items()})
        with torch.no_grad():
            l2, mp, mg = Q.feature_loss_maps(dec(fmap), dev["gt_fmap"], dev["mask"])
        res.update(l2=l2, mean_abs_pred=mp, mean_abs_gt=mg)
        return res
    return run


CASES["query_images_and_loss_maps"] = Case(_decoder_inputs("exact", _view_extra), _query_view_run("exact"))
CASES["query_images_f16_fused_query"] = Case(_decoder_inputs("f16", _view_extra), _query_view_run("f16"))
CASES["query_images_bf16_fused_query"] = Case(_decoder_inputs("bf16", _view_extra), _query_view_run("bf16"))


def _cloud_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    return {"points": torch.rand(1000, 3, generator=g), "colors": torch.rand(1000, 3, generator=g)}


def _knn_run(dev):
    from gags_amd import knn
    from gags_amd.scene import BasicPointCloud, GaussianModel
    res = {"dist2": knn.dist2(dev["points"])}
    pts, cols = dev["points"].cpu().numpy(), dev["colors"].cpu().numpy()  # (create_from_pcd takes host arrays)
    m = GaussianModel(3).create_from_pcd(BasicPointCloud(points=pts, colors=cols, normals=np.zeros_like(pts)), 1.0, 16, False)
    for a in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "_semantic_feature"):
        res[a] = getattr(m, a).detach()
    return res


CASES["knn3_dist2_and_create_from_pcd"] = Case(_cloud_inputs, _knn_run)


def _rect_masks(rng, m, h, w):
    """m masks [m, h, w] uint8: rectangles at least three pixels wide and high with a tenth of their pixels knocked out (the first
    and last pixel kept), some shifted copies of an earlier one -- what mask_nms reacts to, and boxes cut_tiles accepts."""
    out = np.zeros((m, h, w), np.uint8)
    for k in range(m):
        if k and rng.random() < 0.4:
            out[k] = np.roll(out[rng.integers(k)], (int(rng.integers(-1, 2)), int(rng.integers(-1, 2))), (0, 1))
            continue
        hh, ww = int(rng.integers(3, h // 2)), int(rng.integers(3, w // 2))
        y, x = int(rng.integers(1, h - hh - 1)), int(rng.integers(1, w - ww - 1))
        box = (rng.random((hh, ww)) > 0.1).astype(np.uint8)
        box[0, :] = box[-1, :] = box[:, 0] = box[:, -1] = 1
        out[k, y:y + hh, x:x + ww] = box
    return out


def _masks_inputs(seed, m=33, h=37, w=70):
    rng = np.random.default_rng(seed)
    return {"masks": torch.from_numpy(_rect_masks(rng, m, h, w)), "scores": torch.from_numpy(rng.uniform(0.6, 1.0, m)),
            "image": torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))}


def _masks_run(dev):
    from gags_amd import sam_masks as SM, tilecut as TC
    masks, scores = dev["masks"], dev["scores"]
    h, w = masks.shape[1:]
    bits, area = SM.pack_masks(masks)
    inter = SM.pair_intersections(bits)
    order = torch.argsort(scores, descending=True, stable=True)
    res = {"bits": bits, "area": area, "inter": inter, "colmax": SM.column_maxima(inter, area, order),
           "selected": SM.mask_nms(masks, scores)}
    res["seg_map"] = SM.seg_map(bits, torch.sort(res["selected"]).values, h, w, offset=2)
    maps, lengths = SM.assemble_seg_maps([masks[:9], masks[9:9], masks[9:10], masks[10:]])
    res.update(maps=maps, lengths=lengths)
    boxes = TC.mask_boxes(bits, h, w)
    u8, f32 = TC.cut_tiles(dev["image"], bits, TC.sam_xywh(boxes), dtype=None)
    res.update(boxes=boxes, tiles_u8=u8, tiles_f32=f32)
    return res


CASES["sam_masks_nms_seg_maps_and_tilecut"] = Case(_masks_inputs, _masks_run)


def _featurevis_run(dev):
    from gags_amd import featurevis as FV
    feature = dev["fmap"].permute(2, 0, 1)
    s, g = FV.feature_moments(feature)
    vis, u8 = FV.feature_visualize(feature, return_uint8=True)
    t = FV.feature_project(feature, dev["mean"], dev["comps"])
    return {"sum": s, "gram": g, "vis": vis, "u8": u8, "t": t, "select": FV.order_statistics(t, [0, 7, 100, t.numel() - 1])}


def _featurevis_inputs(seed, h=37, w=53):
    g = torch.Generator().manual_seed(seed)
    return {"fmap": torch.randn(h, w, 16, generator=g), "mean": torch.randn(16, generator=g) / 4,
            "comps": torch.randn(3, 16, generator=g)}


CASES["featurevis_moments_project_select"] = Case(_featurevis_inputs, _featurevis_run)


def _depth_inputs(seed, n=700, c=3, h=48, w=64):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.cat([2 * torch.rand(n, 2, generator=g) - 1, 2 + 2 * torch.rand(n, 1, generator=g)], 1)
    vm = torch.eye(4).repeat(c, 1, 1)
    vm[:, :3, 3] = 0.3 * (torch.rand(c, 3, generator=g) - 0.5)
    K = torch.tensor([[40.0, 0, w / 2], [0, 40.0, h / 2], [0, 0, 1]]).repeat(c, 1, 1)
    depths = 3 + torch.rand(c, h, w, generator=g)
    samples = torch.where(torch.rand(c, h, w, generator=g) < 0.3, depths, torch.zeros(()))
    return {"xyz": xyz, "viewmats": vm, "Ks": K, "depths": depths, "samples": samples}


def _depth_run(dev):
    from gags_amd import depthsample as DS, prompts as PR
    x, v, k, d = dev["xyz"], dev["viewmats"], dev["Ks"], dev["depths"]
    mapping, visible = DS.point_pixel_mapping(x, v, k, d)
    samples, md = DS.depth_samples(x, v, k, d, return_min_depth=True)
    res = {"mapping": mapping, "visible": visible, "samples": samples, "min_depth": md}
    res.update({f"stats.{n}": t for n, t in PR.crop_stats(d, dev["samples"], n_per_side=4).items()})
    res.update({f"stats_depth_only.{n}": t for n, t in PR.crop_stats(d, None, n_per_side=8).items()})
    return res


CASES["depthsample_map_scatter_and_prompt_grids"] = Case(_depth_inputs, _depth_run)


def _adam_inputs(seed, n=257):
    import test_selective_adam_gpu as SA
    g = torch.Generator().manual_seed(seed)
    t = {"vis": (torch.rand(n, generator=g) < 0.3).to(torch.uint8), "table": torch.randn(n, 48, generator=g)}
    for i, shape in enumerate(SA.RGB_SHAPES + ((2, 2),)):
        t[f"p{i}"] = torch.randn(n, *shape, generator=g)
        for step in (0, 1):
            t[f"g{i}.{step}"] = torch.randn(n, *shape, generator=g)
    for step in (0, 1):
        t[f"gtable.{step}"] = torch.randn(n, 48, generator=g) * (torch.rand(n, 1, generator=g) < 0.5)
    return t


def _adam_run(dev):
    from gags_amd.optim import FeatureAdam, SelectiveAdam
    params = [torch.nn.Parameter(dev[f"p{i}"]) for i in range(8)]
    table = torch.nn.Parameter(dev["table"])
    sel = SelectiveAdam([{"params": [p], "lr": 1e-3 * (i + 1), "name": f"t{i}"} for i, p in enumerate(params)], lr=0.0, eps=1e-15)
    skip = SelectiveAdam([{"params": [table], "lr": 1e-3, "name": "table"}], lr=0.0, eps=1e-15, skip_zero_rows=True)
    plain = FeatureAdam([{"params": [torch.nn.Parameter(dev["table"].clone())], "lr": 1e-3}], lr=0.0, eps=1e-15)
    for step in (0, 1):
        for i, p in enumerate(params):
            p.grad = dev[f"g{i}.{step}"]
        table.grad = plain.param_groups[0]["params"][0].grad = dev[f"gtable.{step}"]
        sel.step(dev["vis"])
        skip.step()
        plain.step()
    res = {}
    for name, opt in (("sel", sel), ("skip", skip), ("plain", plain)):
        for i, grp in enumerate(opt.param_groups):
            p = grp["params"][0]
            res.update({f"{name}.{i}": p.detach(), f"{name}.{i}.m": opt.state[p]["exp_avg"], f"{name}.{i}.v": opt.state[p]["exp_avg_sq"]})
    return res


CASES["selective_adam_eight_tensors"] = Case(_adam_inputs, _adam_run)


def _sh_inputs(seed, n=700):
    g = torch.Generator().manual_seed(seed)
    return {"coeffs": torch.randn(n, 16, 3, generator=g) / 3, "means": 4 * torch.randn(n, 3, generator=g),
            "campos": torch.randn(3, generator=g), "v_col": torch.randn(n, 3, generator=g),
            "radii": torch.randint(0, 3, (n,), generator=g, dtype=torch.int32)}


def _sh_run(dev):
    """_SH on its own (tests/test_parity_gpu.py::test_sh_view_direction_gradient_matches_the_reference_eval_sh drives it this
    way): colours, and the gradients of the coefficients, the positions and the camera position -- the last one a column sum
    in double in a fixed order (gags_colsum_f32).  Through rasterization() these sit behind the narrow VALU backward's atomics."""
    from gags_amd.rasterization import _SH
    res = {}
    for deg in (3, 1):
        leaf = {k: dev[k].detach().requires_grad_(True) for k in ("coeffs", "means", "campos")}
        col = _SH.apply(leaf["coeffs"], leaf["means"], leaf["campos"], dev["radii"], deg)
        (col * dev["v_col"]).sum().backward()
        res.update({f"deg{deg}.col": col, **{f"deg{deg}.grad.{k}": v.grad for k, v in leaf.items()}})
    return res


CASES["sh_colours_directions_and_camera_position"] = Case(_sh_inputs, _sh_run)


def _losses_inputs(seed, h=24, w=32):
    g = torch.Generator().manual_seed(seed)
    seg = torch.randint(-1, 21, (4, h // 4, w // 4), generator=g).float().repeat_interleave(4, 1).repeat_interleave(4, 2)
    return {"emb": torch.nn.functional.normalize(torch.randn(21, 512, generator=g), dim=-1), "seg": seg.contiguous(),
            "scale": torch.softmax(torch.randn(3, h, w, generator=g), 0), "loss_map": torch.rand(h, w, generator=g),
            "x": torch.randn(16, h, w, generator=g), "v_feat": torch.randn(512, h, w, generator=g)}


def _losses_run(dev):
    """The loss kernels a direct caller reaches and the composed iteration does not: the ground-truth assembly on its own (and
    its max mode), both kernels of the segment moments, the region variance without the tee, and the remembered segment-id
    bound (losses._NSEG_CACHE: filled and hit within the run; the composed iteration never uses it)."""
    from gags_amd import losses as L
    res = {}
    scale = dev["scale"].detach().requires_grad_(True)
    feat, mask = L.read_sam_clip_feature(dev["emb"], dev["seg"], scale)
    (feat * dev["v_feat"]).sum().backward()
    res.update(feat=feat, mask=mask.float(), v_scale=scale.grad)  # (masks as floats: _compare subtracts)
    fmax, mmax = L.read_sam_clip_feature(dev["emb"], dev["seg"], dev["scale"], max_mode=True)
    res.update(feat_max=fmax, mask_max=mmax.float())
    # a map without a bound handed on: the first loss fills losses._NSEG_CACHE (a readback of the map's maximum on the current
    # stream), every later one hits it
    level0, entry = dev["seg"][0], None
    assert getattr(level0, "_gags_n_seg", None) is None and id(level0) not in L._NSEG_CACHE
    for call in (0, 1):
        lm = dev["loss_map"].detach().requires_grad_(True)
        x = dev["x"].detach().requires_grad_(True)
        bal = L.Scale_balance_loss(lm, level0, None, mix_seg=True)
        assert call == 0 or L._NSEG_CACHE[id(level0)] is entry, "the second call did not hit the cache"
        entry = L._NSEG_CACHE[id(level0)]
        var = L.scale_region_regulation_loss(x, level0, mix_seg=True)
        assert L._NSEG_CACHE[id(level0)] is entry
        (bal + var).backward()
        res.update({f"cached{call}.balance": bal.detach().reshape(1), f"cached{call}.v_loss_map": lm.grad,
                    f"cached{call}.regionvar": var.detach().reshape(1), f"cached{call}.v_x": x.grad})
    res["n_seg"] = torch.tensor([float(entry[3])])
    trained = L.get_trained_seg(dev["seg"], dev["scale"], n_seg=21)
    res["trained"] = trained
    saved = L.RUNS
    try:
        for runs in (True, False):
            L.RUNS = runs
            lm = dev["loss_map"].detach().requires_grad_(True)
            x = dev["x"].detach().requires_grad_(True)
            bal = L.Scale_balance_loss(lm, trained, None, mix_seg=True)
            var = L.scale_region_regulation_loss(x, trained, mix_seg=True)
            (bal + var).backward()
            res.update({f"runs{int(runs)}.balance": bal.detach().reshape(1), f"runs{int(runs)}.v_loss_map": lm.grad,
                        f"runs{int(runs)}.regionvar": var.detach().reshape(1), f"runs{int(runs)}.v_x": x.grad})
    finally:
        L.RUNS = saved
    sc = dev["scale"].detach().requires_grad_(True)
    ce = L.scale_regulation_loss(sc)
    ce.backward()
    res.update(ce=ce.detach().reshape(1), v_ce=sc.grad)
    return res


CASES["losses_called_directly"] = Case(_losses_inputs, _losses_run, spread=True)


# ----------------------------------------------------------------------------------------------------------------------
# parts 2 and 3: the comparison and the audit
# ----------------------------------------------------------------------------------------------------------------------
def _check_case(name, oracle, got, calls, stream):
    case = CASES[name]
    refs = _reference(name)
    if case.spread:
        MS._compare(got, refs[0], refs[1], name, {})
    else:
        skip = case.loose(oracle, case.inputs(REAL_SEED), got, refs[0]) if case.loose is not None else ()
        bad = _mismatches(got, refs[0], skip)
        assert not bad, (name, bad)


def _check_audit(name, calls, stream):
    streamed = [c for c in calls if c[0] in SH.streamed_entries()]
    assert streamed, (name, "no streamed entry was called")
    own = {int(h) for h in getattr(calls, "own", ())}
    assert 0 not in own
    wrong = [w for w in SH.audit_streams(calls, stream) if w[2] not in own]
    assert not wrong, (name, wrong[:8])


@pytest.mark.parametrize("name", list(CASES))
def test_side_stream_behind_late_producers_equals_the_default_stream(oracle, name):
    """Part 2 (values) and part 3 (every streamed entry received the side stream's handle) for one case of CASES."""
    _ORACLE["oracle"] = oracle
    _reference(name)
    got, calls, stream = _side_run(CASES[name])
    RECORDED[name] = {c[0] for c in calls}
    _check_audit(name, calls, stream)
    _check_case(name, oracle, got, calls, stream)


# ----------------------------------------------------------------------------------------------------------------------
# part 6: the harness bites
# ----------------------------------------------------------------------------------------------------------------------
MUTANT_CASE = "raster_d16_forward"


def test_a_wrapper_that_passes_the_null_stream_is_caught_by_value_and_by_the_audit(oracle, monkeypatch):
    """gags_amd._lib.stream returning the null stream's handle while the caller is on the side stream: every kernel of the
    D = 16 forward runs ahead of the copy of its inputs, on the decoy (valid buffers, true sizes: a wrong answer, no fault).
    The audit names the calls, and the render differs from the reference."""
    import ctypes
    from gags_amd import _lib
    ref = _reference(MUTANT_CASE)[0]
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "stream", lambda device=None: ctypes.c_void_p(0))
        got, calls, stream = _side_run(CASES[MUTANT_CASE])
    with pytest.raises(AssertionError):
        _check_audit(MUTANT_CASE, calls, stream)
    assert len(SH.audit_streams(calls, stream)) == sum(1 for c in calls if c[0] in SH.streamed_entries())
    assert not torch.equal(got["0.out"], ref["0.out"])
    with pytest.raises(AssertionError):
        _check_case(MUTANT_CASE, oracle, got, calls, stream)


def test_a_producer_on_the_default_stream_is_caught_by_value(oracle):
    """The torch-side twin: the copy that brings the real inputs into the case's buffers issued on the DEFAULT stream.  It runs
    at once, while its own producer (the staging copy on the side stream) is still behind the first delay, and copies the decoy;
    the kernels, all on the right stream, then render the decoy.  The audit cannot see this one; the values do."""
    ref = _reference(MUTANT_CASE)[0]
    got, calls, stream = _side_run(CASES[MUTANT_CASE], copy_on_default=True)
    _check_audit(MUTANT_CASE, calls, stream)
    assert not torch.equal(got["0.out"], ref["0.out"])
    with pytest.raises(AssertionError):
        _check_case(MUTANT_CASE, oracle, got, calls, stream)


# ----------------------------------------------------------------------------------------------------------------------
# part 5: state carried across a change of stream
# ----------------------------------------------------------------------------------------------------------------------
STAGED = PAR.STAGED  # argument 9 of the staged entry: the row count its scratch was sized by


def _stateless_grad_and_rows(pc, feat0, view, G, w, h):
    with spy_entries(STAGED) as staged:
        want = MS._stateless_feature_grad(pc, feat0, view, G, w, h)
    assert staged
    return want, staged[0][1][9]


@pytest.mark.parametrize("capacity", [False, True], ids=["early_rowmap", "capacity_mode"])
@pytest.mark.parametrize("d", [128, 513])
def test_six_steps_alternating_between_two_streams_equal_the_stateless_step(d, capacity):
    """render -> <render, G> -> backward -> FeatureAdam.step -> zero_grad(set_to_none=True) six times in ONE RasterContext
    (tests/test_multistep_gpu.py::test_twelve_steps_equal_the_stateless_step_bit_for_bit), the steps alternating between two
    side streams, each under late_producers; the caller orders the streams as torch requires for any tensor shared across
    streams (b.wait_stream(a) before a step on b, and the reverse), and nothing else does: no block waits for its stream, the
    gradients are compared and the delays checked once all steps are enqueued.
    early_rowmap (the default context): the persistent gradient buffer and its flag arrays, the pinned pool and the early row
    map's event cross a stream boundary at every step.  capacity_mode (which switches those off, raster_route._route): the
    remembered capacities cap_isects / cap_rows, the _DeferredCount readbacks, the context's own side stream and its one
    pinned word do -- every shape's capacity is filled by a step on one stream and hit by a step on the other (asserted: from
    the second step on, the staged entry reads its row count from the device).
    Every step's gradient equals the stateless recomputation from a snapshot of its inputs, bit for bit, and every streamed
    entry received the stream of its step.  Then a forward on `a` that is never differentiated, followed at once by a
    differentiated forward on `b`: _EarlyRowmap.__del__ runs while the copy into its pinned word is in flight (asserted) and
    drops the word; the second step's row count and gradient are the stateless ones.  (The caller's wait_stream orders the two
    copies on the device as well, so a __del__ that recycled the word would not be caught here: that rule is pinned with stub
    events by tests/test_host_cpu.py.)"""
    from gags_amd import rasterization as R, synthetic as syn
    from gags_amd.gaussian_renderer import render
    n, w, h = 6000, 200, 138
    pc = MS._make_model(n, d, w, h, seed=4, mult=3)
    opt = pc.training_setup()
    cams = {v: syn.make_camera(w, h, view=v, device=DEV) for v in (0, 7, 3)}
    G = syn.make_cotangent(d, h, w, seed=2, device=DEV)
    bg = torch.zeros(3, device=DEV)
    ctx = R.RasterContext(capacity_mode=capacity)
    assert ctx.capacity_mode == capacity and ctx.keep_grad_buffer and ctx.early_rowmap
    torch.cuda.synchronize()
    a = SH.concurrent_stream()
    b = SH.concurrent_stream(avoid=(a,))
    ptrs, prev, pending, pairs = set(), None, [], []

    def step(s, view, label):
        """One differentiated step on `s` under late_producers and its stateless twin (outside the wrapper, same stream)."""
        with torch.cuda.stream(s):
            feat0 = pc._semantic_feature.detach().clone()
            hit = bool(ctx.cap_rows)  # (remembered per (N, width, height): every step after the first finds a capacity)
            with SH.late_producers(s, pending) as calls:
                (render(cams[view], pc, None, bg, feature_mode=True, context=ctx)["render"] * G).sum().backward()
                got = pc._semantic_feature.grad.detach().clone()
                staged = [c[1] for c in calls if c[0] == STAGED]
                opt.step()
            assert not SH.audit_streams(calls, s), (label, SH.audit_streams(calls, s)[:4])
            want, want_rows = _stateless_grad_and_rows(pc, feat0, view, G, w, h)
            assert staged
            if capacity:
                # (argument 18: the row count on the device, argument 9 then a capacity; a capacity that proved too small is
                # followed by an exact re-run, so the last call covers the rows either way)
                assert (staged[0][18] is not None) == hit and staged[-1][9] >= want_rows, (label, hit, staged[-1][9], want_rows)
                assert (n, w, h, DEV.index) in ctx.cap_isects and (n, w, h, DEV.index) in ctx.cap_rows, label
            else:
                assert all(c[9] == want_rows and c[18] is None for c in staged), (label, [c[9] for c in staged], want_rows)
                ptrs.update(MS._kept_ptrs(ctx))
            pairs.append((label, got, want))
            opt.zero_grad(set_to_none=True)
        return calls

    for t, view in enumerate((0, 7, 3, 3, 0, 7)):
        s = (a, b)[t % 2]
        if prev is not None:
            s.wait_stream(prev)
        step(s, view, f"step {t}")
        prev = s
    # a forward on `a` that nobody differentiates, then at once a differentiated forward on `b`
    a.wait_stream(prev)
    with torch.cuda.stream(a), SH.late_producers(a, pending) as calls_a:
        dropped = render(cams[7], pc, None, bg, feature_mode=True, context=ctx)["render"]
        assert dropped.requires_grad
        pool = sum(len(v) for v in ctx._pinned_pool.values())
        del dropped
        if not capacity:
            assert sum(len(v) for v in ctx._pinned_pool.values()) == pool, "the unused row map's word went back while its copy was in flight"
    b.wait_stream(a)
    calls_b = step(b, 3, "after the dropped forward")
    if not capacity:
        assert "gags_bwd_rowmap" in {c[0] for c in calls_a}  # (the dropped forward did enqueue its row map)
    assert not SH.audit_streams(calls_a, a) and calls_b
    SH.check_delays(pending)
    for label, got, want in pairs:
        assert float(want.abs().max()) > 0, label
        assert torch.equal(got, want), (d, label, float((got - want).abs().max()))
    if not capacity:
        assert len(ptrs) == 1, "the persistent buffer was not reused over the steps"
    assert all(v == 0 for v in ctx._kept_fails.values()), ctx._kept_fails


# ----------------------------------------------------------------------------------------------------------------------
# part 4: coverage is accounted for (keep this test last)
# ----------------------------------------------------------------------------------------------------------------------
def test_every_streamed_entry_the_package_names_was_reached_on_a_side_stream():
    """The union of the entries recorded over all cases contains every entry that takes a stream and is named in some
    gags_amd/*.py other than _lib.py (computed from the sources here; the 16-bit twins are reached through their base names).
    Entries no module names are printed: a user of the package cannot reach them."""
    from gags_amd import _lib
    if set(RECORDED) != set(CASES):
        pytest.skip(f"only {len(RECORDED)} of {len(CASES)} cases ran in this session: the union would not mean anything")
    streamed = SH.streamed_entries() & set(_lib.SIGNATURES)
    named = SH.package_named_entries()
    reached = set().union(*RECORDED.values())
    print("streamed entries no module of the package names:", sorted(streamed - set(named)))
    missing = sorted(n for n in streamed & set(named) if n not in reached)
    assert not missing, "no case reaches: " + ", ".join(f"{n} ({'/'.join(named[n])})" for n in missing)
