"""N8 (include/gags_next.h): adaptive density control without a GPU -- the restatement tests/densify_ref.py against the
reference's own results (tests/golden/densify_vectors.npz, written by make_golden_densify.py) in float32 and float64, the output
order of the contract, the position schedule, the new entry points' declarations and argument checks, and the Python layer's
refusal of CPU tensors."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import densify_ref as R  # noqa: E402

Z = np.load(os.path.join(ROOT, "golden", "densify_vectors.npz"))
CASES = [str(c) for c in Z["cases"]]
N8 = ("gags_densify_stats", "gags_densify_decide", "gags_densify_plan", "gags_densify_gather", "gags_densify_children",
      "gags_reset_opacity")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _par(name):
    pd, max_grad, min_op, extent, mss, shd, step = (float(v) for v in Z[name + "_par"])
    return pd, max_grad, min_op, extent, (mss or None), int(shd), step


def _run_ref(name, dtype):
    pd, max_grad, min_op, extent, mss, _, _ = _par(name)
    t = {k: torch.from_numpy(Z[f"{name}_{k}"]).to(dtype) for k in R.NAMES}
    # the moments the fixture stores as inputs are the float32 run's; they are only copied or zeroed
    mom = {k: (torch.from_numpy(Z[f"{name}_m1_{k}"]).to(dtype), torch.from_numpy(Z[f"{name}_m2_{k}"]).to(dtype)) for k in R.NAMES}
    return R.densify_and_prune(t, torch.from_numpy(Z[name + "_accum"]).to(dtype), torch.from_numpy(Z[name + "_denom"]).to(dtype),
                               pd, max_grad, min_op, extent, mss, torch.from_numpy(Z[name + "_Z"]).to(dtype), moments=mom)


def test_fixture_holds_every_case_and_is_small():
    assert os.path.getsize(os.path.join(ROOT, "golden", "densify_vectors.npz")) <= 1 << 20
    assert set(CASES) == {"mixed", "mixed_nomss", "sh0", "none", "allpruned", "allsplit", "tie_dense", "tie_world"}
    for name in CASES:
        assert Z[name + "_xyz"].shape[0] <= 300
        assert Z[name + "_f32_xyz"].dtype == np.float32 and Z[name + "_f64_xyz"].dtype == np.float64
    assert Z["sh0_f_rest"].shape[1:] == (0, 3) and Z["mixed_f_rest"].shape[1:] == (15, 3) and Z["mixed_semantic_feature"].shape[1] == 16
    assert Z["allpruned_f32_xyz"].shape[0] == 0 and Z["none_f32_xyz"].shape[0] == Z["none_xyz"].shape[0]
    assert (Z["allsplit_kind"] >= R.CHILD_A).all() and len(Z["allsplit_kind"]) == 2 * Z["allsplit_xyz"].shape[0]
    assert _par("mixed")[4] == 20 and _par("mixed_nomss")[4] is None and float(Z["mixed_max_radii"].max()) > 20
    norms = np.linalg.norm(Z["mixed_rotation"].astype(np.float64), axis=1)
    assert (np.abs(norms - 0.3) < 1e-5).any() and (np.abs(norms - 7) < 1e-4).any()
    with np.errstate(all="ignore"):
        g = Z["mixed_accum"] / Z["mixed_denom"]
    assert np.isnan(g).any() and np.isinf(g).any() and (g < 0).any()
    # the built ties are exact in float32 and in double
    assert (Z["tie_dense_scaling"][:12] == 0).all() and 0.01 * 100.0 == 1.0 and 0.1 * 10.0 == 1.0
    assert ((Z["tie_dense_accum"] / Z["tie_dense_denom"]) == np.float32(0.25)).sum() >= 12 and _par("tie_dense")[1] == 0.25


@pytest.mark.parametrize("tag,dtype", [("f32", torch.float32), ("f64", torch.float64)])
@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(name, tag, dtype):
    res = _run_ref(name, dtype)
    for k in R.NAMES:
        want = Z[f"{name}_{tag}_{k}"]
        assert tuple(res[k].shape) == want.shape, k
        assert np.array_equal(res[k].numpy(), want), k
        assert np.array_equal(res["moments"][k][0].numpy().astype(np.float32), Z[f"{name}_f32_m1_{k}"]), k
        assert np.array_equal(res["moments"][k][1].numpy().astype(np.float32), Z[f"{name}_f32_m2_{k}"]), k
    assert np.array_equal(res["src"].numpy(), Z[name + "_src"]) and np.array_equal(res["kind"].numpy(), Z[name + "_kind"])


@pytest.mark.parametrize("name", CASES)
def test_output_order_is_the_contracts(name):
    """Kept originals, surviving clones, first children, second children; each in source order; both children of a source
    survive together; kept rows are exactly the inputs' rows (bit for bit), clones copy their source."""
    src, kind = Z[name + "_src"].astype(np.int64), Z[name + "_kind"]
    assert (np.diff(kind.astype(int)) >= 0).all()
    for k in range(4):
        assert (np.diff(src[kind == k]) > 0).all()
    assert np.array_equal(src[kind == R.CHILD_A], src[kind == R.CHILD_B])
    assert not set(src[kind == R.KEEP]) & set(src[kind == R.CHILD_A])          # a split parent never keeps itself
    assert set(src[kind == R.CLONE]) <= set(src[kind == R.KEEP])                # a clone's source survives with it
    for k in R.NAMES:
        out, inp = Z[f"{name}_f32_{k}"], Z[f"{name}_{k}"]
        copied = kind <= R.CLONE if k in ("xyz", "scaling") else np.ones(len(kind), bool)
        assert np.array_equal(out[copied], inp[src[copied]]), k
        m1 = Z[f"{name}_f32_m1_{k}"]
        assert np.array_equal(m1[kind == R.KEEP], Z[f"{name}_m1_{k}"][src[kind == R.KEEP]]) and not m1[kind != R.KEEP].any()
    if (kind >= R.CHILD_A).any():
        assert not np.array_equal(Z[f"{name}_f32_xyz"][kind >= R.CHILD_A], Z[f"{name}_xyz"][src[kind >= R.CHILD_A]])


def test_a_parent_above_the_world_threshold_keeps_children_below_it():
    pd, max_grad, min_op, extent, mss, _, _ = _par("mixed")
    m = np.exp(Z["mixed_scaling"].astype(np.float64)).max(1)
    src, kind = Z["mixed_src"], Z["mixed_kind"]
    parents = set(src[kind == R.CHILD_A])
    big = {i for i in parents if m[i] > 0.1 * extent}
    assert len(big) >= 3 and all(m[i] / 1.6 < 0.1 * extent for i in big) and not big & set(src[kind == R.KEEP])


@pytest.mark.parametrize("tag,dtype", [("f32", torch.float32), ("f64", torch.float64)])
def test_statistics_and_reset_restatements_equal_the_reference(tag, dtype):
    n = Z["st_grad"].shape[1]
    acc, den, mr = torch.zeros(n, 1, dtype=dtype), torch.zeros(n, 1, dtype=dtype), torch.zeros(n, dtype=dtype)
    for v in range(3):
        acc, den, mr = R.add_stats(acc, den, mr, torch.from_numpy(Z["st_grad"][v]).to(dtype), torch.from_numpy(Z["st_radii"][v]),
                                   torch.from_numpy(Z["st_update"][v]), torch.from_numpy(Z["st_visible"][v]),
                                   int(Z["st_wh"][v, 0]), int(Z["st_wh"][v, 1]))
    assert np.array_equal(acc.numpy(), Z[f"st_{tag}_accum"]) and np.array_equal(den.numpy(), Z[f"st_{tag}_denom"])
    assert np.array_equal(mr.numpy(), Z[f"st_{tag}_max_radii"])
    assert (Z["st_wh"][:, 0] != Z["st_wh"][:, 1]).all() and (Z["st_update"][2] & ~Z["st_visible"][2]).any()
    got = R.reset_opacity(torch.from_numpy(Z["ro_opacity"]).to(dtype)).numpy()
    assert np.array_equal(got, Z[f"ro_{tag}"])
    lg = float(np.log(0.01 / 0.99))
    assert (Z["ro_opacity"] < lg).sum() > 10 and (Z["ro_opacity"] > lg).sum() > 10
    assert np.abs(Z["ro_f64"][Z["ro_opacity"] > lg] - lg).max() < 1e-12          # capped at logit(0.01)
    below = Z["ro_opacity"] < lg
    assert np.abs(Z["ro_f64"][below] - Z["ro_opacity"][below]).max() < 1e-9       # left where they were


def test_update_learning_rate_equals_the_references_schedule():
    from gags_amd import densify
    from gags_amd.scene import GaussianModel
    lr_init, lr_final, mult, max_steps, delay_steps = (float(v) for v in Z["lr_args"])
    m = GaussianModel(0)
    p = torch.nn.Parameter(torch.zeros(2, 3))
    m.optimizer = torch.optim.Adam([{"params": [p], "lr": 0.5, "name": "xyz"}], lr=0.0, eps=1e-15)
    for row, extra in ((0, {}), (1, {"lr_delay_steps": int(delay_steps)})):
        m.xyz_scheduler_args = dict(lr_init=lr_init, lr_final=lr_final, lr_delay_mult=mult, max_steps=int(max_steps), **extra)
        for step, want in zip(Z["lr_steps"], Z["lr_values"][row]):
            assert m.update_learning_rate(int(step)) == want == m.optimizer.param_groups[0]["lr"]
            assert densify.expon_lr(int(step), **m.xyz_scheduler_args) == R.expon_lr(int(step), **m.xyz_scheduler_args)
    assert Z["lr_values"][0][0] == 0.0 and abs(Z["lr_values"][0][1] / lr_init - 1) < 1e-14 and abs(Z["lr_values"][0][-1] / lr_final - 1) < 1e-14
    m.active_sh_degree, m.max_sh_degree = 0, 1
    m.oneupSHdegree()
    m.oneupSHdegree()
    assert m.active_sh_degree == 1


def test_signatures_match_the_header():
    """Argument by argument: the ctypes list of every N8 entry against its prototype in include/gags_next.h."""
    from gags_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(ROOT), "include", "gags_next.h")).read(), flags=re.S)
    to_c = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "double": ctypes.c_double}
    for name in N8:
        ret, args = re.search(r"(\w+)\s+" + name + r"\s*\((.*?)\)\s*;", src, re.S).groups()
        want = []
        for a in args.split(","):
            a = a.strip()
            want.append(ctypes.c_void_p if "*" in a else to_c[a.replace("const ", "").split()[0]])
        assert _lib.SIGNATURES[name] == (to_c[ret], want), name
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(GAGS_(?:KIND|GATHER)_\w+)\s+(\d+)\b", src, flags=re.M)}
    assert len(defs) == 7
    for k, v in defs.items():
        assert getattr(_lib, k) == v, k
    assert ctypes.sizeof(_lib.GatherDesc) == 24 and _lib.GatherDesc.row_floats.offset == 16 and _lib.GatherDesc.mode.offset == 20


def test_argument_validation_returns_codes_without_launching(lib):
    """No GPU here: a call that reached a launch would come back as GAGS_ELAUNCH (-2) or crash, not as -1 / 0."""
    from gags_amd import _lib
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gags_densify_stats(-1, p, p, p, p, 1.0, 1.0, p, p, p, None) == EINVAL
    assert lib.gags_densify_stats(0, None, None, None, None, 1.0, 1.0, None, None, None, None) == 0
    assert lib.gags_densify_stats(4, None, p, None, None, 1.0, 1.0, p, p, None, None) == EINVAL      # nothing to do
    assert lib.gags_densify_stats(4, p, p, None, None, 1.0, 1.0, None, p, p, None) == EINVAL         # accum missing
    assert lib.gags_densify_stats(4, p, None, None, None, 1.0, 1.0, p, p, None, None) == EINVAL      # no filter and no radii
    assert lib.gags_densify_stats(4, None, None, None, p, 1.0, 1.0, None, None, p, None) == EINVAL   # max_radii without radii
    assert lib.gags_densify_decide(-1, p, p, p, p, 1.0, 1.0, 1.0, 1.0, 0.0, 0, p, None) == EINVAL
    assert lib.gags_densify_decide(0, None, None, None, None, 1.0, 1.0, 1.0, 1.0, 0.0, 0, None, None) == 0
    for k in range(5):
        a = [p] * 5
        a[k] = None
        assert lib.gags_densify_decide(4, a[0], a[1], a[2], a[3], 1.0, 1.0, 1.0, 1.0, 0.0, 0, a[4], None) == EINVAL
    assert lib.gags_densify_plan(-1, p, p, p, 4, p, p, p, None) == EINVAL
    assert lib.gags_densify_plan(4, p, p, p, -1, p, p, p, None) == EINVAL
    assert lib.gags_densify_plan(4, p, p, p, 1 << 31, p, p, p, None) == EINVAL
    assert lib.gags_densify_plan(0, None, None, None, 0, None, None, None, None) == 0
    for k in range(6):
        a = [p] * 6
        a[k] = None
        assert lib.gags_densify_plan(4, a[0], a[1], a[2], 4, a[3], a[4], a[5], None) == EINVAL
    ok = _lib.GatherDesc(p.value, p.value, 4, _lib.GAGS_GATHER_COPY)
    table = lambda *d: ctypes.cast((_lib.GatherDesc * len(d))(*d), ctypes.c_void_p)  # noqa: E731
    assert lib.gags_densify_gather(-1, p, p, 1, table(ok), None) == EINVAL
    assert lib.gags_densify_gather(1 << 31, p, p, 1, table(ok), None) == EINVAL
    assert lib.gags_densify_gather(4, p, p, 25, table(*[ok] * 25), None) == EINVAL
    assert lib.gags_densify_gather(4, p, p, -1, table(ok), None) == EINVAL
    assert lib.gags_densify_gather(4, p, p, 1, None, None) == EINVAL
    assert lib.gags_densify_gather(4, None, p, 1, table(ok), None) == EINVAL
    assert lib.gags_densify_gather(4, p, None, 1, table(ok), None) == EINVAL
    assert lib.gags_densify_gather(4, p, p, 1, table(_lib.GatherDesc(p.value, p.value, 0, 0)), None) == EINVAL
    assert lib.gags_densify_gather(4, p, p, 1, table(_lib.GatherDesc(p.value, p.value, -3, 0)), None) == EINVAL
    assert lib.gags_densify_gather(4, p, p, 1, table(_lib.GatherDesc(None, p.value, 4, 0)), None) == EINVAL
    assert lib.gags_densify_gather(4, p, p, 1, table(_lib.GatherDesc(p.value, None, 4, 0)), None) == EINVAL
    assert lib.gags_densify_gather(4, p, p, 1, table(_lib.GatherDesc(p.value, p.value, 4, 2)), None) == EINVAL
    assert lib.gags_densify_gather(0, None, None, 1, table(ok), None) == 0
    assert lib.gags_densify_gather(4, p, p, 0, None, None) == 0
    assert lib.gags_densify_children(-1, 0, 4, p, p, p, p, p, p, 4, p, p, None) == EINVAL
    assert lib.gags_densify_children(4, 5, 4, p, p, p, p, p, p, 4, p, p, None) == EINVAL
    assert lib.gags_densify_children(4, -1, 4, p, p, p, p, p, p, 4, p, p, None) == EINVAL
    assert lib.gags_densify_children(4, 2, -1, p, p, p, p, p, p, 4, p, p, None) == EINVAL
    assert lib.gags_densify_children(4, 2, 4, p, p, p, p, p, p, -1, p, p, None) == EINVAL
    assert lib.gags_densify_children(4, 4, 4, None, None, None, None, None, None, 0, None, None, None) == 0
    assert lib.gags_densify_children(0, 0, 0, None, None, None, None, None, None, 0, None, None, None) == 0
    for k in range(8):
        a = [p] * 8
        a[k] = None
        assert lib.gags_densify_children(4, 2, 4, a[0], a[1], a[2], a[3], a[4], a[5], 4, a[6], a[7], None) == EINVAL
    assert lib.gags_reset_opacity(-1, p, p, p, None) == EINVAL
    assert lib.gags_reset_opacity(4, None, p, p, None) == EINVAL
    assert lib.gags_reset_opacity(0, None, None, None, None) == 0
    assert lib.gags_abi_version() == 2


def test_cpu_tensors_are_rejected_not_rerouted(lib):
    from gags_amd import densify
    from gags_amd.scene import GaussianModel
    n = 8
    m = GaussianModel.from_tensors(torch.zeros(n, 3), torch.zeros(n, 3), torch.ones(n, 4), torch.zeros(n, 1),
                                   semantic_feature=torch.zeros(n, 4), sh_degree=0)
    m.percent_dense = 0.01
    vp = types.SimpleNamespace(grad=torch.zeros(1, n, 2))
    calls = [lambda: m.add_densification_stats(vp, torch.ones(n, dtype=torch.bool), 8, 8),
             lambda: m.update_max_radii(torch.ones(n, dtype=torch.int32), torch.ones(n, dtype=torch.bool)),
             lambda: m.densify_and_prune(0.0002, 0.005, 10.0, None),
             lambda: m.prune_points(torch.zeros(n, dtype=torch.bool)),
             lambda: m.reset_opacity(),
             lambda: m.training_setup_rgb(types.SimpleNamespace(percent_dense=0.01)),
             lambda: densify.accumulate(m, {"viewspace_points": vp, "render": torch.zeros(3, 8, 8),
                                            "radii": torch.ones(n, dtype=torch.int32)})]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    assert m._xyz.shape[0] == n and m.optimizer is None
