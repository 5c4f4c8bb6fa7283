#!/usr/bin/env python
"""Generate tests/golden/densify_vectors.npz by running the reference's OWN `GaussianModel` methods (densify_and_prune,
add_densification_stats, reset_opacity; utils.general_utils.get_expon_lr_func) on the CPU.  Only data is stored.

    python tests/golden/make_golden_densify.py

The methods run unmodified; what is replaced is what this container lacks:
  * plyfile, simple_knn, ... are empty stand-in modules (as in make_golden_depthsample.py).
  * inside scene.gaussian_model and utils.general_utils, `torch` is a proxy whose zeros(..., device="cuda") stays on the CPU
    and whose normal(mean, std) is mean + std * Z for a RECORDED standard-normal Z (asserted below to be what the real
    torch.normal computes from the same draws); torch.cuda.empty_cache is a no-op.
Every case runs twice, in float32 and in float64 (torch's default dtype switched, the same float32-representable inputs), on a
seven-group torch.optim.Adam that has taken three steps with lr = 0 on random gradients: the parameters stay what they
were, the moments are non-zero and `step` is set.

The inputs and the margin check come from tests/densify_cases.py (shared with the GPU tests; it never touches the
reference).  Asserted here: tests/densify_ref.py equals both runs exactly (tensors, moments, order, statistics); every decision quantity
that is not a built tie lies at least 1e-3 (relative, float64) from its threshold; the built ties are exact.

Arrays: `cases` (names); per case c: c_<name> inputs (float32; moments c_m1_<name>, c_m2_<name> of the float32 run), c_accum,
c_denom, c_max_radii, c_Z, c_par = (percent_dense, max_grad, min_opacity, extent, max_screen_size or 0, sh_degree, adam step);
outputs c_f32_<name>, c_f64_<name>, c_f32_m1_<name>, ..., c_src, c_kind (the restatement's plan, equal for both runs).
Statistics: st_grad [3,N,2], st_radii [3,N], st_update [3,N], st_visible [3,N], st_wh [3,2], st_f32_accum, ... st_f64_max_radii.
Reset: ro_opacity, ro_m1, ro_m2, ro_f32, ro_f64.  Schedule: lr_steps, lr_values, lr_args.
"""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "densify_vectors.npz")
STUB_ROOTS = {"plyfile", "open3d", "cv2", "matplotlib", "simple_knn", "gsplat", "torchvision", "tqdm", "sklearn", "PIL"}
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "semantic_feature")
ATTRS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation", "_semantic_feature")


class _AnyModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        v = type(name, (), {"__init__": lambda self, *a, **k: None})
        setattr(self, name, v)
        return v


class _Stubs(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in STUB_ROOTS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        m = _AnyModule(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, m):
        pass


class TorchProxy:
    """`torch` as the reference's two modules see it: "cuda" stays on the CPU, normal() uses the recorded draws."""

    def __init__(self):
        self.Z = None
        self.cuda = types.SimpleNamespace(empty_cache=lambda: None)

    def __getattr__(self, name):
        return getattr(torch, name)

    def zeros(self, *a, **k):
        if str(k.get("device", "")).startswith("cuda"):
            k.pop("device")
        return torch.zeros(*a, **k)

    def normal(self, mean, std):
        assert self.Z is not None and tuple(self.Z.shape) == tuple(std.shape), (self.Z.shape, std.shape)
        return mean + std * self.Z.to(std.dtype)


def run_reference(GM, proxy, t, accum, denom, max_radii, par, Z, dtype, m_in=None):
    """The reference's densify_and_prune on one case; returns (outputs, moments_in, moments_out, steps)."""
    torch.set_default_dtype(dtype)
    try:
        gm = GM.GaussianModel(par["sh_degree"])
        groups = []
        for name, attr in zip(NAMES, ATTRS):
            p = torch.nn.Parameter(torch.tensor(t[name]).to(dtype).requires_grad_(True))
            setattr(gm, attr, p)
            groups.append({"params": [p], "lr": 0.0, "name": name})
        gm.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        g_rng = torch.Generator().manual_seed(11)
        for _ in range(3):
            for grp in groups:
                p = grp["params"][0]
                p.grad = torch.randn(p.shape, generator=g_rng, dtype=torch.float32).to(dtype)
            gm.optimizer.step()
        m_before = {grp["name"]: (gm.optimizer.state[grp["params"][0]]["exp_avg"].clone(),
                                  gm.optimizer.state[grp["params"][0]]["exp_avg_sq"].clone()) for grp in groups}
        for name, attr in zip(NAMES, ATTRS):
            assert torch.equal(getattr(gm, attr).detach(), torch.tensor(t[name]).to(dtype)), name  # lr = 0: untouched
        gm.percent_dense = par["percent_dense"]
        gm.xyz_gradient_accum = torch.tensor(accum).to(dtype)
        gm.denom = torch.tensor(denom).to(dtype)
        gm.max_radii2D = torch.tensor(max_radii).to(dtype)
        proxy.Z = Z
        gm.densify_and_prune(par["max_grad"], par["min_opacity"], par["extent"], par["mss"])
        proxy.Z = None
        out = {name: getattr(gm, attr).detach().clone() for name, attr in zip(NAMES, ATTRS)}
        m_after, steps = {}, {}
        for grp in gm.optimizer.param_groups:
            st = gm.optimizer.state[grp["params"][0]]
            assert grp["params"][0] is getattr(gm, ATTRS[NAMES.index(grp["name"])])
            m_after[grp["name"]] = (st["exp_avg"].clone(), st["exp_avg_sq"].clone())
            steps[grp["name"]] = float(st["step"])
        out["accum"], out["denom"], out["max_radii"] = gm.xyz_gradient_accum, gm.denom, gm.max_radii2D
        return out, m_before, m_after, steps
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    sys.meta_path.insert(0, _Stubs())
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.dirname(HERE))
    import densify_ref as R
    from densify_cases import MARGIN, build_case, check_margin, logit
    import scene.gaussian_model as GM
    import utils.general_utils as GU
    torch.set_num_threads(1)
    proxy = TorchProxy()
    GM.torch = proxy
    GU.torch = proxy

    # torch.normal(mean, std) is mean + std * randn of the same draws
    std = torch.rand(34, 3) + 0.1
    torch.manual_seed(3)
    a = torch.normal(mean=torch.zeros(34, 3), std=std)
    torch.manual_seed(3)
    assert torch.equal(a, torch.zeros(34, 3) + std * torch.randn(34, 3)), "torch.normal is not mean + std * randn"

    rng = np.random.default_rng(2024)
    out = {}
    specs = [  # name, n, sh_degree, D, extent, max_grad, max_screen_size, kind
        ("mixed", 80, 3, 16, 10.0, 0.0002, 20, "mixed"),
        ("mixed_nomss", 100, 1, 7, 10.0, 0.0002, None, "mixed"),
        ("sh0", 100, 0, 3, 10.0, 0.0002, 20, "mixed"),
        ("none", 64, 1, 7, 10.0, 0.0002, None, "none"),
        ("allpruned", 50, 1, 7, 10.0, 0.0002, 20, "allpruned"),
        ("allsplit", 40, 1, 7, 10.0, 0.0002, 20, "allsplit"),
        ("tie_dense", 60, 1, 7, 100.0, 0.25, None, "tie_dense"),
        ("tie_world", 60, 1, 7, 10.0, 0.0002, 20, "tie_world"),
    ]
    seen = {"clone": 0, "child": 0, "pruned_parent_kept_children": 0, "ties": 0}
    for name, n, shd, d, extent, max_grad, mss, kind in specs:
        t, accum, denom, max_radii, par = build_case(rng, n, shd, d, extent, max_grad, mss, kind)
        seen["ties"] += check_margin(t, accum, denom, par, kind.startswith("tie"))
        tt = {k: torch.tensor(v) for k, v in t.items()}
        keep, clone_ok, split, child_ok = R.decide(torch.tensor(accum), torch.tensor(denom), tt["scaling"], tt["opacity"],
                                                   par["percent_dense"], max_grad, par["min_opacity"], extent, mss)
        n_split = int(split.sum())
        Z = torch.tensor(rng.standard_normal((2 * n_split, 3)).astype(np.float32))
        res = {}
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            o, m_in, m_out, steps = run_reference(GM, proxy, t, accum, denom, max_radii, par, Z, dtype)
            mine = R.densify_and_prune({k: v.to(dtype) for k, v in tt.items()}, torch.tensor(accum).to(dtype),
                                       torch.tensor(denom).to(dtype), par["percent_dense"], max_grad, par["min_opacity"],
                                       extent, mss, Z.to(dtype), moments=m_in)
            for k in NAMES:
                assert o[k].shape == mine[k].shape, (name, tag, k, o[k].shape, mine[k].shape)
                assert torch.equal(o[k], mine[k]), (name, tag, k, (o[k] - mine[k]).abs().max())
                assert torch.equal(m_out[k][0], mine["moments"][k][0]) and torch.equal(m_out[k][1], mine["moments"][k][1])
                assert steps[k] == 3.0
                out[f"{name}_{tag}_{k}"] = o[k].numpy()
                out[f"{name}_{tag}_m1_{k}"], out[f"{name}_{tag}_m2_{k}"] = m_out[k][0].numpy(), m_out[k][1].numpy()
            n_out = o["xyz"].shape[0]
            assert tuple(o["accum"].shape) == (n_out, 1) and tuple(o["denom"].shape) == (n_out, 1)
            assert tuple(o["max_radii"].shape) == (n_out,)
            assert not o["accum"].any() and not o["denom"].any() and not o["max_radii"].any()
            res[tag] = (mine, m_in)
        assert torch.equal(res["f32"][0]["src"], res["f64"][0]["src"]) and torch.equal(res["f32"][0]["kind"], res["f64"][0]["kind"])
        mine, m_in = res["f32"]
        for k in NAMES:
            out[f"{name}_{k}"] = t[k]
            out[f"{name}_m1_{k}"], out[f"{name}_m2_{k}"] = m_in[k][0].numpy(), m_in[k][1].numpy()
        out[f"{name}_accum"], out[f"{name}_denom"], out[f"{name}_max_radii"], out[f"{name}_Z"] = accum, denom, max_radii, Z.numpy()
        out[f"{name}_par"] = np.array([par["percent_dense"], max_grad, par["min_opacity"], extent, mss or 0, shd, 3.0])
        out[f"{name}_src"], out[f"{name}_kind"] = mine["src"].numpy().astype(np.int32), mine["kind"].numpy().astype(np.uint8)
        kd = mine["kind"].numpy()
        seen["clone"] += int((kd == 1).sum())
        seen["child"] += int((kd >= 2).sum())
        world = np.exp(t["scaling"].astype(np.float64)).max(1)
        if mss:
            seen["pruned_parent_kept_children"] += int((child_ok.numpy() & (world > 0.1 * extent)).sum())
        n_o = len(kd)
        print(f"{name}: N={n} -> {n_o} (keep {(kd == 0).sum()}, clone {(kd == 1).sum()}, children {(kd >= 2).sum()}, split-selected {n_split})")
        if kind == "none":
            assert n_o == n and (kd == 0).all()
        if kind == "allpruned":
            assert n_o == 0
        if kind == "allsplit":
            assert n_split == n and (kd >= 2).all()
    assert seen["clone"] > 20 and seen["child"] > 40 and seen["pruned_parent_kept_children"] > 5 and seen["ties"] >= 20, seen
    out["cases"] = np.array([s[0] for s in specs])

    # statistics over three views, different filters, W != H
    n = 200
    grad = (rng.standard_normal((3, n, 2)) * 1e-3).astype(np.float32)
    radii = rng.integers(0, 60, (3, n)).astype(np.int32)
    visible = radii > 0
    update = visible & (rng.random((3, n)) < 0.8)
    update[2] = rng.random(n) < 0.5  # a filter that is not a subset of `visible`
    wh = np.array([[64, 48], [80, 33], [17, 96]])
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        torch.set_default_dtype(dtype)
        gm = GM.GaussianModel(0)
        gm.xyz_gradient_accum, gm.denom, gm.max_radii2D = torch.zeros(n, 1), torch.zeros(n, 1), torch.zeros(n)
        acc, den, mr = torch.zeros(n, 1), torch.zeros(n, 1), torch.zeros(n)
        for v in range(3):
            vp = types.SimpleNamespace(grad=torch.tensor(grad[v:v + 1]).to(dtype))
            u, vis, r = torch.tensor(update[v]), torch.tensor(visible[v]), torch.tensor(radii[v]).to(dtype)
            gm.max_radii2D[vis] = torch.maximum(gm.max_radii2D[vis], r[vis])  # train.py:209
            gm.add_densification_stats(vp, u, int(wh[v, 0]), int(wh[v, 1]))
            acc, den, mr = R.add_stats(acc, den, mr, torch.tensor(grad[v]).to(dtype), torch.tensor(radii[v]), u, vis,
                                       int(wh[v, 0]), int(wh[v, 1]))
        torch.set_default_dtype(torch.float32)
        assert torch.equal(acc, gm.xyz_gradient_accum) and torch.equal(den, gm.denom) and torch.equal(mr, gm.max_radii2D), tag
        out[f"st_{tag}_accum"], out[f"st_{tag}_denom"], out[f"st_{tag}_max_radii"] = acc.numpy(), den.numpy(), mr.numpy()
    out.update(st_grad=grad, st_radii=radii, st_update=update, st_visible=visible, st_wh=wh)

    # reset_opacity on logits either side of logit(0.01)
    n = 100
    p = np.where(rng.random(n) < 0.5, rng.uniform(0.0005, 0.0099, n), rng.uniform(0.0101, 0.99, n))
    assert np.all(np.abs(p - 0.01) / 0.01 >= MARGIN) and np.all(np.abs(p - float(np.float32(0.01))) / 0.01 >= MARGIN)
    op = logit(p).astype(np.float32)[:, None]
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        torch.set_default_dtype(dtype)
        gm = GM.GaussianModel(0)
        gm._opacity = torch.nn.Parameter(torch.tensor(op).to(dtype))
        gm.optimizer = torch.optim.Adam([{"params": [gm._opacity], "lr": 0.0, "name": "opacity"}], lr=0.0, eps=1e-15)
        gm._opacity.grad = torch.tensor(rng.standard_normal((n, 1)).astype(np.float32)).to(dtype)
        gm.optimizer.step()
        st = gm.optimizer.state[gm._opacity]
        if tag == "f32":
            out["ro_m1"], out["ro_m2"] = st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
        gm.reset_opacity()
        st = gm.optimizer.state[gm._opacity]
        assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and float(st["step"]) == 1.0
        assert torch.equal(gm._opacity.detach(), R.reset_opacity(torch.tensor(op).to(dtype))), tag
        out[f"ro_{tag}"] = gm._opacity.detach().numpy().copy()
        torch.set_default_dtype(torch.float32)
    out["ro_opacity"] = op

    # the position schedule
    args = dict(lr_init=0.00016 * 3.7, lr_final=0.0000016 * 3.7, lr_delay_mult=0.01, max_steps=30000)
    steps = np.array([-1, 0, 1, 7, 100, 2999, 15000, 29999, 30000, 40000])
    f = GU.get_expon_lr_func(**args)
    f2 = GU.get_expon_lr_func(lr_delay_steps=500, **args)
    vals = np.array([[f(int(s)) for s in steps], [f2(int(s)) for s in steps]], np.float64)
    for j, s in enumerate(steps):
        assert R.expon_lr(int(s), **args) == vals[0, j] and R.expon_lr(int(s), lr_delay_steps=500, **args) == vals[1, j], s
    out.update(lr_steps=steps, lr_values=vals, lr_args=np.array([args["lr_init"], args["lr_final"], args["lr_delay_mult"],
                                                                args["max_steps"], 500]))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", seen)


if __name__ == "__main__":
    main()
