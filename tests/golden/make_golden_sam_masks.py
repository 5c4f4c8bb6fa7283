#!/usr/bin/env python
"""Generate tests/golden/sam_masks_vectors.npz by running the reference's OWN `mask_nms` and `masks_update`
(preprocess.py:380-462) in this container.  Only data is stored.

    python tests/golden/make_golden_sam_masks.py

preprocess.py is imported unmodified; segment_anything, open_clip, cv2, torchvision, ... are empty stand-in modules (as in
the other make_golden_* scripts) -- the two functions use none of them.  The reference returns only the selected indices;
its internal vectors (iou_max, inner_iou_max_u, inner_iou_max_l, keep_conf, keep_inner_u, keep_inner_l) are read from the
function's own frame when it returns (sys.settrace), so the fixture holds the reference's numbers and not a recomputation.

Scenes: three images (37 x 70, 64 x 64, 37 x 70), each with the four SAM levels default / s / m / l as lists of dicts with
seeded random-rectangle masks that lose 10 % of their pixels (tests/sam_masks_ref.py rect_masks: free, nested and
near-copy rectangles), M from 1 to 40 over the twelve levels, distinct float64 scores = stability_score * predicted_iou.
Every level runs under both threshold sets: "def" = the function's defaults (0.7, 0.1, 0.2) and "call" = sam_encoder's
iou_thr=0.8, score_thr=0.7, inner_thr=0.5.  A seed whose level would enter one of the reference's top-3 fallbacks (which
raise IndexError) is skipped: the fallbacks are a documented deviation and are tested by hand.

Asserted here: the reference's outputs equal tests/sam_masks_ref.py bit for bit; for each of the four keep conditions at
least one case loses a mask to that condition alone, and in at least one case the tril(diagonal=1) quirk decides the
"lower" keep vector (recorded as decided_by_*).  The quirk: the first superdiagonal of the inner matrix enters the lower
maximum too, which flips entries of keep_inner_l.  Such an entry also enters the upper maximum and meets the same threshold
there, so outside the fallbacks the final selection cannot differ -- asserted as well; what the quirk decides is the
fourth keep vector (and with it whether the lower fallback is entered).

Arrays.  cases [12] str "<scene>_<level>"; per case c: c_shape (M, H, W), c_masks = np.packbits of the bool masks [M, H, W]
(big bit order, numpy's default), c_iou / c_stab [M] float64; per case and threshold set t in (def, call): c_t_selected
(the reference's return value), c_t_colmax [3, M] fp32, c_t_keeps [4, M] bool (IoU, score, inner upper, inner lower),
c_t_kept (ascending indices masks_update keeps).  thresholds_def / thresholds_call [3]; decided_by_iou / _score /
_inner_u / _inner_l / _quirk: lists of "<case>_<t>"."""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "sam_masks_vectors.npz")
STUB_ROOTS = {"plyfile", "open3d", "cv2", "matplotlib", "open_clip", "segment_anything", "simple_knn", "gsplat",
              "torchvision", "mediapy", "jaxtyping", "tqdm", "sklearn", "PIL", "lpipsPyTorch", "scipy"}
THRESHOLDS = {"def": {}, "call": {"iou_thr": 0.8, "score_thr": 0.7, "inner_thr": 0.5}}
SCENES = (("a", 37, 70, (1, 5, 17, 40)), ("b", 64, 64, (2, 8, 24, 33)), ("c", 37, 70, (3, 12, 6, 29)))
LEVELS = ("default", "s", "m", "l")


class _AnyModule(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        v = type(name, (), {"__init__": lambda self, *a, **k: None, "__class_getitem__": classmethod(lambda c, i: c)})
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


def traced(fn, *args, **kwargs):
    """fn(*args, **kwargs) and the locals of fn's own frame at its return."""
    seen = {}

    def local(frame, event, arg):
        if event == "return":
            seen.update(frame.f_locals)
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code is fn.__code__ else None

    sys.settrace(tracer)
    try:
        out = fn(*args, **kwargs)
    finally:
        sys.settrace(None)
    return out, seen


def main():
    sys.meta_path.insert(0, _Stubs())
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.dirname(HERE))
    import sam_masks_ref as R
    import preprocess as P
    P.print = lambda *a, **k: None

    out = {"cases": [], "thresholds_def": np.array([0.7, 0.1, 0.2]), "thresholds_call": np.array([0.8, 0.7, 0.5])}
    decided = {k: [] for k in ("iou", "score", "inner_u", "inner_l", "quirk")}
    seed = 100
    for sname, H, W, counts in SCENES:
        levels = []
        for lname, M in zip(LEVELS, counts):
            case = f"{sname}_{lname}"
            while True:  # the next seed whose level stays out of the reference's (raising) fallbacks under both sets
                seed += 1
                rng = np.random.default_rng(seed)
                masks = R.rect_masks(rng, M, H, W, holes=0.1)
                iou_pred = rng.uniform(0.75, 1.0, M)
                stab = rng.uniform(0.85, 1.0, M)
                scores = torch.from_numpy(stab * iou_pred)
                assert len(set(scores.tolist())) == M
                runs = {}
                try:
                    for t, kw in THRESHOLDS.items():
                        runs[t] = traced(P.mask_nms, torch.from_numpy(masks), scores.clone(), **kw)
                except IndexError:
                    continue
                break
            out["cases"].append(case)
            out[f"{case}_shape"] = np.array([M, H, W])
            out[f"{case}_masks"] = np.packbits(masks)
            out[f"{case}_iou"], out[f"{case}_stab"] = iou_pred, stab
            for t, kw in THRESHOLDS.items():
                selected, loc = runs[t]
                thr = {"iou_thr": 0.7, "score_thr": 0.1, "inner_thr": 0.2, **kw}
                colmax = torch.stack([loc["iou_max"], loc["inner_iou_max_u"], loc["inner_iou_max_l"]])
                keeps = torch.stack([loc["iou_max"] <= thr["iou_thr"], loc["keep_conf"], loc["keep_inner_u"], loc["keep_inner_l"]])
                assert colmax.dtype == torch.float32 and selected.dtype == torch.int64
                assert torch.equal(loc["idx"][keeps.all(dim=0)], selected)
                mine = R.nms(masks, scores, **kw)
                assert torch.equal(mine["idx"], loc["idx"]), case
                assert torch.equal(mine["colmax"], colmax), (case, t)
                assert torch.equal(mine["keeps"], keeps), (case, t)
                assert torch.equal(mine["selected"], selected), (case, t)
                out[f"{case}_{t}_selected"] = selected.numpy()
                out[f"{case}_{t}_colmax"] = colmax.numpy()
                out[f"{case}_{t}_keeps"] = keeps.numpy()
                for k, name in enumerate(("iou", "score", "inner_u", "inner_l")):
                    others = torch.cat([keeps[:k], keeps[k + 1:]]).all(dim=0)
                    if bool((~keeps[k] & others).any()):
                        decided[name].append(f"{case}_{t}")
                plain = R.nms(masks, scores, quirk=False, **kw)
                if not torch.equal(plain["keeps"][3], keeps[3]):
                    decided["quirk"].append(f"{case}_{t}")
                assert torch.equal(plain["selected"], selected)  # (see the note on the quirk above)
            levels.append([{"segmentation": masks[k], "predicted_iou": iou_pred[k], "stability_score": stab[k], "id": k}
                           for k in range(M)])
        for t, kw in THRESHOLDS.items():
            kept = P.masks_update(*levels, **kw)
            mine = R.masks_update(*levels, **kw)
            assert isinstance(kept, tuple) and len(kept) == 4
            for lname, lvl, mlvl in zip(LEVELS, kept, mine):
                ids = [m["id"] for m in lvl]
                assert ids == [m["id"] for m in mlvl] and ids == sorted(ids)
                assert ids == sorted(out[f"{sname}_{lname}_{t}_selected"].tolist())
                out[f"{sname}_{lname}_{t}_kept"] = np.array(ids, np.int64)
    for name, cases in decided.items():
        assert cases, f"no case is decided by {name}: {decided}"
        out[f"decided_by_{name}"] = np.array(cases)
    out["cases"] = np.array(out["cases"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; decided", {k: len(v) for k, v in decided.items()})


if __name__ == "__main__":
    main()
