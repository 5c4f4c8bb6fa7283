#!/usr/bin/env python
"""Generate tests/golden/tilecut_vectors.npz by running the reference's OWN get_seg_img and pad_img (preprocess.py:356-371) in
this container, on the CPU.  Only data is stored.

    python tests/golden/make_golden_tilecut.py            # tilecut_vectors.npz
    python tests/golden/make_golden_tilecut.py --cv2      # tilecut_cv2_vectors.npz from the former, where cv2 imports

preprocess.py is imported unmodified; segment_anything, open_clip, cv2, torchvision, ... are empty stand-in modules (as in the
other make_golden_* scripts) -- the two functions are pure numpy.

Cases (tests/tilecut_ref.py image_a, image_b): the nine masks of the 37 x 70 image A, each through
pad_img(get_seg_img({"segmentation", "bbox"}, image)), and the one l = 224 box of the 450 x 9 image B.  The squares are mostly
zeros, so the compressed file stays at a few tens of KB; no square of B's longer boxes is stored.  Asserted here: every
square equals tests/tilecut_ref.py square_ref bit for bit.

Arrays.  a_image [37, 70, 3] uint8, a_shape, a_masks (np.packbits of [9, 37, 70]), a_boxes [9, 4] int32 (x, y, w, h),
a_cases [9] str, a_square_k [l_k, l_k, 3] uint8; b_image [224, 9, 3] (the rows of B under its l = 224 box), b_shape, b_mask
(packbits of [224, 9]), b_box [4], b_square [224, 224, 3].

--cv2 (cv2.resize is the one part of N14 that no file of the reference states; the restatement of tests/tilecut_ref.py
resize_ref is pinned to it only by this file): tilecut_cv2_vectors.npz holds sides [n], square_l [l, l, 3] uint8 random
squares and tile_l = cv2.resize(square_l, (224, 224)) for every side tests/test_tilecut_cpu.py lists (SIDES), plus the tiles
of the fixture's own squares (a_tile_k, b_tile).  tests/test_tilecut_cpu.py compares resize_ref with them where the file
exists and is skipped where it does not."""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "tilecut_vectors.npz")
OUT_CV2 = os.path.join(HERE, "tilecut_cv2_vectors.npz")
STUB_ROOTS = {"plyfile", "open3d", "cv2", "matplotlib", "open_clip", "segment_anything", "simple_knn", "gsplat",
              "torchvision", "mediapy", "jaxtyping", "tqdm", "sklearn", "PIL", "lpipsPyTorch", "scipy"}
SIDES = (1, 2, 3, 7, 37, 100, 223, 224, 225, 300, 447, 448, 449, 640, 1080)


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


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), what


def write_cv2(squares):
    import cv2
    g = np.random.default_rng(224)
    out = {"sides": np.array(SIDES, np.int64), "cv2_version": np.array(cv2.__version__)}
    for l in SIDES:
        sq = g.integers(0, 256, (l, l, 3), dtype=np.uint8)
        out[f"square_{l}"], out[f"tile_{l}"] = sq, cv2.resize(sq, (224, 224))
    for key, sq in squares.items():
        out[key.replace("square", "tile")] = cv2.resize(sq, (224, 224))
    np.savez_compressed(OUT_CV2, **out)
    print("wrote", OUT_CV2, os.path.getsize(OUT_CV2), "bytes, cv2", cv2.__version__)


def main():
    sys.path.insert(0, os.path.dirname(HERE))
    import tilecut_ref as R
    if "--cv2" in sys.argv[1:]:   # the real cv2 and the stand-in cannot share a process: this run only resizes stored squares
        try:
            import cv2  # noqa: F401
        except ImportError:
            sys.exit("--cv2: cv2 does not import here; tilecut_cv2_vectors.npz is not written")
        z = np.load(OUT)
        write_cv2({k: z[k] for k in z.files if "square" in k})
        return
    sys.meta_path.insert(0, _Stubs())
    sys.path.insert(0, REF)
    import preprocess as P

    def reference_square(image, mask, box):
        before = image.copy()
        sq = P.pad_img(P.get_seg_img({"segmentation": mask, "bbox": [int(v) for v in box]}, image))
        same(image, before, "get_seg_img works on a copy")
        return sq

    out = {}
    image, masks, boxes = R.image_a()
    H, W = masks.shape[1:]
    out.update(a_image=image, a_shape=np.array([H, W], np.int64), a_masks=np.packbits(masks), a_boxes=boxes,
               a_cases=np.array(R.A_CASES))
    for k, name in enumerate(R.A_CASES):
        sq = reference_square(image, masks[k], boxes[k])
        same(sq, R.square_ref(image, masks[k], boxes[k]), name)
        assert sq.shape[0] == sq.shape[1] == max(R.clip_box(boxes[k], H, W)[2:])
        out[f"a_square_{k}"] = sq
        print(name, tuple(int(v) for v in boxes[k]), "l", sq.shape[0], "set", int(sq.any(axis=2).sum()))
    # the case list promises these properties
    l_of = {name: out[f"a_square_{k}"].shape[0] for k, name in enumerate(R.A_CASES)}
    assert l_of == {"tall": 9, "wide": 9, "one": 1, "last": 12, "overhang": 12, "whole": 70, "holes": 42, "outside": 17, "roomy": 21}
    assert not out["a_square_0"][:, :2].any() and out["a_square_0"][:, 2:6].all() and not out["a_square_0"][:, 6:].any()
    assert not out["a_square_1"][:2].any() and out["a_square_1"][2:6].all() and not out["a_square_1"][6:].any()
    assert masks[7].sum() > masks[7, 10:23, 20:37].sum() > 0 and masks[4, 36, 69] and masks[3, 36, 69]

    image, mask, boxes = R.image_b()
    x, y, w, h = (int(v) for v in boxes[R.B_SIDES.index(224)])
    image, mask, box = np.ascontiguousarray(image[y:y + h]), np.ascontiguousarray(mask[0, y:y + h]), np.array([x, 0, w, h], np.int32)
    sq = reference_square(image, mask, box)   # (only the 224 rows of B that the box covers are stored)
    same(sq, R.square_ref(image, mask, box), "b224")
    assert sq.shape == (224, 224, 3) and y > 0
    out.update(b_image=image, b_shape=np.array(mask.shape, np.int64), b_mask=np.packbits(mask), b_box=box, b_square=sq)

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
