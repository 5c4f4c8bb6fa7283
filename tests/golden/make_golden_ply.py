#!/usr/bin/env python
"""Generate tests/golden/ply_attribute_names.json by calling the reference's OWN `GaussianModel.construct_list_of_attributes`
(scene/gaussian_model.py:222-238) on a model of this repository's shapes: features_dc [N,1,3], features_rest [N,15,3],
scaling [N,3], rotation [N,4], semantic_feature [N,16].  Only the returned list of column names is stored.

    python tests/golden/make_golden_ply.py PATH_TO_THE_REFERENCE_TREE
"""
import json
import os
import sys
import types

import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ply_attribute_names.json")


def main(ref):
    for name in ("plyfile", "simple_knn", "simple_knn._C"):  # imported by the module, not used by the function
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = object
    sys.modules["simple_knn._C"].distCUDA2 = None
    sys.path.insert(0, ref)
    from scene.gaussian_model import GaussianModel as RefModel
    n = 7
    m = RefModel.__new__(RefModel)
    m._features_dc, m._features_rest = torch.zeros(n, 1, 3), torch.zeros(n, 15, 3)
    m._scaling, m._rotation, m._semantic_feature = torch.zeros(n, 3), torch.zeros(n, 4), torch.zeros(n, 16)
    names = RefModel.construct_list_of_attributes(m)
    with open(OUT, "w") as f:
        json.dump(names, f)
        f.write("\n")
    print(f"{OUT}: {len(names)} names")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
