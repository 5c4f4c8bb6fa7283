#!/usr/bin/env python3
"""Record what every size-reporting export of libgags_hip.so returns over a fixed table of arguments.

    python tools/record_scratch_bytes.py tests/golden/scratch_bytes.json

The functions are every `*_scratch_bytes` of _lib.SIGNATURES plus the three other exports a caller sizes a buffer with
(gags_bwd_rowmap_elems, gags_photometric_partials, gags_segment_stats_runs_copies).  They are pure host arithmetic: no GPU is
needed.  tests/test_scratch_layout_cpu.py compares the library under test with the recorded file, so the file is recorded
from the commit BEFORE a change to a scratch layout, never from the change itself.  Per function the table holds a tiny
shape, shapes that are no multiple of 64, a workload-sized shape (1.5 M Gaussians, 1920 x 1080, D = 512, ~30 M
intersections) and every rejected case the CPU tests name.

A size function that is added later (LATER) has no earlier commit to be recorded from, and the first file stays as it was
recorded: such a function gets a fixture of its own next to it, written once by

    python tools/record_scratch_bytes.py --later tests/golden

and checked by the tests of the change that adds it, together with the arithmetic that ties it to an existing layout.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gags_amd import _lib  # noqa: E402

EXTRA = ("gags_bwd_rowmap_elems", "gags_photometric_partials", "gags_segment_stats_runs_copies")
N, W, H, D, ISECTS, ROWS = 1_500_000, 1920, 1080, 512, 30_000_000, 9_000_000  # the workload
HW = W * H
I31 = (1 << 31) - 1


DEPTH = [(1, 1, 1, 1), (1000, 2, 32, 40), (1000, 3, 32, 40), (1000, 2, 32, 32), (999, 17, 33, 41),
         (1000, 300, H, W), (N, 300, H, W), (N, 16, H, W), (0, 2, 32, 32), (-1, 2, 32, 32),
         (10, 0, 32, 32), (10, 2, 0, 32), (10, 2, 32, -1), (10, 2, 1 << 16, 1 << 15),
         (I31, 2, 8, 8)]
# added after the first file was recorded: function -> (its own fixture under tests/golden, its table)
# (N22: gags_depthsample_scratch_bytes with a 96-byte camera block where that one has 64 bytes)
# (N24: the slabs of the bilateral grid's v_grid; arguments (L, gh, gw))
BILAGRID = [(2, 2, 2), (4, 3, 5), (8, 16, 16), (16, 64, 64), (8, 32, 32), (3, 7, 9), (16, 2, 2), (8, 45, 46), (1, 16, 16),
            (17, 16, 16), (8, 1, 16), (8, 16, 1), (8, 16, 65), (8, 65, 16), (8, 0, 16), (-8, 16, 16)]
LATER = {"gags_rig_depth_scratch_bytes": ("scratch_bytes_rig_depth.json", DEPTH),
         "gags_bilagrid_scratch_bytes": ("scratch_bytes_bilagrid.json", BILAGRID)}


def table(lib):
    cap = lib.gags_masks_max_count()
    counts32 = [(-1,), (0,), (1,), (3,), (63,), (65,), (1000,), (100000,), (N,), (I31,)]
    counts64 = counts32 + [(ISECTS,), (1 << 31,), (1 << 40,)]
    wgrad = [(1, 8, 8), (77, 16, 16), (1000, 48, 19), (HW, 128, 64), (HW, 256, 128), (HW, 512, 256), (HW, 16, 512), (2 * HW + 7, 24, 40),
             (0, 16, 16), (-1, 16, 16), (100, 0, 16), (100, 16, 0), (100, -8, 16), (100, 16, -8), (100, 1024, 16), (100, 16, 1024)]
    khw = [(1, 1, 1), (2, 9, 11), (3, 8, 9), (6, 8, 8), (7, 131, 197), (40, H, W), (300, H, W),
           (0, 8, 8), (-1, 8, 8), (2, 0, 8), (2, 8, 0), (2, -3, 8), (2, 8, -2), (1 << 16, 8, 8), (2, 1 << 15, 1 << 16)]
    kn = [(1, 1), (2, 500), (3, 1000), (7, 1001), (5, N), (40, N), (0, 1000), (3, 0), (0, 10), (2, 0), (-1, 10), (2, -1),
          (2, 1 << 30), (3, (1 << 31) // 3 + 1), (1, I31), (1, 1 << 31)]
    return {
        "gags_scan_scratch_bytes": counts32,
        "gags_compact_mask_scratch_bytes": counts32,
        "gags_depth_order_scratch_bytes": counts32,
        "gags_sort_scratch_bytes": counts64,
        "gags_bwd_rowmap_scratch_bytes": counts64,
        "gags_knn3_dist2_scratch_bytes": counts64 + [(4,), (300,), (1 << 19,), (1 << 20,)],
        "gags_dot_scratch_bytes": [()],
        "gags_raster_fwd_scratch_bytes": [(1, 16, 16), (1000, 64, 48), (12345, 161, 113), (ISECTS, W, H), ((1 << 28) - 64, W, H),
                                          (0, 64, 48), (-1, 64, 48), (1000, 0, 48), (1000, 64, 0), (1000, -16, 48), (1 << 28, W, H),
                                          (1 << 31, W, H)],
        "gags_bwd_rowmap_elems": [(1, 16, 16), (1000, 64, 48), (12345, 161, 113), (ISECTS, W, H), ((1 << 28) - 64, W, H),
                                  (0, 64, 48), (-1, 64, 48), (1000, 0, 48), (1000, 64, 0), (1000, -16, 48), (1 << 28, W, H)],
        "gags_bwd_staged_scratch_bytes": [(1, 1, 16), (1000, 300, 16), (12345, 3001, 24), (777, 100, 3), (ROWS, N, D), (ROWS, N, 32),
                                          (ROWS, N, 128), (ISECTS, N, 16), (0, 300, 16), (-1, 300, 16), (1000, 0, 16), (1000, -1, 16),
                                          (1000, 300, 0), (1000, 300, -16), (1 << 31, N, 16), (1 << 40, N, D)],
        "gags_raster_bwd_geom_scratch_bytes": [(1, 16, 16, 1, 16, 0), (1000, 64, 48, 300, 16, 0), (1000, 64, 48, 300, 16, 700),
                                               (12345, 161, 113, 3001, 24, 5001), (12345, 161, 113, 3001, 136, 0),
                                               (ISECTS, W, H, N, D, ROWS), (ISECTS, W, H, N, D, 0), (ISECTS, W, H, N, 128, ROWS),
                                               (ISECTS, W, H, N, 16, ROWS), (1000, 64, 48, 300, 16, -1),
                                               (0, 64, 48, 300, 16, 0), (-1, 64, 48, 300, 16, 0), (1000, 0, 48, 300, 16, 0),
                                               (1000, 64, 0, 300, 16, 0), (1000, 64, 48, 0, 16, 0), (1000, 64, 48, -1, 16, 0),
                                               (1000, 64, 48, 300, 0, 0), (1000, 64, 48, 300, 12, 0), (1000, 64, 48, 300, 8, 0),
                                               (1 << 28, W, H, N, D, 0), (1 << 31, W, H, N, D, ROWS)],
        "gags_decoder_wgrad_scratch_bytes": wgrad,
        "gags_decoder_wgrad_scratch_bytes_h16": wgrad,
        "gags_decoder_wgrad_exact_scratch_bytes": wgrad,
        "gags_relevancy_activate_scratch_bytes": khw,
        "gags_query_images_scratch_bytes": khw,
        "gags_photometric_partials": khw + [(1, 16, 32), (1, 16, 33), (1, 17, 32), (1, 17, 33), (3, 5, 7), (3, H, W), (6, 131, 197),
                                            (3, 8, -2), (3, 0, 8)],
        "gags_point_relevancy_mask_scratch_bytes": kn,
        "gags_point_mask_smooth_scratch_bytes": kn,
        "gags_depthsample_scratch_bytes": DEPTH,
        "gags_masks_nms_scratch_bytes": [(1, 1), (5, 17 * 19), (40, 37 * 70), (63, 65), (300, HW), (cap, HW), (cap, (1 << 24) - 1),
                                         (-1, 37 * 70), (cap + 1, 37 * 70), (40, 0), (40, -5), (40, 1 << 24), (0, 37 * 70)],
        "gags_featvis_moments_scratch_bytes": [(c, p) for c in (16, 3, 8, 32, 64, 128, 512, 24, 0, -16, 1024)
                                               for p in (1, 12, 12 * 13, 100003, HW, 0, -1, 1 << 31)],
        "gags_featvis_select_scratch_bytes": [(r,) for r in range(-1, 11)],
        "gags_promptgrid_scratch_bytes": [(1, 270, 480, 1, 270), (1, 3, 5, 1, 3), (2, 271, 481, 2, 135), (3, 540, 960, 4, 135),
                                          (1, H, W, 1, H), (1, H, W, 2, 540), (200, H, W, 8, 135), (300, H, W, 32, 34),
                                          (4, H, W, 4, 270), (0, 3, 5, 1, 3), (-1, 270, 480, 1, 270), (1, 0, 480, 1, 270),
                                          (1, 270, 0, 1, 270), (1, 270, 480, 0, 270), (1, 270, 480, 1, 0), (1, 270, 480, 1, 271),
                                          (1, 270, 480, 1, -1)],
        "gags_segment_stats_runs_copies": [(HW, 16, 300, 1), (HW, 1, 300, 0), (1000, 16, 300, 1), (HW, 16, 300, 0), (HW, 16, 20000, 1),
                                           (1, 1, 1, 0), (12345, 3, 77, 1), (12345, 3, 77, 0), (HW, 512, 300, 1), (HW, 3, 300, 1),
                                           (0, 16, 300, 1), (-1, 16, 300, 1), (HW, 0, 300, 1), (HW, 16, 0, 1), (HW, 16, 300, 2)],
    }


def functions():
    return sorted(k for k in _lib.SIGNATURES
                  if (k.endswith("_scratch_bytes") or k.endswith("_scratch_bytes_h16") or k in EXTRA) and k not in LATER)


def record(lib):
    tab = table(lib)
    missing = set(functions()) ^ set(tab)
    assert not missing, f"the table and _lib.SIGNATURES disagree about {sorted(missing)}"
    return [{"fn": fn, "args": list(a), "value": int(getattr(lib, fn)(*a))} for fn in functions() for a in tab[fn]]


def record_later(lib, fn):
    return [{"fn": fn, "args": list(a), "value": int(getattr(lib, fn)(*a))} for a in LATER[fn][1]]


def _write(path, rows):
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--later":
        directory = sys.argv[2] if len(sys.argv) > 2 else os.path.join("tests", "golden")
        for fn, (name, _) in LATER.items():
            _write(os.path.join(directory, name), record_later(_lib.load(), fn))
            print(f"{fn} -> {os.path.join(directory, name)}")
        return
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join("tests", "golden", "scratch_bytes.json")
    rows = record(_lib.load())
    _write(out, rows)
    print(f"{len(rows)} entries of {len(functions())} functions -> {out}")


if __name__ == "__main__":
    main()
