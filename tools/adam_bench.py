#!/usr/bin/env python
"""Row-selective Adam (gags_adam_step_rows) against the dense kernel it stands beside (gags_adam_step, the
baseline) in one process, alternating, one warm-up round of each, then the median, minimum and maximum of --reps rounds, HIP
events around each call.  The baseline's minimum .. 90th percentile is the run-to-run spread every other line is read against
(the maximum is printed too; one late round in forty moves it by a third).

Per width W in --widths (default 16, 64, 512) at N = 1.5 M (C3's N), tables [N, W]:
  dense             gags_adam_step over the whole table (28 B per element)
  a_all_live        gags_adam_step_rows, no mask, no zero test (every row updated)
  a_all_live_mask   the same rows through an all-true mask, a_all_live_test through the zero test of a gradient without zero rows
  b_scattered_mask  27 % of the rows live, scattered, selected by the mask; b_scattered_test: the other rows' gradient is zero
  c_contiguous_mask the same number of rows as one contiguous block, by the mask; c_contiguous_test by the zero test
Then the seven tensors of the RGB stage ([N,3] [N,1,3] [N,15,3] [N,1] [N,3] [N,4] [N,16]): seven gags_adam_step launches
against one gags_adam_step_rows launch, all rows live, and that launch with the 27 % scattered mask.
GB/s figures count the bytes the rule HAS to move: 28 B per element of a live row, 4 B per element of a row the zero test
skips, 1 B per row for a mask.  Prints one JSON line.

    python tools/adam_bench.py [--n 1500000] [--widths 16,64,512] [--reps 20]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gags_amd import _lib  # noqa: E402

DEV = "cuda"
LIVE = 0.27
RGB_SHAPES = ((3,), (1, 3), (15, 3), (1,), (3,), (4,), (16,))
HYPER = (1e-3, 0.9, 0.999, 1e-15)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "p90": round(ts[(9 * len(ts)) // 10], 4),
            "max": round(ts[-1], 4)}


class Table:
    """Parameter, two moments and a gradient of one shape."""

    def __init__(self, n, shape, gen):
        self.n, self.width = n, 1
        for s in shape:
            self.width *= s
        self.p = torch.randn((n,) + shape, device=DEV, generator=gen)
        self.m = 0.1 * torch.randn((n,) + shape, device=DEV, generator=gen)
        self.v = 0.01 * torch.rand((n,) + shape, device=DEV, generator=gen)
        self.g = torch.randn((n,) + shape, device=DEV, generator=gen)

    def desc(self, grad=None):
        g = self.g if grad is None else grad
        return _lib.AdamTensor(self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.width, *HYPER)


def dense_call(lib, tables, stream):
    def run():
        for t in tables:
            _lib.check(lib.gags_adam_step(t.p.numel(), _lib.ptr(t.p), _lib.ptr(t.g), _lib.ptr(t.m), _lib.ptr(t.v), *HYPER, 3,
                                          stream), "gags_adam_step")
    return run


def rows_call(lib, n, descs, mask, flags, stream):
    table = (_lib.AdamTensor * len(descs))(*descs)

    def run():
        _lib.check(lib.gags_adam_step_rows(n, len(descs), ctypes.cast(table, ctypes.c_void_p), _lib.ptr(mask), flags, 3, stream),
                   "gags_adam_step_rows")
    return run


def measure(paths, reps):
    for fn in paths.values():
        fn()
    ts = {k: [] for k in paths}
    for _ in range(reps):
        for k, fn in paths.items():
            ts[k].append(timed(fn))
    return {k: stats(v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_500_000)
    ap.add_argument("--widths", default="16,64,512")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_bench: needs a GPU (no time is reported without one)")
    lib = _lib.load()
    n = args.n
    stream = _lib.stream(torch.device(DEV, 0))
    gen = torch.Generator(device=DEV).manual_seed(0)
    scattered = torch.rand(n, device=DEV, generator=gen) < LIVE
    n_live = int(scattered.sum())
    contiguous = torch.zeros(n, dtype=torch.bool, device=DEV)
    contiguous[n // 3:n // 3 + n_live] = True
    masks = {"scattered": scattered.view(torch.uint8), "contiguous": contiguous.view(torch.uint8)}
    everything = torch.ones(n, dtype=torch.uint8, device=DEV)
    TEST = _lib.GAGS_ADAM_SKIP_ZERO_ROWS
    row = {"tool": "adam_bench", "unit": "ms", "n": n, "reps": args.reps, "live_rows": n_live, "widths": {}}
    for w in [int(s) for s in args.widths.split(",")]:
        t = Table(n, (w,), gen)
        zeroed = {k: t.g * m.view(torch.bool)[:, None] for k, m in masks.items()}
        paths = {"dense": dense_call(lib, [t], stream),
                 "a_all_live": rows_call(lib, n, [t.desc()], None, 0, stream),
                 "a_all_live_mask": rows_call(lib, n, [t.desc()], everything, 0, stream),
                 "a_all_live_test": rows_call(lib, n, [t.desc()], None, TEST, stream)}
        for k, letter in (("scattered", "b"), ("contiguous", "c")):
            paths[f"{letter}_{k}_mask"] = rows_call(lib, n, [t.desc()], masks[k], 0, stream)
            paths[f"{letter}_{k}_test"] = rows_call(lib, n, [t.desc(zeroed[k])], None, TEST, stream)
        res = measure(paths, args.reps)
        full = 28.0 * n * w
        must = {"dense": full, "a_all_live": full, "a_all_live_mask": full + n, "a_all_live_test": full}
        for k in ("b_scattered", "c_contiguous"):
            must[k + "_mask"] = 28.0 * n_live * w + n
            must[k + "_test"] = 28.0 * n_live * w + 4.0 * (n - n_live) * w
        for k in res:
            res[k]["GBps_of_required_bytes"] = round(must[k] / (res[k]["median"] * 1e-3) / 1e9, 1)
            res[k]["time_over_dense"] = round(res[k]["median"] / res["dense"]["median"], 3)
        res["a_all_live_within_dense_spread"] = bool(res["a_all_live"]["median"] <= res["dense"]["p90"])
        row["widths"][str(w)] = res
        del t, zeroed, paths
        torch.cuda.empty_cache()
    tables = [Table(n, s, gen) for s in RGB_SHAPES]
    descs = [t.desc() for t in tables]
    row["rgb_groups"] = measure({"seven_dense_launches": dense_call(lib, tables, stream),
                                 "one_rows_launch": rows_call(lib, n, descs, None, 0, stream),
                                 "one_rows_launch_scattered_mask": rows_call(lib, n, descs, masks["scattered"], 0, stream)},
                                args.reps)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
