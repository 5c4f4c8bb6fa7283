#!/usr/bin/env python
"""Times of the open-vocabulary query (N15): CNN_decoder.query's one kernel (csrc/decoder_query.hip) against the composition it
replaces, decoder(x) -> RelevancyHead.get_max_across, on the same GPU, in one process.

  view   rasterized features [16, H, W] (pixel-major memory, as render() returns them) -> [n_pos, H, W] relevancy, at 731 x 989
         (LERF) and 1080 x 1920, 5 positive + 4 negative phrases
  points pointquery.point_relevancy over N = 1.5 M Gaussians, fused=False (chunks of 1 M) against fused=True

for both 16-bit tiers.  HIP events; the two paths alternate, --reps rounds each after a warm-up of both; (median, min, max) ms.
Per path also: `lib_calls`, the library entry points one call goes through (kernel launches of this library; torch's own copies
are not counted), `peak_MB`, the rise of torch's peak allocation over one call, and `GBps`, the bytes the path must move over
the median -- fused: the features in and the probabilities out; composition: what its three kernels read and write by design
(the forward's kept activations, ReLU masks and logits, the normalised map written and read back, the probabilities).
Prints one JSON line.

--lib PATH times another build of the library, e.g. one whose decoder_query.hip was compiled with -DGAGS_ABL=1024 (no phrase
dots) or 2048 (no head reads at all): timing-only ablations, their results are wrong by construction.

    python tools/query_bench.py [--reps 20] [--views 731x989 1080x1920] [--points 1500000] [--tiers bf16 f16] [--lib PATH]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from gags_amd import _lib, decoders, pointquery, relevancy  # noqa: E402

N_POS, N_NEG, C_IN, C_OUT = 5, 4, 16, 512


def timed_pair(fa, fb, reps):
    """(stats of fa, stats of fb) in ms, the two alternating."""
    fa(), fb()
    torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(reps):
        for fn, acc in ((fa, ts[0]), (fb, ts[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            del out
            acc.append(a.elapsed_time(b))
    return tuple((round(sorted(t)[len(t) // 2], 4), round(min(t), 4), round(max(t), 4)) for t in ts)


def lib_calls(fn):
    """How many library entry points fn() goes through (every one is checked by _lib.check under the modules' own names)."""
    n = [0]
    saved = [(m, m.check) for m in (decoders, relevancy, pointquery)]

    def counting(code, what):
        n[0] += 1
        return saved[0][1](code, what)
    for m, _ in saved:
        m.check = counting
    try:
        fn()
    finally:
        for m, c in saved:
            m.check = c
    return n[0]


def peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)


def needed_bytes(p):
    """(fused, composition) bytes per call over p pixels."""
    fused = p * (4 * C_IN + 8 * N_POS)
    kept = p * (32 * 2 + 8 * 256 * 2 + 8 * 32)          # a0, eight activations, eight mask rows
    comp = p * 4 * C_IN + kept + 4 * p * C_OUT * 4 + 8 * p * N_POS   # logits out + in, map out + in, probabilities
    return fused, comp


def compare(fused, comp, p, reps):
    tf, tc = timed_pair(fused, comp, reps)
    bf, bc = needed_bytes(p)
    a, b = fused(), comp()
    r = {"fused_ms": tf, "composition_ms": tc, "speedup_median": round(tc[0] / tf[0], 2),
         "fused": {"lib_calls": lib_calls(fused), "peak_MB": peak_rise(fused), "needed_GB": round(bf / 1e9, 3),
                   "GBps": round(bf / tf[0] / 1e6, 1)},
         "composition": {"lib_calls": lib_calls(comp), "peak_MB": peak_rise(comp), "needed_GB": round(bc / 1e9, 3),
                         "GBps": round(bc / tc[0] / 1e6, 1)},
         "max_abs_diff": float((a - b).abs().max())}
    del a, b
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--views", nargs="*", default=["731x989", "1080x1920"])
    ap.add_argument("--points", type=int, default=1_500_000)
    ap.add_argument("--tiers", nargs="+", default=["bf16", "f16"])
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    if not torch.cuda.is_available():
        raise SystemExit("query_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    unit = torch.nn.functional.normalize
    head = relevancy.RelevancyHead(unit(torch.randn(N_POS, C_OUT, device=dev, generator=g), dim=1),
                                   unit(torch.randn(N_NEG, C_OUT, device=dev, generator=g), dim=1))
    res = {"tool": "query_bench", "unit": "ms (median, min, max)", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "phrases": [N_POS, N_NEG], "lib": args.lib or "default"}
    for tier in args.tiers:
        torch.manual_seed(0)
        dec = decoders.CNN_decoder(C_IN, C_OUT, tier).to(dev)
        out = {}
        for view in args.views:
            h, w = (int(v) for v in view.split("x"))
            x = torch.randn(h, w, C_IN, device=dev, generator=g).permute(2, 0, 1)
            with torch.no_grad():
                out[view] = compare(lambda: dec.query(x, head), lambda: head.get_max_across(dec(x).permute(1, 2, 0)[None])[0],
                                    h * w, args.reps)
            del x
        if args.points > 0:
            feat = torch.randn(args.points, C_IN, device=dev, generator=g)
            out[f"points_{args.points}"] = compare(lambda: pointquery.point_relevancy(feat, dec, head, fused=True),
                                                   lambda: pointquery.point_relevancy(feat, dec, head), args.points, args.reps)
            del feat
        res[tier] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
