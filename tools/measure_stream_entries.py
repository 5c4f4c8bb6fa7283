"""Longest single C entry over all cases of tests/test_streams_gpu.py on the default stream, and over a step of its two-stream
test: the figure behind tests/stream_harness.py's MEASURED_ENTRY_MS (the delay of late_producers is at least 10 x that).
Run on an MI355X after adding a case: python tools/measure_stream_entries.py; exits 1 when DELAY_MS no longer covers it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import stream_harness as SH  # noqa: E402
import test_multistep_gpu as MS  # noqa: E402
import test_streams_gpu as TS  # noqa: E402
from gags_amd import rasterization as R, synthetic as syn  # noqa: E402
from gags_amd.gaussian_renderer import render  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def main():
    orc.build()
    TS._ORACLE["oracle"] = orc
    SH.calibrate()
    print("calibration:", SH._CAL, flush=True)
    worst = []
    for name in TS.CASES:
        TS._reference(name)  # (warm: module loads, the allocator)
        TS._REFERENCE.pop(name)
        with SH.time_entries() as spans:
            TS._reference(name)
        times = SH.entry_times(spans)
        print(f"{name}: {len(times)} entries, longest {times[:3]}", flush=True)
        worst += times[:3]
    for d in (128, 513):  # the shapes of test_six_steps_alternating_between_two_streams_equal_the_stateless_step
        pc = MS._make_model(6000, d, 200, 138, seed=4, mult=3)
        opt = pc.training_setup()
        cam = syn.make_camera(200, 138, view=3, device=TS.DEV)
        G = syn.make_cotangent(d, 138, 200, seed=2, device=TS.DEV)
        ctx = R.RasterContext()
        for _ in range(2):
            with SH.time_entries() as spans:
                (render(cam, pc, None, torch.zeros(3, device=TS.DEV), feature_mode=True, context=ctx)["render"] * G).sum().backward()
                opt.step()
                opt.zero_grad(set_to_none=True)
            times = SH.entry_times(spans)
        print(f"two-stream test, D = {d}: longest {times[:3]}", flush=True)
        worst += times[:3]
    worst.sort(reverse=True)
    print("LONGEST:", worst[:8])
    ok = 10.0 * worst[0][0] <= SH.DELAY_MS
    print(f"longest entry {worst[0][0]:.3f} ms ({worst[0][1]}); DELAY_MS = {SH.DELAY_MS} is {'at least' if ok else 'LESS THAN'} 10 x that")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
