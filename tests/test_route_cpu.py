"""raster_route._route: which kernels serve a call, decided once from plain values -- a hand-written table of named cases
(the expected _Route and the flag words that reach the C entries), and invariants over the whole input grid.  No GPU, no
library: the function takes no tensor.  tests/test_route_gpu.py runs the same cases on the kernels."""
import itertools
import os
import re

import pytest

from gags_amd import _lib as L
from gags_amd import rasterization as R

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NONE, COL, ALL, BG = (False,) * 5, (False, False, True, False, False), (True, True, True, True, False), (False,) * 4 + (True,)
# the header's values, by hand (tests/test_abi_cpu.py compares _lib's mirrors with the header itself)
COLORS_ONLY, NO_MFMA, FEAT_F16, F16MFMA_C, RECS, EXACT = 1, 2, 32, 64, 256, 2048
BIG = 1 << 21  # Gaussians: BIG x 16 channels reaches ZERO_FILL_MIN_ELEMS


def route(d, needs, n=300, f16=False, flags=0, prof=False, **ctx):
    return R._route(n, d, f16, needs, flags, prof, **ctx)


def expect(fwd, bwd, **kw):
    """The expected record: what a narrow, colour-blind, flag-less call gets, plus the stated fields."""
    base = dict(fwd_per_kernel=False, records=True, half=False, geom=False, colors=False, early_rowmap=False, trim=None,
                zero_fill=False, flags=0)
    return R._Route(fwd=fwd, bwd=bwd, **dict(base, **kw))


# name: (the route, the expected record, expected words: fwd / bwd / geom / stage -- None where that entry is not called)
CASES = {
    "D=3, colours only": (
        route(3, COL), expect("valu", "valu", records=False, colors=True, trim=False), (RECS, RECS | COLORS_ONLY, None, None)),
    "D=16, no gradient: lean": (
        route(16, NONE), expect("lean16", "none"), (RECS, None, None, None)),
    "D=16, no gradient, profiler on: split in two launches": (
        route(16, NONE, prof=True), expect("split", "none", fwd_per_kernel=True), (RECS, None, None, None)),
    "D=16, no gradient, GAGS_FWD_EXACT: split": (
        route(16, NONE, flags=L.GAGS_FWD_EXACT), expect("split", "none", flags=L.GAGS_FWD_EXACT), (RECS | EXACT, None, None, None)),
    "D=16, colours only: split, early row map, staged": (
        route(16, COL), expect("split", "staged", colors=True, early_rowmap=True), (RECS, None, None, 0)),
    "D=16, only the background requires grad: VALU colours-only backward": (
        route(16, BG), expect("split", "valu"), (RECS, RECS | COLORS_ONLY, None, None)),
    "D=24, all gradients: staged + matrix-core geometry, no early row map": (
        route(24, ALL), expect("split", "staged+geom", geom=True, colors=True), (RECS, None, RECS, 0)),
    "D=24, geometry without colours": (
        route(24, (True, True, False, True, False)), expect("split", "staged+geom", geom=True), (RECS, None, RECS, 0)),
    "D=24, all gradients, GAGS_BWD_F32MFMA": (
        route(24, ALL, flags=L.GAGS_BWD_F32MFMA), expect("split", "staged+geom", geom=True, colors=True, flags=L.GAGS_BWD_F32MFMA),
        (RECS, None, RECS | 32, 32)),
    "D=20, all gradients: VALU backward, nothing kept": (
        route(20, ALL), expect("split", "valu", geom=True, colors=True), (RECS, RECS, None, None)),
    "D=1028, colours only: split forward, no staged backward": (
        route(1028, COL), expect("split", "valu", colors=True), (RECS, RECS | COLORS_ONLY, None, None)),
    "fp16 table, D=128": (
        route(128, COL, f16=True), expect("split", "staged", half=True, colors=True, early_rowmap=True),
        (RECS | FEAT_F16, None, None, 64)),
    "fp16 table, D=128, GAGS_FWD_F16MFMA": (
        route(128, COL, f16=True, flags=L.GAGS_FWD_F16MFMA),
        expect("split", "staged", half=True, colors=True, early_rowmap=True, flags=L.GAGS_FWD_F16MFMA),
        (RECS | FEAT_F16 | F16MFMA_C, None, None, 64)),
    "fp16 table, D=64, GAGS_FWD_F16MFMA: the request does not apply": (
        route(64, COL, f16=True, flags=L.GAGS_FWD_F16MFMA), expect("split", "staged", half=True, colors=True, early_rowmap=True),
        (RECS | FEAT_F16, None, None, 64)),
    "fp16 table, D=128, GAGS_FWD_NO_MFMA: not half": (
        route(128, COL, f16=True, flags=L.GAGS_FWD_NO_MFMA), expect("valu", "valu", colors=True, trim=False, flags=NO_MFMA),
        (RECS | NO_MFMA, RECS | NO_MFMA | COLORS_ONLY, None, None)),
    "GAGS_BWD_ATOMIC, D=128": (
        route(128, COL, flags=L.GAGS_BWD_ATOMIC), expect("split", "valu", colors=True, flags=L.GAGS_BWD_ATOMIC),
        (RECS, RECS | COLORS_ONLY, None, None)),
    "GAGS_BWD_ATOMIC, D=128, all gradients": (
        route(128, ALL, flags=L.GAGS_BWD_ATOMIC), expect("split", "valu", geom=True, colors=True, flags=L.GAGS_BWD_ATOMIC),
        (RECS, RECS, None, None)),
    "GAGS_FWD_FUSED, D=128": (
        route(128, COL, flags=L.GAGS_FWD_FUSED), expect("fused", "valu", colors=True, trim=False, flags=L.GAGS_FWD_FUSED),
        (RECS, RECS | COLORS_ONLY, None, None)),
    "capacity_mode: no early row map": (
        route(16, COL, capacity_mode=True), expect("split", "staged", colors=True), (RECS, None, None, 0)),
    "early_rowmap switched off": (
        route(16, COL, early_rowmap=False), expect("split", "staged", colors=True), (RECS, None, None, 0)),
    "rows-kernel flags reach the stage word": (
        route(16, COL, flags=L.GAGS_BWD_BLOCKWAVES | L.GAGS_BWD_EXACT_WEIGHTS),
        expect("split", "staged", colors=True, early_rowmap=True, flags=L.GAGS_BWD_BLOCKWAVES | L.GAGS_BWD_EXACT_WEIGHTS),
        (RECS, None, None, 512 | 1024)),
    "overlap_zero_fill at a size worth it": (
        route(16, COL, n=BIG, overlap_zero_fill=True), expect("split", "staged", colors=True, early_rowmap=True, zero_fill=True),
        (RECS, None, None, 0)),
    "overlap_zero_fill, small table: no zero-fill": (
        route(16, COL, overlap_zero_fill=True), expect("split", "staged", colors=True, early_rowmap=True), (RECS, None, None, 0)),
    "grad_range_hook set: no zero-fill": (
        route(16, COL, n=BIG, overlap_zero_fill=True, hooked=True), expect("split", "staged", colors=True, early_rowmap=True),
        (RECS, None, None, 0)),
    "trim_lists forced / forbidden": (
        (route(16, COL, trim_lists=True).trim, route(16, COL, trim_lists=False).trim, route(3, COL, trim_lists=True).trim),
        (True, False, False), None),
    "n = 0": (
        route(16, COL, n=0), expect("fused", "valu", colors=True, trim=False), (RECS, RECS | COLORS_ONLY, None, None)),
    "late: no intersection, the lean render becomes the split one": (
        route(16, NONE).without_isects(), expect("split", "none"), (RECS, None, None, None)),
    "late: no intersection, one launch under the profiler and no early row map": (
        route(16, COL, prof=True).without_isects(), expect("split", "staged", colors=True), (RECS, None, None, 0)),
    "late: the scratch does not fit, fp16 table with GAGS_FWD_F16MFMA": (
        route(128, COL, f16=True, flags=L.GAGS_FWD_F16MFMA).without_scratch(),
        expect("fused", "valu", colors=True, flags=L.GAGS_FWD_F16MFMA), (RECS, RECS | COLORS_ONLY, None, None)),
    "late: the scratch does not fit, all gradients": (
        route(24, ALL).without_scratch(), expect("fused", "valu", geom=True, colors=True), (RECS, RECS, None, None)),
    "late: the scratch does not fit, nothing requires grad": (
        route(32, NONE, prof=True).without_scratch(), expect("fused", "none"), (RECS, None, None, None)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_named_case(name):
    got, want, words = CASES[name]
    assert got == want
    if words is None:
        return
    fwd, bwd, geom, stage = words
    assert R._fwd_flags(got) == fwd
    assert got.keeps_scratch == (stage is not None)  # a staged backward reads the scratch; nobody else does
    assert (got.bwd == "valu") == (bwd is not None) and (got.bwd == "staged+geom") == (geom is not None)
    if bwd is not None:
        assert R._bwd_flags(got) == bwd
    if geom is not None:
        assert R._geom_flags(got) == geom
    if stage is not None:
        assert R._stage_bits(got.flags, got.half) == stage


def _header_forward_bits():
    src = open(os.path.join(ROOT, "include", "gags_raster.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define\s+(GAGS_(?:FWD|FEAT|RECS)_\w+)\s+(\d+)\b", src, flags=re.M)}
    assert len(defs) == 7, defs
    return sum(defs.values())


FLAGS = [0, L.GAGS_BWD_COLORS_ONLY, L.GAGS_FWD_NO_MFMA, L.GAGS_BWD_ATOMIC, L.GAGS_FWD_FUSED, L.GAGS_FEAT_F16, L.GAGS_BWD_F32MFMA,
         L.GAGS_FWD_F16MFMA, L.GAGS_RECS_BY_GAUSSIAN, L.GAGS_FWD_ONLY_WEIGHTS, L.GAGS_FWD_ONLY_FEATURES, L.GAGS_FWD_EXACT,
         L.GAGS_BWD_BLOCKWAVES, L.GAGS_BWD_EXACT_WEIGHTS,
         L.GAGS_FWD_NO_MFMA | L.GAGS_FWD_FUSED, L.GAGS_BWD_ATOMIC | L.GAGS_FWD_FUSED, L.GAGS_FWD_F16MFMA | L.GAGS_BWD_F32MFMA,
         L.GAGS_FWD_EXACT | L.GAGS_BWD_ATOMIC, L.GAGS_FWD_F16MFMA | L.GAGS_FWD_EXACT]
SETTINGS = [dict(n=300), dict(n=0), dict(n=300, capacity_mode=True), dict(n=300, early_rowmap=False),
            dict(n=BIG, overlap_zero_fill=True), dict(n=BIG, overlap_zero_fill=True, hooked=True),
            dict(n=300, trim_lists=True), dict(n=300, trim_lists=False), dict(n=BIG, capacity_mode=True, overlap_zero_fill=True,
                                                                             hooked=True, trim_lists=True)]


def test_invariants_over_the_whole_grid():
    """Every combination of width, dtype, `needs`, flag (each alone, a few pairs), profiler and context settings, before and
    after each late downgrade.  The lean 16-channel render walks the same lists as the split forward and is trimmed with it, as
    before; everything else that presumes the split forward's scratch implies the split forward itself."""
    fwd_bits = _header_forward_bits()
    points = 0
    for d, f16, needs, flags, prof, ctx in itertools.product(
            (1, 3, 15, 16, 20, 24, 128, 513, 1024, 1028), (False, True), list(itertools.product((False, True), repeat=5)),
            FLAGS, (False, True), SETTINGS):
        r0 = route(d, needs, f16=f16, flags=flags, prof=prof, **ctx)
        for r in (r0, r0.without_isects(), r0.without_scratch() if r0.fwd == "split" else r0):
            points += 1
            split = r.fwd == "split"
            assert split or not (r.half or r.early_rowmap or r.keeps_scratch or r.fwd_per_kernel), r
            if r is r0:  # (trimming and the zero-fill are acted on before the late facts are known)
                assert r.trim is False or r.fwd in ("split", "lean16"), r
                assert not r.zero_fill or (r.bwd == "staged" and not ctx.get("hooked")), r
            assert r.fwd != "lean16" or (not any(needs) and r.bwd == "none"), r
            assert (r.bwd == "none") == (not any(needs)), r
            assert r.bwd != "staged+geom" or (16 <= d <= 1024 and d % 8 == 0 and r.geom), r
            assert r.bwd != "staged" or (16 <= d <= 1024 and r.colors and not r.geom), r
            assert not r.early_rowmap or (r.bwd == "staged" and not ctx.get("capacity_mode")), r
            assert r.records == (d >= 16), r
            # (a caller's own GAGS_BWD_COLORS_ONLY bit is handed on as it is, as before; gags_raster_fwd does not read it)
            word = R._fwd_flags(r)
            assert not (word & ~(fwd_bits | (flags & L.GAGS_BWD_COLORS_ONLY))), (r, word)
            assert not (word & (L.GAGS_FWD_ONLY_WEIGHTS | L.GAGS_FWD_ONLY_FEATURES)), (r, word)  # (the launches add them)
            assert bool(word & L.GAGS_FEAT_F16) == r.half and (not (word & L.GAGS_FWD_F16MFMA_C) or (r.half and d >= 128)), (r, word)
    assert points == 10 * 2 * 32 * len(FLAGS) * 2 * len(SETTINGS) * 3
