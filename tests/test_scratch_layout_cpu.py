"""Every size-reporting export returns what it returned before the scratch layouts were rewritten as carve functions.

tests/golden/scratch_bytes.json was written by tools/record_scratch_bytes.py from the library of the commit BEFORE that
change (575dd8f), never from the code under test: a layout whose total drifts is a driver that writes past what its caller
allocated.  Re-record it only from the parent of a commit that changes a layout on purpose.
"""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import record_scratch_bytes as rec  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "scratch_bytes.json")


@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_covers_every_size_function_and_the_whole_table(lib, golden):
    recorded = {(r["fn"], tuple(r["args"])) for r in golden}
    table = {(fn, tuple(a)) for fn, rows in rec.table(lib).items() for a in rows}
    assert recorded == table                                   # no entry dropped from either side
    assert {fn for fn, _ in recorded} == set(rec.functions())  # every *_scratch_bytes export of _lib.SIGNATURES and the three others
    for fn in rec.functions():
        values = [r["value"] for r in golden if r["fn"] == fn]
        assert any(v > 0 for v in values), fn  # not a table of refusals


def test_byte_counts_equal_the_recorded_ones(lib, golden):
    wrong = [(r["fn"], r["args"], r["value"], got) for r in golden
             for got in [int(getattr(lib, r["fn"])(*r["args"]))] if got != r["value"]]
    assert not wrong, wrong[:10]
