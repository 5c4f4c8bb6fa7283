"""Late producers: what turns a kernel, memset or copy that went to the wrong stream into a wrong VALUE.

torch creates its streams non-blocking: the null stream does not wait for them, nor they for it.  late_producers(stream) wraps
every entry of the loaded library and enqueues a device-side delay (torch.cuda._sleep) on the current stream ahead of each real
call, so whatever a case enqueues on `stream` -- the copy of its inputs, every kernel of the package -- completes late.  Work
that was sent anywhere else (the null stream, a stream of another device's, a side stream that waits for no event) runs ahead
of its producers and reads what was in memory before: the decoy inputs of a case (valid data of another seed; see
tests/test_streams_gpu.py) or an unwritten intermediate.  The wrapper records (name, args) of every call; audit_streams() then
checks, without any race, that every entry that takes a `void *stream` received the handle of the stream it was called under.

The length of the delay is DELAY_MS, at least ten times the longest single C entry of the cases of tests/test_streams_gpu.py
(docs/LAB_NOTES.md, "Stream tests": how it was measured, with time_entries() below).  torch.cuda._sleep counts cycles; how many
make a millisecond is calibrated once per process with two timing events, and every use of late_producers() times its own
first delay and asserts that it lasted DELAY_MS: a sleep that returned early would make every test vacuous.
"""
import ast
import contextlib
import glob
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Longest single C entry over all cases of tests/test_streams_gpu.py on the default stream (event pairs placed by
# time_entries(), one MI355X): MEASURED_ENTRY_MS.  The delay is at least 10 x that (launch gaps, a busy card).
MEASURED_ENTRY_MS = 0.25
DELAY_MS = 3.0
assert DELAY_MS >= 10.0 * MEASURED_ENTRY_MS

_CAL = {}


def _prototypes():
    """{name: parameter list} of every function include/*.h declares (comments stripped as tests/test_abi_cpu.py does; the CPU
    twins of gags_cpu.h are not in the library)."""
    out = {}
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.basename(h) == "gags_cpu.h":
            continue
        src = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        src = re.sub(r"//[^\n]*", "", src)
        for name, params in re.findall(r"\b(gags_\w+)\s*\(([^;{}()]*)\)\s*;", src):
            out[name] = params
    return out


def streamed_entries():
    """Names of the C entries whose signature ends in `void *stream`."""
    return {n for n, p in _prototypes().items() if re.search(r"\bvoid\s*\*\s*stream\s*$", p.strip())}


def _code_names(source):
    """The gags_* names a module's CODE holds: attribute and variable names, and string constants (decoders.py looks its entries
    up through strings) -- not comments, and not docstrings or other bare strings."""
    tree = ast.parse(source)
    bare = {id(n.value) for n in ast.walk(tree) if isinstance(n, ast.Expr) and isinstance(n.value, ast.Constant)}
    names = set()
    for n in ast.walk(tree):
        if isinstance(n, ast.Attribute):
            names.add(n.attr)
        elif isinstance(n, ast.Name):
            names.add(n.id)
        elif isinstance(n, ast.Constant) and isinstance(n.value, str) and id(n) not in bare:
            names.update(re.findall(r"\bgags_\w+", n.value))
    return names


def _twin_bases(source):
    """The base names a module completes with a tier's suffix: the string handed to a call of `<tier>.fn(...)`
    (decoders._HalfTier.fn returns the entry base + "" or "_h16") and the left side of `"gags_..." + suffix`."""
    bases = set()
    for n in ast.walk(ast.parse(source)):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "fn":
            bases.update(a.value for a in n.args if isinstance(a, ast.Constant) and isinstance(a.value, str))
        elif isinstance(n, ast.BinOp) and isinstance(n.op, ast.Add) and isinstance(n.left, ast.Constant) \
                and isinstance(n.left.value, str) and re.fullmatch(r"gags_\w+", n.left.value):
            bases.add(n.left.value)
    return bases


def package_named_entries():
    """{entry name: [modules]} for every entry of _lib.SIGNATURES that the code of some gags_amd/*.py other than _lib.py names
    (_code_names), and for the "_h16" twin of every base name a module completes with a tier's suffix (_twin_bases): the f16
    decoder tier calls those."""
    from gags_amd import _lib
    text = {os.path.basename(f): open(f).read() for f in glob.glob(os.path.join(ROOT, "gags_amd", "*.py"))
            if os.path.basename(f) != "_lib.py"}
    src = {f: _code_names(t) | {b + "_h16" for b in _twin_bases(t)} for f, t in text.items()}
    out = {}
    for name in _lib.SIGNATURES:
        mods = sorted(f for f, names in src.items() if name in names)
        if mods:
            out[name] = mods
    return out


def calibrate():
    """Cycles of torch.cuda._sleep that last DELAY_MS (with a quarter to spare), measured once per process."""
    if "cycles" not in _CAL:
        probe = 20_000_000
        torch.cuda._sleep(1_000_000)  # (first launch: module load)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(probe)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0.05, f"torch.cuda._sleep({probe}) lasted {ms} ms: no usable delay on this build"
        _CAL["cycles_per_ms"] = probe / ms
        _CAL["cycles"] = int(1.25 * DELAY_MS * probe / ms)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(_CAL["cycles"])
        e1.record()
        e1.synchronize()
        _CAL["delay_ms"] = e0.elapsed_time(e1)
        assert _CAL["delay_ms"] >= DELAY_MS, f"the calibrated delay lasted {_CAL['delay_ms']} ms, {DELAY_MS} ms wanted"
    return _CAL["cycles"]


def delay():
    """One delay on the current stream."""
    torch.cuda._sleep(calibrate())


def runs_beside_the_null_stream(stream):
    """Whether work on the null stream completes while `stream` is held up by a delay.  Streams share a few hardware queues;
    one that shares the null stream's is served in submission order with it, and nothing sent to the null stream by mistake
    could run ahead of a late producer there."""
    null = torch.cuda.default_stream()
    held, early = torch.cuda.Event(), torch.cuda.Event()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        delay()
        held.record()
    with torch.cuda.stream(null):
        torch.zeros(1, device="cuda")
        early.record()
    early.synchronize()
    beside = not held.query()
    stream.synchronize()
    return beside


def concurrent_stream(avoid=()):
    """A torch.cuda.Stream() (not one of `avoid`) that was SEEN to run beside the null stream (torch hands out its streams from
    a pool of 32): on any other the tests of tests/test_streams_gpu.py would pass whatever the package did."""
    seen = set(int(s.cuda_stream) for s in avoid)
    for _ in range(64):
        s = torch.cuda.Stream()
        if int(s.cuda_stream) in seen:
            continue
        seen.add(int(s.cuda_stream))
        if int(s.cuda_stream) != 0 and runs_beside_the_null_stream(s):
            return s
    raise AssertionError(f"none of {len(seen)} streams ran beside the null stream: late producers cannot be staged here")


@contextlib.contextmanager
def _wrapped(before, after=None):
    """Every entry of _lib.SIGNATURES on the loaded library behind a wrapper (the pattern of helpers.spy_entries): before(name,
    args) runs ahead of the real call, after(name) behind it.  The real entries come back in a finally."""
    from gags_amd import _lib
    lib = _lib.load()
    real = {name: getattr(lib, name) for name in _lib.SIGNATURES}

    def wrap(name):
        fn = real[name]

        def f(*args):
            before(name, args)
            try:
                return fn(*args)
            finally:
                if after is not None:
                    after(name)
        return f
    for name in real:
        setattr(lib, name, wrap(name))
    try:
        yield
    finally:
        for name, fn in real.items():
            setattr(lib, name, fn)


@contextlib.contextmanager
def late_producers(stream, pending=None):
    """See the module docstring.  To be entered with `stream` current (`with torch.cuda.stream(s), late_producers(s) as calls`).
    Enqueues a first delay on `stream` at once -- a case copies its real inputs over the decoys behind it -- and one on the
    current stream ahead of every entry; yields the list that receives (name, args) of every call.  On a clean exit it waits
    for `stream` and asserts that the first delay lasted DELAY_MS -- or, given a list `pending`, leaves the stream running,
    appends its two events to the list and leaves the assertion to check_delays(pending) (a test that must not drain the
    device between two blocks)."""
    cycles = calibrate()
    calls = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()

    def before(name, args):
        torch.cuda._sleep(cycles)
        calls.append((name, args))
    with _wrapped(before):
        yield calls
    if pending is not None:
        pending.append((e0, e1))
        return
    stream.synchronize()
    check_delays([(e0, e1)])


def check_delays(pending):
    """Every first delay of `pending` (late_producers(stream, pending)) lasted DELAY_MS; waits for the device."""
    torch.cuda.synchronize()
    assert pending
    for e0, e1 in pending:
        lasted = e0.elapsed_time(e1)
        assert lasted >= DELAY_MS, f"the delay lasted {lasted} ms, {DELAY_MS} ms wanted: nothing was late"


@contextlib.contextmanager
def time_entries():
    """An event pair around every entry, on the current stream: yields the list of (name, start, end).  How MEASURED_ENTRY_MS
    was obtained (entry_times() after a synchronize); tools/measure_stream_entries.py repeats the measurement over CASES."""
    spans, open_ = [], []

    def before(name, args):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        open_.append(e)

    def after(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        spans.append((name, open_.pop(), e))
    with _wrapped(before, after):
        yield spans


def entry_times(spans):
    """[(milliseconds, name)] of time_entries()'s spans, longest first."""
    torch.cuda.synchronize()
    return sorted(((a.elapsed_time(b), name) for name, a, b in spans), reverse=True)


def _handle(arg):
    return getattr(arg, "value", arg) or 0


def audit_streams(calls, stream):
    """The calls of `calls` that took a `void *stream` and did NOT receive stream.cuda_stream, as [(index, name, handle)].  The
    handle of a side stream is not 0, the null stream's; a wrapper that passes none, or asks current_stream of another device,
    shows here without any race."""
    want = int(stream.cuda_stream)
    assert want != 0, "a side stream is wanted: the null stream's handle is 0"
    streamed = streamed_entries()
    assert len(streamed) > 100
    return [(i, name, _handle(args[-1])) for i, (name, args) in enumerate(calls)
            if name in streamed and _handle(args[-1]) != want]
