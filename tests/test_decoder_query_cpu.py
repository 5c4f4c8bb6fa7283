"""N15 without a GPU: what CNN_decoder.query and the fused= keyword of the 3-D query refuse before anything is launched, the
phrase operand's cache, and that header, ctypes prototypes and exported symbols of the two new entry points agree."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _head(n_pos, n_neg, c=512, seed=0):
    from gags_amd.relevancy import RelevancyHead
    g = torch.Generator().manual_seed(seed)
    return RelevancyHead(torch.randn(n_pos, c, generator=g), torch.randn(n_neg, c, generator=g))


def _dec(tier="bf16", out_dim=512):
    from gags_amd.decoders import CNN_decoder
    return CNN_decoder(16, out_dim, tier)


@pytest.mark.parametrize("tier", ["exact", "bf16x2", "bf16", "f16"])
def test_cpu_tensors_raise(tier):
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        _dec(tier).query(torch.zeros(16, 4, 4), _head(2, 3))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        _dec(tier).query(torch.zeros(16, 4, 4), _head(2, 3), pairs=True)


def test_head_width_must_be_the_decoders_output_width():
    with pytest.raises(ValueError, match="wide"):
        _dec(out_dim=512).query(torch.zeros(16, 4, 4), _head(2, 3, c=256))
    with pytest.raises(ValueError, match="wide"):
        _dec(out_dim=256).query(torch.zeros(16, 4, 4), _head(2, 3, c=512))


def test_empty_phrase_lists_raise():
    for n_pos, n_neg in ((0, 3), (2, 0), (0, 0)):
        with pytest.raises(ValueError, match="at least one positive and one negative"):
            _dec().query(torch.zeros(16, 4, 4), _head(n_pos, n_neg))


def test_more_than_32_phrases_raise_as_documented():
    from gags_amd import decoders
    assert decoders.QUERY_MAX_PHRASES == 32
    assert re.search(r"more than\s+32 phrases", decoders.CNN_decoder.query.__doc__)
    for tier in ("exact", "bf16"):  # (the composition's gags_relevancy has the same cap: no tier is served)
        with pytest.raises(ValueError, match="at most 32"):
            _dec(tier).query(torch.zeros(16, 4, 4), _head(29, 4))
    with pytest.raises(RuntimeError, match="must live on the GPU"):  # 32 pass the check (and stop at the CPU tensor)
        _dec().query(torch.zeros(16, 4, 4), _head(28, 4))


def test_x_must_be_three_dimensional():
    with pytest.raises(ValueError, match=r"\[C_in, H, W\]"):
        _dec().query(torch.zeros(16, 4), _head(2, 3))


def test_phrase_operand_is_cached_and_follows_the_head():
    from gags_amd.decoders import _query_phrases
    head = _head(2, 3)
    dev = torch.device("cpu")
    t0 = _query_phrases(head, dev)
    assert t0.shape == (5, 512) and t0.dtype == torch.float32 and t0.is_contiguous()
    assert torch.equal(t0[:2], head.pos_embeds) and torch.equal(t0[2:], head.neg_embeds)
    assert _query_phrases(head, dev) is t0                                   # nothing changed: the same tensor
    head.set_positives(torch.ones(4, 512))
    t1 = _query_phrases(head, dev)
    assert t1 is not t0 and t1.shape == (7, 512) and torch.equal(t1[:4], torch.ones(4, 512))
    head.neg_embeds.mul_(2.0)                                                # in place: the version counter moves
    t2 = _query_phrases(head, dev)
    assert t2 is not t1 and torch.equal(t2[4:], head.neg_embeds)
    head.pos_embeds[1].zero_()                                               # ... through a view as well
    t3 = _query_phrases(head, dev)
    assert t3 is not t2 and torch.equal(t3[1], torch.zeros(512))
    assert _query_phrases(head, dev) is t3


def test_point_query_functions_take_fused_and_default_to_the_old_path():
    from gags_amd import pointquery
    for fn in (pointquery.point_relevancy, pointquery.query_points, pointquery.query_ply):
        assert inspect.signature(fn).parameters["fused"].default is False
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        pointquery.point_relevancy(torch.zeros(10, 16), _dec(), _head(2, 3), fused=True)


# ---------------------------------------------------------------- header, prototypes, symbols

NAMES = ("gags_decoder_query_fused", "gags_decoder_query_fused_h16")
C_TYPES = {"int64_t": ctypes.c_int64, "int": ctypes.c_int}


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gags_next.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, f"{name} is not declared in include/gags_next.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.mark.parametrize("name", NAMES)
def test_header_prototype_ctypes_signature_and_export_agree(lib, name):
    from gags_amd import _lib
    args = _prototype(name)
    # the issue's order: n_pix, c_in, n_last, x, nine weights, nine biases, phrases, n_pos, n_neg, probs, stream
    assert [a.split()[-1].lstrip("*") for a in args] == ["n_pix", "c_in", "n_last", "x", "w_bf16", "bias", "phrases", "n_pos",
                                                         "n_neg", "probs", "stream"]
    want = [ctypes.c_void_p if "*" in a else C_TYPES[a.split()[0]] for a in args]
    res, argtypes = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and argtypes == want
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT %s$" % name, out, flags=re.M), f"{name} is not exported"
    assert _prototype(NAMES[0]) == _prototype(NAMES[1])  # the f16 twin: the same signature
    assert lib.gags_abi_version() == 2


@pytest.mark.parametrize("name", NAMES)
def test_argument_validation_returns_einval_without_launching(lib, name):
    fn = getattr(lib, name)
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    al = base + (-base % 16)
    P = ctypes.c_void_p(al)
    nine = (ctypes.c_void_p * 9)(*[al] * 9)
    holed = (ctypes.c_void_p * 9)(*([al] * 8 + [None]))
    assert fn(0, 16, 512, None, nine, nine, P, 5, 4, None, None) == 0            # n_pix == 0 is fine, and launches nothing
    assert fn(0, 16, 512, None, nine, nine, P, 0, 4, None, None) == -1           # ... but is validated like any call
    assert fn(-1, 16, 512, P, nine, nine, P, 5, 4, P, None) == -1
    assert fn(8, 0, 512, P, nine, nine, P, 5, 4, P, None) == -1
    assert fn(8, 33, 512, P, nine, nine, P, 5, 4, P, None) == -1
    assert fn(8, 16, 0, P, nine, nine, P, 5, 4, P, None) == -1
    assert fn(8, 16, 384, P, nine, nine, P, 5, 4, P, None) == -1                 # n_last % 256
    assert fn(8, 16, 512, P, nine, nine, P, 0, 4, P, None) == -1
    assert fn(8, 16, 512, P, nine, nine, P, 5, 0, P, None) == -1
    assert fn(8, 16, 512, P, nine, nine, P, 29, 4, P, None) == -1                # more than 32 phrases
    assert fn(8, 16, 512, None, nine, nine, P, 5, 4, P, None) == -1
    assert fn(8, 16, 512, P, None, nine, P, 5, 4, P, None) == -1
    assert fn(8, 16, 512, P, nine, None, P, 5, 4, P, None) == -1
    assert fn(8, 16, 512, P, holed, nine, P, 5, 4, P, None) == -1
    assert fn(8, 16, 512, P, nine, holed, P, 5, 4, P, None) == -1
    assert fn(8, 16, 512, P, nine, nine, None, 5, 4, P, None) == -1
    assert fn(8, 16, 512, P, nine, nine, P, 5, 4, None, None) == -1
    assert fn(8, 16, 512, P, nine, nine, ctypes.c_void_p(al + 4), 5, 4, P, None) == -1   # phrases: 16-byte loads
