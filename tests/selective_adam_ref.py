"""Restatement of the row-selective Adam step (gags_adam_step_rows, optim.SelectiveAdam) for the tests.

No arithmetic of its own: `oracle.adam_step` (float32 on the CPU, held bit-equal to the dense kernel by
test_parity_gpu.py::test_adam_step_matches_oracle_and_fixture) runs on a copy of the WHOLE arrays, the result is taken for
the selected rows and the inputs are kept elsewhere.  The selection -- mask and / or the bit-pattern zero test -- is numpy.

bias_correction=False is the oracle at step 10**6: with beta <= 0.999, pow(beta, 1e6) underflows to 0 in double
(1e6 ln 0.999 = -1000.5, below ln of the smallest subnormal, -744.4), both corrections are exactly 1, which is the declared
rule (step_size = lr, sqrt(v) undivided).  `no_bias_step_is_exact` is that statement as a predicate; the CPU test asserts it.
"""
import numpy as np

NO_BIAS_STEP = 10 ** 6


def no_bias_step_is_exact(beta1, beta2):
    return float(beta1) ** float(NO_BIAS_STEP) == 0.0 and float(beta2) ** float(NO_BIAS_STEP) == 0.0


def nonzero_rows(grad):
    """[N] bool: some element of the row has a bit pattern other than +-0 (NaN counts as non-zero)."""
    g = np.ascontiguousarray(grad, np.float32)
    g = g.reshape(g.shape[0], -1)
    return ((g.view(np.uint32) & np.uint32(0x7FFFFFFF)) != 0).any(axis=1)


def selection(grad, mask=None, skip_zero_rows=False):
    sel = np.ones(grad.shape[0], bool)
    if mask is not None:
        sel &= np.asarray(mask).reshape(-1) != 0
    if skip_zero_rows:
        sel &= nonzero_rows(grad)
    return sel


def step(oracle, p, g, m, v, lr, mask=None, skip_zero_rows=False, bias_correction=True, beta1=0.9, beta2=0.999, eps=1e-15,
         step=1):
    """(p, m, v) after the step, as new arrays of the inputs' shape [N, ...]; the inputs are not modified."""
    f = lambda a: np.array(a, dtype=np.float32, order="C", copy=True)  # noqa: E731
    p, g, m, v = f(p), f(g), f(m), f(v)
    po, mo, vo = p.copy(), m.copy(), v.copy()
    if not bias_correction:
        assert no_bias_step_is_exact(beta1, beta2)
    oracle.adam_step(po, g, mo, vo, lr, beta1, beta2, eps, step if bias_correction else NO_BIAS_STEP)
    sel = selection(g, mask, skip_zero_rows).reshape((-1,) + (1,) * (p.ndim - 1))
    return np.where(sel, po, p), np.where(sel, mo, m), np.where(sel, vo, v)


def assert_same_bits(got, want, label=""):
    """== on the bit patterns.  Where the reference holds a NaN (a NaN gradient was asked for) the result must be a NaN: IEEE
    754 leaves a NaN's sign and payload to the implementation, so there is no bit pattern to compare."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{label}: NaNs in other places"
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    bad = (gb != wb) & ~nan
    assert not bad.any(), f"{label}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0].tolist()}"
