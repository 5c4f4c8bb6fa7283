"""N18 without a GPU: the restatement tests/mcmc_ref.py against independent arithmetic (the r = 1 anchor, the centre identity, the
integral form, 60-digit decimals), the tie rules of the sampling on hand-made cdfs, the schedule and the growth target as pure
functions, and the argument validation of the new C entries (GAGS_EINVAL before any launch)."""
import ctypes
import decimal
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mcmc_ref as R  # noqa: E402

OPACITIES = (0.005, 0.1, 0.5, 0.9, 0.99, 1.0 - 2.0 ** -23)
RATIOS = (1, 2, 7, 51)
GRID = [(o, r) for o in OPACITIES for r in RATIOS]


def test_ratio_one_changes_nothing():
    for o in OPACITIES:
        o_new, d, coeff = R.relocation(np.array([o]), 1)
        assert abs(o_new[0] - o) <= 2e-16 * o and abs(coeff[0] - 1.0) <= 4e-16, (o, o_new, coeff)
    # ratios outside [1, 51] are clamped
    assert np.array_equal(R.relocation(np.array([0.3]), 0)[0], R.relocation(np.array([0.3]), 1)[0])
    assert np.array_equal(R.relocation(np.array([0.3]), 99)[1], R.relocation(np.array([0.3]), 51)[1])


@pytest.mark.parametrize("o,r", GRID)
def test_centre_identity(o, r):
    """r coincident copies of opacity o_new composite to the original alpha at the centre: (1 - o_new)^r = 1 - o."""
    o_new = float(R.new_opacity(o, r))
    got, want = (1.0 - o_new) ** r, 1.0 - o
    print(f"\no={o!r} r={r}: (1 - o_new)^r = {got!r}, 1 - o = {want!r}")
    assert abs(got - want) <= 1e-13 * max(want, 1e-3)  # ((1 - o_new) carries 1e-16 absolute, raised to the power r <= 51)


@pytest.mark.parametrize("o,r", GRID)
def test_denominator_equals_the_integral_form(o, r):
    """denom = (2 / sqrt(pi)) sum_i int_0^inf o_new e^{-t^2} (1 - o_new e^{-t^2})^{i-1} dt: all terms positive."""
    from scipy.integrate import quad
    o_new = float(R.new_opacity(o, r))

    def f(t):
        a = o_new * math.exp(-t * t)
        return sum(a * (1.0 - a) ** (i - 1) for i in range(1, r + 1))
    val, err = quad(f, 0.0, np.inf, epsabs=0.0, epsrel=1e-12, limit=200)
    want = 2.0 / math.sqrt(math.pi) * val
    got = float(R.denom(np.array([o_new]), r)[0])
    rel = abs(got - want) / want
    print(f"\no={o!r} r={r}: denom {got!r}, integral {want!r} (quad's estimate {err:.1e}), relative difference {rel:.2e}")
    assert rel <= 1e-9  # (the quadrature's own accuracy, not the sum's: the decimal test below holds the sum to 1e-11)


@pytest.mark.parametrize("o,r", GRID)
def test_denominator_against_sixty_digit_decimals(o, r):
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        od = D(o)  # exact
        o_new = 1 - ((1 - od).ln() / r).exp()
        den = D(0)
        for i in range(1, r + 1):
            for k in range(i):
                den += D(math.comb(i - 1, k)) * (-1) ** k * o_new ** (k + 1) / D(k + 1).sqrt()
        coeff = od / den
        got_new, got_den, got_coeff = (float(v[0]) for v in R.relocation(np.array([o]), r))
        rels = [abs(float((D(g) - w) / w)) for g, w in ((got_new, o_new), (got_den, den), (got_coeff, coeff))]
    print(f"\no={o!r} r={r}: relative error of o_new {rels[0]:.2e}, denom {rels[1]:.2e}, coeff {rels[2]:.2e} (bound 1e-11)")
    assert max(rels) <= 1e-11


def test_sampling_tie_rules():
    def draw(w, u):
        cdf = np.cumsum(np.asarray(w, np.float64))
        return R.sample(cdf, u)[0].tolist(), cdf
    # zero weights at the front, in the middle and at the end are never drawn
    w = [0.0, 0.0, 1.0, 0.0, 2.0, 0.0, 0.0]
    us = [0.0, 0.2, 1.0 / 3.0, 0.5, 0.999999, np.nextafter(1.0, 0.0)]
    got, cdf = draw(w, us)
    assert got == [2, 2, 4, 4, 4, 4]  # u = 0 -> the first positive row; t == cdf[2] (u = 1/3: 3 * (1/3) == 1.0) -> the next one
    assert us[2] * cdf[-1] == cdf[2]
    # t >= total: the first row that reaches the total, not a zero-weight row behind it
    assert draw(w, [1.0, 1.5])[0] == [4, 4]
    assert draw([0.0, 0.0, 0.0], [0.0, 0.7])[0] == [0, 0]  # total 0: cdf[0] == total
    assert draw([3.0], [0.0, 0.99])[0] == [0, 0]
    d, c = R.sample(np.cumsum([1.0, 0.0, 1.0]), [0.1, 0.6, 0.7, 0.2])
    assert d.tolist() == [0, 2, 2, 0] and c.tolist() == [2, 0, 2]


def test_schedule_and_growth_target_as_pure_functions():
    from gags_amd import mcmc
    for n, cap in ((1000, 1000), (999, 1000), (1000, 1049), (1000, 2000), (19, 100), (20, 100), (0, 10), (200, 205), (200, 100)):
        assert mcmc.n_target(n, cap) == R.n_target(n, cap) == min(cap, int(1.05 * n))
    assert mcmc.n_target(1000, 1000) - 1000 == 0                  # at the cap
    assert mcmc.n_target(999, 1000) - 999 == 1                    # one below the cap: 1048 is capped to 1000
    assert all(mcmc.n_target(n, 10 ** 9) == n for n in range(20)) and mcmc.n_target(20, 10 ** 9) == 21
    assert max(0, mcmc.n_target(200, 100) - 200) == 0             # above the cap: nothing is added (and nothing removed)
    s = mcmc.MCMCStrategy()
    assert (s.cap_max, s.noise_lr, s.refine_start_iter, s.refine_stop_iter, s.refine_every, s.min_opacity) == \
        (1_000_000, 5e5, 500, 25_000, 100, 0.005)
    on = [t for t in range(0, 26_000) if s.refines(t)]
    assert on[0] == 600 and on[-1] == 24_900 and len(on) == 244 and all(t % 100 == 0 for t in on)
    assert on == [t for t in range(0, 26_000) if R.refines(t, 500, 25_000, 100)]
    t = mcmc.MCMCStrategy(refine_start_iter=0, refine_every=2, refine_stop_iter=7)
    assert [k for k in range(10) if t.refines(k)] == [2, 4, 6]


@pytest.fixture(scope="module")
def lib():
    from gags_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_new_entries_validate_their_arguments_without_launching(lib):
    from gags_amd import _lib
    buf = (ctypes.c_double * 64)()
    P = ctypes.c_void_p(ctypes.addressof(buf))
    E = -1  # GAGS_EINVAL
    assert lib.gags_mcmc_sample(-1, P, 1, P, P, P, None) == E
    assert lib.gags_mcmc_sample(4, P, -1, P, P, P, None) == E
    assert lib.gags_mcmc_sample(4, P, 1 << 31, P, P, P, None) == E
    assert lib.gags_mcmc_sample(0, P, 1, P, P, P, None) == E                  # a draw from no rows
    for k in range(4):
        args = [P] * 4
        args[k] = None
        assert lib.gags_mcmc_sample(4, args[0], 2, args[1], args[2], args[3], None) == E
    assert lib.gags_mcmc_sample(4, None, 0, None, None, None, None) == 0       # no draws: nothing to do
    assert lib.gags_mcmc_relocation(-1, P, 1, 0.005, P, P, None) == E
    assert lib.gags_mcmc_relocation(4, P, 2, 0.005, P, P, None) == E           # ratio_bias
    assert lib.gags_mcmc_relocation(4, P, -1, 0.005, P, P, None) == E
    for bad in (0.0, 1.0, -0.1, float("nan")):
        assert lib.gags_mcmc_relocation(4, P, 1, bad, P, P, None) == E         # min_opacity outside (0, 1)
    assert lib.gags_mcmc_relocation(4, None, 1, 0.005, P, P, None) == E
    assert lib.gags_mcmc_relocation(4, P, 1, 0.005, None, P, None) == E
    assert lib.gags_mcmc_relocation(4, P, 1, 0.005, P, None, None) == E
    assert lib.gags_mcmc_relocation(0, None, 1, 0.005, None, None, None) == 0

    def table(*descs):
        return ctypes.cast((_lib.GatherDesc * len(descs))(*descs), ctypes.c_void_p), len(descs)
    a = ctypes.addressof(buf)
    good = _lib.GatherDesc(a, a, 3, _lib.GAGS_GATHER_COPY)
    t, k = table(good)
    assert lib.gags_mcmc_copy_rows(-1, P, P, 4, k, t, None) == E
    assert lib.gags_mcmc_copy_rows(1 << 31, P, P, 4, k, t, None) == E
    assert lib.gags_mcmc_copy_rows(2, P, P, -1, k, t, None) == E
    assert lib.gags_mcmc_copy_rows(2, P, P, 4, _lib.GAGS_GATHER_MAX_DESC + 1, t, None) == E
    assert lib.gags_mcmc_copy_rows(2, P, P, 4, 1, None, None) == E
    assert lib.gags_mcmc_copy_rows(2, None, P, 4, k, t, None) == E
    assert lib.gags_mcmc_copy_rows(2, P, None, 4, k, t, None) == E
    for bad in (_lib.GatherDesc(a, a + 64, 3, 0), _lib.GatherDesc(None, None, 3, 0), _lib.GatherDesc(a, a, 0, 0),
                _lib.GatherDesc(a, a, 3, 2)):                                   # not in place, null, empty rows, unknown mode
        t2, k2 = table(good, bad)
        assert lib.gags_mcmc_copy_rows(2, P, P, 4, k2, t2, None) == E
    assert lib.gags_mcmc_copy_rows(0, None, None, 4, k, t, None) == 0
    assert lib.gags_mcmc_noise(-1, P, P, P, P, 1.0, P, None) == E
    assert lib.gags_mcmc_noise(4, P, P, P, P, float("inf"), P, None) == E
    assert lib.gags_mcmc_noise(4, P, P, P, P, float("nan"), P, None) == E
    for k in range(5):
        args = [P] * 5
        args[k] = None
        assert lib.gags_mcmc_noise(4, args[0], args[1], args[2], args[3], 1.0, args[4], None) == E
    assert lib.gags_mcmc_noise(0, None, None, None, None, 1.0, None, None) == 0
    assert lib.gags_mcmc_reg_partials(1) == 1 and lib.gags_mcmc_reg_partials(256) == 1 and lib.gags_mcmc_reg_partials(257) == 2
    assert lib.gags_mcmc_reg_partials(0) == 1
    assert lib.gags_mcmc_reg_fwd(-1, P, P, 0.01, 0.01, P, 64, P, None) == E
    assert lib.gags_mcmc_reg_fwd(4, P, P, 0.01, 0.01, P, 64, None, None) == E
    assert lib.gags_mcmc_reg_fwd(4, None, P, 0.01, 0.01, P, 64, P, None) == E
    assert lib.gags_mcmc_reg_fwd(4, P, None, 0.01, 0.01, P, 64, P, None) == E
    assert lib.gags_mcmc_reg_fwd(4, P, P, 0.01, 0.01, None, 64, P, None) == E
    assert lib.gags_mcmc_reg_fwd(257, P, P, 0.01, 0.01, P, 4, P, None) == E     # short scratch: two rows wanted
    assert lib.gags_mcmc_reg_fwd(4, P, P, 0.01, 0.01, P, 3, P, None) == E
    assert lib.gags_mcmc_reg_fwd(4, P, P, float("nan"), 0.01, P, 64, P, None) == E
    assert lib.gags_mcmc_reg_bwd(-1, P, P, 0.01, 0.01, P, P, P, None) == E
    assert lib.gags_mcmc_reg_bwd(4, P, P, 0.01, float("inf"), P, P, P, None) == E
    for k in range(5):
        args = [P] * 5
        args[k] = None
        assert lib.gags_mcmc_reg_bwd(4, args[0], args[1], 0.01, 0.01, args[2], args[3], args[4], None) == E
    assert lib.gags_mcmc_reg_bwd(0, None, None, 0.01, 0.01, None, None, None, None) == 0
    # the binding's mirror of the header's constant
    src = open(os.path.join(HERE, "..", "include", "gags_next.h")).read()
    assert f"#define GAGS_MCMC_MAX_RATIO {_lib.GAGS_MCMC_MAX_RATIO}\n" in src and _lib.GAGS_MCMC_MAX_RATIO == R.MAX_RATIO


def test_cpu_tensors_are_refused():
    import torch
    from gags_amd import mcmc
    with pytest.raises(RuntimeError, match="no CPU path"):
        mcmc.sample(torch.ones(4, dtype=torch.float64), 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mcmc.relocation_values(torch.zeros(4), torch.zeros(4, 3), torch.ones(4, dtype=torch.int32))
