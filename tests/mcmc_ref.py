"""numpy restatement of the MCMC density rules R1-R6 (DESIGN.md section 7 "N18"), written from the declared rules and not from
the kernels.  float64 unless a dtype is passed; the float32 runs of the noise and the regularisers give the tests' bounds."""
import math

import numpy as np

TOP = 1.0 - 2.0 ** -23
MAX_RATIO = 51


# ---- R1 -------------------------------------------------------------------------------------------------------------------
def new_opacity(o, r):
    """1 - (1 - o)^(1/r), written so that a small o keeps its digits."""
    return -np.expm1(np.log1p(-np.asarray(o, np.float64)) / r)


def denom(o_new, r):
    """sum_{i=1..r} sum_{k=0..i-1} C(i-1, k) (-1)^k o_new^(k+1) / sqrt(k+1), in that order; o_new an array, r one integer."""
    o_new = np.asarray(o_new, np.float64)
    d = np.zeros_like(o_new)
    for i in range(1, r + 1):
        for k in range(i):
            d = d + float(math.comb(i - 1, k)) * (-1.0) ** k * o_new ** (k + 1) / math.sqrt(k + 1)
    return d


def relocation(o, r):
    """(o_new, denom, coeff) for opacities o (already clamped to TOP) and ONE ratio r, clamped to [1, 51]."""
    r = min(max(int(r), 1), MAX_RATIO)
    o = np.asarray(o, np.float64)
    o_new = new_opacity(o, r)
    d = denom(o_new, r)
    return o_new, d, o / d


def relocation_values(logit, scaling, ratios, min_opacity):
    """Stored float32 (logit [N], scaling [N, 3]) and integer ratios [N] -> the new stored values in float64."""
    x = np.asarray(logit, np.float64).reshape(-1)
    s = np.asarray(scaling, np.float64).reshape(-1, 3)
    ratios = np.clip(np.asarray(ratios).reshape(-1), 1, MAX_RATIO)
    o = np.minimum(1.0 / (1.0 + np.exp(-x)), TOP)
    new_x, new_s = np.empty_like(x), np.empty_like(s)
    for r in np.unique(ratios):
        m = ratios == r
        o_new, _, coeff = relocation(o[m], r)
        c = np.clip(o_new, min_opacity, TOP)
        new_x[m] = np.log(c / (1.0 - c))
        new_s[m] = s[m] + np.log(coeff)[:, None]
    return new_x, new_s


# ---- R2 -------------------------------------------------------------------------------------------------------------------
def sample(cdf, u):
    """draws [n], counts [N] from a cdf [N] (float64) and uniforms u [n]: the first j with cdf[j] > u cdf[N-1], else the first
    j with cdf[j] == cdf[N-1]."""
    cdf = np.asarray(cdf, np.float64)
    total = cdf[-1]
    draws = np.empty(len(u), np.int64)
    for a, uu in enumerate(np.asarray(u, np.float64)):
        above = np.nonzero(cdf > uu * total)[0]
        draws[a] = above[0] if len(above) else np.nonzero(cdf == total)[0][0]
    return draws, np.bincount(draws, minlength=len(cdf))


# ---- R4 / R7 --------------------------------------------------------------------------------------------------------------
def n_target(n, cap_max):
    return min(cap_max, int(1.05 * n))


def refines(step, start, stop, every):
    return start < step < stop and step % every == 0


# ---- R5 -------------------------------------------------------------------------------------------------------------------
def rotation_matrices(q, dtype):
    """utils/general_utils.py:78-99 on the normalised (w, x, y, z)."""
    q = np.asarray(q, dtype)
    q = q / np.sqrt((q * q).sum(1, dtype=dtype))[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3), dtype)
    two, one = dtype(2), dtype(1)
    R[:, 0, 0] = one - two * (y * y + z * z); R[:, 0, 1] = two * (x * y - r * z); R[:, 0, 2] = two * (x * z + r * y)
    R[:, 1, 0] = two * (x * y + r * z); R[:, 1, 1] = one - two * (x * x + z * z); R[:, 1, 2] = two * (y * z - r * x)
    R[:, 2, 0] = two * (x * z - r * y); R[:, 2, 1] = two * (y * z + r * x); R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def noise(xyz, logit, scaling, rotation, z, scaler, dtype=np.float64):
    with np.errstate(over="ignore"):
        f = lambda a: np.asarray(a, dtype)  # noqa: E731
        one = dtype(1)
        o = one / (one + np.exp(-f(logit).reshape(-1)))
        gate = one / (one + np.exp(dtype(-100) * ((one - o) - dtype(0.995))))
        M = rotation_matrices(rotation, dtype) * np.exp(f(scaling))[:, None, :]
        sigma = M @ M.transpose(0, 2, 1)
        v = f(z) * gate[:, None] * dtype(scaler)
        return f(xyz) + (sigma @ v[:, :, None])[:, :, 0]


# ---- R6 -------------------------------------------------------------------------------------------------------------------
def regularisation(logit, scaling, opacity_reg, scale_reg, dtype=np.float64):
    """(value, d value / d logit [N], d value / d scaling [N, 3])."""
    x, s = np.asarray(logit, dtype).reshape(-1), np.asarray(scaling, dtype).reshape(-1, 3)
    one = dtype(1)
    o, e = one / (one + np.exp(-x)), np.exp(s)
    n = dtype(len(x))
    value = dtype(opacity_reg) * o.mean(dtype=dtype) + dtype(scale_reg) * e.mean(dtype=dtype)
    return value, dtype(opacity_reg) / n * (o * (one - o)), dtype(scale_reg) / (dtype(3) * n) * e
