"""A float64 restatement of one layer of the 16-bit decoder tiers (gags_decoder_layer / gags_decoder_layer_h16,
csrc/decoder_gemm.hip), written from the kernel's contract (no import of gags_amd), with the error bound the kernel is held to
and the operand generators of its tests:

    a    = a1                                         one source
         = 16-bit( fp32(a1) + fp32(a2) )              two sources: added in fp32, rounded ONCE to the 16-bit type
    z    = sum_k a[p, k] w[n, k] + bias[n]            (float64 here; fp32 accumulation in the kernel)
    v    = max(z, 0) with relu, else z
    pre  = v + residual[p, n]
    post = pre where mask_src[p, n] > 0, else exactly +0
    S    = sum_k |a[p, k]| |w[n, k]| + |bias[n]| + |residual[p, n]|

`bound(S, K) = 2 (K + 3) U S`, U = 2^-24: the kernel forms `pre` with K accumulations and the bias, floor and residual adds.
The product of two bfloat16 (8 x 8 significand bits) or two half (11 x 11) values is exact in fp32, so each of those K + 3 steps
errs by less than one fp32 ulp of a partial result no larger than S, i.e. by less than 2 U S, whether the matrix core rounds
to nearest or truncates inside an instruction.  The bound is derived, not measured.

tests/test_decoder_layer_cpu.py checks this file against torch's float64 conv2d + relu and checks that the generated operands
make the bound a sensitive one; tests/test_decoder_layer_gpu.py then holds the HIP kernels to it element by element.
"""
import torch

from loss_ref import U

F16_MAX = 65504.0


# ------------------------------------------------------------------------------------------------------- the restatement
def layer_input(a1, a2, dtype):
    """The 16-bit activation the layer multiplies: a1, or the two sources added in fp32 and rounded once."""
    if a2 is None:
        return a1
    return (a1.float() + a2.float()).to(dtype)


def layer_ref(a1, a2, w, bias, relu, mask_src, residual, dtype):
    """(pre, post, S) in float64 from the kernel's own 16-bit operands: a1 / a2 [P, K], w [N, K], bias fp32 [N] or None,
    mask_src / residual 16-bit [P, N] or None."""
    a = layer_input(a1, a2, dtype).double()
    wd = w.double()
    z = a @ wd.t()
    S = a.abs() @ wd.abs().t()
    if bias is not None:
        z = z + bias.double()
        S = S + bias.double().abs()
    v = torch.clamp_min(z, 0.0) if relu else z
    pre = v
    if residual is not None:
        pre = v + residual.double()
        S = S + residual.double().abs()
    post = pre
    if mask_src is not None:
        post = torch.where(mask_src.float() > 0, pre, torch.zeros_like(pre))
    return pre, post, S


def bound(S, K):
    """Per-element error bound of the kernel's fp32 result: K accumulations + bias + floor + residual, each < 2 U S."""
    return 2.0 * (K + 3) * U * S


# ------------------------------------------------------------------------------------------------------------ generators
# Every operand is random in sign and magnitude with the magnitude kept away from zero, so that a single missing or doubled
# product, a neighbouring channel's bias or a neighbouring row's residual moves an element by far more than `bound` (checked
# at K = 32, 256 and 512 by tests/test_decoder_layer_cpu.py).  Nothing is symmetric: rows, columns, sources and the mask are
# independent draws, so no transposition or swap of operands gives the same result.
def _signed(shape, lo, hi, g):
    mag = lo + (hi - lo) * torch.rand(shape, generator=g)
    return torch.where(torch.rand(shape, generator=g) < 0.5, -mag, mag)


def subnormal_bits(dtype):
    """(lowest, highest) bit pattern of the positive subnormals of the 16-bit type."""
    return (1, 0x007F) if dtype == torch.bfloat16 else (1, 0x03FF)


def gen_mask_src(p, n, dtype, g):
    """[P, N] of the 16-bit type over the alphabet +0, -0, a negative, a positive subnormal, a positive normal value:
    15 % / 15 % / 20 % / 20 % / 30 %, so half of it is masked (mask_src > 0 is false)."""
    kind = torch.rand(p, n, generator=g)
    lo, hi = subnormal_bits(dtype)
    sub = torch.randint(lo, hi + 1, (p, n), generator=g).to(torch.int16).view(dtype)
    m = (0.25 + 3.0 * torch.rand(p, n, generator=g)).to(dtype)               # positive normal
    m = torch.where(kind < 0.70, sub, m)                                      # positive subnormal
    m = torch.where(kind < 0.50, -(0.25 + 3.0 * torch.rand(p, n, generator=g)).to(dtype), m)  # negative
    m = torch.where(kind < 0.30, torch.full((), -0.0).to(dtype), m)           # -0
    m = torch.where(kind < 0.15, torch.zeros(()).to(dtype), m)                # +0
    return m


def gen_operands(n, k, p, dtype, seed, scale_a=1.0, scale_w=1.0):
    """The operands of one test case, on the CPU: a1, a2 [P, K], w [N, K], mask_src, residual [P, N] in `dtype`, bias [N] fp32.
    |a1| in [0.5, 1.5], |a2| in [1/32, 1/4] (so |a1 + a2| >= 1/4), |w| in [0.5, 1.5], |bias| in [1, 9], |residual| in [1, 16],
    all with random signs.  scale_a / scale_w (powers of two) move the products without changing a significand."""
    g = torch.Generator().manual_seed(seed)
    a1 = (_signed((p, k), 0.5, 1.5, g) * scale_a).to(dtype)
    a2 = (_signed((p, k), 1.0 / 32, 0.25, g) * scale_a).to(dtype)
    w = (_signed((n, k), 0.5, 1.5, g) * scale_w).to(dtype)
    bias = _signed((n,), 1.0, 9.0, g) * (scale_a * scale_w)
    residual = (_signed((p, n), 1.0, 16.0, g) * (scale_a * scale_w)).clamp(-6e4, 6e4).to(dtype)  # (half: no operand beyond 6e4)
    return {"a1": a1, "a2": a2, "w": w, "bias": bias, "residual": residual, "mask_src": gen_mask_src(p, n, dtype, g)}


def case_seed(n, k, p, dtype):
    """One seed per (shape, pixel count, type): the CPU sensitivity test and the GPU test generate the same operands."""
    return ((n * 1009 + k) * 1013 + p) * 2 + (dtype == torch.float16)
