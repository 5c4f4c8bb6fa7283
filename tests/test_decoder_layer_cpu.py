"""The yardstick of tests/test_decoder_layer_gpu.py, checked without a GPU: tests/decoder_layer_ref.py agrees with torch's
float64 conv2d + relu as models/networks.py composes them, its generated operands make `bound` a sensitive bound (a single
wrong product, bias or residual row moves >= 99 % of the elements it touches past it), and the generated mask source holds the
whole alphabet the kernel's `> 0` has to decide."""
import pytest
import torch
import torch.nn.functional as F

import decoder_layer_ref as R

DTYPES = [torch.bfloat16, torch.float16]


@pytest.mark.parametrize("dtype", DTYPES)
def test_layer_ref_equals_float64_conv2d_and_relu(dtype):
    """x3 = relu(conv(x1 + x2)) (CNN_decoder.forward), plus a residual and a mask, on operands that the 16-bit type and the sum
    of the two sources hold exactly (small integers and halves): the restatement and conv2d then compute the same real numbers."""
    g = torch.Generator().manual_seed(4)
    h, w_, k, n = 3, 5, 32, 8
    p = h * w_
    a1 = (torch.randint(-8, 9, (p, k), generator=g) / 2.0).to(dtype)
    a2 = (torch.randint(-8, 9, (p, k), generator=g) / 2.0).to(dtype)
    wt = (torch.randint(-6, 7, (n, k), generator=g) / 4.0).to(dtype)
    bias = torch.randint(-5, 6, (n,), generator=g) / 8.0
    res = (torch.randint(-9, 10, (p, n), generator=g) / 2.0).to(dtype)
    mask_src = R.gen_mask_src(p, n, dtype, g)
    assert torch.equal((a1.float() + a2.float()).to(dtype).float(), a1.float() + a2.float())  # the single rounding is exact here

    def image(t):  # [P, C] pixel-major -> [1, C, H, W]
        return t.double().t().reshape(1, -1, h, w_)

    conv = F.conv2d(image(a1) + image(a2), wt.double()[:, :, None, None], bias.double())
    want_pre = (F.relu(conv) + image(res))[0].reshape(n, p).t()
    want_post = want_pre * (mask_src.float() > 0)
    pre, post, S = R.layer_ref(a1, a2, wt, bias, True, mask_src, res, dtype)
    torch.testing.assert_close(pre, want_pre, rtol=1e-14, atol=0.0)
    torch.testing.assert_close(post, want_post, rtol=1e-14, atol=0.0)
    assert torch.equal(post == 0, ~(mask_src.float() > 0) | (pre == 0))
    want_S = (a1.double() + a2.double()).abs() @ wt.double().abs().t() + bias.double().abs() + res.double().abs()
    torch.testing.assert_close(S, want_S, rtol=1e-14, atol=0.0)
    # one source, no relu, no bias, nothing in the epilogue: the bare product
    pre1, post1, S1 = R.layer_ref(a1, None, wt, None, False, None, None, dtype)
    bare = F.conv2d(image(a1), wt.double()[:, :, None, None])[0].reshape(n, p).t()
    torch.testing.assert_close(pre1, bare, rtol=1e-14, atol=0.0)
    assert post1 is pre1 and float(pre1.min()) < 0
    assert R.bound(torch.tensor(2.0), 29) == 2.0 * 32 * 2.0 ** -24 * 2.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,k,two", [(264, 32, False), (256, 256, True), (512, 256, False), (256, 512, False)])
def test_generated_operands_make_the_bound_sensitive(n, k, two, dtype):
    """The GPU test's own operands (same generator, same seed) at K = 32, 256 and 512: one k-term removed, one k-term counted
    twice, the bias of channel n + 1, the residual of row p + 1 -- each perturbation of the float64 reference must leave at
    least 99 % of the elements it touches further than `bound` from the unperturbed one.  (Without this a kernel with exactly
    these defects could sit inside the bound.)"""
    p = 129
    ops = R.gen_operands(n, k, p, dtype, R.case_seed(n, k, p, dtype))
    a2 = ops["a2"] if two else None
    pre, _, S = R.layer_ref(ops["a1"], a2, ops["w"], ops["bias"], False, None, ops["residual"], dtype)
    B = R.bound(S, k)
    a, w = R.layer_input(ops["a1"], a2, dtype).double(), ops["w"].double()
    shares = {}
    for k0 in (0, k // 3, k - 1):
        term = a[:, k0:k0 + 1] * w[:, k0][None, :]
        shares[f"k-term {k0} removed"] = ((pre - term) - pre).abs() > B
        shares[f"k-term {k0} twice"] = ((pre + term) - pre).abs() > B
    b = ops["bias"].double()
    shares["bias of channel n + 1"] = (b.roll(-1) - b).abs()[None, :].expand_as(pre) > B
    r = ops["residual"].double()
    shares["residual of row p + 1"] = (r.roll(-1, 0) - r).abs() > B
    for what, over in shares.items():
        share = over.double().mean().item()
        print(f"{dtype} N={n} K={k}: {what}: {share:.4f} of the elements beyond the bound")
        assert share >= 0.99, (what, share)


@pytest.mark.parametrize("dtype", DTYPES)
def test_generated_mask_source_holds_the_whole_alphabet(dtype):
    """+0, -0, negative, positive subnormal and positive normal values of the 16-bit type, 30 % .. 70 % of them masked."""
    g = torch.Generator().manual_seed(8)
    m = R.gen_mask_src(129, 264, dtype, g)
    assert m.dtype == dtype
    bits = m.view(torch.int16).int() & 0xFFFF
    lo, hi = R.subnormal_bits(dtype)
    kinds = {"+0": bits == 0, "-0": bits == 0x8000, "negative": (bits > 0x8000) & torch.isfinite(m),
             "positive subnormal": (bits >= lo) & (bits <= hi), "positive normal": (bits > hi) & (bits < 0x8000) & torch.isfinite(m)}
    total = 0
    for name, sel in kinds.items():
        assert int(sel.sum()) > 0.05 * m.numel(), name
        total += int(sel.sum())
    assert total == m.numel()
    tiny = torch.finfo(dtype).tiny
    assert float(m[kinds["positive subnormal"]].float().max()) < tiny and float(m[kinds["positive subnormal"]].float().min()) > 0
    on = (m.float() > 0)
    assert torch.equal(on, kinds["positive subnormal"] | kinds["positive normal"])
    assert 0.3 <= 1.0 - on.double().mean().item() <= 0.7
    # the same holds for the mask of a generated case, and the case's half operands stay inside the type's range
    ops = R.gen_operands(24, 96, 129, dtype, R.case_seed(24, 96, 129, dtype))
    assert 0.3 <= 1.0 - (ops["mask_src"].float() > 0).double().mean().item() <= 0.7
    assert all(float(ops[name].float().abs().max()) <= 6e4 for name in ("a1", "a2", "w", "residual", "mask_src"))
