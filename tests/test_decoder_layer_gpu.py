"""The root of trust of the 16-bit decoder tiers, alone: gags_decoder_layer / _h16 (csrc/decoder_gemm.hip) against the float64
restatement of tests/decoder_layer_ref.py, element by element, at every shape the two decoders send through it and at the edges
of its tile code; and the kernels that feed it (csrc/decoder_pack.hip) bit for bit against torch.

The fused chains are tested for bit-identity with the layer-by-layer chain (tests/test_decoders_gpu.py) and the query head against
the fused forward (tests/test_decoder_query_gpu.py): this file is what those rest on.  The bound is derived
(decoder_layer_ref.bound) and tests/test_decoder_layer_cpu.py shows that a missing or doubled product, a neighbour's bias or a
neighbour's residual row lies outside it.  Every case prints its worst err / bound (docs/LAB_NOTES.md records them).

The layer entry is called directly, with the same arguments decoders._layer passes: _layer allocates its own outputs and returns
one of them, while these tests want every output inside a guarded buffer and all three from one call."""
import pytest
import torch

import decoder_layer_ref as R

pytestmark = pytest.mark.gpu

TIERS = [pytest.param("", torch.bfloat16, id="bf16"), pytest.param("_h16", torch.float16, id="f16")]
GUARD = 256           # sentinel elements after (and, below one pixel tile, before) every output
SENT16 = 0x7FDB       # a NaN of either 16-bit type: an element the kernel should have written and did not fails every comparison
SENT32 = 0x7FDB5A5A   # ... and of fp32

# (N, K) = (n_out, k_in): every shape CNN_decoder and CNN_scale_decoder send through the kernel, forward and backward
PRODUCTION = [(256, 32), (256, 256), (512, 256), (256, 512), (32, 256), (64, 32), (128, 64), (64, 128), (32, 64), (32, 32)]
# ... and the edges of what the entry accepts (k_in % 32 == 0, n_out % 8 == 0): one 8-channel group; three K-halves; NJ = 4 with
# most of the tile dead; two column tiles, the second with 8 live channels; three column tiles and a K that ends mid-step
EDGE = [(8, 32), (24, 96), (136, 96), (264, 32), (520, 160)]
PIXELS = [1, 127, 128, 129, 1029]  # below, around and above one 128-pixel tile; 9 tiles: with N > 256 the decode's early return runs


def _cases():
    out = []
    for i, (n, k) in enumerate(PRODUCTION):
        ps = PIXELS if (n, k) == (512, 256) else [129, [1, 127, 128, 1029][i % 4]]
        out += [(n, k, p) for p in ps]
    out += [(n, k, p) for n, k in EDGE for p in PIXELS]
    return out


# the operand sets the chains use, and their union
SETS = {
    "forward hidden": dict(bias=True, relu=True, outs=("y",)),
    "forward, two sources": dict(two=True, bias=True, relu=True, outs=("y",)),
    "logits": dict(bias=True, outs=("yf",)),
    "backward": dict(mask=True, outs=("y",)),
    "backward, residual and premask": dict(mask=True, res=True, outs=("y", "ypre")),
    "backward, first layer": dict(outs=("y",)),
    "everything": dict(two=True, bias=True, relu=True, mask=True, res=True, outs=("y", "ypre", "yf")),
}


def _tier(sfx):
    from gags_amd import decoders as D
    return D._F16 if sfx else D._BF16


def _guarded(p, n, dtype):
    """(buffer, [P, N] view, first element of the view): the view sits between sentinels."""
    head = GUARD if p < 128 else 0
    buf = torch.empty(head + p * n + GUARD, dtype=dtype, device="cuda")
    if dtype == torch.float32:
        buf.view(torch.int32).fill_(SENT32)
    else:
        buf.view(torch.int16).fill_(SENT16)
    return buf, buf[head:head + p * n].view(p, n), head


def _guards_intact(buf, head, live):
    raw = buf.view(torch.int32 if buf.dtype == torch.float32 else torch.int16)
    sent = SENT32 if buf.dtype == torch.float32 else SENT16
    return bool((raw[:head] == sent).all()) and bool((raw[head + live:] == sent).all()) and raw.numel() == head + live + GUARD


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _round16(yf, dtype):
    """fp32 -> the 16-bit type as h16_pack does it: round to nearest even; half saturates at +-65504 (csrc/half16.h) where
    torch's cast would give inf."""
    return (yf.clamp(-R.F16_MAX, R.F16_MAX) if dtype == torch.float16 else yf).to(dtype)


def _call(tier, ops, p, n, k, two=False, bias=False, relu=False, mask=False, res=False, outs=("y",)):
    """One gags_decoder_layer launch.  Absent operands and outputs are NULL; every output is a guarded view.  Returns
    {name: [P, N] tensor}; the guards are checked here."""
    from gags_amd.decoders import _st, check, ptr
    dt = tier.dtype
    got = {name: _guarded(p, n, torch.float32 if name == "yf" else dt) for name in outs}
    view = {name: v[1] for name, v in got.items()}
    check(tier.fn("gags_decoder_layer")(p, n, k, ptr(ops["a1"]), ptr(ops["a2"] if two else None), ptr(ops["w"]),
                                        ptr(ops["bias"] if bias else None), int(relu), ptr(ops["mask_src"] if mask else None),
                                        ptr(ops["residual"] if res else None), ptr(view.get("y")), ptr(view.get("ypre")),
                                        ptr(view.get("yf")), _st()), "gags_decoder_layer")
    torch.cuda.synchronize()
    for name, (buf, _, head) in got.items():
        assert _guards_intact(buf, head, p * n), f"{name}: the kernel wrote outside its [P, N] output"
    return view


def _reference(ops, dtype, two=False, bias=False, relu=False, mask=False, res=False, outs=None):
    return R.layer_ref(ops["a1"], ops["a2"] if two else None, ops["w"], ops["bias"] if bias else None, relu,
                       ops["mask_src"] if mask else None, ops["residual"] if res else None, dtype)


def _check_set(tier, ops, p, n, k, name, opt):
    """Every assertion of one operand set; returns the worst err / bound of its fp32 output."""
    dt = tier.dtype
    outs = opt["outs"]
    first = _call(tier, ops, p, n, k, **opt)
    again = _call(tier, ops, p, n, k, **opt)
    for o in outs:
        assert torch.equal(_bits(first[o]), _bits(again[o])), (name, o, "two calls differ")
    # the fp32 result of the same arithmetic: the call itself when it asks for y and y_f32, else a second call that asks for
    # them in addition, whose other outputs must be the first call's bit for bit
    full = first
    if not {"y", "yf"} <= set(outs):
        full = _call(tier, ops, p, n, k, **dict(opt, outs=tuple(sorted(set(outs) | {"y", "yf"}))))
        for o in outs:
            assert torch.equal(_bits(first[o]), _bits(full[o])), (name, o, "changes when more outputs are requested")
    pre, post, S = _reference(ops, dt, **opt)
    B = R.bound(S, k)
    err = (full["yf"].double() - post).abs()
    assert bool((err <= B).all()), (name, "fp32 output", float((err / B).max()), int((~(err <= B)).sum()))
    ratio = float((err / B).max())
    if opt.get("mask"):
        off = ~(ops["mask_src"].float() > 0)
        assert 0.3 * off.numel() <= int(off.sum()) <= 0.7 * off.numel() or off.numel() < 64
        assert bool((full["yf"].view(torch.int32)[off] == 0).all()), (name, "a masked element is not +0")
    assert torch.equal(_bits(full["y"]), _bits(_round16(full["yf"], dt))), (name, "y is not y_f32 rounded once")
    if "ypre" in outs:
        bare = _call(tier, ops, p, n, k, **dict(opt, mask=False, outs=("yf",)))
        e2 = (bare["yf"].double() - pre).abs()
        assert bool((e2 <= B).all()), (name, "fp32 output without the mask", float((e2 / B).max()))
        ratio = max(ratio, float((e2 / B).max()))
        assert torch.equal(_bits(first["ypre"]), _bits(_round16(bare["yf"], dt))), (name, "y_premask is not the unmasked value rounded once")
    return ratio


@pytest.mark.parametrize("sfx,dtype", TIERS)
@pytest.mark.parametrize("n,k,p", _cases())
def test_layer_kernel_against_float64_per_element(n, k, p, sfx, dtype):
    """Every operand set on one (N, K, P): |y_f32 - float64| <= bound(S, K) at EVERY element, masked elements +0 exactly, the
    16-bit outputs the fp32 ones rounded once, the premask output the unmasked call's, sentinels around every output intact,
    two calls bit-identical."""
    tier = _tier(sfx)
    ops = {name: t.cuda() for name, t in R.gen_operands(n, k, p, dtype, R.case_seed(n, k, p, dtype)).items()}
    worst = {name: _check_set(tier, ops, p, n, k, name, opt) for name, opt in SETS.items()}
    print(f"err/bound {tier.name} N={n} K={k} P={p}: worst {max(worst.values()):.4f} "
          + " ".join(f"[{name}: {v:.4f}]" for name, v in worst.items()))


def test_half_outputs_saturate_at_the_largest_finite_value():
    """f16 only: operands scaled by 2^7 each so that the sums pass 65504 on both sides.  The fp32 output still meets the bound
    (powers of two change no significand); the half outputs are exactly +-65504 there (h16_pack's clamp; torch's cast would
    give inf) and finite everywhere."""
    tier = _tier("_h16")
    n, k, p = 24, 96, 129
    ops = {name: t.cuda() for name, t in R.gen_operands(n, k, p, torch.float16, 77, scale_a=128.0, scale_w=128.0).items()}
    assert all(float(ops[name].float().abs().max()) <= 6e4 for name in ("a1", "a2", "w", "residual"))
    opt = dict(two=True, bias=True, relu=False, mask=True, res=True, outs=("y", "ypre", "yf"))
    ratio = _check_set(tier, ops, p, n, k, "saturation", opt)
    out = _call(tier, ops, p, n, k, **opt)
    bare = _call(tier, ops, p, n, k, **dict(opt, mask=False, outs=("yf",)))["yf"]
    for y16, yf in ((out["y"], out["yf"]), (out["ypre"], bare)):
        hi, lo = yf >= 65520.0, yf <= -65520.0  # (what rounds to nearest as beyond the largest finite half)
        assert int(hi.sum()) > 10 and int(lo.sum()) > 10 and int((yf.abs() < 6e4).sum()) > 10
        assert bool((y16[hi] == R.F16_MAX).all()) and bool((y16[lo] == -R.F16_MAX).all())
        assert bool(torch.isfinite(y16).all())
    print(f"err/bound f16 saturation N={n} K={k} P={p}: worst {ratio:.4f}")


@pytest.mark.parametrize("sfx,dtype", TIERS)
def test_layer_wrapper_passes_its_operands_through(sfx, dtype):
    """decoders._layer (what the chains call) gives the bits of the direct call, for the 16-bit output, the fp32 one and the
    premask pair."""
    from gags_amd import decoders as D
    tier = _tier(sfx)
    n, k, p = 264, 32, 129
    ops = {name: t.cuda() for name, t in R.gen_operands(n, k, p, dtype, R.case_seed(n, k, p, dtype)).items()}
    y = D._layer(p, ops["w"], ops["bias"], ops["a1"], ops["a2"], tier=tier)
    assert torch.equal(_bits(y), _bits(_call(tier, ops, p, n, k, two=True, bias=True, relu=True)["y"]))
    yf = D._layer(p, ops["w"], ops["bias"], ops["a1"], relu=False, f32=True, tier=tier)
    assert torch.equal(_bits(yf), _bits(_call(tier, ops, p, n, k, bias=True, outs=("yf",))["yf"]))
    y, ypre = D._layer(p, ops["w"], None, ops["a1"], relu=False, mask_src=ops["mask_src"], residual=ops["residual"], premask=True,
                       tier=tier)
    want = _call(tier, ops, p, n, k, mask=True, res=True, outs=("y", "ypre"))
    assert torch.equal(_bits(y), _bits(want["y"])) and torch.equal(_bits(ypre), _bits(want["ypre"]))


# ------------------------------------------------------------------------------------------------------ the pack kernels
def _specials(dtype):
    """-0; values exactly halfway between two neighbours of the 16-bit type (round-to-even decides: down to 1, up to 1 + 2 ulp);
    subnormals of the type, one of them halfway; and for half, finite values above 65504, where the contract is +-65504
    (h16_from, csrc/half16.h) and torch's cast gives inf: the expected values clamp first."""
    if dtype == torch.bfloat16:
        return [-0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 2.0 ** -130, 3.5 * 2.0 ** -133, -5 * 2.0 ** -133]
    return [-0.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 2.0 ** -20, 2.5 * 2.0 ** -24, -5 * 2.0 ** -24,
            70000.0, -1.0e6, 65520.0, 65519.0]


def _to16(src, dtype):
    """The contract of h16_from on the CPU (torch's CPU cast rounds to nearest even, subnormals included)."""
    s = src.detach().cpu().float()
    return (s.clamp(-R.F16_MAX, R.F16_MAX) if dtype == torch.float16 else s).to(dtype)


def _source(shape, dtype, g, scale=0.3):
    t = torch.randn(shape, generator=g) * scale
    sp = torch.tensor(_specials(dtype), dtype=torch.float32)
    m = min(sp.numel(), t.numel())
    t.view(-1)[:m] = sp[:m]
    return t


def _check_packed(wb, params, dtype):
    for (w, b), (wt, bs) in zip(wb, params):
        co, ci = wt.shape[:2]
        n, k = (co + 31) // 32 * 32, (ci + 31) // 32 * 32
        what = f"layer ({co}, {ci})"
        assert w.shape == (n, k) and w.dtype == dtype and b.shape == (n,) and b.dtype == torch.float32, what
        ref = torch.zeros(n, k, dtype=dtype)
        ref[:co, :ci] = _to16(wt.reshape(co, ci), dtype)
        rt = ref.t().contiguous()
        assert torch.equal(_bits(w.cpu()), _bits(ref)), what + ": padded weight"
        assert torch.equal(_bits(w._gags_t.cpu()), _bits(rt)), what + ": transpose"
        # the pure-torch formula of decoders._frag_layout's fallback branch
        assert torch.equal(_bits(w._gags_frag.cpu()), _bits(ref.view(n // 32, 32, k // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous())), \
            what + ": fragment order"
        assert torch.equal(_bits(w._gags_t._gags_frag.cpu()),
                           _bits(rt.view(k // 32, 32, n // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous())), what + ": fragment order of the transpose"
        bref = torch.zeros(n)
        bref[:co] = bs.detach().cpu()
        assert torch.equal(_bits(b.cpu()), _bits(bref)), what + ": bias"
        if dtype == torch.float16:
            assert bool(torch.isfinite(w).all())


def _params(shapes, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for co, ci in shapes:
        bias = _source((co,), torch.bfloat16, g, scale=1.0)  # (fp32 in, fp32 out: -0 and fp32 subnormals must survive as they are)
        out.append((torch.nn.Parameter(_source((co, ci, 1, 1), dtype, g).cuda()), torch.nn.Parameter(bias.cuda())))
    return out


PACK7 = [(256, 16), (256, 3), (3, 16), (512, 256), (16, 32), (1, 1), (33, 17)]
# thirteen layers: the second launch of the twelve-per-launch loop; the largest (160 x 96 padded) is neither first nor last
PACK13 = [(16, 32), (33, 17), (64, 16), (1, 1), (256, 16), (3, 16), (130, 70), (8, 40), (32, 32), (65, 33), (5, 3), (128, 64), (17, 100)]


@pytest.mark.parametrize("sfx,dtype", TIERS)
@pytest.mark.parametrize("shapes", [PACK7, PACK13], ids=["7 layers", "13 layers"])
def test_pack_layers_writes_every_form_of_every_weight_exactly(shapes, sfx, dtype):
    """gags_decoder_pack_layers through _pack_weights: the padded 16-bit weight, its transpose, both in MFMA-fragment order and
    the padded fp32 bias, bit for bit against torch on the CPU (half: after the clamp to +-65504 the contract states)."""
    from gags_amd import decoders as D
    params = _params(shapes, dtype, 5 + len(shapes))
    wb = D._pack_weights([w for w, _ in params], [b for _, b in params], _tier(sfx))
    torch.cuda.synchronize()
    assert len(wb) == len(shapes)
    _check_packed(wb, params, dtype)


@pytest.mark.parametrize("sfx,dtype", TIERS)
def test_pack_layer_gives_the_bytes_of_the_batched_entry(sfx, dtype):
    """gags_decoder_pack_layer, the single-layer entry, on (33, 17)."""
    from gags_amd import decoders as D
    from gags_amd.decoders import _st, check, ptr
    tier = _tier(sfx)
    params = _params(PACK7, dtype, 12)
    wb = D._pack_weights([w for w, _ in params], [b for _, b in params], tier)
    (w, b), (wt, bs) = wb[-1], params[-1]
    co, ci = 33, 17
    assert tuple(wt.shape[:2]) == (co, ci)
    one = [torch.empty_like(t) for t in (w, w._gags_t, w._gags_frag, w._gags_t._gags_frag, b)]
    src = wt.detach().reshape(co, ci).contiguous()
    check(tier.fn("gags_decoder_pack_layer")(co, ci, ptr(src), ptr(bs.detach()), *[ptr(t) for t in one], _st()), "gags_decoder_pack_layer")
    torch.cuda.synchronize()
    for got, want in zip(one, (w, w._gags_t, w._gags_frag, w._gags_t._gags_frag, b)):
        assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("sfx,dtype", TIERS)
@pytest.mark.parametrize("c", [1, 3, 16, 32])
def test_pack_input_rounds_and_pads_exactly(c, sfx, dtype):
    """gags_decoder_pack_input: the first c columns are the fp32 rows rounded to nearest even (half: saturated), the padding is
    +0, nothing is written past the last row."""
    from gags_amd.decoders import _st, check, ptr
    tier = _tier(sfx)
    g = torch.Generator().manual_seed(40 + c)
    for c_pad in (32, 64):
        for p in (1, 257):
            x = _source((p, c), dtype, g, scale=3.0)
            xd = x.cuda()
            buf, y, head = _guarded(p, c_pad, dtype)
            check(tier.fn("gags_decoder_pack_input")(p, c, c_pad, ptr(xd), ptr(y), _st()), "gags_decoder_pack_input")
            torch.cuda.synchronize()
            assert _guards_intact(buf, head, p * c_pad), (c_pad, p)
            assert torch.equal(_bits(y[:, :c].cpu()), _bits(_to16(x, dtype))), (c_pad, p)
            assert bool((_bits(y[:, c:]) == 0).all()), (c_pad, p)


@pytest.mark.parametrize("sfx,dtype", TIERS)
@pytest.mark.parametrize("c,ld", [(3, 32), (16, 32), (32, 32), (5, 8)])
def test_unpack_grad_widens_exactly(c, ld, sfx, dtype):
    """gags_decoder_unpack_grad: the first c of ld columns as a dense [P, c] fp32, every finite bit pattern of the 16-bit type
    among the inputs (zeros of both signs and subnormals included), nothing written past the last row."""
    from gags_amd.decoders import _st, check, ptr
    tier = _tier(sfx)
    g = torch.Generator().manual_seed(60 + c + ld)
    expo = 0x7F80 if dtype == torch.bfloat16 else 0x7C00
    for p in (1, 257):
        raw = torch.randint(0, 65536, (p, ld), generator=g)
        raw = torch.where((raw & expo) == expo, raw & ~0x4000, raw)  # (no inf / NaN: clear one exponent bit)
        raw[0, :3] = torch.tensor([0x8000, 0x0001, 0x8001])          # -0 and the smallest subnormals
        x = (raw - ((raw >= 32768) * 65536)).to(torch.int16).view(dtype)
        xd = x.cuda()
        buf, y, head = _guarded(p, c, torch.float32)
        check(tier.fn("gags_decoder_unpack_grad")(p, c, ld, ptr(xd), ptr(y), _st()), "gags_decoder_unpack_grad")
        torch.cuda.synchronize()
        assert _guards_intact(buf, head, p * c), p
        assert torch.equal(_bits(y.cpu()), _bits(x[:, :c].float().contiguous())), p
