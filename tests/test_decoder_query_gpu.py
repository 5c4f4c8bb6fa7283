"""N15 on the GPU: CNN_decoder.query -- decoder + relevancy head in one kernel (csrc/decoder_query.hip) -- against the float64
head applied to the fp32 logits gags_decoder_fwd_fused writes for the same inputs and tier.  That truth isolates the new code:
the hidden layers are the training forward's (csrc/decoder_tile.h), so any deviation there shows up as error in the head.
That forward is itself checked at these c_in and widths: bit for bit against the layer-by-layer chain
(tests/test_decoders_gpu.py), whose layer kernel is held to float64 per element (tests/test_decoder_layer_gpu.py).

The bound.  Measured on an MI355X against that truth over the cases below (docs/LAB_NOTES.md "Query head (N15)"): the existing
composition decoder(x) -> get_max_across is within COMPOSITION_ERR = 6.3e-7 of it (worst case, both tiers: 6.286e-7 at
P = 60000), the fused kernel within 9.1e-7.  BOUND = 4 x COMPOSITION_ERR = 2.5e-6: two fp32 sums of the same length in
different orders.  It stays below
CEILING = 1.6e-4, what a direct fp32 head can be shown to keep: for unit phrases |d sim| <= gamma_516 ~ 3.1e-5 and
|d p| <= 10 * 1/4 * 2 |d sim|."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

COMPOSITION_ERR = 6.3e-7
CEILING = 1.6e-4
BOUND = min(4 * COMPOSITION_ERR, CEILING)
TIERS = ("bf16", "f16")
# (c_in, output_dim, (H, W), (n_pos, n_neg)): P = 1, 63, 64, 65, 209 and 60000 -- below, at and above one tile, several and many
# workgroups -- with every c_in, width and phrase count of the issue in at least one case of each kind
CASES = [(16, 512, (1, 1), (1, 4)), (16, 512, (7, 9), (5, 4)), (16, 512, (8, 8), (1, 1)), (16, 512, (5, 13), (28, 4)),
         (3, 512, (11, 19), (5, 4)), (16, 256, (11, 19), (1, 4)), (3, 256, (5, 13), (5, 4)), (16, 256, (7, 9), (28, 4)),
         (3, 512, (8, 8), (1, 1)), (3, 256, (1, 1), (1, 1)), (16, 512, (200, 300), (5, 4)), (3, 256, (200, 300), (28, 4))]


def _decoder(tier, c_in, out_dim, seed=0):
    from gags_amd.decoders import CNN_decoder
    torch.manual_seed(seed)  # nn.Conv2d's default initialisation, seeded
    return CNN_decoder(c_in, out_dim, tier).cuda()


@functools.lru_cache(maxsize=None)
def _shared_decoder(tier, c_in, out_dim):
    return _decoder(tier, c_in, out_dim)


def _input(c_in, h, w, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(h, w, c_in, generator=g).cuda().permute(2, 0, 1)  # the rasterizer's layout: pixel-major memory


def _logits(dec, x):
    """The fp32 logits [P, n_last] of the EXISTING fused forward (nothing kept: acts and masks NULL)."""
    from gags_amd import decoders as D
    tier = D._tier(dec.precision)
    wb = tier.weights([t for m in dec.convs() for t in (m.weight, m.bias)])
    xp, h, w = D._pixel_major(x)
    assert D._fusable(wb, xp.shape[1])
    out = torch.empty(h * w, wb[-1][0].shape[0], device="cuda")
    arr = ctypes.c_void_p * 9
    D.check(tier.fn("gags_decoder_fwd_fused")(h * w, xp.shape[1], out.shape[1], D.ptr(xp),
                                              arr(*[D._frag_layout(wgt).data_ptr() for wgt, _ in wb]),
                                              arr(*[b.data_ptr() for _, b in wb]), None, None, D.ptr(out), D._st()), "fwd")
    return out


def _truth(logits, pos, neg):
    """The float64 head: normalise with the 1e-12 clamp, the dots, softmax(10 (pos, neg_k)), the first minimum over k.  [n_pos, P, 2]"""
    z = logits.double()
    n = z.norm(dim=1, keepdim=True).clamp_min(1e-12)
    sp, sn = (z @ pos.double().t()) / n, (z @ neg.double().t()) / n  # [P, n_pos], [P, n_neg]
    pair = torch.softmax(10.0 * torch.stack([sp.t()[:, :, None].expand(-1, -1, sn.shape[1]),
                                             sn[None].expand(sp.shape[1], -1, -1)], dim=-1), dim=-1)  # [n_pos, P, n_neg, 2]
    k = pair[..., 0].argmin(dim=2)  # (torch returns the first minimum)
    return torch.gather(pair, 2, k[:, :, None, None].expand(-1, -1, 1, 2))[:, :, 0]


def _phrases(logits, n_pos, n_neg, seed=2):
    """Unit rows: positives at pixels 0 and P // 2, negatives at two other pixels, the rest random unit vectors (random
    vectors alone keep every probability near 0.5)."""
    from gags_amd.relevancy import RelevancyHead
    p, c = logits.shape
    g = torch.Generator().manual_seed(seed)
    unit = torch.nn.functional.normalize
    pos = unit(torch.randn(n_pos, c, generator=g), dim=1).cuda()
    neg = unit(torch.randn(n_neg, c, generator=g), dim=1).cuda()
    zn = unit(logits.double(), dim=1).float()
    pos[0] = zn[0]
    if n_pos > 1:
        pos[1] = zn[p // 2]
    neg[0] = zn[p // 3]
    if n_neg > 1:
        neg[1] = zn[(2 * p) // 3]
    return RelevancyHead(pos, neg)


def _check_pairs(got, truth, what):
    err = (got.double() - truth).abs().max().item()
    ulp2 = 2 * torch.finfo(torch.float32).eps
    s = (got[..., 0].double() + got[..., 1].double() - 1).abs().max().item()
    print(f"{what}: max |p - float64| = {err:.3e} (bound {BOUND:.1e}), max |p0 + p1 - 1| = {s:.2e}")
    assert torch.isfinite(got).all()
    assert err <= BOUND, (what, err)
    assert s <= ulp2, (what, s)
    return err


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("c_in,out_dim,hw,n_phr", CASES)
def test_query_is_within_four_times_the_compositions_error_of_the_float64_head(tier, c_in, out_dim, hw, n_phr):
    dec = _shared_decoder(tier, c_in, out_dim)
    x = _input(c_in, *hw)
    logits = _logits(dec, x)
    head = _phrases(logits, *n_phr)
    truth = _truth(logits, head.pos_embeds, head.neg_embeds)
    spread = (truth[..., 0].max() - truth[..., 0].min()).item()
    print(f"probabilities span {spread:.3f}")
    assert spread > 0.1 or hw == (1, 1)  # the planted phrases spread the probabilities (random ones alone: all near 0.5)
    pairs = dec.query(x, head, pairs=True)
    assert pairs.shape == (n_phr[0], hw[0] * hw[1], 2) and pairs.dtype == torch.float32
    _check_pairs(pairs, truth, f"fused {tier} c_in={c_in} out={out_dim} hw={hw} phrases={n_phr}")
    maps = dec.query(x, head)
    assert maps.shape == (n_phr[0], *hw) and maps.is_contiguous()
    assert torch.equal(maps.reshape(n_phr[0], -1), pairs[..., 0])
    # the yardstick: the existing composition against the same truth (reported; COMPOSITION_ERR is its worst case)
    if sum(n_phr) * out_dim * 4 <= 60000:  # (gags_relevancy keeps its phrases in LDS: 32 phrases of 512 do not fit there)
        comp = head._all(dec(x).permute(1, 2, 0).reshape(hw[0] * hw[1], -1))
        print(f"    composition: max |p - float64| = {(comp.double() - truth).abs().max().item():.3e}")


@pytest.mark.parametrize("tier", TIERS)
def test_contiguous_input_and_pixel_major_view_give_identical_bits(tier):
    dec = _shared_decoder(tier, 16, 512)
    x = _input(16, 11, 19)
    head = _phrases(_logits(dec, x), 5, 4)
    assert not x.is_contiguous()
    assert torch.equal(dec.query(x, head, pairs=True), dec.query(x.contiguous(), head, pairs=True))


@pytest.mark.parametrize("tier", TIERS)
def test_all_zero_logits_give_exactly_one_half_and_no_nan(tier):
    dec = _decoder(tier, 16, 512)
    with torch.no_grad():
        dec.convs()[-1].weight.zero_()
        dec.convs()[-1].bias.zero_()
    x = _input(16, 5, 13)
    head = _phrases(torch.randn(65, 512).cuda(), 5, 4)
    got = dec.query(x, head, pairs=True)
    assert torch.equal(got, torch.full_like(got, 0.5))  # sim = 0 / max(0, 1e-12) = 0 for every phrase


def test_exact_tier_runs_the_composition_bit_for_bit():
    dec = _decoder("exact", 16, 512)
    x = _input(16, 7, 9)
    head = _phrases(torch.randn(63, 512).cuda(), 5, 4)
    feat = dec(x).permute(1, 2, 0)
    assert torch.equal(dec.query(x, head), head.get_max_across(feat[None])[0])
    assert torch.equal(dec.query(x, head, pairs=True), head._all(feat.reshape(63, 512)))


@pytest.mark.parametrize("tier", TIERS)
def test_results_follow_set_positives_and_in_place_updates(tier):
    """No stale phrase operand and no stale packed weights: after every change the result matches the float64 head on
    logits from a FRESH decoder holding the same parameters (its weights are packed anew)."""
    dec = _decoder(tier, 16, 512)
    x = _input(16, 5, 13)
    head = _phrases(_logits(dec, x), 5, 4)

    def fresh_truth():
        ref = _decoder(tier, 16, 512, seed=7)
        ref.load_state_dict(dec.state_dict())
        return _truth(_logits(ref, x), head.pos_embeds, head.neg_embeds)

    first = dec.query(x, head, pairs=True)
    _check_pairs(first, fresh_truth(), "before")
    head.set_positives(torch.nn.functional.normalize(torch.randn(3, 512), dim=1).cuda())
    got = dec.query(x, head, pairs=True)
    assert got.shape[0] == 3
    _check_pairs(got, fresh_truth(), "after set_positives")
    with torch.no_grad():
        head.neg_embeds.copy_(head.neg_embeds.flip(0) * 1.0)
        head.pos_embeds[0].copy_(head.neg_embeds[2])
    got2 = dec.query(x, head, pairs=True)
    assert not torch.equal(got2, got)
    _check_pairs(got2, fresh_truth(), "after in-place phrase writes")
    with torch.no_grad():
        dec.convs()[3].weight.mul_(-1.5)
    got3 = dec.query(x, head, pairs=True)
    assert not torch.equal(got3, got2)
    _check_pairs(got3, fresh_truth(), "after weight.mul_")


def test_fused_query_allocates_less_than_one_fp32_map_where_the_composition_needs_more_than_two():
    dec = _shared_decoder("bf16", 16, 512)
    x = _input(16, 200, 300)
    head = _phrases(torch.randn(60000, 512).cuda(), 5, 4)
    one_map = 60000 * 512 * 4

    def rise(fn):
        fn()  # (weights packed, phrase operand cached)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        del out
        return torch.cuda.max_memory_allocated() - base

    fused = rise(lambda: dec.query(x, head))
    with torch.no_grad():
        comp = rise(lambda: head.get_max_across(dec(x).permute(1, 2, 0)[None])[0])
    print(f"peak allocation rise at P = 60000: fused {fused / 1e6:.1f} MB, composition {comp / 1e6:.1f} MB, one [P,512] fp32 map {one_map / 1e6:.1f} MB")
    assert fused < one_map
    assert comp > 2 * one_map


@pytest.mark.parametrize("n", [1000, 70001])
def test_point_relevancy_fused_matches_the_chunked_path(n):
    from gags_amd.pointquery import point_relevancy, query_points
    dec = _shared_decoder("bf16", 16, 512)
    g = torch.Generator().manual_seed(n)
    feat = torch.randn(n, 16, generator=g).cuda()
    xyz = torch.rand(n, 3, generator=g).cuda()
    head = _phrases(_logits(dec, feat.t()[..., None]), 5, 4)
    a = point_relevancy(feat, dec, head, chunk=30000)
    b = point_relevancy(feat, dec, head, chunk=30000, fused=True)
    assert a.shape == b.shape == (5, n)
    d = (a.double() - b.double()).abs().max().item()
    print(f"point_relevancy N = {n}: max |fused - chunked| = {d:.3e} (bound {BOUND:.1e})")
    assert d <= BOUND
    qa = query_points(feat, xyz, dec, head, chunk=30000)
    qb = query_points(feat, xyz, dec, head, chunk=30000, fused=True)
    assert (qa["relevancy"].double() - qb["relevancy"].double()).abs().max().item() <= BOUND
    differ = qa["mask_raw"] != qb["mask_raw"]
    near = (qa["normalized"] - 0.4).abs() <= BOUND  # rel_thresh's default
    share = near.float().mean().item()
    print(f"query_points N = {n}: {int(differ.sum())} raw mask bits differ, {int((qa['mask'] != qb['mask']).sum())} after smoothing; "
          f"{100 * share:.4f} % of the points are within the bound of rel_thresh")
    assert not (differ & ~near).any()
    assert share <= 0.01


def test_c_abi_rejects_bad_arguments_and_accepts_an_empty_call():
    from gags_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64, device="cuda")
    P = ctypes.c_void_p(buf.data_ptr())
    nine, st = (ctypes.c_void_p * 9)(*[buf.data_ptr()] * 9), None
    holed = (ctypes.c_void_p * 9)(*([buf.data_ptr()] * 4 + [None] + [buf.data_ptr()] * 4))
    for fn in (lib.gags_decoder_query_fused, lib.gags_decoder_query_fused_h16):
        assert fn(0, 16, 512, None, nine, nine, P, 1, 1, None, st) == 0          # n_pix == 0: nothing to do
        assert fn(-1, 16, 512, P, nine, nine, P, 1, 1, P, st) == -1
        for c_in in (0, 33):
            assert fn(8, c_in, 512, P, nine, nine, P, 1, 1, P, st) == -1
        for n_last in (0, 128, 300, -256):
            assert fn(8, 16, n_last, P, nine, nine, P, 1, 1, P, st) == -1
        for n_pos, n_neg in ((0, 4), (4, 0), (-1, 4), (29, 4), (1, 32)):
            assert fn(8, 16, 512, P, nine, nine, P, n_pos, n_neg, P, st) == -1
        assert fn(8, 16, 512, None, nine, nine, P, 1, 1, P, st) == -1            # x
        assert fn(8, 16, 512, P, None, nine, P, 1, 1, P, st) == -1               # weights
        assert fn(8, 16, 512, P, nine, None, P, 1, 1, P, st) == -1               # biases
        assert fn(8, 16, 512, P, holed, nine, P, 1, 1, P, st) == -1              # one weight
        assert fn(8, 16, 512, P, nine, holed, P, 1, 1, P, st) == -1              # one bias
        assert fn(8, 16, 512, P, nine, nine, None, 1, 1, P, st) == -1            # phrases
        assert fn(8, 16, 512, P, nine, nine, P, 1, 1, None, st) == -1            # probs
    torch.cuda.synchronize()
