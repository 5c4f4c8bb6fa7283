"""The distillation step's loss kernels (csrc/seg_losses.hip, distill_l1.hip, head_distill.hip) against the float64 restatement of tests/loss_ref.py, at the
shapes, channel counts and segment counts where the kernels take different paths.  tests/test_loss_ref_cpu.py ties the
restatement to the reference's own outputs; here it is the yardstick for every kernel at sizes the fixture cannot reach.

Bounds are stated per element in terms of the magnitudes of the summands (U = 2^-24, fp32's unit roundoff): a chain of k
fp32 roundings moves a result by at most about k U times the sum of the magnitudes of what was summed.  Every k below comes
with its count.  Where an L1 sign may legitimately differ from float64 (|diff| under its own fp32 error bound), exactly
those elements are excluded from the per-element check, their largest possible effect is charged to the sums they enter,
and the excluded fraction is asserted to be tiny."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import loss_ref as R

pytestmark = pytest.mark.gpu
U = R.U
DEV = "cuda"

# the ground-truth feature: the bilinear weight (1 - ly)(1 - lx) is 3 roundings, the tap chain (fma) at most 4, the blend by
# the scale map (f0 s0 + f1 s1) + f2 s2 another 3 -> 10 roundings against T = sum_l s_l sum_k w_k |e_lk|
KG = 10
# F.normalize in the fused head: |x|^2 by a chain of 64 fma per lane + 3 shuffle adds (67), the square root halves that
# (33.5) and rounds (1), 1 / n rounds (1), x * (1 / n) rounds (1): |y - x / |x|| <= 37 U |y|, rounded up
KY = 38


def chain_vs(c):
    """v_scale sums c products: every kernel here forms it in chains of at most c / 4 + 10 fp32 additions (channel-major:
    c / 4 per thread + a 2-level tree; pixel-major: 4 per lane + a 6-level wave sum or c / 4 LDS atomics; fused head: 32 +
    1 + 3); each product carries at most 10 roundings (7 in F_l, 2 in v / c, 1 the product)."""
    return c / 4 + 20


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def within(got, ref, bound, what):
    err = (got.detach().double() - ref.double()).abs()
    bad = err > bound
    if bool(bad.any()):
        ratio = float((err / bound.clamp_min(1e-300)).max())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements over the bound (worst err / bound {ratio:.3g})")


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def sam_inputs(c, src, dst, n_emb, seed, dead_level=None):
    """Embeddings (unit rows), a seg map with ids in [-1, n_emb) plus 5 % extra -1 per level (so pixels where exactly one
    level is -1 are common), optionally one level entirely -1, and a softmax scale map."""
    g = gen(seed)
    (h, w), (H, W) = src, dst
    emb = F.normalize(torch.randn(n_emb, c, device=DEV, generator=g), dim=1)
    seg = torch.randint(-1, n_emb, (4, h, w), device=DEV, generator=g).float()
    seg[1:][torch.rand(3, h, w, device=DEV, generator=g) < 0.05] = -1.0
    seg[1:, 0, 0] = 0.0                                           # (a 1 x 1 map then still has a valid pixel)
    if dead_level is not None:
        seg[dead_level] = -1.0
    sc = torch.softmax(2.0 * torch.randn(3, H, W, device=DEV, generator=g), 0)
    return emb, seg, sc, g


def bands(H, W, c, budget=1 << 24):
    rows = max(1, budget // (W * c))
    for r0 in range(0, H, rows):
        yield r0, min(H, r0 + rows)


def sam_ref(emb, seg, sc, r0, r1):
    """(F_l [3, c, R, W], A_l = sum_k w_k |e_lk|, mask [R, W], gt [c, R, W], T = sum_l s_l A_l) for rows r0..r1, float64."""
    H, W = sc.shape[1:]
    Fl, Al, mref = R.sam_levels(emb, seg, H, W, range(r0, r1))
    s = sc[:, r0:r1].double()
    gt = Fl[0] * s[0] + Fl[1] * s[1] + Fl[2] * s[2]
    T = Al[0] * s[0] + Al[1] * s[1] + Al[2] * s[2]
    return Fl, Al, mref, gt, T


# ------------------------------------------------------------------------------------------------ ground truth and L1
GT_CASES = [  # (c, seg map size, render size, n_emb, dead level)
    (16, (1, 1), (1, 1), 1, None),
    (80, (1, 97), (1, 97), 11, None),
    (528, (97, 1), (97, 1), 300, None),
    (512, (37, 53), (37, 53), 1500, None),
    (16, (37, 53), (37, 53), 300, 2),
    (16, (7, 9), (67, 93), 11, None),
    (80, (7, 9), (67, 93), 300, None),
    (528, (7, 9), (67, 93), 1, None),
    (80, (1440, 1080), (730, 541), 11, 3),
    (528, (1440, 1080), (730, 541), 1500, None),
    (512, (540, 960), (1080, 1920), 300, None),
    (512, (1080, 1920), (1080, 1920), 1500, None),
]


@pytest.mark.parametrize("c,src,dst,n_emb,dead", GT_CASES)
def test_ground_truth_and_distillation_l1_against_float64(c, src, dst, n_emb, dead):
    """read_sam_clip_feature (forward, mask, v_scale) and distill_l1_map (forward, mask, v_pred, v_scale) with the prediction
    channel-major (sam_feature_kernel<0..3>) and pixel-major (sam_l1_pm_kernel<2,3>: the wave-sum branch at c % 256 == 0,
    the per-lane LDS atomics otherwise) against the float64 restatement."""
    from gags_amd import losses as L
    H, W = dst
    emb, seg, sc0, g = sam_inputs(c, src, dst, n_emb, seed=c + 7 * H + W + n_emb, dead_level=dead)
    pred0 = F.normalize(torch.randn(c, H, W, device=DEV, generator=g), dim=0)
    G = torch.randn(c, H, W, device=DEV, generator=g)
    V = torch.rand(H, W, device=DEV, generator=g) + 0.5

    sc = sc0.clone().requires_grad_(True)
    feat, fmask = L.read_sam_clip_feature(emb, seg, sc)
    feat.backward(G)
    vs_feat = sc.grad
    outs = {}
    for layout in ("cm", "pm"):
        sc = sc0.clone().requires_grad_(True)
        if layout == "cm":
            p = pred0.clone().requires_grad_(True)
            pv = p
        else:
            p = pred0.permute(1, 2, 0).contiguous().requires_grad_(True)
            pv = p.permute(2, 0, 1)
            assert L._pixel_major(pv) or pv.is_contiguous()  # (1 x 1: the two layouts are the same memory)
        l1, m = L.distill_l1_map(pv, emb, seg, sc)
        l1.backward(V)
        vp = p.grad if layout == "cm" else p.grad.permute(2, 0, 1)
        outs[layout] = (l1.detach(), m, vp, sc.grad)
        del p, pv
    torch.cuda.synchronize()

    pow2 = (c & (c - 1)) == 0
    vc32 = V / c
    ulp = torch.nextafter(vc32, torch.full_like(vc32, math.inf)) - vc32  # one ulp of v / c (fp32)
    n_flip = n_live = 0
    for r0, r1 in bands(H, W, c):
        Fl, Al, mref, gt, T = sam_ref(emb, seg, sc0, r0, r1)
        assert torch.equal(fmask[0, r0:r1], mref), "read_sam_clip_feature mask"
        within(feat[:, r0:r1], gt, KG * U * T, "feature map")
        Gd = G[:, r0:r1].double()
        within(vs_feat[:, r0:r1], (Gd[None] * Fl).sum(1), chain_vs(c) * U * (Gd.abs()[None] * Al).sum(1), "feature v_scale")
        m = mref.double()
        pd = pred0[:, r0:r1].double()
        d = (pd - gt) * m
        # |diff| of the kernel: the ground truth's KG roundings, the subtraction's 1 (the products by m in {0, 1} are exact)
        eb = (KG + 1) * U * (T + pd.abs())
        flip = (m > 0) & (d.abs() <= eb)
        n_flip += int(flip.sum())
        n_live += int(m.sum()) * c
        vc = V[r0:r1].double() / c
        want = torch.sign(d).float() * mref.float() * vc32[r0:r1]
        vs_ref = -((torch.sign(d) * m * vc)[None] * Fl).sum(1)
        # a flipped sign moves v_scale by at most 2 |v| / c |f_l| per flipped channel (|f_l| <= A_l (1 + 7 U))
        vs_b = chain_vs(c) * U * ((m * vc)[None] * Al).sum(1) + 2.0 * (1 + 1e-5) * ((flip * vc)[None] * Al).sum(1)
        for layout, (l1, lm, vp, vs) in outs.items():
            assert torch.equal(lm[0, r0:r1], mref), f"distill_l1_map mask ({layout})"
            # mean over c of |diff|: each |diff| within (KG + 1) U (T + |p|) and the sum a chain of <= c / 4 + 10 additions
            # plus the division: (c / 4 + 22) U sum_c (|p| + T) m / c
            within(l1[r0:r1], d.abs().mean(0), (c / 4 + 22) * U * ((pd.abs() + T) * m).sum(0) / c, f"l1 map ({layout})")
            got = vp[:, r0:r1]
            keep = ~flip
            if pow2:  # v / c is exact: the kernel's sign * m * v * (1 / c) is torch's sign * m * v / c, bit for bit
                assert torch.equal(got[keep], want[keep]), f"v_pred ({layout})"
            else:  # the kernel multiplies by the rounded 1 / c: one ulp of v / c
                err = (got - want).abs()
                assert bool((err[keep] <= ulp[r0:r1].expand_as(err)[keep]).all()), f"v_pred ({layout})"
            within(vs[:, r0:r1], vs_ref, vs_b, f"l1 v_scale ({layout})")
    if dead is None:
        assert n_live > 0
    assert n_flip <= 1e-4 * max(n_live, 1), (n_flip, n_live)


# ------------------------------------------------------------------------------------------------ fused head + loss
HEAD_CASES = [((37, 53), (37, 53), 300), ((7, 9), (67, 93), 11), ((1080, 1920), (1080, 1920), 1500), ((540, 960), (1080, 1920), 300)]


@pytest.mark.parametrize("src,dst,n_emb", HEAD_CASES)
def test_fused_head_and_distillation_loss_against_float64(src, dst, n_emb):
    """gags_decoder_head_distill_fwd and its three backward variants (fp32, bf16, half with dz_scale) -- one-tap (equal
    resolutions) and four-tap resize -- against float64 F.normalize(dim=0) + the L1 map of the restatement."""
    from gags_amd import _lib
    lib = _lib.load()
    c = 512
    H, W = dst
    h, w = src
    emb, seg, sc, g = sam_inputs(c, src, dst, n_emb, seed=31 + H + W)
    x = torch.randn(H * W, c, device=DEV, generator=g) * (0.25 + torch.rand(H * W, 1, device=DEV, generator=g))
    V = torch.rand(H, W, device=DEV, generator=g) + 0.5
    st = stream()
    l1 = torch.empty(H, W, device=DEV)
    mk = torch.empty(H, W, device=DEV)
    assert lib.gags_decoder_head_distill_fwd(c, c, H, W, h, w, n_emb, P(x), P(emb), P(seg), P(sc), P(l1), P(mk), st) == 0
    dz32 = torch.empty(H * W, c, device=DEV)
    vs32 = torch.empty(3, H, W, device=DEV)
    assert lib.gags_decoder_head_distill_bwd_f32(c, c, H, W, h, w, n_emb, P(x), P(emb), P(seg), P(sc), P(V), P(dz32), P(vs32), st) == 0
    dzb = torch.empty(H * W, c, dtype=torch.bfloat16, device=DEV)
    vsb = torch.empty(3, H, W, device=DEV)
    assert lib.gags_decoder_head_distill_bwd(c, c, H, W, h, w, n_emb, P(x), P(emb), P(seg), P(sc), P(V), P(dzb), P(vsb), st) == 0
    torch.cuda.synchronize()
    S = 2.0 ** math.floor(math.log2(8192.0 / float(dz32.abs().max())))  # a power of two: max |dz| S in [8192, 16384)
    s_dev = torch.tensor([S], device=DEV)
    dzh = torch.empty(H * W, c, dtype=torch.float16, device=DEV)
    vsh = torch.empty(3, H, W, device=DEV)
    assert lib.gags_decoder_head_distill_bwd_h16(c, c, H, W, h, w, n_emb, P(x), P(emb), P(seg), P(sc), P(V), P(dzh), P(s_dev),
                                                 P(vsh), st) == 0
    torch.cuda.synchronize()
    # v_scale does not depend on the gradient's storage format: the same sums in every variant
    assert torch.equal(vsb, vs32) and torch.equal(vsh, vs32)

    n_flip = n_live = 0
    for r0, r1 in bands(H, W, c):
        p0, p1 = r0 * W, r1 * W
        Fl, Al, mref, gt, T = sam_ref(emb, seg, sc, r0, r1)
        assert torch.equal(mk[r0:r1] != 0, mref), "mask"
        xb = x[p0:p1].double()                                   # [n, c]
        nrm = xb.norm(dim=1).clamp_min(1e-12)
        yp = xb / nrm[:, None]
        y = yp.t().reshape(c, r1 - r0, W)
        m = mref.double()
        d = (y - gt) * m
        # forward: |diff| within (KY + 1) U |y| + (KG + 1) U T, a lane's chain of 64 additions + 3 shuffles + the division
        # (68): (KY + KG + 70) U sum_c (|y| + T) m / c, rounded up to 120
        within(l1[r0:r1], d.abs().mean(0), 120 * U * ((y.abs() + T) * m).sum(0) / c, "head l1 map")
        eb = (KY + 1) * U * y.abs() + (KG + 1) * U * T
        flip = (m > 0) & (d.abs() <= eb)
        n_flip += int(flip.sum())
        n_live += int(m.sum()) * c
        vc = V[r0:r1].double() / c
        gch = torch.sign(d) * m * vc                                  # d l1 / d y, [c, R, W]
        vs_ref = -(gch[None] * Fl).sum(1)
        vs_b = chain_vs(c) * U * ((m * vc)[None] * Al).sum(1) + 2.0 * (1 + 1e-5) * ((flip * vc)[None] * Al).sum(1)
        within(vs32[:, r0:r1], vs_ref, vs_b, "head v_scale")
        # dz = (g - y <y, g>) / |x|, pixel-major
        gp = gch.reshape(c, -1).t()
        flp = flip.reshape(c, -1).t()
        vcp = vc.reshape(-1)[:, None]
        dz_ref = (gp - yp * (yp * gp).sum(1, keepdim=True)) / nrm[:, None]
        A1 = gp.abs() / nrm[:, None]
        A2 = xb.abs() * ((xb.abs() * gp.abs()).sum(1) / nrm ** 3)[:, None]
        # g / n: 2 roundings in v / c, 36 in 1 / n, 1 product (39); <x, g> / n^3: a chain of 32 fma + 1 + 3 shuffles with
        # v / c's 2 (38), three products (3) and 1 / n cubed (108) = 149; the final fma 1: 151 U (A1 + A2), rounded up to 160.
        # A flipped channel j moves every element i of the pixel by |x_i| |x_j| 2 |v| / c / n^3 through <x, g>.
        fb = 160 * U * (A1 + A2) + xb.abs() * (2.0 * (1 + 1e-5) * (xb.abs() * flp * vcp).sum(1) / nrm ** 3)[:, None]
        keep = ~flp
        got32 = dz32[p0:p1]
        within(got32[keep], dz_ref[keep], fb[keep], "head dz (fp32)")
        # bf16: round to nearest of the fp32 value, half an ulp = 2^-8 of the magnitude
        within(dzb[p0:p1].float()[keep], dz_ref[keep], 2.0 ** -8 * (dz_ref.abs() + fb)[keep] + fb[keep], "head dz (bf16)")
        # half, scaled by S: half an ulp = 2^-11 of the magnitude, or 2^-25 among the subnormals
        within(dzh[p0:p1].float()[keep] / S, dz_ref[keep], (2.0 ** -11 * (dz_ref.abs() + fb) + 2.0 ** -25 / S + fb)[keep],
               "head dz (half)")
    assert n_live > 0 and n_flip <= 1e-4 * n_live, (n_flip, n_live)


# ------------------------------------------------------------------------------------------------ segment losses
def chain_len(lib, n_pix, c, n_seg, pm):
    """Longest fp32 chain of a segment's partial sums in the kernel that serves this shape: the runs kernel sums a run of
    at most 128 (16 lanes per pixel) or 32 (one plane) pixels; the wave-sum kernel 4 pixels per lane + a 6-level tree."""
    from gags_amd import losses as L
    if L.RUNS and lib.gags_segment_stats_runs_copies(n_pix, c, n_seg, 1 if pm else 0) > 0:
        return 128 if c == 16 else 32
    return 10


def region_seg_map(H, W, n_seg, g):
    """ids in 8x8 blocks from [0, n_seg) minus a few absent ones, the largest id present; 2 % -1 pixels; three segments of
    one pixel and three of two pixels placed on their own."""
    bh, bw = (H + 7) // 8, (W + 7) // 8
    pool = torch.arange(n_seg - 7, device=DEV)
    pool = pool[pool % 11 != 5]                                   # absent ids
    blk = pool[torch.randint(0, pool.numel(), (bh, bw), device=DEV, generator=g)].float()
    seg = blk.repeat_interleave(8, 0).repeat_interleave(8, 1)[:H, :W].contiguous()
    seg[torch.rand(H, W, device=DEV, generator=g) < 0.02] = -1.0
    flat = seg.view(-1)
    pix = torch.randperm(H * W - 1, device=DEV, generator=g)[:9]
    for k in range(3):
        flat[pix[k]] = n_seg - 7 + k                              # one pixel
        flat[pix[3 + 2 * k: 5 + 2 * k]] = n_seg - 4 + k          # two pixels
    flat[H * W - 1] = n_seg - 1                                   # the largest id (so n_seg is what the loss sees)
    return seg


REGION_CASES = [  # (c, H, W, n_seg, pixel-major)
    (16, 200, 300, 590, True),   # the runs kernel's LDS table at its cap
    (16, 200, 300, 591, True),   # one beyond: the wave-sum kernel, 16 private copies
    (512, 128, 160, 512, True),  # n_seg c 16 = 2^22: 16 copies, float4 pixel-major rows
    (512, 128, 160, 513, True),  # one copy
    (3, 96, 128, 40, False),     # channel-major, n_pix % 4 == 0 (float4 rows)
    (3, 97, 131, 40, False),     # n_pix % 4 != 0
]


@pytest.mark.parametrize("c,H,W,n_seg,pm", REGION_CASES)
def test_region_variance_loss_and_gradient_against_float64(c, H, W, n_seg, pm):
    """scale_region_regulation_loss (mix_seg=True) and its gradient, plain and _tee, across the dispatch boundaries of the
    segment moments; segments absent, of 1 and 2 pixels, -1 pixels, nearly constant regions (spread 1e-4 under 0.7)."""
    from gags_amd import _lib, losses as L
    lib = _lib.load()
    g = gen(1000 + c + n_seg)
    seg = region_seg_map(H, W, n_seg, g)
    ids = seg.long().clamp(min=0)
    quiet = (torch.arange(n_seg, device=DEV) % 3 == 0)            # nearly constant segments
    base = torch.where(quiet[:, None], torch.full((n_seg, c), 0.7, device=DEV), torch.rand(n_seg, c, device=DEV, generator=g))
    spread = torch.where(quiet, 1e-4, 0.3)[ids]                   # [H, W]
    xhw = base[ids] + spread[..., None] * torch.randn(H, W, c, device=DEV, generator=g)
    x0 = xhw.contiguous() if pm else xhw.permute(2, 0, 1).contiguous()  # memory [H, W, c] or [c, H, W]
    v = 0.625

    vt = torch.tensor(v, device=DEV)

    def run(tee):
        xl = x0.clone().requires_grad_(True)
        xv = xl.permute(2, 0, 1) if pm else xl
        if tee:  # the next consumer's gradient in the map's own layout (pixel-major: the fused add kernel)
            loss, nxt = L.scale_region_regulation_loss_tee(xv, seg)
            torch.autograd.backward([loss, nxt], [vt, Gn])
        else:
            loss = L.scale_region_regulation_loss(xv, seg, mix_seg=True)
            loss.backward(vt)
        return loss.detach(), (xl.grad.permute(2, 0, 1) if pm else xl.grad)

    Gn = torch.randn(c, H, W, device=DEV, generator=g)
    Gn = Gn.permute(1, 2, 0).contiguous().permute(2, 0, 1) if pm else Gn
    loss, vx = run(False)
    loss_t, vx_t = run(True)
    torch.cuda.synchronize()
    assert torch.equal(loss_t, loss)
    assert torch.equal(vx_t, vx + Gn)                              # the next consumer's gradient arrives exactly

    xr = (x0.permute(2, 0, 1) if pm else x0).double()              # [c, H, W]
    xf = xr.reshape(c, -1)
    n, mean, css = R.segment_moments(xr, seg)
    ok = seg.reshape(-1) != -1
    idx = seg.reshape(-1).long()
    HW = H * W
    Lc = chain_len(lib, HW, c, n_seg, pm)
    # D = max |x - mean| per segment and channel; x^2 sums for the double-precision part
    dev_ = (xf[:, ok].t() - mean[idx[ok]]).abs()
    D = torch.zeros_like(mean).scatter_reduce(0, idx[ok][:, None].expand(-1, c), dev_, "amax")
    sq = torch.zeros_like(mean).index_add(0, idx[ok], xf[:, ok].t() ** 2)
    keep = n >= 2
    nk = n.double()
    ref = float((nk[keep] * (css[keep] / (nk[keep] - 1)[:, None]).mean(1)).sum() / HW)
    assert abs(ref - float(R.scale_region_regulation_loss(xr, seg))) <= 1e-12 * ref
    # centred sum of squares per segment and channel: a run of L fp32 partials about one of its own values s (|x - s| <= 2D)
    # is off by (L + 2) U 4 D^2 per pixel in sum t^2 and (L + 1) U 2 D in sum t, the latter entering through 2 (s - mean):
    # (8 L + 12) U n D^2; the double-precision sums and the cancellation s2 - n mean^2: (n + 8) 2^-53 2 sum x^2
    dN = (8 * Lc + 12) * U * nk[:, None] * D ** 2 + (nk[:, None] + 8) * R.U64 * 2 * sq
    lb = float((nk[keep] * (dN[keep] / (nk[keep] - 1)[:, None]).mean(1)).sum() / HW) + U * abs(ref)
    assert abs(float(loss) - ref) <= lb, (float(loss), ref, lb)

    coef = torch.zeros(mean.shape[0], dtype=torch.float64, device=DEV)
    coef[keep] = 2 * nk[keep] / ((nk[keep] - 1) * c * HW) * v
    cpix = torch.where(ok, coef[idx.clamp(min=0)], torch.zeros_like(coef[:1]))          # [n_pix]
    mpix = mean[idx.clamp(min=0)].t()                                                     # [c, n_pix]
    Dpix = D[idx.clamp(min=0)].t()
    vref = cpix * (xf - mpix)
    # the kernel's mean is the double sum (off by 2 (L + 1) U D) rounded to fp32 (U |mean|); x - mean, the product and the
    # coefficient (2 roundings, its product by v one more) add U (|x| + |mean|) and 4 U |ref|
    vb = cpix * U * (2 * (Lc + 1) * Dpix + 2 * (xf.abs() + mpix.abs())) + 4 * U * vref.abs()
    within(vx.reshape(c, -1), vref, vb, "region-variance gradient")
    dead = (cpix == 0)
    assert bool((vx.reshape(c, -1)[:, dead] == 0).all())            # -1 pixels, 1-pixel segments: exactly nothing
    assert int(keep.sum()) < int((n > 0).sum()) and int((n == 2).sum()) >= 3 and int((n == 0).sum()) > 0


BAL_CASES = [  # (n_seg, H, W, runs, unaligned)
    (7680, 192, 256, True, False),   # the one-plane runs kernel's LDS table at its cap
    (7681, 192, 256, True, False),   # one beyond: the wave-sum kernel
    (7680, 192, 256, False, False),
    (2000, 97, 131, True, False),    # n_seg > 1024: the finalize kernel's strided loops wrap
    (2000, 97, 131, False, False),
    (2000, 97, 131, True, True),     # a loss map at storage offset 1: the runs kernel's scalar loads
    (2000, 97, 131, False, True),
]


@pytest.mark.parametrize("n_seg,H,W,runs,unaligned", BAL_CASES)
def test_scale_balance_loss_and_gradient_against_float64(n_seg, H, W, runs, unaligned):
    """Scale_balance_loss (mix_seg=True) and its gradient (gather_seg_coef_kernel) across the one-plane runs kernel's cap,
    above 1024 segments, on an unaligned loss map, with both GAGS_SEGMENT_RUNS settings."""
    from gags_amd import _lib, losses as L
    lib = _lib.load()
    g = gen(n_seg + H)
    seg = torch.randint(0, n_seg - 1, (H, W), device=DEV, generator=g).float()
    seg[seg % 13 == 4] = -1.0                                      # -1 pixels, and those ids absent
    seg.view(-1)[-1] = n_seg - 1
    buf = torch.rand(H * W + 1, device=DEV, generator=g) * 2.0
    lm0 = buf[1:].view(H, W) if unaligned else buf[:-1].clone().view(H, W)
    assert lm0.is_contiguous() and ((lm0.data_ptr() % 16) != 0) == unaligned
    v = 1.375
    old = L.RUNS
    try:
        L.RUNS = runs
        Lc = chain_len(lib, H * W, 1, n_seg, False)
        lm = lm0.requires_grad_(True)
        loss = L.Scale_balance_loss(lm, seg, None, mix_seg=True)
        (loss * v).backward()
    finally:
        L.RUNS = old
    torch.cuda.synchronize()
    ref = R.Scale_balance_loss(lm0.detach(), seg)
    idx = seg.reshape(-1).long()
    ok = idx >= 0
    n = torch.bincount(idx[ok], minlength=n_seg)
    M = torch.zeros(n_seg, dtype=torch.float64, device=DEV).scatter_reduce(0, idx[ok], lm0.detach().reshape(-1)[ok].double(),
                                                                           "amax")
    K = int((n > 0).sum())
    # a segment's sum: fp32 runs of L partials about one of their values (|t| <= 2 M) -> 2 (L + 1) U n M; over n and K in
    # double; the result rounded to fp32
    bound = float((2 * (Lc + 1) * U * M[n > 0]).sum() / K) + U * float(ref) + 1e-15
    assert abs(loss.item() - float(ref)) <= bound, (loss.item(), float(ref), bound)
    # gradient: v / (n K) formed as fp32(1 / (n K)) times v, rounded: 2 roundings
    want = torch.where(ok, v / (n[idx.clamp(min=0)].double() * K), torch.zeros((), dtype=torch.float64, device=DEV))
    got = lm.grad.reshape(-1)
    within(got, want, 2 * U * want.abs(), "balance gradient")
    assert bool((got[~ok] == 0).all()) and K > 1024


def test_scale_balance_loss_without_segments_is_zero():
    """Deliberate deviation from the reference: with every pixel -1 the reference raises (torch.stack of an empty list);
    this port returns a loss of 0 with a zero gradient."""
    from gags_amd import losses as L
    lm = torch.rand(33, 47, device=DEV).requires_grad_(True)
    seg = torch.full((33, 47), -1.0, device=DEV)
    with pytest.raises(ValueError):
        R.Scale_balance_loss(lm.detach(), seg)
    loss = L.Scale_balance_loss(lm, seg, None, mix_seg=True)
    loss.backward()
    assert loss.item() == 0.0 and bool((lm.grad == 0).all())


# ------------------------------------------------------------------------------------------------ get_trained_seg
@pytest.mark.parametrize("H,W", [(1, 1), (3, 3), (5, 67), (67, 5), (130, 259), (1080, 1920)])
def test_trained_seg_against_float64(H, W):
    """trained_seg_kernel (64 x 4 LDS patches with a 2-pixel halo): the restatement's level wherever the top two float64
    scores are further apart than the fp32 error of two 25-tap sums; either of the near-tied levels elsewhere (rare)."""
    from gags_amd import losses as L
    g = gen(H * 7 + W)
    seg = torch.stack([torch.randint(0, 100, (H, W), device=DEV, generator=g) + 1000 * lev for lev in range(4)]).float()
    sc = torch.softmax(torch.randn(3, H, W, device=DEV, generator=g), 0)
    got = L.get_trained_seg(seg, sc)
    torch.cuda.synchronize()
    sm = R.smoothed_scale(sc)
    # a score is 25 fma of p * fp32(1 / 25): 25 roundings of the partial sum, and fp32(1/25) is 0.37 U off 1/25 -> 26 U
    # times the sum of its |taps| / 25; two scores: 52 U
    mag = F.conv2d(sc.double().abs()[None], torch.full((3, 1, 5, 5), 1 / 25, dtype=torch.float64, device=DEV), padding=2,
                   groups=3)[0]
    thr = 52 * U * mag.max(0).values
    top = sm.max(0).values
    near = sm >= (top - thr)[None]                                 # [3, H, W]: the levels within the bound of the best
    certain = near.sum(0) == 1
    ref = R.get_trained_seg(seg, sc)
    assert torch.equal(got[certain], ref[certain].float())
    lev = (got[None] == seg[1:]) & near                            # the kernel's id is one of the near-tied levels' ids
    assert bool(lev.any(0).all())
    assert int((~certain).sum()) <= max(1, 1e-3 * H * W)


def test_trained_seg_exact_ties_pick_the_first_level():
    """torch.argmax keeps the first maximum: identical channels and a constant map both pick level s (seg[1])."""
    from gags_amd import losses as L
    H, W = 70, 131
    g = gen(5)
    seg = torch.stack([torch.randint(0, 50, (H, W), device=DEV, generator=g) + 1000 * lev for lev in range(4)]).float()
    one = torch.rand(1, H, W, device=DEV, generator=g)
    for sc in (one.expand(3, H, W).contiguous(), torch.full((3, H, W), 1 / 3, device=DEV)):
        got = L.get_trained_seg(seg, sc)
        assert torch.equal(got, seg[1]) and torch.equal(R.get_trained_seg(seg, sc).float(), seg[1])


# ------------------------------------------------------------------------------------------------ entropy
def test_scale_regulation_loss_at_1080p_against_float64():
    """mean(-s log(s + 1e-6)) and its gradient at 1080p, with entries exactly 0 and 1 and entries near 1e-6."""
    from gags_amd import losses as L
    g = gen(77)
    H, W = 1080, 1920
    s0 = torch.softmax(3.0 * torch.randn(3, H, W, device=DEV, generator=g), 0)
    flat = s0.view(-1)
    pick = torch.randperm(flat.numel(), device=DEV, generator=g)[:30000]
    flat[pick[:10000]] = 0.0
    flat[pick[10000:20000]] = 1.0
    flat[pick[20000:]] = 2e-6 * torch.rand(10000, device=DEV, generator=g)
    s = s0.clone().requires_grad_(True)
    v = 0.8125
    loss = L.scale_regulation_loss(s)
    (loss * v).backward()
    torch.cuda.synchronize()
    sd = s0.double()
    lg = torch.log(sd + R.EPS_LOG)
    ref = float(R.scale_regulation_loss(s0))
    # per element: s + 1e-6 rounds (1 U in the log's argument: U absolute in the log), logf is within 2 ulp, the product 1:
    # |s| U (1 + 3 |log|); summed in double; the mean rounded to fp32
    bound = float((sd.abs() * U * (1 + 3 * lg.abs())).sum() / sd.numel()) + U * abs(ref)
    assert abs(loss.item() - ref) <= bound, (loss.item(), ref, bound)
    q = sd / (sd + R.EPS_LOG)
    vn = v / sd.numel()
    want = -(lg + q) * vn
    # log: (1 + 2) U |log| + U, the quotient 2 U q, the sum U (|log| + q), the factor v / n rounded 1 and the product 1
    vb = vn * U * (4 * lg.abs() + 3 * q + 3) + 2 * U * want.abs()
    within(s.grad, want, vb, "entropy gradient")


def test_entropy_gradient_with_a_host_cotangent_one_past_a_workgroup():
    """gags_entropy_bwd (entropy_bwd_kernel: the factor v / n arrives as a host float; gags_amd.losses calls the device-scalar
    form above) at n = 257, one element past a workgroup, with entries 0, 1 and near 1e-6: the gradient's bound of the test
    above, and nothing written past the end."""
    from gags_amd import _lib
    g = gen(78)
    n = 257
    s0 = torch.softmax(3.0 * torch.randn(3, n, device=DEV, generator=g), 0)[0].contiguous()
    s0[0], s0[1], s0[255], s0[256] = 0.0, 1.0, 1.5e-6, 1.0
    v = 0.8125
    vn = v / n
    vs = torch.full((n + 1,), float("nan"), device=DEV)
    assert _lib.load().gags_entropy_bwd(n, P(s0), vn, P(vs), stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(vs[n])) and not bool(torch.isnan(vs[:n]).any())
    sd = s0.double()
    lg = torch.log(sd + R.EPS_LOG)
    q = sd / (sd + R.EPS_LOG)
    want = -(lg + q) * vn
    vb = vn * U * (4 * lg.abs() + 3 * q + 3) + 2 * U * want.abs()
    within(vs[:n], want, vb, "entropy gradient, host cotangent")
