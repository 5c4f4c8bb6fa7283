"""N5 on the GPU: the 3-D open-vocabulary query (gags_amd/pointquery.py, csrc/pointquery.hip) against the reference's own
smooth_pcd_mask and pcd_relvancy (tests/golden/pcd_query_vectors.npz, make_golden_pcd.py), and against an independent
float64 brute force of the neighbour rule at real size, at the edges and on random clouds."""
import os
import sys

import numpy as np
import pytest
import torch
from hypothesis import given, settings, strategies as st

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
Z = np.load(os.path.join(HERE, "golden", "pcd_query_vectors.npz"))
sys.path.insert(0, os.path.join(HERE, "golden"))
PARAMS = [(0.05, 20), (0.1, 10), (0.0625, 4)]  # make_golden_pcd.PARAMS
CLOUDS = ("lattice", "blobs", "dups")


def dev(a):
    return torch.from_numpy(np.asarray(a)).cuda()


def brute(xyz, masks, r, threshold, rows=None, chunk_pairs=1 << 25):
    """Independent float64 restatement on the GPU: counts c [K, Q] of masked points j with ((dx*dx + dy*dy) + dz*dz) <= r*r
    (torch's elementwise ops in eager mode do not fuse) for the query points `rows` (all by default); returns
    (out, min(c, cap)) for those points."""
    x = xyz.double()
    q = x if rows is None else x[rows]
    cap = max(threshold + 1, 10)
    r2 = r * r
    outs, cnts = [], []
    for k in range(masks.shape[0]):
        cand = x[masks[k]]
        c = torch.zeros(q.shape[0], dtype=torch.int64, device=x.device)
        if cand.shape[0]:
            step = max(1, chunk_pairs // cand.shape[0])
            for s in range(0, q.shape[0], step):
                qq = q[s:s + step]
                dx = qq[:, None, 0] - cand[None, :, 0]
                dy = qq[:, None, 1] - cand[None, :, 1]
                dz = qq[:, None, 2] - cand[None, :, 2]
                d2 = dx * dx
                d2 = d2 + dy * dy
                d2 = d2 + dz * dz
                c[s:s + step] = (d2 <= r2).sum(1)
        m = masks[k] if rows is None else masks[k][rows]
        outs.append((c > threshold) | (m & (c >= 10)))
        cnts.append(c.clamp(max=cap).int())
    return torch.stack(outs), torch.stack(cnts)


def _decoder_and_head():
    from gags_amd.decoders import CNN_decoder
    from gags_amd.relevancy import RelevancyHead
    from make_golden_next import decoder_weights
    dec = CNN_decoder(16, 512).cuda()
    with torch.no_grad():
        for m, (W, b) in zip(dec.convs(), decoder_weights(0)[0]):
            m.weight.copy_(W[:, :, None, None])
            m.bias.copy_(b)
    return dec, RelevancyHead(dev(Z["e2e_pos"]), dev(Z["e2e_neg"]))


# ---------------------------------------------------------------- against the reference fixture

@pytest.mark.parametrize("cloud", CLOUDS)
@pytest.mark.parametrize("p", range(len(PARAMS)))
def test_smooth_equals_reference_smooth_pcd_mask(cloud, p):
    from gags_amd.pointquery import smooth_point_mask
    r, thr = PARAMS[p]
    xyz, masks = dev(Z[f"{cloud}_xyz"]), dev(Z[f"{cloud}_mask"])
    out, cnt = smooth_point_mask(masks, xyz, r, thr, return_counts=True)
    assert torch.equal(out, dev(Z[f"{cloud}_p{p}_out"]))
    assert torch.equal(cnt, dev(Z[f"{cloud}_p{p}_count"]).clamp(max=max(thr + 1, 10)))
    for k in range(masks.shape[0]):  # a single [N] mask
        assert torch.equal(smooth_point_mask(masks[k], xyz, r, thr), out[k])


def test_query_points_equals_reference_pcd_relvancy():
    from gags_amd.pointquery import query_points
    dec, head = _decoder_and_head()
    res = query_points(dev(Z["e2e_sem"]), dev(Z["e2e_xyz"]), dec, head, rel_thresh=float(Z["e2e_rel_thresh"]))
    rel = res["relevancy"].cpu().numpy()
    assert np.abs(rel - Z["e2e_relevancy"]).max() <= 1e-4
    assert np.abs(res["normalized"].cpu().numpy() - Z["e2e_normalized"]).max() <= 1e-3
    assert torch.equal(res["mask_raw"], dev(Z["e2e_mask_raw"]))
    assert torch.equal(res["mask"], dev(Z["e2e_mask"]))


def test_relevancy_alone_matches_get_relevancy_on_the_decoded_features():
    """Given the decoded features, the relevancy is get_relevancy (eval/openclip_encoder.py:42-56) restated in float64."""
    from gags_amd.pointquery import point_relevancy
    dec, head = _decoder_and_head()
    sem = dev(Z["e2e_sem"])
    with torch.no_grad():
        emb = dec(sem.t()[..., None]).squeeze(-1).t().double()
    p = torch.cat([head.pos_embeds, head.neg_embeds]).double()
    sims = emb @ p.T
    n_pos = head.pos_embeds.shape[0]
    want = []
    for j in range(n_pos):
        pos = sims[:, j:j + 1].expand(-1, sims.shape[1] - n_pos)
        sm = torch.softmax(10 * torch.stack((pos, sims[:, n_pos:]), -1), -1)
        want.append(sm[..., 0].min(1).values)
    got = point_relevancy(sem, dec, head)
    np.testing.assert_allclose(got.cpu().numpy(), torch.stack(want).cpu().numpy(), rtol=2e-5, atol=1e-7)


@pytest.mark.parametrize("bg", ["RGB", "gray", "mix"])
def test_recolor_dc_equals_reference_save_pcd(bg):
    from gags_amd.pointquery import recolor_dc
    got = recolor_dc(dev(Z["e2e_f_dc"]), dev(Z["e2e_mask"]), bg_color=bg).cpu().numpy()
    assert got.shape == Z[f"e2e_fdc_{bg}"].shape
    assert np.abs(got - Z[f"e2e_fdc_{bg}"]).max() <= 1e-6


def test_query_ply_writes_only_f_dc(tmp_path):
    from gags_amd import io_formats as io
    from gags_amd.pointquery import query_ply, recolor_dc
    dec, head = _decoder_and_head()
    xyz, sem, fdc = Z["e2e_xyz"], Z["e2e_sem"], Z["e2e_f_dc"]
    n = xyz.shape[0]
    g = np.random.default_rng(0)
    src = tmp_path / "point_cloud.ply"
    io.write_ply(str(src), xyz, fdc.reshape(n, 1, 3), g.standard_normal((n, 15, 3)), g.standard_normal((n, 1)),
                 g.standard_normal((n, 3)), g.standard_normal((n, 4)), sem)
    res = query_ply(str(src), dec, head, prompts=["chair", "table"], rel_thresh=float(Z["e2e_rel_thresh"]),
                    bg_color="mix", save_dir=str(tmp_path / "out"))
    assert torch.equal(res["mask"], dev(Z["e2e_mask"]))
    names0, t0 = io.read_ply_table(str(src))
    for k, path in enumerate(res["paths"]):
        assert path.endswith(f"point_cloud_{['chair', 'table'][k]}.ply")
        names1, t1 = io.read_ply_table(path)
        assert names1 == names0
        want = recolor_dc(dev(fdc), res["mask"][k], "mix").cpu().numpy()
        for nm in names0:
            if nm.startswith("f_dc_"):
                assert np.array_equal(t1[nm], want[:, int(nm[-1])])
            else:
                assert np.array_equal(t1[nm], t0[nm]), nm


# ---------------------------------------------------------------- real size

def _synthetic_cloud(n, seed=0):
    from gags_amd import synthetic as syn
    return syn.make_gaussians(n, 0, 1920, 1080, seed=seed, device="cuda")["xyz"].contiguous()


def _coherent_masks(xyz, frac, centres, flip=0.003, seed=1):
    """Points within the frac-quantile distance R of each centre, XOR a few random flips (isolated points and holes).
    Returns (masks [K, N], distances to the centres [K, N], R [K])."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    out, dist, rad = [], [], []
    for c in centres:
        d = (xyz - torch.tensor(c, device="cuda")).norm(dim=1)
        R = torch.quantile(d[torch.randperm(len(d), device="cuda", generator=g)[:100000]], frac)
        out.append((d < R) ^ (torch.rand(len(d), device="cuda", generator=g) < flip))
        dist.append(d)
        rad.append(R)
    return torch.stack(out), torch.stack(dist), torch.stack(rad)


def test_real_size_equals_float64_brute_force():
    """1.5 M Gaussians, K = 3 coherent masks of ~2 %, a radius at which the counts straddle 10 and the threshold: masks
    and capped counts equal the brute force on 6000 points sampled in and around each mask's ball and 2000 sampled from
    the whole cloud (the brute force over all 1.5 M points would take minutes)."""
    from gags_amd.pointquery import smooth_point_mask
    n, r, thr = 1_500_000, 0.06, 20
    xyz = _synthetic_cloud(n)
    masks, dist, rad = _coherent_masks(xyz, 0.02, [(0.0, 0.0, 3.0), (0.5, 0.2, 2.6), (-0.6, -0.3, 3.4)])
    out, cnt = smooth_point_mask(masks, xyz, r, thr, return_counts=True)
    g = torch.Generator(device="cuda").manual_seed(3)
    for k in range(3):
        # a sample of the points in and around the mask's ball (where the counts cross 10 and the threshold), and random
        # points of the whole cloud (mostly a count of 0 or of an isolated flipped point)
        mk = masks[k]
        near = torch.nonzero(dist[k] < rad[k] + 2 * r).squeeze(1)
        rows = torch.cat([near[torch.randperm(len(near), device="cuda", generator=g)[:6000]],
                          torch.randint(0, n, (2000,), device="cuda", generator=g)])
        bo, bc = brute(xyz, masks[k:k + 1], r, thr, rows=rows)
        assert torch.equal(out[k, rows], bo[0])
        assert torch.equal(cnt[k, rows], bc[0])
        c = bc[0]
        assert ((c >= 10) & (c <= thr)).sum() > 50 and (c < 10).sum() > 50 and (c > thr).sum() > 50
        assert (mk.sum() / n).item() < 0.03


def test_k_masks_in_one_call_equal_single_calls_and_runs_are_bit_identical():
    from gags_amd.pointquery import smooth_point_mask
    xyz = _synthetic_cloud(300_000, seed=2)
    masks = _coherent_masks(xyz, 0.05, [(0.0, 0.0, 3.0), (0.4, 0.1, 2.5), (0.0, 0.0, 3.0), (-0.5, 0.2, 4.0)])[0]
    masks[2] = masks[0]
    a, ca = smooth_point_mask(masks, xyz, 0.08, 20, return_counts=True)
    b, cb = smooth_point_mask(masks, xyz, 0.08, 20, return_counts=True)
    assert torch.equal(a, b) and torch.equal(ca, cb)
    assert torch.equal(a[0], a[2])  # the same mask twice in one call
    for k in range(masks.shape[0]):
        o, c = smooth_point_mask(masks[k], xyz, 0.08, 20, return_counts=True)
        assert torch.equal(o, a[k]) and torch.equal(c, ca[k])


def test_decode_chunking_does_not_change_the_relevancy():
    from gags_amd.pointquery import point_relevancy
    dec, head = _decoder_and_head()
    g = torch.Generator(device="cuda").manual_seed(5)
    n = 1_200_000
    sem = torch.randn(n, 16, device="cuda", generator=g)
    a = point_relevancy(sem, dec, head)  # chunk = 1 000 000: two decoder calls
    b = point_relevancy(sem, dec, head, chunk=n)
    assert torch.equal(a, b)
    h = sem[:4096].half()
    assert torch.equal(point_relevancy(h, dec, head), point_relevancy(h.float(), dec, head))  # fp16 tables upcast exactly


# ---------------------------------------------------------------- edges

def _check(xyz, masks, r, thr):
    from gags_amd.pointquery import smooth_point_mask
    out, cnt = smooth_point_mask(masks, xyz, r, thr, return_counts=True)
    bo, bc = brute(xyz, masks, r, thr)
    assert torch.equal(out, bo)
    assert torch.equal(cnt, bc)
    return out, cnt


def test_empty_cloud():
    from gags_amd.pointquery import smooth_point_mask
    xyz = torch.zeros(0, 3, device="cuda")
    assert smooth_point_mask(torch.zeros(0, dtype=torch.bool, device="cuda"), xyz).shape == (0,)
    o, c = smooth_point_mask(torch.zeros(2, 0, dtype=torch.bool, device="cuda"), xyz, return_counts=True)
    assert o.shape == (2, 0) and c.shape == (2, 0)


def test_all_false_and_all_true_masks():
    g = torch.Generator(device="cuda").manual_seed(7)
    xyz = torch.rand(5000, 3, device="cuda", generator=g) * 0.5
    masks = torch.stack([torch.zeros(5000, dtype=torch.bool, device="cuda"), torch.ones(5000, dtype=torch.bool, device="cuda")])
    out, cnt = _check(xyz, masks, 0.05, 20)
    assert not out[0].any() and (cnt[0] == 0).all()


def test_coincident_points():
    g = torch.Generator(device="cuda").manual_seed(8)
    base = torch.rand(200, 3, device="cuda", generator=g)
    xyz = torch.cat([base, base[:50].repeat(30, 1), torch.full((40, 3), 0.25, device="cuda")])
    masks = torch.rand(2, xyz.shape[0], device="cuda", generator=g) < torch.tensor([[0.3], [0.7]], device="cuda")
    _check(xyz, masks, 0.05, 20)
    _check(xyz, masks, 1e-200, 5)  # (r * r underflows to 0: only exact duplicates count)


def test_radius_larger_than_the_cloud():
    g = torch.Generator(device="cuda").manual_seed(9)
    xyz = torch.rand(3000, 3, device="cuda", generator=g)
    masks = torch.rand(2, 3000, device="cuda", generator=g) < 0.01
    out, cnt = _check(xyz, masks, 100.0, 20)
    assert (cnt[0] == min(int(masks[0].sum()), 21)).all()


def test_far_coordinates_clamp_the_cells():
    """Coordinates of +-1e6 at r = 0.05: 4e7 cells per axis, clamped to 2^16 -- the candidate set stays a superset."""
    g = torch.Generator(device="cuda").manual_seed(10)
    near = torch.randn(4000, 3, device="cuda", generator=g) * 0.05
    far = torch.tensor([[1e6, 0, 0], [-1e6, 0, 0], [0, 1e6, -1e6]], device="cuda").repeat_interleave(100, 0)
    far = far + torch.randn(300, 3, device="cuda", generator=g) * 0.03
    xyz = torch.cat([near, far, far[:50]])
    masks = torch.rand(2, xyz.shape[0], device="cuda", generator=g) < torch.tensor([[0.5], [0.9]], device="cuda")
    _check(xyz, masks, 0.05, 20)


def test_threshold_below_ten():
    g = torch.Generator(device="cuda").manual_seed(11)
    xyz = torch.rand(6000, 3, device="cuda", generator=g) * 0.6
    masks = torch.rand(2, 6000, device="cuda", generator=g) < 0.3
    for thr in (0, 3, 9):
        _check(xyz, masks, 0.05, thr)


# ---------------------------------------------------------------- property

@settings(max_examples=60, deadline=None)
@given(n=st.integers(1, 300), k=st.integers(1, 3), seed=st.integers(0, 2 ** 31 - 1),
       r=st.sampled_from([0.0625, 0.05, 0.1, 0.25]), thr=st.integers(0, 30), lattice=st.booleans(),
       dup=st.floats(0.0, 0.5), p=st.floats(0.0, 1.0))
def test_random_clouds_equal_the_float64_rule(n, k, seed, r, thr, lattice, dup, p):
    rng = np.random.default_rng(seed)
    if lattice:  # binary spacing: pairs at exactly r
        xyz = (rng.integers(-6, 6, (n, 3)) * 2.0 ** -5).astype(np.float32)
    else:
        xyz = (rng.random((n, 3)) * 0.4).astype(np.float32)
    d = rng.random(n) < dup
    if d.any():
        xyz[d] = xyz[rng.integers(0, n, int(d.sum()))]
    masks = rng.random((k, n)) < p
    _check(dev(xyz), dev(masks), r, thr)
