"""world_size-2 `gloo` tests of the view-sharded step's only exchange (gags_amd/dist.py)."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, mode, n, d, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gags_amd.dist import reduce_feature_grad, shard_views
    g = torch.Generator().manual_seed(100 + rank)
    grad = torch.randn(n, d, generator=g)
    expect = sum(torch.randn(n, d, generator=torch.Generator().manual_seed(100 + r)) for r in range(world))
    reduce_feature_grad(grad, mode=mode, bucket_bytes=4096)
    ok = torch.allclose(grad, expect, rtol=1e-6, atol=1e-6)
    # smaller than one bucket (the default 256 MB against the 228 MB union-row blocks of the C4 step): still
    # reduce-scatter + all-gather over one bucket, only the < world-size tail is all-reduced
    import gags_amd.dist as D
    calls = []
    real_rs = D._reduce_scatter
    D._reduce_scatter = lambda shard, full: (calls.append(full.numel()), real_rs(shard, full))[1]
    g2 = torch.randn(n, d, generator=torch.Generator().manual_seed(100 + rank))
    reduce_feature_grad(g2, mode=mode)
    D._reduce_scatter = real_rs
    ok = ok and torch.allclose(g2, expect, rtol=1e-6, atol=1e-6)
    if mode == "rs_ag":
        ok = ok and calls == [n * d // world * world]
    # the out-of-place form the overlapped exchange uses: the sum in a NEW tensor, the source left as it is (it stays the
    # rank's local rows), bucketed and un-bucketed
    from gags_amd.dist import reduce_feature_grad_oop
    g3 = torch.randn(n, d, generator=torch.Generator().manual_seed(100 + rank))
    keep = g3.clone()
    for bb in (4096, 256 << 20):
        s3 = reduce_feature_grad_oop(g3, mode=mode, bucket_bytes=bb)
        ok = ok and torch.equal(g3, keep) and s3.data_ptr() != g3.data_ptr() and s3.shape == g3.shape
        ok = ok and torch.allclose(s3, expect, rtol=1e-6, atol=1e-6)
    views = shard_views(8)
    q.put((rank, bool(ok), views))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["rs_ag", "allreduce"])
def test_feature_grad_reduction_two_ranks(mode):
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, mode, 1037, 7, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    res.sort()
    assert all(ok for _, ok, _ in res)
    assert res[0][2] == [0, 2, 4, 6] and res[1][2] == [1, 3, 5, 7]


def test_single_process_is_noop():
    from gags_amd.dist import reduce_feature_grad, shard_views
    g = torch.arange(12.0).reshape(3, 4)
    assert reduce_feature_grad(g.clone()).equal(g)
    assert shard_views(5, rank=0, world_size=1) == [0, 1, 2, 3, 4]


def test_channel_shards_partition_the_feature_width():
    from gags_amd.dist import channel_shard
    for d, ws in ((512, 8), (512, 2), (512, 3), (16, 8), (48, 2), (100, 4), (33, 2)):
        got = [channel_shard(d, rank=r, world_size=ws) for r in range(ws)]
        assert got[0][0] == 0 and got[-1][1] == d
        for (a0, a1), (b0, b1) in zip(got, got[1:]):
            assert a1 == b0 and a0 <= a1
        for c0, c1 in got[:-1]:
            assert (c1 - c0) % 16 == 0
    assert channel_shard(512, rank=3, world_size=8) == (192, 256)


def _channel_worker(rank, world, port, q):
    """by-channel step on a linear stand-in renderer (render = features^T pooled over a fixed weight map):
    the shards' gradients, concatenated, equal the full-width single-process gradient -- with no collective."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gags_amd.dist import channel_shard, distributed_step
    n, d, h, w, views = 50, 64, 6, 5, 3
    gen = torch.Generator().manual_seed(0)
    feats = torch.randn(n, d, generator=gen)
    W = [torch.rand(h * w, n, generator=gen) for _ in range(views)]   # per-view blending weights (the "geometry")
    G = [torch.randn(d, h, w, generator=gen) for _ in range(views)]

    class PC:
        pass

    def render_fn(cam, pc, pipe, bg, feature_mode=True):
        return {"render": (W[cam] @ pc._semantic_feature).t().reshape(-1, h, w)}

    c0, c1 = channel_shard(d)
    pc = PC()
    pc._semantic_feature = torch.nn.Parameter(feats[:, c0:c1].clone())
    distributed_step(render_fn, list(range(views)), pc, None, [g[c0:c1] for g in G], mode="channel")
    full = PC()
    full._semantic_feature = torch.nn.Parameter(feats.clone())
    for v in range(views):
        (render_fn(v, full, None, None)["render"] * G[v]).sum().backward()
    ok = torch.allclose(pc._semantic_feature.grad, full._semantic_feature.grad[:, c0:c1], rtol=1e-5, atol=1e-5)
    q.put((rank, bool(ok), (c0, c1)))
    dist.barrier()
    dist.destroy_process_group()


def test_channel_sharded_step_two_ranks():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_channel_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res)
    assert res[0][2] == (0, 32) and res[1][2] == (32, 64)


def _overlap_worker(rank, world, port, wire, q):
    """OverlappedGradReducer fed range by range the way the staged backward feeds it (gags_amd/raster_staged.py):
    exact fp32 sum on the default wire; bfloat16 wire within its stated bound; and every way autograd may hand the
    gradient on -- adopted, copied, accumulated onto an existing gradient, behind a dtype cast -- must end with the
    sum over the ranks ONCE (a copied gradient used to be reduced a second time)."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gags_amd import rasterization
    from gags_amd.dist import OverlappedGradReducer
    n, d = 333, 512
    grads = [torch.randn(n, d, generator=torch.Generator().manual_seed(7 + r)) for r in range(world)]
    expect = sum(grads)
    rel = lambda a, b: ((a - b).double().norm() / b.double().norm()).item()

    def feed(red, local):
        with red:
            assert rasterization.default_context().grad_range_hook is not None
            for c0 in range(0, d, 128):
                rasterization.default_context().grad_range_hook(local.detach(), c0, c0 + 128)  # alias with its own TensorImpl
        assert rasterization.default_context().grad_range_hook is None

    out = {}
    mode = "allreduce" if wire == "bf16" else "rs_ag"
    # 1. adopted: autograd keeps the very tensor the hook saw
    grad = grads[rank].clone()
    red = OverlappedGradReducer(mode=mode, wire=wire, bucket_bytes=8192)
    feed(red, grad)
    out["adopted"] = (red.finish(grad), rel(grad, expect), red.assigned)
    # 2. copied: another consumer forced a clone (param unknown: the reducer falls back on local + (sum - local))
    local = grads[rank].clone()
    feed(red, local)
    copied = local * 1.0
    out["copied"] = (red.finish(copied), rel(copied, expect))
    assert torch.equal(local, grads[rank])  # the tensor autograd consumed was never written by the exchange
    # 3. accumulated onto an existing gradient (a second view of the step)
    old = torch.randn(n, d, generator=torch.Generator().manual_seed(99))
    local = grads[rank].clone()
    feed(red, local)
    acc = old + local
    out["accumulated"] = (red.finish(acc), rel(acc, old + expect))
    # 4. param known, its gradient None on entry, but the parameter has a SECOND consumer in the graph (a regulariser on
    #    the features): autograd sums both terms into a fresh tensor.  The other term must survive, un-reduced (ADVICE r3:
    #    an assignment on "grad was None on entry" silently dropped it on the union rows)
    prm = torch.nn.Parameter(torch.zeros(n, d))
    red_p = OverlappedGradReducer(mode=mode, wire=wire, bucket_bytes=8192, param=prm)
    local = grads[rank].clone()
    feed(red_p, local)
    other_term = torch.randn(n, d, generator=torch.Generator().manual_seed(500 + rank))
    prm.grad = local + other_term
    out["param_fresh"] = (red_p.finish(prm.grad), rel(prm.grad, expect + other_term), not red_p.assigned)
    # 4a. ... or adds the second term IN PLACE into the adopted tensor (same storage; its version counter moved)
    prm.grad = None
    local = grads[rank].clone()
    feed(red_p, local)
    local += other_term
    out["param_inplace"] = (red_p.finish(local), rel(local, expect + other_term), not red_p.assigned)
    prm.grad = local
    # 4b. the same parameter with a gradient already there: the next block accumulates
    local = grads[rank].clone()
    feed(red_p, local)
    before = prm.grad.clone()
    prm.grad += local
    out["param_accumulate"] = (red_p.finish(prm.grad), rel(prm.grad, before + expect))
    # 5. an fp32 master gradient behind a cast of the table's fp16 gradient
    if wire is None:
        l16 = grads[rank].half()
        red_h = OverlappedGradReducer(mode=mode, bucket_bytes=8192, param=torch.nn.Parameter(torch.zeros(1)))
        feed(red_h, l16)
        master = l16.float()  # what autograd's cast node hands the fp32 master parameter
        out["cast"] = (red_h.finish(master), rel(master, sum(g.half().float() for g in grads)))
    # 6. a gradient the hook never saw in this block: finish() reduces it itself, once
    with red:
        pass
    other = grads[rank].clone()
    out["unseen"] = (red.finish(other), rel(other, expect))
    # 7. two backwards inside one block are refused, not silently mixed
    try:
        with red:
            for _ in range(2):
                rasterization.default_context().grad_range_hook(grads[rank].clone().detach(), 0, 128)
        out["second_refused"] = False
    except RuntimeError:
        out["second_refused"] = True
        red._reset()
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("wire,tol", [(None, 1e-6), ("bf16", 1e-2)])
def test_overlapped_reducer_two_ranks(wire, tol):
    """bf16 wire: every value is rounded to 8 bits of mantissa before the sum (rel. error <= 2^-9 each) and the sum is
    rounded again: rel-L2 of the result <= 1e-2 (measured ~3e-3); the fp32 wire reproduces the plain sum."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_overlap_worker, args=(r, world, port, wire, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for _, out in res:
        for case in ("adopted", "copied", "accumulated", "param_fresh", "param_inplace", "param_accumulate"):
            assert out[case][0] and out[case][1] <= tol, (case, out[case])
        assert out["adopted"][2] and out["param_fresh"][2] and out["param_inplace"][2]
        if wire is None:
            assert out["cast"][0] and out["cast"][1] <= 1e-6, out["cast"]
        assert not out["unseen"][0] and out["unseen"][1] <= 1e-6  # the plain path is always the exact fp32 reduction
        assert out["second_refused"]


def _union_worker(rank, world, port, q):
    """rows="union": every rank's gradient is non-zero in its own subset of rows; the reducer is handed the row mask
    first (RasterContext.grad_rows_hook), exchanges only the union's rows and must reproduce the plain sum exactly."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gags_amd import rasterization
    from gags_amd.dist import OverlappedGradReducer
    n, d = 1001, 256
    masks = [torch.rand(n, generator=torch.Generator().manual_seed(40 + r)) < 0.2 for r in range(world)]
    grads = [torch.randn(n, d, generator=torch.Generator().manual_seed(7 + r)) * masks[r][:, None] for r in range(world)]
    expect = sum(grads)
    union = int(torch.stack(masks).any(0).sum())
    grad = grads[rank].clone()
    red = OverlappedGradReducer(mode="rs_ag", bucket_bytes=8192)
    with red:
        assert rasterization.default_context().grad_rows_hook is not None
        rasterization.default_context().grad_rows_hook(masks[rank].to(torch.uint8))
        for c0 in range(0, d, 128):
            rasterization.default_context().grad_range_hook(grad.detach(), c0, c0 + 128)
    assert rasterization.default_context().grad_rows_hook is None
    used = red.finish(grad)
    ok = torch.equal(grad, expect) if world == 2 else bool(((grad - expect).abs() <= 1e-6 * expect.abs().max()).all())
    q.put((rank, used, bool(ok), red.rows_exchanged, union))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_overlapped_reducer_exchanges_only_the_union_of_nonzero_rows(world):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_union_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for _, used, exact, rows, union in res:
        assert used and exact           # (three ranks: every rank adds the same shards in the same order)
        assert rows == union and union < 1001


def _geometry_worker(rank, world, port, q):
    """reduce_geometry_grads: the four geometry gradients travel as ONE packed [N,11] block and come back as
    the exact sum; frozen parameters are left alone; a rank whose view produced no gradient contributes zeros."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import gags_amd.dist as D
    n = 517
    shapes = {"_xyz": (n, 3), "_rotation": (n, 4), "_scaling": (n, 3), "_opacity": (n, 1)}

    class PC:
        pass

    def grads_of(r):
        g = torch.Generator().manual_seed(900 + r)
        return {k: torch.randn(*s, generator=g) for k, s in shapes.items()}

    pc = PC()
    for k, s in shapes.items():
        setattr(pc, k, torch.nn.Parameter(torch.zeros(*s)))
    mine = grads_of(rank)
    for k in shapes:
        getattr(pc, k).grad = mine[k].clone()
    pc._scaling.requires_grad_(False)          # frozen: must not be touched
    if rank == 1:
        pc._opacity.grad = None                # this rank's view blended nothing
    calls = []
    real = D.reduce_feature_grad
    D.reduce_feature_grad = lambda g, **kw: (calls.append(tuple(g.shape)), real(g, **kw))[1]
    done = D.reduce_geometry_grads(pc, mode="rs_ag")
    D.reduce_feature_grad = real
    expect = {k: sum(grads_of(r)[k] for r in range(world)) for k in shapes}
    expect["_opacity"] = sum(grads_of(r)["_opacity"] for r in range(world) if r != 1)
    ok = done == ["_xyz", "_rotation", "_opacity"] and calls == [(n, 8)]
    for k in done:
        ok = ok and torch.equal(getattr(pc, k).grad, expect[k])
    ok = ok and torch.equal(pc._scaling.grad, mine["_scaling"])
    q.put((rank, bool(ok)))
    dist.barrier()
    dist.destroy_process_group()


def test_geometry_gradients_reduce_as_one_packed_block_two_ranks():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_geometry_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok in res)


def _kept_backward(ctx, n, d, rows, values):
    """What the staged colours-only backward does with the persistent gradient buffer (raster_context._KeptGrad), on the host:
    the rows this view has are written, the rows flagged by the previous step and absent now are zeroed, no other row is
    touched, the flags are recorded for the next step -- all through `.data`, as the kernels write through raw pointers."""
    alias, prev, cur = ctx.kept_grad(n, d, torch.float32, torch.device("cpu"))
    hit = torch.zeros(n, dtype=torch.bool)
    hit[rows] = True
    alias.data[(prev != 0) & ~hit] = 0
    alias.data[rows] = values
    cur.data.copy_(hit.to(torch.uint8))
    return alias


def _two_step_worker(rank, world, port, mode, bucket_bytes, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gags_amd.dist import reduce_feature_grad
    from gags_amd.rasterization import RasterContext
    n, d = 1037, 7  # (7259 elements: odd, so the reduce-scatter buckets leave a tail for the plain all-reduce)
    ctx = RasterContext()
    assert ctx.keep_grad_buffer
    ok, ptrs = [], set()
    for step in range(3):
        local = []
        for r in range(world):  # rows and values of every rank's view this step: different rows every step and rank
            g = torch.Generator().manual_seed(1000 * step + r)
            rows = torch.randperm(n, generator=g)[:200]
            local.append((rows, torch.randn(200, d, generator=g)))
        expect = torch.zeros(n, d)
        for rows, values in local:
            expect[rows] += values
        grad = _kept_backward(ctx, n, d, *local[rank])
        ptrs.add(grad.data_ptr())
        reduce_feature_grad(grad, mode=mode, bucket_bytes=bucket_bytes)
        ok.append(bool(torch.allclose(grad, expect, rtol=1e-6, atol=1e-6)))
        del grad  # (zero_grad(set_to_none=True): the buffer's only other holder lets go)
    q.put((rank, ok, len(ptrs), dict(ctx._kept_fails)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode,bucket_bytes", [("allreduce", 4096), ("rs_ag", 4096), ("rs_ag", 256 << 20)])
def test_reduction_into_the_kept_buffer_over_three_steps(mode, bucket_bytes):
    """reduce_feature_grad writes the other ranks' rows into the very buffer the next backward reuses, and c10d's
    collectives do not move torch's version counter: the reduction itself must tell the buffer (rasterization.grad_written),
    or rows of step 1's other rank are summed again in step 2.  Host tensors and a host restatement of the keep kernel's
    protocol (gloo cannot reduce-scatter device tensors); both bucketed forms of rs_ag and its ragged tail, and allreduce.
    The buffer stays in use (wiped, not replaced) and no step counts towards the switch-off."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_two_step_worker, args=(r, world, port, mode, bucket_bytes, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok, n_ptrs, fails in res:
        assert ok == [True, True, True], (rank, ok)
        assert n_ptrs == 1 and all(v == 0 for v in fails.values()), (rank, n_ptrs, fails)
