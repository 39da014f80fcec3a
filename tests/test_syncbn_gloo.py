"""Host logic of the statistics exchange of the fused norm groups (ops._bn_group_fwd / _bn_group_bwd) at world size 2
on gloo, without a GPU: the HIP kernels are replaced by oracle/bn_ref.FakeLib (float64 stand-ins on the same pointers),
everything else — buffer layout, channel offsets, ONE all_gather forward and ONE all_reduce backward per group, local
parameter gradients — is the product's code.  Reference: plain float64 batch norm over the whole batch, which is what
nn.SyncBatchNorm computes (train_segmentation.py:128 converts every norm of the reference's models).

Three routes through the same host code, each against the same reference and tolerance: the whole group in one launch per
phase, its norms one by one (ops.BN_GROUP_LAUNCH off), and a join of nine norms (more than a launch holds: one by one too) —
the buffers and the ONE collective per direction belong to the group, whatever the launches are."""
import os
import socket

import pytest
import torch


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ref_bn(x, w, b, eps, relu):
    mean = x.mean(dim=(0, 2), keepdim=True)
    var = x.var(dim=(0, 2), unbiased=False, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * w[None, :, None] + b[None, :, None]
    return torch.relu(y) if relu else y


def _worker(rank, world, port, q, route):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cloud_transformers_amd import _lib, ops
        from oracle.bn_ref import FakeLib
        fake = FakeLib()
        _lib.load = lambda: fake                     # the HIP kernels' stand-ins (CPU, float64 inside)
        _lib.check = lambda status, what: None if status == 0 else (_ for _ in ()).throw(RuntimeError(what))
        ops._dev = lambda *t: None                   # (the product refuses CPU tensors; this test is about the host logic)
        ops._stream = lambda: None
        if route == "one_by_one":
            ops.BN_GROUP_LAUNCH = False
        calls = []                                   # (entry point, n, first, run) of every exchange-phase launch
        for name in ("ct_bn_group_stats_fwd", "ct_bn_group_apply_fwd", "ct_bn_group_reduce_bwd", "ct_bn_group_apply_bwd"):
            def spy(items, n, first, run, *rest, _f=getattr(fake, name), _name=name):
                calls.append((_name, n, first, run))
                return _f(items, n, first, run, *rest)
            setattr(fake, name, spy)
        g = torch.Generator().manual_seed(11)
        # ragged shards: rank 0 holds 1 cloud, rank 1 holds 3 (counts differ: the merge must weight by count)
        shards = [slice(0, 1), slice(1, 4)]
        Bg, N = 4, 64
        sl = shards[rank]
        Ck, Cv = 6, 10
        xg = torch.randn(Bg, Ck + Cv, N, generator=g) * 2 + 0.5
        cot = torch.randn(Bg, Ck + Cv, N, generator=g)

        def sbn(C, seed):
            torch.manual_seed(seed)
            m = torch.nn.SyncBatchNorm(C)
            with torch.no_grad():
                m.weight.copy_(torch.rand(C) + 0.5)
                m.bias.copy_(torch.randn(C) * 0.1)
            return m.train()

        # the join's norms on channel ranges of cat([a, b]): the two halves, or nine ranges (more than one launch holds)
        sizes = [1, 2, 3, 1, 1, 2, 2, 2, 2] if route == "nine" else [Ck, Cv]
        bk, bv = sbn(Ck, 1), sbn(Cv, 2)
        js = [sbn(C, 3 + i) for i, C in enumerate(sizes)]
        ja = js[0]
        assert ops._sync_group(bk) is not None
        before = ops.sync_stats_collectives()
        x = xg[sl].clone().requires_grad_(True)
        a, b = ops.split_bn(x, bk, bv)
        mid, split_calls = ops.sync_stats_collectives(), len(calls)
        y = ops.join_bn_relu(list(torch.cat([a, b], dim=1).split(sizes, dim=1)), js)
        (y * cot[sl]).sum().backward()
        ncoll = ops.sync_stats_collectives() - before
        # reference on the whole batch in float64
        xr = xg.double().clone().requires_grad_(True)
        P = {m: (m.weight.detach().double().requires_grad_(True), m.bias.detach().double().requires_grad_(True)) for m in [bk, bv] + js}
        ar = _ref_bn(xr[:, :Ck], *P[bk], bk.eps, False)
        br = _ref_bn(xr[:, Ck:], *P[bv], bv.eps, False)
        yr = torch.cat([_ref_bn(p, *P[m], m.eps, True) for p, m in zip(torch.cat([ar, br], dim=1).split(sizes, dim=1), js)], dim=1)
        (yr * cot.double()).sum().backward()
        res = {"y": float((y.detach().double() - yr.detach()[sl]).abs().max()),
               "gx": float((x.grad.double() - xr.grad[sl]).abs().max()),
               "collectives": ncoll, "after_split": mid - before,
               "join_runs": [c[1:] for c in calls[split_calls:] if c[0] == "ct_bn_group_stats_fwd"],
               "phases": sorted({c[0] for c in calls})}
        # parameter gradients are this rank's share; summed over the ranks they are the whole batch's
        for name, m in (("bk", bk), ("ja", ja)):
            gw = m.weight.grad.detach().clone()
            dist.all_reduce(gw)
            res["gw_" + name] = float((gw.double() - P[m][0].grad).abs().max())
        M = Bg * N
        res["running_var"] = float((bk.running_var.double() - (0.9 + 0.1 * xg[:, :Ck].double().var(dim=(0, 2), unbiased=False) * M / (M - 1))).abs().max())
        res["nbt"] = int(bk.num_batches_tracked)
        q.put((rank, res))
    finally:
        dist.barrier()
        dist.destroy_process_group()


def _exchange_at_world_size_2(route):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, route)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=150) for _ in range(world))
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    for rank in range(world):
        r = got[rank]
        assert r["y"] <= 1e-5 and r["gx"] <= 1e-5, r
        assert r["gw_bk"] <= 1e-4 and r["gw_ja"] <= 1e-4, r
        assert r["running_var"] <= 1e-5 and r["nbt"] == 1, r
        assert r["after_split"] == 1                # two norms, one all_gather
        assert r["collectives"] == 4                # (split_bn + join_bn_relu) x (forward gather + backward reduce)
        # the launches of the join's statistics phase: the whole table once, or every norm of it in turn
        n = 9 if route == "nine" else 2
        assert r["join_runs"] == ([(n, 0, n)] if route == "group" else [(n, i, 1) for i in range(n)]), r
        assert len(r["phases"]) == 4


@pytest.mark.timeout(180)
def test_norm_group_statistics_exchange_world_size_2():
    _exchange_at_world_size_2("group")


@pytest.mark.timeout(180)
@pytest.mark.parametrize("route", ["one_by_one", "nine"])
def test_norm_group_statistics_exchange_one_norm_per_launch(route):
    """The same comparison with the group's norms launched one by one: the switch off, and nine norms in the join."""
    _exchange_at_world_size_2(route)
