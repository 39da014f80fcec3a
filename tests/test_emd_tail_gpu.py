"""ct_emd_fwd_tail / emd_with_info on the GPU: dist and assignment bit for bit those of the existing calls (and of
oracle/emd_ref.c where it is affordable) wherever a cloud enters the tail kernel — at the first check, midway, never — with
`info` against the numpy restatement (tests/emd_tail_ref.py); ragged batches, GetMax ties, one and sixteen targets per
thread, the gradient, no host synchronisation, graph replay with other clouds and counts, and the refusals."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import emd_ref
from tests import emd_tail_ref as R
from tests.emd_counts_cases import batch

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module", autouse=True)
def _stream_pool():
    """The graph test here creates a side stream; the pool's round robin is left where the suite before this module had it."""
    from tests.stream_pool import neutral_stream_pool
    with neutral_stream_pool():
        yield


U_CAP = 2048                    # the longest list the tail kernel can take (ct_debug_set_emd_tail clamps to it)


@contextlib.contextmanager
def tail_hook(u_tail, every):
    from cloud_transformers_amd import _lib
    lib = _lib.load()
    lib.ct_debug_set_emd_tail(u_tail, every)
    try:
        yield
    finally:
        lib.ct_debug_set_emd_tail(-1, 0)


# how a cloud meets the tail kernel: (u_tail, every, tail_from as a function of iters)
ENTRIES = {
    "first_check": (U_CAP, 1, lambda iters: 0),            # taken at the first launch that finds at most 2048 bidders
    "midway": (64, 7, lambda iters: 10),                   # the defaults' regime: a few dozen bidders, some checks decline
    "declined": (0, 5, lambda iters: 3),                   # tail launches that never take a cloud with a bidder
    "never": (U_CAP, 1, lambda iters: iters),              # no tail launch at all: the ordinary iterations alone
}


def _cuda(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _run(a, b, eps, iters, entry, count=None):
    from cloud_transformers_amd.emd import emd_with_info
    u, every, tf = ENTRIES[entry]
    with tail_hook(u, every):
        return emd_with_info(a, b, eps, iters, count=count, tail_from=tf(iters))


@pytest.fixture(scope="module")
def clouds():
    """The uniform batches of the entry tests, their existing-call results and the restatement's bidder counts, once."""
    from cloud_transformers_amd.emd import emd_distance
    out = {}
    for B, n, eps, seed in ((2, 1024, 0.005, 11), (3, 2048, 0.004, 12)):
        a, b = R.uniform_pair(n, seed, B)
        ac, bc = _cuda(a, b)
        out[n] = dict(a=a, b=b, ac=ac, bc=bc, eps=eps, B=B, last30=[R.auction(a[k], b[k], eps, 30)[2][-1] for k in range(B)])
    return out


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("n,iters", [(1024, 300), (2048, 200)])
def test_entry_point_of_the_tail(clouds, n, iters, entry):
    from cloud_transformers_amd.emd import emd_distance
    c = clouds[n]
    d0, a0 = emd_distance(c["ac"], c["bc"], c["eps"], iters)
    d, a, info = _run(c["ac"], c["bc"], c["eps"], iters, entry)
    assert torch.equal(a, a0) and torch.equal(d, d0)
    if n == 1024:
        st, d_ref, a_ref = emd_ref.forward(c["a"], c["b"], c["eps"], iters)
        assert np.array_equal(a.cpu().numpy(), a_ref) and np.array_equal(d.cpu().numpy(), d_ref)
    info = info.cpu().numpy()
    # an unfinished auction leaves unassigned bidders to the last iteration, a finished one none
    assert np.all((info[:, 1] == 0) == (info[:, 0] < iters)) and np.all(info[:, 0] <= iters) and np.all(info[:, 1] >= 0)
    ref = _run(c["ac"], c["bc"], c["eps"], iters, "never")[2].cpu().numpy()
    assert np.array_equal(info, ref)


@pytest.mark.parametrize("entry", ["first_check", "midway", "never"])
@pytest.mark.parametrize("n", [1024, 2048])
def test_forced_last_iteration_inside_the_tail(clouds, n, entry):
    from cloud_transformers_amd.emd import emd_distance
    c, iters = clouds[n], 30
    d0, a0 = emd_distance(c["ac"], c["bc"], c["eps"], iters)
    d, a, info = _run(c["ac"], c["bc"], c["eps"], iters, entry)
    assert torch.equal(a, a0) and torch.equal(d, d0)
    assert info.cpu().tolist() == [[iters, u] for u in c["last30"]] and min(c["last30"]) > 0


@pytest.mark.parametrize("iters,tail_from", [(1, 0), (1, 5), (7, 7), (7, 100), (2, 0)])
def test_tail_never_reached_still_reports(clouds, iters, tail_from):
    from cloud_transformers_amd.emd import emd_distance, emd_with_info
    c = clouds[1024]
    d0, a0 = emd_distance(c["ac"], c["bc"], c["eps"], iters)
    with tail_hook(U_CAP, 1):
        d, a, info = emd_with_info(c["ac"], c["bc"], c["eps"], iters, tail_from=tail_from)
    assert torch.equal(a, a0) and torch.equal(d, d0)
    want = [[iters, R.auction(c["a"][k], c["b"][k], c["eps"], iters)[2][-1]] for k in range(c["B"])]
    assert info.cpu().tolist() == want
    if iters == 1:
        assert want == [[1, 1024], [1, 1024]]


@pytest.mark.parametrize("entry", ["first_check", "midway"])
def test_mixed_batch_one_cloud_finishes(entry):
    """seed 2 at eps 0.05 finishes at iteration 199, seed 0 needs 698: at iters = 400 one cloud of the batch is over, its rows
    those of a run of 199 iterations, and the other is force-assigned."""
    from cloud_transformers_amd.emd import emd_distance
    a2, b2 = R.uniform_pair(1024, 2)
    a0, b0 = R.uniform_pair(1024, 0)
    a, b = np.concatenate([a2, a0]), np.concatenate([b2, b0])
    ac, bc = _cuda(a, b)
    d, ass, info = _run(ac, bc, 0.05, 400, entry)
    u = R.auction(a0[0], b0[0], 0.05, 400)[2][-1]
    assert u > 0 and info.cpu().tolist() == [[199, 0], [400, u]]
    d0, as0 = emd_distance(ac, bc, 0.05, 400)
    assert torch.equal(ass, as0) and torch.equal(d, d0)
    d199, as199 = emd_distance(ac[:1], bc[:1], 0.05, 199)
    assert torch.equal(ass[0], as199[0]) and torch.equal(d[0], d199[0])
    assert ass[0].unique().numel() == 1024


def test_sixteen_targets_per_thread_and_the_batching_loop():
    """n = 16384: sixteen targets in every thread's registers; entry forced as soon as a cloud is down to 2048 bidders, which the
    tail then takes a batch at a time.  (n = 1024, one target per thread: the tests above.)"""
    from cloud_transformers_amd.emd import emd_distance
    B, n, iters = 2, 16384, 12
    a, b = R.uniform_pair(n, 77, B)
    ac, bc = _cuda(a, b)
    d0, a0 = emd_distance(ac, bc, 0.005, iters)
    d, ass, info = _run(ac, bc, 0.005, iters, "first_check")
    assert torch.equal(ass, a0) and torch.equal(d, d0)
    st, d_ref, a_ref = emd_ref.forward(a, b, 0.005, iters)
    assert st == 1 and np.array_equal(ass.cpu().numpy(), a_ref) and np.array_equal(d.cpu().numpy(), d_ref)
    info = info.cpu().numpy()
    assert np.all(info[:, 0] == iters) and np.all(info[:, 1] > 100) and np.all(info[:, 1] <= U_CAP)     # the tail did take them
    # eight and four targets per thread as well, against the existing call
    for n2 in (8192, 4096):
        x, y = _cuda(*R.uniform_pair(n2, 78, 1))
        d0, a0 = emd_distance(x, y, 0.005, 15)
        d, ass, _ = _run(x, y, 0.005, 15, "first_check")
        assert torch.equal(ass, a0) and torch.equal(d, d0)


@pytest.mark.parametrize("seed", [30, 31])
def test_getmax_ties_inside_the_tail(seed):
    from cloud_transformers_amd.emd import emd_distance
    from tests.test_emd_gpu import _collapsed
    a, b = _collapsed(2, 4096, seed)
    ac, bc = _cuda(a, b)
    d0, a0 = emd_distance(ac, bc, 0.005, 25)
    st, d_ref, a_ref = emd_ref.forward(a, b, 0.005, 25)
    assert st == 1 and emd_ref.last_getmax_ties() > 0
    for it0 in (0, 6):                                        # every point twice: thousands of bidders, 2048 after a few rounds
        with tail_hook(U_CAP, 1):
            from cloud_transformers_amd.emd import emd_with_info
            d, ass, info = emd_with_info(ac, bc, 0.005, 25, tail_from=it0)
        assert torch.equal(ass, a0) and torch.equal(d, d0)
        assert np.array_equal(ass.cpu().numpy(), a_ref) and np.array_equal(d.cpu().numpy(), d_ref)
        assert int(info[:, 1].min()) > 0 and int(info[:, 1].max()) <= U_CAP and info[:, 0].tolist() == [25, 25]


RAGGED_COUNTS = [1500, 1025, 1024, 700, 2, 1, 0]


@pytest.mark.parametrize("entry", ["first_check", "midway", "never"])
def test_ragged_batch(entry):
    from cloud_transformers_amd.emd import emd_with_counts
    n, eps, iters = 1500, 0.005, 40
    x1, x2, refs = batch(n, RAGGED_COUNTS, 40, eps, iters)
    ac, bc = _cuda(x1, x2)
    ac.requires_grad_(True)
    cnt = torch.tensor(RAGGED_COUNTS, dtype=torch.int32, device="cuda")
    d0, a0 = emd_with_counts(ac.detach(), bc, eps, iters, cnt)
    d, ass, info = _run(ac, bc, eps, iters, entry, count=cnt)
    assert torch.equal(ass, a0) and torch.equal(d.detach(), d0)
    dn, an = d.detach().cpu().numpy(), ass.cpu().numpy()
    for k, c in enumerate(RAGGED_COUNTS):
        if refs[k] is not None:
            assert np.array_equal(an[k, :c], refs[k][1]) and np.array_equal(dn[k, :c], refs[k][0]), k
        assert np.all(an[k, c:] == -1) and np.all(dn[k, c:] == 0.0)
    info = info.cpu().numpy()
    assert info[6].tolist() == [0, 0]
    assert info[5].tolist() == [1, 0]                         # one row: assigned in iteration 0, nothing left at iteration 1
    assert np.all((info[:, 1] == 0) == (info[:, 0] < iters))
    (d * torch.rand_like(d)).sum().backward()
    g = ac.grad.cpu().numpy()
    for k, c in enumerate(RAGGED_COUNTS):
        assert np.all(g[k, c:] == 0.0) and not np.signbit(g[k, c:]).any() and np.isfinite(g[k, :c]).all()


@pytest.mark.parametrize("ragged", [False, True])
def test_gradient_equals_the_existing_call(ragged):
    from cloud_transformers_amd.emd import emd_distance, emd_with_info
    n = 1100 if ragged else 1024
    a, b = _cuda(*R.uniform_pair(n, 5, 2))
    cnt = torch.tensor([1100, 900], dtype=torch.int32, device="cuda") if ragged else None
    g = torch.rand(2, n, device="cuda")
    grads = []
    for fn in (lambda x: emd_distance(x, b, 0.005, 60, cnt)[0], lambda x: emd_with_info(x, b, 0.005, 60, count=cnt, tail_from=8)[0],
               lambda x: emd_distance(x, b, 0.005, 60, cnt, tail=True)[0]):
        x = a.clone().requires_grad_(True)
        with tail_hook(U_CAP, 4):
            (fn(x) * g).sum().backward()
        grads.append(x.grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2]) and float(grads[0].abs().max()) > 0


def test_no_synchronisation_and_graph_replay():
    from cloud_transformers_amd.emd import emd_with_counts, emd_with_info
    n, eps, iters = 1300, 0.005, 80
    sets = []
    for seed, counts in ((50, [1300, 640, 1]), (51, [7, 1300, 1024]), (52, [0, 1025, 300])):
        x1, x2, _ = batch(n, counts, seed, eps, 1)
        sets.append(_cuda(x1, x2) + [torch.tensor(counts, dtype=torch.int32, device="cuda")])
    eager = [emd_with_counts(a, b, eps, iters, c) for a, b, c in sets]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with tail_hook(64, 4):
            d, ass, info = emd_with_info(sets[0][0], sets[0][1], eps, iters, count=sets[0][2], tail_from=6)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(ass, eager[0][1]) and torch.equal(d, eager[0][0])
    info0 = info.clone()
    sa, sb, sc = (t.clone() for t in sets[0])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with tail_hook(64, 4), torch.cuda.stream(stream):
        emd_with_info(sa, sb, eps, iters, count=sc, tail_from=6)                 # warm-up outside the capture
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            gd, ga, gi = emd_with_info(sa, sb, eps, iters, count=sc, tail_from=6)
    torch.cuda.current_stream().wait_stream(stream)
    for k in (1, 2, 0):
        sa.copy_(sets[k][0]); sb.copy_(sets[k][1]); sc.copy_(sets[k][2])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ga, eager[k][1]) and torch.equal(gd, eager[k][0]), k
        with tail_hook(64, 4):
            assert torch.equal(gi, emd_with_info(sets[k][0], sets[k][1], eps, iters, count=sets[k][2], tail_from=6)[2])
    assert torch.equal(gi, info0)


def test_preconditions_are_refused_before_any_launch():
    from cloud_transformers_amd import _lib
    from cloud_transformers_amd.emd import emd_with_info, emd_distance
    lib = _lib.load()
    buf = torch.zeros(1 << 22, device="cuda", dtype=torch.uint8)
    p, nb = buf.data_ptr(), 1 << 22
    ok = (p, p, None, p, p, p, p, nb, 1, 1024, 0.005, 5, -1, None)
    for i in (0, 1, 3, 4, 6):                                                    # each required pointer
        args = list(ok)
        args[i] = None
        assert lib.ct_emd_fwd_tail(*args) == -1                                  # CT_EINVAL
    assert lib.ct_emd_fwd_tail(p, p, None, p, p, p, p, nb, 1, 1024, 0.005, 0, -1, None) == -1
    assert lib.ct_emd_fwd_tail(p, p, None, p, p, p, p, nb, 1, 16385, 0.005, 5, -1, None) == -1       # a shape the query declines
    assert lib.ct_emd_fwd_tail(p, p, None, p, p, p, p, nb, 513, 8, 0.005, 5, -1, None) == -4         # CT_EPRECOND
    assert lib.ct_emd_fwd_tail(p, p, None, p, p, p, p, lib.ct_emd_tail_workspace_bytes(1, 1024) - 1, 1, 1024, 0.005, 5, -1, None) == -3
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0                                                   # nothing was launched
    x = torch.rand(1, 16500, 3, device="cuda")
    with pytest.raises(ValueError):
        emd_with_info(x, x, 0.005, 2)
    d0, a0 = emd_distance(x, x, 0.005, 2)                                        # tail=True falls back where unsupported
    d1, a1 = emd_distance(x, x, 0.005, 2, tail=True)
    assert torch.equal(a0, a1) and torch.equal(d0, d1)
