"""The auction EMD for any cloud size and per-cloud counts (ct_emd_fwd_counts / ct_emd_bwd_counts) against oracle/emd_ref.c
through the far padding of tests/emd_counts_cases.py, and against the dense entry points where a count is a multiple of 1024.
Assignments are compared exactly and squared distances bit for bit throughout; only the gradients against the oracle's
backward (another multiplication order) and the loss (another summation order) carry a tolerance."""
import numpy as np
import pytest
import torch

from oracle import emd_ref
from tests.emd_counts_cases import batch, case

pytestmark = pytest.mark.gpu

EPS, ITERS = 0.005, 30
RAGGED = {"wide": (2500, (2500, 1024, 700, 0)), "narrow": (2100, (1, 2, 1025, 2047))}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _run(x1, x2, eps, iters, counts=None, g=None):
    """emd_with_counts on numpy clouds -> (dist, assignment, grad of xyz1 for the upstream gradient g or None) as numpy."""
    from cloud_transformers_amd.emd import emd_with_counts
    a = torch.from_numpy(np.array(x1)).cuda().requires_grad_(g is not None)       # (copies: the shared references are read-only)
    b = torch.from_numpy(np.array(x2)).cuda()
    cnt = None if counts is None else torch.tensor(list(counts), dtype=torch.int32, device="cuda")
    dist, ass = emd_with_counts(a, b, eps, iters, cnt)
    assert dist.shape == x1.shape[:2] and dist.dtype == torch.float32
    assert ass.shape == x1.shape[:2] and ass.dtype == torch.int32
    grad = None
    if g is not None:
        dist.backward(torch.from_numpy(g).cuda())
        grad = a.grad.cpu().numpy()
    return dist.detach().cpu().numpy(), ass.cpu().numpy(), grad


def _check_cloud(dist, ass, ref, c):
    """rows [0, c) are the oracle's, rows at or beyond c are padding"""
    d_ref, a_ref = ref
    assert np.array_equal(ass[:c], a_ref), float((ass[:c] == a_ref).mean())
    assert np.array_equal(_bits(dist[:c]), _bits(d_ref))
    assert np.all(ass[c:] == -1) and np.all(_bits(dist[c:]) == 0)


@pytest.mark.parametrize("B,n,eps,iters", [(2, 1500, 0.005, 30),      # one full tile and a partial one
                                           (1, 700, 0.004, 300), (1, 63, 0.004, 300),      # a single partial tile
                                           (1, 1025, 0.005, 20), (1, 1023, 0.005, 20),
                                           (1, 1500, 0.005, 1)])       # forced assignment at once
def test_any_n_without_counts(B, n, eps, iters):
    cases = [case(n, 100 + n + k, eps, iters) for k in range(B)]
    x1, x2 = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    g = np.random.default_rng(n).random((B, n), dtype=np.float32)
    dist, ass, grad = _run(x1, x2, eps, iters, None, g)
    for k in range(B):
        _check_cloud(dist[k], ass[k], cases[k][2:], n)
    np.testing.assert_allclose(grad, emd_ref.backward(x1, x2, g, ass), atol=1e-6)


@pytest.mark.parametrize("name", sorted(RAGGED))
def test_ragged_batch(name):
    n, counts = RAGGED[name]
    x1, x2, refs = batch(n, counts, 500, EPS, ITERS)
    rng = np.random.default_rng(7)
    g = rng.random((len(counts), n), dtype=np.float32)
    for k, c in enumerate(counts):
        g[k, c:] = np.nan
    dist, ass, grad = _run(x1, x2, EPS, ITERS, counts, g)
    for k, c in enumerate(counts):
        if c >= 2:
            _check_cloud(dist[k], ass[k], refs[k], c)
        else:
            assert np.all(ass[k, c:] == -1) and np.all(_bits(dist[k, c:]) == 0)
            if c == 1:
                d = x1[k, 0] - x2[k, 0]
                assert ass[k, 0] == 0
                assert _bits(dist[k, :1])[0] == _bits(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        # backward: the oracle's on the kept rows, an exact +0.0 (sign bit clear) beyond, whatever g_dist holds there
        assert np.all(_bits(grad[k, c:]) == 0)
        if c:
            want = emd_ref.backward(x1[k:k + 1, :c], x2[k:k + 1, :c], g[k:k + 1, :c], ass[k:k + 1, :c])
            np.testing.assert_allclose(grad[k:k + 1, :c], want, atol=1e-6)
    assert not np.isnan(grad).any() and not np.isnan(dist).any()


def test_counts_that_are_multiples_of_1024_give_the_dense_kernels_bits():
    from cloud_transformers_amd.emd import emd_with_counts, emdModule
    n, counts = 3000, (1024, 2048, 3000)
    rng = np.random.default_rng(11)
    x1, x2 = rng.random((3, n, 3), dtype=np.float32), rng.random((3, n, 3), dtype=np.float32)
    for k, c in enumerate(counts):
        x1[k, c:], x2[k, c:] = np.nan, np.nan
    a, b = torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda()
    dist, ass = emd_with_counts(a, b, EPS, ITERS, torch.tensor(counts, dtype=torch.int32, device="cuda"))
    for k, c in enumerate(counts[:2]):
        d_alone, a_alone = emdModule()(a[k:k + 1, :c].contiguous(), b[k:k + 1, :c].contiguous(), EPS, ITERS)
        assert torch.equal(ass[k, :c], a_alone[0])
        assert torch.equal(dist[k, :c].view(torch.int32), d_alone[0].view(torch.int32))
        assert bool((ass[k, c:] == -1).all()) and bool((dist[k, c:].view(torch.int32) == 0).all())
    assert int(ass[2].min()) >= 0 and int(ass[2].max()) < n
    # no count, n a multiple of 1024: the dense entry itself
    a2, b2 = torch.from_numpy(rng.random((2, 2048, 3), dtype=np.float32)).cuda(), torch.from_numpy(rng.random((2, 2048, 3), dtype=np.float32)).cuda()
    d_c, a_c = emd_with_counts(a2, b2, EPS, ITERS)
    d_d, a_d = emdModule()(a2, b2, EPS, ITERS)
    assert torch.equal(a_c, a_d) and torch.equal(d_c.view(torch.int32), d_d.view(torch.int32))
    # ... and the ragged kernels with every row counted agree with it as well
    d_r, a_r = emd_with_counts(a2, b2, EPS, ITERS, torch.full((2,), 2048, dtype=torch.int32, device="cuda"))
    assert torch.equal(a_r, a_d) and torch.equal(d_r.view(torch.int32), d_d.view(torch.int32))


def test_update_slow_path_with_a_ragged_extent():
    """n = 9000: more than 8192 list entries in the first iterations, so the update's GetMax / Assign passes and its
    scan-based compaction run with an extent that is no multiple of 1024"""
    a, b, d_ref, a_ref = case(9000, 900, 0.005, 4)
    dist, ass, _ = _run(a[None], b[None], 0.005, 4)
    _check_cloud(dist[0], ass[0], (d_ref, a_ref), 9000)


@pytest.mark.parametrize("kind,eps,iters,seed", [("uniform", 1.0, 200, 41),      # prices in the hundreds: the filter switches itself off
                                                 ("collapsed", 0.005, 25, 42)])  # hundreds of bidders to the end, exact ties
def test_filter_off_and_collapsed_clouds(kind, eps, iters, seed):
    a, b, d_ref, a_ref = case(1500, seed, eps, iters, kind)
    dist, ass, _ = _run(a[None], b[None], eps, iters)
    _check_cloud(dist[0], ass[0], (d_ref, a_ref), 1500)


def test_loss_and_module_with_counts():
    from cloud_transformers_amd.emd import emd_with_counts, emdModule, loss_emd_counts
    n, counts = RAGGED["wide"]
    counts = counts[:3]                                            # (the zero-count cloud makes the loss NaN, as documented)
    x1, x2, _ = batch(n, RAGGED["wide"][1], 500, EPS, ITERS)
    x1, x2 = x1[:3], x2[:3]
    a = torch.from_numpy(x1).cuda()
    b = torch.from_numpy(x2).cuda()
    cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    pc1 = a.permute(0, 2, 1)[:, :, None].contiguous().requires_grad_(True)     # [B, 3, 1, N], as the training scripts hold clouds
    pc2 = b.permute(0, 2, 1)[:, :, None].contiguous()
    loss = loss_emd_counts(pc1, pc2, EPS, ITERS, cnt)
    # per pair alone: the dense entry where the count is a multiple of 1024, the counts entry on the cut tensors otherwise
    means = []
    for k, c in enumerate(counts):
        d_alone, _ = emd_with_counts(a[k:k + 1, :c].contiguous(), b[k:k + 1, :c].contiguous(), EPS, ITERS)
        means.append(float(d_alone.double().sqrt().mean()))
    # float32 sums of at most 2500 roots against float64 ones: a relative 2500 * 2^-24 = 1.5e-4 at the very worst
    assert abs(loss.item() - float(np.mean(means))) <= 1.5e-4 * float(np.mean(means))
    loss.backward()
    g = pc1.grad[:, :, 0].permute(0, 2, 1).cpu().numpy()
    assert np.isfinite(g).all()
    for k, c in enumerate(counts):
        assert np.all(g[k, c:] == 0.0)
        assert np.abs(g[k, :c]).max() > 0
    d_m, a_m = emdModule()(a, b, EPS, ITERS, cnt)
    d_f, a_f = emd_with_counts(a, b, EPS, ITERS, cnt)
    assert torch.equal(a_m, a_f) and torch.equal(d_m.view(torch.int32), d_f.view(torch.int32))
    assert bool(torch.isnan(loss_emd_counts(pc1.detach(), pc2, EPS, ITERS, torch.tensor([5, 0, 7], dtype=torch.int32, device="cuda"))))


def test_completion_step_trains_at_a_cloud_size_that_is_no_multiple_of_1024(tmp_path):
    """tests/test_harness_gpu.py's completion step with clouds of 1000 points: the trainer's EMD call routes to the counts
    entry (the dense one asserts n % 1024 == 0) and the step trains."""
    from cloud_transformers_amd import harness as H
    from tests.test_harness_gpu import COMPLETION
    (tmp_path / "inpainter.py").write_text("from tests.test_zoo_gpu import Inpainter as Model\n")
    cfg_path = tmp_path / "inpainting.yaml"
    cfg = COMPLETION.format(root=str(tmp_path))
    assert "num_points: 1024" in cfg
    cfg_path.write_text(cfg.replace("num_points: 1024", "num_points: 1000"))
    torch.manual_seed(0)
    tr = H.Trainer(H.load_config(cfg_path), "completion", n_classes=256, device=torch.device("cuda", 0), dataset_length=4)
    hist = tr.fit(max_iters=2)
    assert len(hist) == 2 and all(v == v and 0.0 < v < 10.0 for v in hist)


def test_graph_replays_with_new_clouds_and_new_counts():
    """The counts are read on the device: a captured call replays on whatever the static tensors hold."""
    from cloud_transformers_amd.emd import emd_with_counts
    B, n, iters = 2, 1500, 12
    rng = np.random.default_rng(5)

    def inputs(counts):
        return (torch.from_numpy(rng.random((B, n, 3), dtype=np.float32)).cuda(), torch.from_numpy(rng.random((B, n, 3), dtype=np.float32)).cuda(),
                torch.tensor(counts, dtype=torch.int32, device="cuda"))
    sa, sb, sc = inputs([1500, 700])
    # warm-up where eager work runs anyway: the op keeps no state per stream.  (No side stream on purpose: every torch.cuda.Stream()
    # moves the round robin of torch's stream pool, and tests/test_graph_replay_gpu.py compares pool-stream handles.)
    emd_with_counts(sa, sb, EPS, iters, sc)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d_s, a_s = emd_with_counts(sa, sb, EPS, iters, sc)
    for counts in ([333, 1500], [1024, 1]):
        na, nb, nc = inputs(counts)
        sa.copy_(na), sb.copy_(nb), sc.copy_(nc)
        graph.replay()
        torch.cuda.synchronize()
        d_e, a_e = emd_with_counts(na, nb, EPS, iters, nc)
        assert torch.equal(a_s, a_e) and torch.equal(d_s.view(torch.int32), d_e.view(torch.int32)), counts
        assert bool((a_s[0, counts[0]:] == -1).all()) and int(a_s[0, :counts[0]].min()) >= 0
