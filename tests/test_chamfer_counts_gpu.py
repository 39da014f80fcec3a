"""Chamfer distance of clouds of different lengths in one batch (ct_chamfer_fwd_counts / ct_chamfer_bwd_counts) and the row
compaction ct_rows_compact: against the CPU oracle and against the dense op on each pair's own rows.  Lattice coordinates make
every distance exact, so equality is torch.equal; the padding rows hold poison (copies of the cloud's own rows, or NaN)."""
import numpy as np
import pytest
import torch

from tests.chamfer_counts_cases import counts_tensor, forward_case, lattice_clouds, oracle_with_counts, poison

pytestmark = pytest.mark.gpu


def _check_forward(a, b, cnt1, cnt2, want):
    """The four outputs of chamfer_with_counts against the oracle (tails included: 0 and -1) and, per pair, against
    chamfer_with_indices on the sliced arrays at B = 1."""
    from cloud_transformers_amd.chamfer import chamfer_with_counts, chamfer_with_indices
    ac, bc = a.cuda(), b.cuda()
    d1, d2, i1, i2 = chamfer_with_counts(ac, bc, counts_tensor(cnt1), counts_tensor(cnt2))
    assert i1.dtype == torch.int32 and i2.dtype == torch.int32
    for got, ref, name in ((d1, want[0], "dist1"), (d2, want[1], "dist2"), (i1, want[2], "idx1"), (i2, want[3], "idx2")):
        assert torch.equal(got.cpu(), ref), name
    for k in range(a.shape[0]):
        c1, c2 = int(cnt1[k]), int(cnt2[k])
        assert bool((d1[k, c1:] == 0).all()) and bool((i1[k, c1:] == -1).all()), k
        assert bool((d2[k, c2:] == 0).all()) and bool((i2[k, c2:] == -1).all()), k
        if c1 == 0 or c2 == 0:
            assert bool((d1[k] == 0).all()) and bool((i1[k] == -1).all()) and bool((d2[k] == 0).all()) and bool((i2[k] == -1).all()), k
            continue
        s = chamfer_with_indices(ac[k:k + 1, :c1].contiguous(), bc[k:k + 1, :c2].contiguous())
        assert torch.equal(d1[k, :c1], s[0][0]) and torch.equal(d2[k, :c2], s[1][0]), k
        assert torch.equal(i1[k, :c1], s[2][0]) and torch.equal(i2[k, :c2], s[3][0]), k
    return d1, d2, i1, i2


def test_forward_with_counts_b4_n300_m1003():
    a, b, cnt1, cnt2, want = forward_case()
    _check_forward(a, b, cnt1, cnt2, want)


def test_forward_both_kernel_variants():
    """B64 n1024 m40: direction 1 has 64 * ceil(1024 / 256) = 256 workgroups of 256 queries (nn_kernel<4>), direction 2
    64 * ceil(40 / 256) = 64 < 256 (nn_kernel<2>)."""
    B, n, m = 64, 1024, 40
    g = torch.Generator().manual_seed(5)
    cnt1 = torch.randint(1, n + 1, (B,), generator=g).tolist()
    cnt2 = torch.randint(1, m + 1, (B,), generator=g).tolist()
    a, b = lattice_clouds(B, n, m, cnt1, cnt2, seed=6)
    _check_forward(a, b, cnt1, cnt2, oracle_with_counts(a, b, cnt1, cnt2))


@pytest.mark.parametrize("B,n,m", [(4, 300, 1003), (64, 1024, 40)])
def test_null_counts_equal_the_dense_entry_point(B, n, m):
    from cloud_transformers_amd.chamfer import chamfer_with_counts, chamfer_with_indices
    g = torch.Generator().manual_seed(B + n)
    a = (torch.randint(0, 6, (B, n, 3), generator=g).float() / 4).cuda()
    b = (torch.randint(0, 6, (B, m, 3), generator=g).float() / 4).cuda()
    dense = chamfer_with_indices(a, b)
    for c1, c2 in ((None, None), (counts_tensor([n] * B), None), (None, counts_tensor([m] * B))):
        got = chamfer_with_counts(a, b, c1, c2)
        assert all(torch.equal(x, y) for x, y in zip(got, dense))


BWD = (3, 200, 260, [200, 71, 0], [131, 260, 5])


def _bwd_inputs():
    B, n, m, cnt1, cnt2 = BWD
    g = torch.Generator().manual_seed(77)
    a = poison(torch.rand(B, n, 3, generator=g), cnt1, [True, False, False])
    b = poison(torch.rand(B, m, 3, generator=g), cnt2, [True, False, False])
    g1, g2 = torch.rand(B, n, generator=g) + 0.5, torch.rand(B, m, generator=g) + 0.5      # non-zero at the padding rows too
    return a.cuda(), b.cuda(), g1.cuda(), g2.cuda(), cnt1, cnt2


def _grads_with_counts(a, b, g1, g2, cnt1, cnt2):
    from cloud_transformers_amd.chamfer import chamfer_with_counts
    ac, bc = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    d1, d2, _, _ = chamfer_with_counts(ac, bc, counts_tensor(cnt1), counts_tensor(cnt2))
    ((d1 * g1).sum() + (d2 * g2).sum()).backward()
    return ac.grad, bc.grad


def _grads_dense_per_pair(a, b, g1, g2, cnt1, cnt2):
    """Autograd through the dense op on each pair's own rows; zeros elsewhere."""
    from cloud_transformers_amd.chamfer import chamfer_with_indices
    ga, gb = torch.zeros_like(a), torch.zeros_like(b)
    for k in range(a.shape[0]):
        c1, c2 = cnt1[k], cnt2[k]
        if c1 == 0 or c2 == 0:
            continue
        ak, bk = a[k:k + 1, :c1].clone().requires_grad_(True), b[k:k + 1, :c2].clone().requires_grad_(True)
        d1, d2, _, _ = chamfer_with_indices(ak, bk)
        ((d1 * g1[k:k + 1, :c1]).sum() + (d2 * g2[k:k + 1, :c2]).sum()).backward()
        ga[k, :c1], gb[k, :c2] = ak.grad[0], bk.grad[0]
    return ga, gb


def _exact_zero_padding(grad, counts, empty):
    for k, c in enumerate(counts):
        rows = grad[k] if empty[k] else grad[k, c:]
        assert bool((rows.view(torch.int32) == 0).all()), k            # +0.0, bit for bit


def test_backward_with_counts_default_mode():
    """Within 1e-5 of autograd through the dense op on each sliced pair (float atomics in arrival order on both sides);
    the rows at or beyond a count, and every row of a pair with an empty cloud, are exactly +0.0."""
    from cloud_transformers_amd.determinism import deterministic
    a, b, g1, g2, cnt1, cnt2 = _bwd_inputs()
    with deterministic(False):
        ga, gb = _grads_with_counts(a, b, g1, g2, cnt1, cnt2)
        ra, rb = _grads_dense_per_pair(a, b, g1, g2, cnt1, cnt2)
    empty = [c1 == 0 or c2 == 0 for c1, c2 in zip(cnt1, cnt2)]
    _exact_zero_padding(ga, cnt1, empty)
    _exact_zero_padding(gb, cnt2, empty)
    ea, eb = float((ga - ra).abs().max()), float((gb - rb).abs().max())
    print("max |grad - dense per pair|: %.3g %.3g" % (ea, eb))
    assert ea <= 1e-5 and eb <= 1e-5
    assert float(ga.abs().max()) > 0.1 and float(gb.abs().max()) > 0.1


def test_backward_with_counts_deterministic_mode():
    """Under deterministic(True): the bits of the dense deterministic op on each sliced pair, and of a second fresh run."""
    from cloud_transformers_amd.determinism import deterministic
    a, b, g1, g2, cnt1, cnt2 = _bwd_inputs()
    with deterministic(True):
        ga, gb = _grads_with_counts(a, b, g1, g2, cnt1, cnt2)
        ga2, gb2 = _grads_with_counts(a, b, g1, g2, cnt1, cnt2)
        ra, rb = _grads_dense_per_pair(a, b, g1, g2, cnt1, cnt2)
    empty = [c1 == 0 or c2 == 0 for c1, c2 in zip(cnt1, cnt2)]
    _exact_zero_padding(ga, cnt1, empty)
    _exact_zero_padding(gb, cnt2, empty)
    assert torch.equal(ga, ra) and torch.equal(gb, rb)
    assert torch.equal(ga, ga2) and torch.equal(gb, gb2)
    assert float(ga.abs().max()) > 0.1 and float(gb.abs().max()) > 0.1


def test_loss_chamfer_counts_and_module_counts():
    """loss_chamfer_counts = the mean over the batch of loss_chamfer on each pair's own rows; ChamferDist takes the counts."""
    from cloud_transformers_amd.chamfer import ChamferDist, loss_chamfer, loss_chamfer_counts
    B, n, m, cnt1, cnt2 = 3, 200, 260, [200, 71, 9], [131, 260, 5]
    g = torch.Generator().manual_seed(3)
    a = poison(torch.rand(B, n, 3, generator=g), cnt1, [True, False, True]).cuda()
    b = poison(torch.rand(B, m, 3, generator=g), cnt2, [True, False, True]).cuda()
    to_pc = lambda x: x.permute(0, 2, 1)[:, :, None].contiguous()          # noqa: E731  [B, 3, 1, N], the training layout
    got = loss_chamfer_counts(to_pc(a), to_pc(b), counts_tensor(cnt1), counts_tensor(cnt2))
    want = np.mean([float(loss_chamfer(to_pc(a[k:k + 1, :cnt1[k]]), to_pc(b[k:k + 1, :cnt2[k]]))) for k in range(B)])
    np.testing.assert_allclose(float(got), want, rtol=1e-5)
    d1, d2 = ChamferDist()(a, b, counts_tensor(cnt1), counts_tensor(cnt2))
    assert bool((d1[1, 71:] == 0).all()) and bool((d2[2, 5:] == 0).all()) and bool(torch.isfinite(d1).all())


def _compact_reference(x):
    B, n, _ = x.shape
    want, counts = torch.zeros_like(x), []
    for b in range(B):
        kept = x[b][x[b].sum(1).ne(0)]
        want[b, :kept.shape[0]] = kept
        counts.append(kept.shape[0])
    return want, counts


def _zero_sum_mask(pattern, B, n):
    i = torch.arange(n)
    z = torch.zeros(B, n, dtype=torch.bool)
    for b in range(B):
        if pattern == "none":
            pass
        elif pattern == "all":
            z[b] = True
        elif pattern == "alternating":
            z[b] = (i + b) % 2 == 0
        elif pattern == "runs":                 # runs over the 64-row wave boundaries (and 1024, 2048: the workgroup's step)
            for edge in range(64, n, 64):
                if (edge // 64 + b) % 2 == 0 or edge % 1024 == 0:
                    z[b, max(edge - 3 - b, 0):min(edge + 5 + b, n)] = True
            z[b, :b] = True
            z[b, n - 2 * b:] = True
        elif pattern == "one_minus_one":
            z[b] = (i * 7 + b) % 3 == 0
    return z


@pytest.mark.parametrize("B,n", [(3, 200), (2, 2500)])
@pytest.mark.parametrize("pattern", ["none", "all", "alternating", "runs", "one_minus_one"])
def test_rows_compact(pattern, B, n):
    """Rows, counts and zero tails against `x[b][x[b].sum(1).ne(0)]` per cloud.  Kept rows have coordinates in {1..5} / 4 (a
    positive sum), dropped rows are zeros or, in `one_minus_one`, (1, -1, 0) and (0.5, -0.25, -0.25): three-term sums that are
    exact in any order.  n = 2500 takes the kernel through three steps of its 1024-row walk."""
    from cloud_transformers_amd.metrics import compact_nonzero
    g = torch.Generator().manual_seed(n + len(pattern))
    x = torch.randint(1, 6, (B, n, 3), generator=g).float() / 4
    z = _zero_sum_mask(pattern, B, n)
    x[z] = 0.0
    if pattern == "one_minus_one":
        rows = z.nonzero()
        x[rows[0::2, 0], rows[0::2, 1]] = torch.tensor([1.0, -1.0, 0.0])
        x[rows[1::2, 0], rows[1::2, 1]] = torch.tensor([0.5, -0.25, -0.25])
    want, counts = _compact_reference(x)
    assert counts == (~z).sum(1).tolist()
    got, count = compact_nonzero(x.cuda())
    assert count.dtype == torch.int32 and count.tolist() == counts
    assert torch.equal(got.cpu(), want)
    again, count2 = compact_nonzero(x.cuda())
    assert torch.equal(again, got) and torch.equal(count2, count)


def test_rows_compact_keeps_nan_rows():
    from cloud_transformers_amd.metrics import compact_nonzero
    x = torch.zeros(1, 70, 3)
    x[0, 3] = torch.tensor([float("nan"), 0.0, 0.0])
    x[0, 66] = torch.tensor([0.25, 0.0, 0.0])
    got, count = compact_nonzero(x.cuda())
    assert count.tolist() == [2] and bool(torch.isnan(got[0, 0, 0])) and got[0, 1].tolist() == [0.25, 0.0, 0.0]
    assert bool((got[0, 2:] == 0).all())
