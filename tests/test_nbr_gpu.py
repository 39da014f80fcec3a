"""GridIndex (csrc/ct_nbr.hip) on the MI355X against exact float32 brute forces in numpy: the squared distance is
((dx*dx) + (dy*dy)) + (dz*dz), d = p - c, and ties go to the lower index, so count / idx / d2 must be bitwise equal.
Also against sklearn's KDTree (float64 sets, up to points within 1e-6 of a boundary) and scipy's cKDTree distances."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _d2(P, c):
    d = P - c[None, :]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def brute_radius(P, C, r, K):
    r32 = np.float32(r)
    r2 = r32 * r32
    Q = C.shape[0]
    idx = np.full((Q, K), -1, np.int64)
    d2 = np.full((Q, K), np.inf, np.float32)
    count = np.zeros(Q, np.int64)
    for q in range(Q):
        dd = _d2(P, C[q])
        sel = np.nonzero(dd <= r2)[0]
        o = sel[np.lexsort((sel, dd[sel]))][:K]
        count[q] = sel.size
        idx[q, :o.size] = o
        d2[q, :o.size] = dd[o]
    return idx, d2, count


def brute_nearest(P, X):
    chunk = max(1, (1 << 22) // P.shape[0])
    idx = np.empty(X.shape[0], np.int64)
    d2 = np.empty(X.shape[0], np.float32)
    for a in range(0, X.shape[0], chunk):
        x = X[a:a + chunk]
        d = P[None, :, :] - x[:, None, :]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        i = np.argmin(dd, axis=1)             # first minimum: the lowest index
        idx[a:a + chunk] = i
        d2[a:a + chunk] = dd[np.arange(x.shape[0]), i]
    return idx, d2


def area_like(n, seed, size=(12.0, 8.0, 3.0)):
    """An Area-like cloud: floor, ceiling and four walls (points on planes) plus boxes of clutter."""
    rng = np.random.default_rng(seed)
    X, Y, Z = size
    parts = []
    k = n // 8
    u = lambda m, lo, hi: rng.uniform(lo, hi, m)       # noqa: E731
    parts.append(np.stack([u(k, 0, X), u(k, 0, Y), np.zeros(k)], 1))
    parts.append(np.stack([u(k, 0, X), u(k, 0, Y), np.full(k, Z)], 1))
    parts.append(np.stack([np.zeros(k), u(k, 0, Y), u(k, 0, Z)], 1))
    parts.append(np.stack([np.full(k, X), u(k, 0, Y), u(k, 0, Z)], 1))
    parts.append(np.stack([u(k, 0, X), np.zeros(k), u(k, 0, Z)], 1))
    parts.append(np.stack([u(k, 0, X), np.full(k, Y), u(k, 0, Z)], 1))
    rest = n - 6 * k
    centres = rng.uniform([1, 1, 0.5], [X - 1, Y - 1, 1.5], (max(rest // 500, 1), 3))
    clutter = centres[rng.integers(0, centres.shape[0], rest)] + rng.normal(0, 0.3, (rest, 3))
    parts.append(clutter)
    P = np.concatenate(parts).astype(np.float32) + np.float32(rng.normal(0, 0.005))
    return P[rng.permutation(P.shape[0])] + np.asarray([3.0, -2.0, 0.1], np.float32)


def _check_radius(P, C, r, K, cell=None):
    from cloud_transformers_amd.neighbors import GridIndex
    index = GridIndex(torch.from_numpy(P).cuda(), cell)
    idx, d2, count = index.query_radius(torch.from_numpy(C).cuda(), r, K)
    torch.cuda.synchronize()
    wi, wd, wc = brute_radius(P, C, r, K)
    np.testing.assert_array_equal(count.cpu().numpy(), wc)
    np.testing.assert_array_equal(idx.cpu().numpy(), wi)
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), wd.view(np.uint32))
    return index, wc


def test_radius_uniform_cube_exact():
    rng = np.random.default_rng(1)
    P = rng.uniform(0, 10, (20000, 3)).astype(np.float32)
    C = rng.uniform(0, 10, (7, 3)).astype(np.float32)
    _, wc = _check_radius(P, C, 1.5, 200)
    assert (wc > 200).any() and (wc < 200).any()           # both sides of the truncation
    _check_radius(P, C, 1.5, 16384)                        # K above every count
    _check_radius(P, C, 0.7, 1)                            # K = 1
    _check_radius(P, C, 1.5, 300, cell=0.05)               # a fine grid (many cells per ball)
    _check_radius(P, C, 1.5, 300, cell=7.0)                # a coarse one (two cells per axis)


def test_radius_area_like_exact():
    P = area_like(120000, 2)
    rng = np.random.default_rng(3)
    C = P[rng.integers(0, P.shape[0], 6)] + rng.normal(0, 0.2, (6, 3)).astype(np.float32)
    _, wc = _check_radius(P, C, 2.0, 8192)
    assert (wc > 8192).any()


def test_radius_duplicated_points_exact_ties():
    rng = np.random.default_rng(4)
    base = np.round(rng.uniform(0, 4, (1500, 3)) * 4) / 4                  # a lattice: many equal distances
    P = np.repeat(base, 5, axis=0).astype(np.float32)[rng.permutation(7500)]
    C = np.asarray([[2.0, 2.0, 2.0], [1.0, 0.5, 3.0], [0.0, 0.0, 0.0]], np.float32)
    for K in (1, 7, 64, 333, 1000):
        _check_radius(P, C, 1.0, K)


def test_radius_centres_outside_box_and_whole_cloud():
    rng = np.random.default_rng(5)
    P = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
    C = np.asarray([[5.0, 0, 0], [-1.5, -1.5, 1.2], [0, 0, -30.0], [0.1, 0.2, 0.3]], np.float32)
    _check_radius(P, C, 1.2, 256)
    _, wc = _check_radius(P, C, 100.0, 16384)              # every point in every ball
    assert (wc == 3000).all()
    _check_radius(P, C, 100.0, 1000)                       # ... cut to K


def test_radius_single_point_and_zero_radius():
    P = np.asarray([[0.25, -0.5, 1.0]], np.float32)
    C = np.asarray([[0.25, -0.5, 1.0], [0.3, -0.5, 1.0], [9.0, 9.0, 9.0]], np.float32)
    _check_radius(P, C, 0.1, 1)
    _check_radius(P, C, 0.0, 4)
    _check_radius(P, C, 50.0, 3)


def test_radius_two_million_points():
    rng = np.random.default_rng(6)
    P = area_like(2_000_000, 7, size=(40.0, 25.0, 3.5))
    C = P[rng.integers(0, P.shape[0], 4)]
    _check_radius(P, C, 2.0, 8192)


def test_radius_against_sklearn_float64():
    neighbors = pytest.importorskip("sklearn.neighbors")
    P = area_like(60000, 8)
    rng = np.random.default_rng(9)
    C = P[rng.integers(0, P.shape[0], 5)] + rng.normal(0, 0.2, (5, 3)).astype(np.float32)
    from cloud_transformers_amd.neighbors import GridIndex
    r, K = 1.0, 4000
    idx, _, count = GridIndex(torch.from_numpy(P).cuda()).query_radius(torch.from_numpy(C).cuda(), r, K)
    idx, count = idx.cpu().numpy(), count.cpu().numpy()
    tree = neighbors.KDTree(P.astype(np.float64), leaf_size=50)
    inds, dists = tree.query_radius(C.astype(np.float64), r=r, return_distance=True, sort_results=True)
    for q in range(C.shape[0]):
        dq = np.sqrt(np.sum((P.astype(np.float64) - C[q].astype(np.float64)) ** 2, axis=1))
        near_r = np.abs(dq - r) <= 1e-6 * r
        ref = inds[q][:K]
        kth = dists[q][min(K, len(dists[q])) - 1]
        near_k = np.abs(dq - kth) <= 1e-6 * max(kth, 1e-12)
        got = set(idx[q][idx[q] >= 0].tolist())
        diff = got.symmetric_difference(ref.tolist())
        assert all(near_r[i] or near_k[i] for i in diff), sorted(diff)[:10]
        assert abs(int(count[q]) - len(inds[q])) <= int(near_r.sum())


def _check_nearest(P, X, cell=None):
    from cloud_transformers_amd.neighbors import GridIndex
    index = GridIndex(torch.from_numpy(P).cuda(), cell)
    idx, d2 = index.nearest(torch.from_numpy(X).cuda())
    torch.cuda.synchronize()
    wi, wd = brute_nearest(P, X)
    np.testing.assert_array_equal(idx.cpu().numpy(), wi)
    assert np.array_equal(d2.cpu().numpy().view(np.uint32), wd.view(np.uint32))
    return idx.cpu().numpy(), d2.cpu().numpy()


def test_nearest_exact_inside_and_far_outside():
    rng = np.random.default_rng(10)
    P = area_like(20000, 11)
    raw = P[rng.integers(0, P.shape[0], 6000)] + rng.normal(0, 0.03, (6000, 3)).astype(np.float32)
    far = rng.uniform(-1000, 1000, (300, 3)).astype(np.float32)
    edge = P.min(0) - rng.uniform(0, 0.5, (200, 3)).astype(np.float32)
    X = np.concatenate([raw, far, edge]).astype(np.float32)
    _check_nearest(P, X)
    _check_nearest(P, X[:2000], cell=0.02)                 # fine cells: many shells
    _check_nearest(P, X[:2000], cell=20.0)                 # one cell


def test_nearest_ties_and_single_point():
    rng = np.random.default_rng(12)
    base = np.round(rng.uniform(0, 2, (400, 3)) * 2) / 2
    P = np.repeat(base, 3, axis=0).astype(np.float32)[rng.permutation(1200)]
    X = (np.round(rng.uniform(-1, 3, (3000, 3)) * 4) / 4).astype(np.float32)     # equidistant from several lattice points
    _check_nearest(P, X)
    one = np.asarray([[1.0, 2.0, 3.0]], np.float32)
    i, _ = _check_nearest(one, X[:100])
    assert (i == 0).all()


def test_nearest_against_ckdtree():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(13)
    P = area_like(50000, 14)
    X = np.concatenate([P[rng.integers(0, P.shape[0], 20000)] + rng.normal(0, 0.05, (20000, 3)).astype(np.float32),
                        rng.uniform(-200, 200, (500, 3)).astype(np.float32)])
    from cloud_transformers_amd.neighbors import GridIndex
    _, d2 = GridIndex(torch.from_numpy(P).cuda()).nearest(torch.from_numpy(X).cuda())
    dist, _ = spatial.cKDTree(P.astype(np.float64)).query(X.astype(np.float64), k=1)
    got = np.sqrt(d2.cpu().numpy().astype(np.float64))
    scale = 1.0 + np.abs(X).max(1)
    assert np.all(np.abs(got - dist) <= 1e-6 * scale), np.abs(got - dist).max()


def test_two_runs_bitwise_equal():
    from cloud_transformers_amd.neighbors import GridIndex
    P = torch.from_numpy(area_like(200000, 15)).cuda()
    rng = np.random.default_rng(16)
    C = torch.from_numpy(rng.uniform(0, 12, (6, 3)).astype(np.float32)).cuda()
    X = P[:50000] + 0.01
    outs = []
    for _ in range(2):
        index = GridIndex(P)
        outs.append((index.cell_start.clone(), index.order.clone()) + index.query_radius(C, 2.0, 8192) + index.nearest(X))
    torch.cuda.synchronize()
    a, b = outs
    assert torch.equal(a[0], b[0])
    # the order inside a cell follows the atomics; each cell's set of points does not
    cs = a[0].cpu().numpy()
    oa, ob = a[1].cpu().numpy(), b[1].cpu().numpy()
    cell = np.repeat(np.arange(cs.size - 1), np.diff(cs))
    np.testing.assert_array_equal(oa[np.lexsort((oa, cell))], ob[np.lexsort((ob, cell))])
    for x, y in zip(a[2:], b[2:]):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def test_index_layout():
    """cell_start / order / sorted describe a counting sort by cell id (iz*ny + iy)*nx + ix, x fastest."""
    from cloud_transformers_amd.neighbors import GridIndex
    rng = np.random.default_rng(17)
    P = rng.uniform(-3, 5, (5000, 3)).astype(np.float32)
    index = GridIndex(torch.from_numpy(P).cuda(), cell=0.75)
    cs, order, srt = index.cell_start.cpu().numpy(), index.order.cpu().numpy(), index.sorted.cpu().numpy()
    nx, ny, nz = index.dims
    o, h = np.asarray(index.origin, np.float32), np.float32(index.h)
    c = np.floor((P - o) / h).astype(np.int64)
    c = np.minimum(np.maximum(c, 0), np.asarray([nx - 1, ny - 1, nz - 1]))
    cid = (c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]
    assert cs[0] == 0 and cs[-1] == P.shape[0] and np.all(np.diff(cs) >= 0)
    np.testing.assert_array_equal(np.sort(order), np.arange(P.shape[0]))
    np.testing.assert_array_equal(np.repeat(np.arange(cs.size - 1), np.diff(cs)), cid[order])
    np.testing.assert_array_equal(srt[:, :3], P[order])
    np.testing.assert_array_equal(srt[:, 3].view(np.int32), order)


def test_default_cell_density():
    from cloud_transformers_amd.neighbors import GridIndex
    P = area_like(300000, 18)
    index = GridIndex(torch.from_numpy(P).cuda())
    occupied = int((torch.diff(index.cell_start) > 0).sum())
    assert 3.0 <= P.shape[0] / occupied <= 10.0, (index.h, P.shape[0] / occupied)
