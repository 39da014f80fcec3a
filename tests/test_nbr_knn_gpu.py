"""GridIndex.query_knn / GridIndexTable.query_knn / GridIndex.interpolate (csrc/ct_nbr_knn.h) on the MI355X against the numpy
restatement of tests/nbr_knn_ref.py, bit for bit: idx with torch.equal, d2 and the interpolated values on their bits.  Every
device call runs under torch's sync-debug mode "error" (nothing may be read back), once through the Python method and once
through the C entry point into outputs preset to a sentinel / NaN, so that an element the kernel did not write shows."""
import contextlib

import numpy as np
import pytest
import torch

from tests.nbr_knn_ref import bits, interp_ref, knn_ref
from tests.test_nbr_gpu import area_like

pytestmark = pytest.mark.gpu

SENTINEL = -7


@contextlib.contextmanager
def no_sync():
    """Sync-debug mode "error" around the calls under test, shown live on an .item() first."""
    probe = torch.ones(1, device="cuda").sum()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _index(P, cell=None):
    from cloud_transformers_amd.neighbors import GridIndex
    return GridIndex(torch.from_numpy(np.ascontiguousarray(P, np.float32)).cuda(), cell)


def _knn_both(index, X, k):
    """(idx, d2) of the method and of the C entry point on preset outputs, as numpy arrays; the two must agree exactly."""
    from cloud_transformers_amd import _lib
    from cloud_transformers_amd.ops import _stream
    q = torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda()
    Q = q.shape[0]
    ridx = torch.full((Q, k), SENTINEL, dtype=torch.int64, device="cuda")
    rd2 = torch.full((Q, k), float("nan"), dtype=torch.float32, device="cuda")
    lib = _lib.load()
    with no_sync():
        idx, d2 = index.query_knn(q, k)
        status = lib.ct_nbr_knn(index.cell_start.data_ptr(), index.sorted.data_ptr(), index._origin_c, index.h, index._dims_c,
                                q.data_ptr(), Q, k, ridx.data_ptr(), rd2.data_ptr(), _stream(q.device))
    assert status == 0
    assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and tuple(idx.shape) == (Q, k) == tuple(d2.shape)
    assert torch.equal(idx, ridx) and np.array_equal(bits(d2.cpu().numpy()), bits(rd2.cpu().numpy()))
    return idx, d2


def _same(idx, d2, want_idx, want_d2):
    assert torch.equal(idx.cpu(), torch.from_numpy(want_idx))
    assert np.array_equal(bits(d2.cpu().numpy()), bits(want_d2))


def _check(P, X, k, cell=None, index=None, want=None):
    index = _index(P, cell) if index is None else index
    idx, d2 = _knn_both(index, X, k)
    wi, wd = knn_ref(P, X, k) if want is None else want
    _same(idx, d2, wi, wd)
    return index


# ---- a small cloud shared by the k x Q grid: one index, one reference at k = 64 (every smaller k is its prefix) ----

@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(21)
    P = rng.uniform(-1, 1, (700, 3)).astype(np.float32)
    X = rng.uniform(-1.2, 1.2, (257, 3)).astype(np.float32)
    X[:40] = P[:40]                                            # some queries are points of the cloud: d2 = 0
    return P, X, _index(P), knn_ref(P, X, 64)


@pytest.mark.parametrize("Q", [1, 3, 257])                     # a workgroup not full of waves, a last partial workgroup
@pytest.mark.parametrize("k", [1, 2, 3, 33, 63, 64])
def test_k_and_q_grid(small, k, Q):
    P, X, index, (wi, wd) = small
    _check(P, X[:Q], k, index=index, want=(wi[:Q, :k].copy(), wd[:Q, :k].copy()))


def test_single_point_cloud():
    P = np.asarray([[0.25, -1.5, 3.0]], np.float32)
    X = np.asarray([[0.25, -1.5, 3.0], [0, 0, 0], [9, 9, 9]], np.float32)
    for k in (1, 3):
        _check(P, X, k)
    wi, _ = knn_ref(P, X, 3)
    assert (wi[:, 0] == 0).all() and (wi[:, 1:] == -1).all()


def test_cloud_smaller_than_k_pads_the_tail():
    rng = np.random.default_rng(22)
    P = rng.uniform(0, 1, (5, 3)).astype(np.float32)
    X = rng.uniform(-1, 2, (9, 3)).astype(np.float32)
    _check(P, X, 8)
    wi, wd = knn_ref(P, X, 8)
    assert (wi[:, :5] >= 0).all() and (wi[:, 5:] == -1).all() and np.isinf(wd[:, 5:]).all()


def test_k1_equals_nearest(small):
    P, X, index, _ = small
    far = np.asarray([[50, 0, 0], [-3, -40, 7], [1e4, 1e4, -1e4]], np.float32)
    q = torch.from_numpy(np.concatenate([X, far])).cuda()
    with no_sync():
        idx, d2 = index.query_knn(q, 1)
        nidx, nd2 = index.nearest(q)
    assert torch.equal(idx[:, 0], nidx) and np.array_equal(bits(d2[:, 0].cpu().numpy()), bits(nd2.cpu().numpy()))


# ---- ties: the order is (d2, index) ----

def test_ties_every_point_four_times():
    rng = np.random.default_rng(23)
    base = rng.uniform(0, 4, (500, 3)).astype(np.float32)
    P = np.tile(base, (4, 1))[rng.permutation(2000)]
    X = np.concatenate([base[:25], rng.uniform(0, 4, (25, 3)).astype(np.float32)])
    index = _index(P)
    for k in (3, 4, 5, 64):
        _check(P, X, k, index=index)
    wi, wd = knn_ref(P, X[:25], 4)
    assert (wd == 0).all() and (np.diff(wi, axis=1) > 0).all()            # four copies at d2 = 0, ids ascending


def test_ties_integer_lattice():
    rng = np.random.default_rng(24)
    g = np.arange(8, dtype=np.float32)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(512)]
    at = P[rng.choice(512, 40, replace=False)]
    X = np.concatenate([at, at[:30] + np.float32(0.5)])
    index = _index(P)
    for k in (7, 27, 64):
        _check(P, X, k, index=index)
    _, wd = knn_ref(P, X, 27)
    assert ((np.diff(wd, axis=1) == 0).sum(1) >= 10).all()                # many equal distances in every row


# ---- geometry ----

def test_queries_far_outside_the_box(small):
    P, _, index, _ = small
    X = np.asarray([[30, 0, 0], [0, -30, 0.5], [0.1, 0.2, 30], [-30, -30, -30], [25, -25, 25], [1e3, 0, 0], [1.5, 1.5, 1.5]],
                   np.float32)
    for k in (1, 5, 64):
        _check(P, X, k, index=index)


def test_queries_on_cell_faces_and_box_corners(small):
    P, _, index, _ = small
    o, h = np.asarray(index.origin, np.float32), np.float32(index.h)
    rng = np.random.default_rng(25)
    faces = []
    for _ in range(40):                                        # one, two or three coordinates exactly on a cell face
        c = rng.uniform(-1, 1, 3).astype(np.float32)
        for a in rng.choice(3, rng.integers(1, 4), replace=False):
            c[a] = o[a] + np.float32(rng.integers(0, index.dims[a] + 1)) * h
        faces.append(c)
    lo, hi = P.min(0), P.max(0)
    corners = [[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[l][2]] for i in (0, 1) for j in (0, 1) for l in (0, 1)]
    X = np.concatenate([np.asarray(faces, np.float32), np.asarray(corners, np.float32)])
    for k in (1, 6, 64):
        _check(P, X, k, index=index)


def test_flat_cloud():
    rng = np.random.default_rng(26)
    P = np.concatenate([rng.uniform(0, 5, (1500, 2)), np.full((1500, 1), 0.75)], 1).astype(np.float32)
    X = np.concatenate([P[:10], rng.uniform(-1, 6, (30, 3)).astype(np.float32)])
    index = _index(P)
    assert index.dims[2] == 1
    for k in (3, 40):
        _check(P, X, k, index=index)


def test_collinear_cloud():
    rng = np.random.default_rng(27)
    t = rng.uniform(-2, 2, (900, 1)).astype(np.float32)
    P = (np.asarray([[1.0, 2.0, -0.5]], np.float32) + t * np.asarray([[0.5, -0.25, 1.0]], np.float32)).astype(np.float32)
    X = np.concatenate([P[:10], rng.uniform(-3, 3, (30, 3)).astype(np.float32)])
    for cell in (None, 0.05):
        index = _index(P, cell)
        for k in (2, 64):
            _check(P, X, k, index=index)


# ---- cell sizes on one clustered cloud: one reference at k = 64 for all three grids ----

@pytest.fixture(scope="module")
def clustered():
    rng = np.random.default_rng(28)
    P = area_like(20000, 29)
    X = np.concatenate([P[rng.choice(P.shape[0], 40, replace=False)] + rng.normal(0, 0.02, (40, 3)).astype(np.float32),
                        rng.uniform(P.min(0), P.max(0), (24, 3)).astype(np.float32)]).astype(np.float32)
    return P, X, knn_ref(P, X, 64)


@pytest.mark.parametrize("cell", [1000.0, 0.05, None], ids=["one_cell", "mostly_empty_cells", "default_cell"])
def test_cell_sizes(clustered, cell):
    P, X, (wi, wd) = clustered
    index = _index(P, cell)
    if cell == 1000.0:
        assert index.dims == [1, 1, 1]                         # one run of 20 000 records: hundreds of batches
    if cell == 0.05:
        assert np.prod(index.dims) > 50 * P.shape[0]           # the stop rule does the work
    for k in (3, 64):
        _check(P, X, k, index=index, want=(wi[:, :k].copy(), wd[:, :k].copy()))


def test_agrees_with_query_radius(clustered):
    """query_radius with a radius beyond the whole cloud keeps the first k by the same key."""
    P, X, _ = clustered
    index = _index(P)
    r = 2.0 * float(np.linalg.norm(P.max(0).astype(np.float64) - P.min(0).astype(np.float64)))
    q = torch.from_numpy(X).cuda()
    assert q.shape[0] == 64
    for k in (16, 64):
        with no_sync():
            ridx, rd2, count = index.query_radius(q, r, k)
            idx, d2 = index.query_knn(q, k)
        assert (count == P.shape[0]).all()
        assert torch.equal(idx, ridx) and np.array_equal(bits(d2.cpu().numpy()), bits(rd2.cpu().numpy()))


def test_non_finite_queries_return_and_leave_their_neighbours_alone(small):
    P, X, index, (wi, wd) = small
    X = X[:9].copy()
    X[2] = np.nan
    X[4, 1] = np.nan
    X[6] = np.inf
    X[7, 0] = -np.inf
    for k in (1, 3, 64):
        idx, d2 = _knn_both(index, X, k)
        want_i, want_d = wi[:9, :k].copy(), wd[:9, :k].copy()
        want_i[[2, 4, 6, 7]], want_d[[2, 4, 6, 7]] = -1, np.inf
        _same(idx, d2, want_i, want_d)
        ri, rd = knn_ref(P, X, k)
        assert np.array_equal(ri, want_i) and np.array_equal(bits(rd), bits(want_d))


# ---- the table form ----

def test_table_equals_per_cloud_calls():
    from cloud_transformers_amd import _lib
    from cloud_transformers_amd.neighbors import GridIndexTable
    from cloud_transformers_amd.ops import _stream
    rng = np.random.default_rng(30)
    clouds = [rng.uniform(-1, 1, (300, 3)).astype(np.float32), area_like(4000, 31),
              (rng.uniform(0, 1, (40, 3)) * [8, 0.5, 0.1] + [20, 20, 20]).astype(np.float32)]
    cells = [None, 0.3, 2.0]
    indices = [_index(P, c) for P, c in zip(clouds, cells)]
    assert len({tuple(ix.dims) for ix in indices}) == 3
    table = GridIndexTable(indices)
    Q = 90
    cid = np.arange(Q) % 3
    X = np.stack([clouds[c][rng.integers(0, clouds[c].shape[0])] + rng.normal(0, 0.05, 3) for c in cid]).astype(np.float32)
    sent = cid.astype(np.int64).copy()
    sent[3], sent[5] = -4, 3 + 17                              # out of range on each side: clamped to clouds 0 and 2
    cid[3], cid[5] = 0, 2
    q, cloud = torch.from_numpy(X).cuda(), torch.from_numpy(sent).cuda()
    for k in (1, 3, 64):
        ridx = torch.full((Q, k), SENTINEL, dtype=torch.int64, device="cuda")
        rd2 = torch.full((Q, k), float("nan"), dtype=torch.float32, device="cuda")
        with no_sync():
            idx, d2 = table.query_knn(cloud, q, k)
            status = _lib.load().ct_nbr_knn_multi(table.table.data_ptr(), 3, cloud.data_ptr(), q.data_ptr(), Q, k, ridx.data_ptr(),
                                                  rd2.data_ptr(), _stream(q.device))
            per = [ix.query_knn(q, k) for ix in indices]
        assert status == 0 and torch.equal(idx, ridx) and np.array_equal(bits(d2.cpu().numpy()), bits(rd2.cpu().numpy()))
        sel = torch.from_numpy(cid).cuda()
        want_i = torch.stack([p[0] for p in per])[sel, torch.arange(Q, device="cuda")]
        want_d = torch.stack([p[1] for p in per])[sel, torch.arange(Q, device="cuda")]
        assert torch.equal(idx, want_i) and np.array_equal(bits(d2.cpu().numpy()), bits(want_d.cpu().numpy()))
        assert (idx[:, -1] == -1).sum() == (30 if k == 64 else 0)         # the 40-point cloud pads its tail at k = 64
        wi, wd = knn_ref(clouds[2], X[cid == 2], k)
        _same(idx[sel == 2], d2[sel == 2], wi, wd)


# ---- interpolation ----

def _interp_both(index, values, X, k, eps=1e-8):
    from cloud_transformers_amd import _lib
    from cloud_transformers_amd.ops import _stream
    q = torch.from_numpy(np.ascontiguousarray(X, np.float32)).cuda()
    v = torch.from_numpy(values).cuda()
    Q, C = q.shape[0], v.shape[1]
    raw = torch.full((Q, C), float(SENTINEL), dtype=torch.float32, device="cuda")
    with no_sync():
        out = index.interpolate(v, q, k, eps)
        idx, d2 = index.query_knn(q, k)
        status = _lib.load().ct_nbr_interp(idx.data_ptr(), d2.data_ptr(), Q, k, v.data_ptr(), v.shape[0], C, eps, raw.data_ptr(),
                                           _stream(q.device))
    assert status == 0 and out.dtype == torch.float32 and tuple(out.shape) == (Q, C)
    assert np.array_equal(bits(out.cpu().numpy()), bits(raw.cpu().numpy()))
    return out.cpu().numpy(), idx.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize("C", [1, 13, 16])
def test_interpolate_bits(small, C):
    P, X, index, (wi, wd) = small
    rng = np.random.default_rng(40 + C)
    values = rng.normal(0, 3, (P.shape[0], C)).astype(np.float32)
    out, idx, d2 = _interp_both(index, values, X, 3)
    assert np.array_equal(idx, wi[:, :3]) and (d2[:40, 0] == 0).all()     # the first 40 queries coincide with a point
    want = interp_ref(wi[:, :3], wd[:, :3], values, 1e-8)
    assert np.array_equal(bits(out), bits(want)) and np.isfinite(out).all()
    # what the bits mean: the mean of the three rows weighted by 1 / (d2 + eps), here in float64 (|values| < ~15, so float32
    # rounding of the three-term sum stays far below 1e-4)
    w = 1.0 / (wd[:, :3].astype(np.float64) + 1e-8)
    mean = ((w / w.sum(1, keepdims=True))[:, :, None] * values[wi[:, :3]].astype(np.float64)).sum(1)
    np.testing.assert_allclose(out, mean, rtol=1e-5, atol=1e-4)
    out5, _, _ = _interp_both(index, values, X[:50], 5, eps=0.5)         # another k and eps
    assert np.array_equal(bits(out5), bits(interp_ref(wi[:50, :5], wd[:50, :5], values, 0.5)))


def test_interpolate_cloud_smaller_than_k():
    P = np.asarray([[0, 0, 0], [1, 0, 0]], np.float32)
    values = np.asarray([[1, 10, -2], [3, 30, 4]], np.float32)
    X = np.asarray([[0.25, 0, 0], [0, 0, 0], [5, 5, 5], [np.nan, 0, 0]], np.float32)
    out, idx, d2 = _interp_both(_index(P), values, X, 3)
    assert (idx[:3, 2] == -1).all() and (idx[3] == -1).all()
    assert np.array_equal(bits(out), bits(interp_ref(idx, d2, values, 1e-8)))
    assert np.isfinite(out[:3]).all() and np.isnan(out[3]).all()          # -1 slots skipped; no neighbour, no value
    np.testing.assert_allclose(out[0], 0.9 * values[0] + 0.1 * values[1], rtol=1e-5)


def test_empty_query_set(small):
    _, _, index, _ = small
    q = torch.zeros(0, 3, device="cuda")
    with no_sync():
        idx, d2 = index.query_knn(q, 5)
        out = index.interpolate(torch.zeros(700, 4, device="cuda"), q, 3)
    assert tuple(idx.shape) == (0, 5) == tuple(d2.shape) and tuple(out.shape) == (0, 4)


# ---- the evaluator ----

def _two_areas(n=1500, dl=0.25):
    """Two small Areas subsampled coarsely: a subsampled point is the barycentre of several raw points, so a raw point's
    three neighbours carry comparable weights and the interpolated vote differs from the nearest point's."""
    from cloud_transformers_amd.data.s3dis_kpconv import Area
    from cloud_transformers_amd.data.subsampling import grid_subsampling
    out = []
    for s in (0, 1):
        rng = np.random.default_rng(300 + s)
        pts = area_like(n, 310 + s, size=(9.0 + s, 6.0, 3.0))
        cols = rng.integers(0, 256, (n, 3)).astype(np.float32)
        labs = rng.integers(0, 13, n).astype(np.int32)
        sp, sc, sl = grid_subsampling(pts, features=cols, labels=labs[:, None], sampleDl=dl)
        out.append(Area("Area_%d" % (s + 1), pts, cols, labs, sp, sc / np.float32(255), sl[:, 0].astype(np.int32)))
    return out


def test_full_ious_with_k3_and_default_unchanged():
    from cloud_transformers_amd.data.s3dis_kpconv import VoteEvaluator
    from tests.test_nbr_gpu import brute_nearest
    from tests.test_s3dis_kpconv_gpu import _confusion, _iou_from_confusions
    C = 13
    areas = _two_areas()
    ev = VoteEvaluator(areas, num_classes=C)
    g = torch.Generator(device="cuda").manual_seed(3)
    ev.logits_sum[:, :ev.total] = torch.randn(C, ev.total, generator=g, device="cuda")
    ev.counts.fill_(2.0)
    vote = ev.vote_logits().cpu().numpy()
    offs = np.concatenate([[0], np.cumsum(ev.sizes)])
    near, k3 = 0, 0
    for i, a in enumerate(areas):
        lg = vote[:, offs[i]:offs[i + 1]]
        proj, _ = brute_nearest(a.sub_points, a.points)
        near = near + _confusion(a.labels, np.argmax(lg[:, proj], axis=0), C)
        idx, d2 = knn_ref(a.sub_points, a.points, 3)
        k3 = k3 + _confusion(a.labels, np.argmax(interp_ref(idx, d2, np.ascontiguousarray(lg.T), 1e-8), axis=1), C)
    assert np.abs(near - k3).sum() > 100                       # the two projections differ on this set, by many points
    for got, conf in ((ev.full_ious(), near), (ev.full_ious(k=1), near), (ev.full_ious(k=3), k3)):
        want = _iou_from_confusions(conf)
        np.testing.assert_allclose(got[0], want, rtol=1e-9, atol=1e-12)
        assert abs(got[1] - np.mean(want)) < 1e-9
    a, b = ev.full_ious(), ev.full_ious(k=1)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
