"""The index table, the table-driven radius query and the device plan without a GPU: ct_nbr_table_*, ct_nbr_radius_multi and
ct_kp_plan refuse bad arguments before touching the device, and the numpy restatement of ct_kp_plan's contract
(tests/kp_plan_ref.py) picks what the reference's own procedure picks (datasets/s3dis_closer.py:249-274: sklearn KDTree,
float64 potentials)."""
import ctypes

import numpy as np
import pytest

from tests import kp_plan_ref

EINVAL, EWORKSPACE = -1, -3


@pytest.fixture(scope="module")
def lib():
    from cloud_transformers_amd import _lib
    _lib.build()
    return _lib.load()


def _buf(n=4096):
    b = ctypes.create_string_buffer(n + 64)
    a = ctypes.addressof(b)
    return b, ctypes.c_void_p((a + 63) & ~63)                      # 64-byte aligned inside b


def test_table_rejects_bad_arguments(lib):
    from cloud_transformers_amd import _lib
    keep, p = _buf()
    o, d = _lib.float_array([0.0, 0.0, 0.0]), _lib.int_array([4, 4, 4])
    assert lib.ct_nbr_table_bytes(0) == 0 and lib.ct_nbr_table_bytes(-2) == 0
    one = lib.ct_nbr_table_bytes(1)
    assert one > 0 and lib.ct_nbr_table_bytes(5) == 5 * one

    def call(*, table=p, n=3, i=1, cs=p, sorted_=p, origin=o, h=0.5, dims=d, M=100, offset=7):
        return lib.ct_nbr_table_set(table, n, i, cs, sorted_, origin, h, dims, M, offset)

    assert call() == 0
    assert call(table=None) == EINVAL and call(cs=None) == EINVAL and call(sorted_=None) == EINVAL
    assert call(origin=None) == EINVAL and call(dims=None) == EINVAL
    assert call(n=0) == EINVAL and call(i=-1) == EINVAL and call(i=3) == EINVAL
    assert call(M=0) == EINVAL and call(M=2 ** 31) == EINVAL and call(offset=-1) == EINVAL
    assert call(sorted_=ctypes.c_void_p(p.value + 4)) == EINVAL     # `sorted` holds float4 records: 16-byte aligned
    assert call(sorted_=ctypes.c_void_p(p.value + 8)) == EINVAL
    assert call(h=0.0) == EINVAL and call(h=float("inf")) == EINVAL and call(h=float("nan")) == EINVAL   # grid_ok, as ct_nbr_radius
    assert call(dims=_lib.int_array([0, 4, 4])) == EINVAL
    assert call(dims=_lib.int_array([1024, 1024, 1024])) == EINVAL  # more than 2^26 cells
    assert call(origin=_lib.float_array([0.0, float("nan"), 0.0])) == EINVAL
    del keep


def test_radius_multi_rejects_bad_arguments(lib):
    from cloud_transformers_amd import _lib
    keep, p = _buf()

    def call(*, table=p, n=2, cloud=p, centres=p, Q=3, r=1.0, K=16, outs=(p, p, p)):
        return lib.ct_nbr_radius_multi(table, n, cloud, centres, Q, r, K, *outs, None)

    assert call(table=None) == EINVAL and call(cloud=None) == EINVAL and call(centres=None) == EINVAL
    for k in range(3):
        outs = [p, p, p]
        outs[k] = None
        assert call(outs=tuple(outs)) == EINVAL, k
    assert call(n=0) == EINVAL and call(n=-1) == EINVAL
    assert call(Q=0) == EINVAL and call(Q=-5) == EINVAL
    assert call(K=0) == EINVAL and call(K=_lib.NBR_K_MAX + 1) == EINVAL
    assert call(r=-0.5) == EINVAL and call(r=float("nan")) == EINVAL
    del keep


def test_kp_plan_rejects_bad_arguments(lib):
    from cloud_transformers_amd import _lib
    keep, p = _buf(1 << 16)
    assert lib.ct_kp_plan_workspace_bytes(0, 100) == 0 and lib.ct_kp_plan_workspace_bytes(2, 0) == 0
    assert lib.ct_kp_plan_workspace_bytes(_lib.KP_PLAN_CLOUDS_MAX + 1, 100) == 0
    need = lib.ct_kp_plan_workspace_bytes(3, 20000)
    assert 0 < need <= 1 << 16
    assert lib.ct_kp_plan_workspace_bytes(3, 2_000_000) > need      # more workgroups in the reduction: more partials

    def call(*, table=p, n_clouds=3, max_points=20000, ins=(p,) * 4, r=2.0, K=64, n=8, outs=(p,) * 3, ws=p, ws_bytes=need):
        return lib.ct_kp_plan(table, n_clouds, max_points, *ins, r, K, n, *outs, ws, ws_bytes, None)

    assert call(table=None) == EINVAL
    for k in range(4):                                                # points, potentials, min_potentials, noise
        ins = [p] * 4
        ins[k] = None
        assert call(ins=tuple(ins)) == EINVAL, k
    for k in range(3):                                                # cloud, point, picks
        outs = [p] * 3
        outs[k] = None
        assert call(outs=tuple(outs)) == EINVAL, k
    assert call(n_clouds=0) == EINVAL and call(n_clouds=-1) == EINVAL
    assert call(max_points=0) == EINVAL
    assert call(n=0) == EINVAL and call(n=-4) == EINVAL
    assert call(K=0) == EINVAL and call(K=_lib.NBR_K_MAX + 1) == EINVAL
    assert call(r=-1.0) == EINVAL and call(r=float("nan")) == EINVAL
    assert call(ws=None) == EWORKSPACE and call(ws_bytes=need - 1) == EWORKSPACE and call(ws_bytes=0) == EWORKSPACE
    del keep


# ---- the restatement against the reference's procedure ----

R, K, PICKS, SEED = 0.5, 256, 40, 0


def _case(seed):
    """Two clouds in a 2 x 2 x 1 box (an inner ball of 0.5 holds ~390 points: more than K) and initial potentials in
    [0, 1e-3) as the reference draws them, but stratified: a random permutation of a ladder with steps of 1e-3 / 5900 =
    1.7e-7 over both clouds, rounded to float32.  Independent uniform draws put two of 3000 values within 1e-7 of each other
    at some pick of nearly every seed (the two smallest lie ~3e-7 apart on average); the ladder keeps untouched points, and
    so the candidates of every pick, more than 1e-7 apart."""
    rng = np.random.default_rng(seed)
    sizes = (3000, 2900)
    points = [rng.uniform(0.0, 1.0, (m, 3)).astype(np.float32) * np.float32([2.0, 2.0, 1.0]) for m in sizes]
    ladder = (rng.permutation(sum(sizes)) * (1e-3 / sum(sizes))).astype(np.float32)
    potentials = [ladder[:sizes[0]], ladder[sizes[0]:]]
    noise = rng.normal(scale=R / 10, size=(PICKS, 3)).astype(np.float32)
    return points, potentials, noise


def _two_smallest_gap(a):
    a = np.asarray(a, dtype=np.float64)
    if a.size < 2:
        return np.inf
    lo = np.partition(a, 1)[:2]
    return float(lo[1] - lo[0])


def _reference_procedure(points, potentials, noise):
    """datasets/s3dis_closer.py:249-274 restated: KDTree balls sorted by distance and cut to num_points, float64 potentials.
    Returns the (cloud_ind, point_ind) sequence and, per pick, the smaller of the two gaps that decided it: between the two
    smallest min_potentials and between the two smallest potentials of the chosen cloud."""
    from sklearn.neighbors import KDTree
    trees = [KDTree(p, leaf_size=50) for p in points]
    pots = [p.astype(np.float64) for p in potentials]
    mins = [float(np.min(p)) for p in pots]
    seq, gaps = [], []
    for i in range(noise.shape[0]):
        cloud_ind = int(np.argmin(mins))
        point_ind = int(np.argmin(pots[cloud_ind]))
        gaps.append(min(_two_smallest_gap(mins), _two_smallest_gap(pots[cloud_ind])))
        seq.append((cloud_ind, point_ind))
        pts = points[cloud_ind]
        pick_point = pts[point_ind, :].reshape(1, -1) + noise[i:i + 1].astype(pts.dtype)
        inds = trees[cloud_ind].query_radius(pick_point, r=R, return_distance=True, sort_results=True)[0][0]
        if K < inds.shape[0]:
            inds = inds[:K]
        dists = np.sum(np.square((pts[inds] - pick_point).astype(np.float32)), axis=1)
        tukeys = np.square(1 - dists / np.square(R))
        tukeys[dists > np.square(R)] = 0
        pots[cloud_ind][inds] += tukeys
        mins[cloud_ind] = float(np.min(pots[cloud_ind]))
    return seq, gaps


def test_restatement_picks_what_the_reference_procedure_picks():
    points, potentials, noise = _case(SEED)
    seq, gaps = _reference_procedure(points, potentials, noise)
    # the case's condition, on the reference side alone: no pick was decided by less than 1e-7
    assert min(gaps) > 1e-7, (int(np.argmin(gaps)), min(gaps))
    cloud, point, picks, pots, _ = kp_plan_ref.plan(points, potentials, noise, R, K)
    assert list(zip(cloud.tolist(), point.tolist())) == seq
    assert len(set(cloud.tolist())) == 2                                         # both clouds were picked
    counts = [kp_plan_ref.ball(points[c], picks[i], R, 1 << 20)[2] for i, c in enumerate(cloud.tolist())]
    assert max(counts) > K and min(counts) < K                                   # truncated balls and whole ones
    for p in pots:
        assert p.dtype == np.float32 and np.isfinite(p).all()
