"""The device voxel-grid subsampling (data.subsampling.compute_device: ct_voxel_keys, torch's stable sort, ct_voxel_reduce;
csrc/ct_voxel.hip) against the host path (data.subsampling.compute, libcloudct_host.so), which is itself pinned to the
reference's C++ by tests/golden/grid_subsampling_reference.json.  Every comparison is np.array_equal on rows IN ORDER:
the same rows, the same order, the same bits."""
import json
import os

import numpy as np
import pytest
import torch

from cloud_transformers_amd.data import subsampling as S
from tests.test_grid_subsampling import GOLDEN, REF_CASES, REF_VARIANTS, cloud, golden_key, reference_cloud, rows_digest

pytestmark = pytest.mark.gpu
f32 = np.float32


def _up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device(points, features=None, classes=None, dl=0.1, **kw):
    """compute_device on uploaded copies; numpy arrays back, always a tuple"""
    got = S.compute_device(_up(points), features=_up(features), classes=_up(classes), sampleDl=dl, **kw)
    got = (got,) if isinstance(got, torch.Tensor) else got
    assert all(t.is_cuda for t in got)
    return tuple(t.cpu().numpy() for t in got)


def host(points, features=None, classes=None, dl=0.1):
    got = S.compute(points, features=features, classes=classes, sampleDl=dl)
    return (got,) if isinstance(got, np.ndarray) else got


def assert_same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), k


def numpy_keys(points, dl):
    """the host file's key arithmetic (tests/test_grid_subsampling.numpy_restatement), keys only"""
    pts = points.astype(f32)
    inv = f32(1) / f32(dl)
    org = np.floor(pts.min(0) * inv) * f32(dl)
    idx = np.floor((pts - org) / f32(dl)).astype(np.int64)
    span = np.floor((pts.max(0) - org) / f32(dl)).astype(np.int64) + 1
    return idx[:, 0] + span[0] * idx[:, 1] + span[0] * span[1] * idx[:, 2], int(span[0]) * int(span[1]) * int(span[2])


def order_sensitive(columns, keys):
    """True when, for some voxel and column, numpy's pairwise float32 sum differs from the sum in input order"""
    for k in np.unique(keys):
        rows = columns[keys == k]
        if rows.shape[0] > 8 and np.any(np.ascontiguousarray(rows.T).sum(1, dtype=f32) != np.add.accumulate(rows, axis=0, dtype=f32)[-1]):
            return True
    return False


@pytest.mark.parametrize("n,dl,seed", REF_CASES)
def test_reference_recorded_results(n, dl, seed):
    with open(GOLDEN) as f:
        golden = json.load(f)
    pts, feats, labels = reference_cloud(n, seed)
    for use_f, use_c in REF_VARIANTS:
        f, c = (feats if use_f else None), (labels if use_c else None)
        got = device(pts, f, c, dl)
        P, F, C = got[0], (got[1] if use_f else None), ((got[2] if use_f else got[1]) if use_c else None)
        assert rows_digest(P, F, C) == golden[golden_key(n, dl, seed, use_f, use_c)], (use_f, use_c)
        assert_same(got, host(pts, f, c, dl))


@pytest.mark.parametrize("n", [1, 257, 300001])
def test_bounds(n):
    """ct_voxel_bounds: exact minima and maxima (one workgroup, a partial second one, the full grid striding), NaN-propagating"""
    from cloud_transformers_amd import _lib
    lib = _lib.load()
    pts = cloud(n, 40 + n % 7)[0]

    def bounds(a):
        P, out = _up(a), torch.full((6,), 7.0, device="cuda")
        ws = torch.empty(lib.ct_voxel_bounds_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        _lib.check(lib.ct_voxel_bounds(P.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
                   "ct_voxel_bounds")
        return out.cpu().numpy()

    assert np.array_equal(bounds(pts), np.concatenate([pts.min(0), pts.max(0)]))
    pts[n // 2, 2] = np.nan
    assert np.isnan(bounds(pts)).all()
    pts[n // 2, 2] = -np.inf
    assert bounds(pts)[2] == -np.inf


def test_cell_edge_keys():
    """Points ON cell faces: the key is decided by the last bit of (p - org) / dl, a true fp32 division."""
    rng = np.random.default_rng(5)
    dl = f32(0.04)
    pts = rng.integers(-6, 7, (4000, 3)).astype(f32) * dl
    feats = rng.random((4000, 5), dtype=f32)
    labels = rng.integers(0, 13, (4000, 2)).astype(np.int32)
    org = np.floor(pts.min(0) * (f32(1) / dl)) * dl
    moved = np.any(np.floor((pts - org) / dl) != np.floor((pts - org) * (f32(1) / dl)), axis=1)
    assert moved.sum() > 0                  # a reciprocal-multiply would put these points into another cell
    got = device(pts, feats, labels, dl)
    assert_same(got, host(pts, feats, labels, dl))
    assert 0 < len(got[0]) < 4000


def test_keys_beyond_32_bits():
    pts, feats, labels = cloud(2000, 21)
    keys, cells = numpy_keys(pts, 1e-3)
    assert cells > 2 ** 38 and keys.max() > 2 ** 32 and len(np.unique(keys)) == 2000
    got = device(pts, feats, labels, 1e-3)
    assert len(got[0]) == 2000
    assert_same(got, host(pts, feats, labels, 1e-3))


@pytest.mark.parametrize("case", ["one_voxel", "one_voxel_three_scan_chunks", "mixed"])
def test_long_runs_sum_in_input_order(case):
    if case != "mixed":
        n = 3000 if case == "one_voxel" else 9000          # 9000: the run's flags cross two boundaries of the row scan's 4096-chunks
        rng = np.random.default_rng(7)
        pts = rng.uniform(0.5, 7.5, (n, 3)).astype(f32)
        feats = rng.random((n, 3), dtype=f32)
        labels = rng.integers(0, 13, (n, 1)).astype(np.int32)
        dl = 100.0
    else:
        pts, feats, labels = reference_cloud(20000, 13)
        dl = 1.5
    keys, _ = numpy_keys(pts, dl)
    assert order_sensitive(np.concatenate([pts, feats], 1), keys)      # else any summation order would pass
    got = device(pts, feats, labels, dl)
    assert_same(got, host(pts, feats, labels, dl))
    if case != "mixed":
        assert len(got[0]) == 1
    else:
        assert np.bincount(np.unique(keys, return_inverse=True)[1]).max() > 2000    # runs of many staging steps beside short ones


@pytest.mark.parametrize("n,dl,seed", [(5000, 0.3, 31), (4097, 0.04, 32), (3000, 100.0, 33)])
def test_inverse_and_counts(n, dl, seed):
    pts, feats, labels = reference_cloud(n, seed)
    keys, _ = numpy_keys(pts, dl)
    _, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    P, F, C, inverse, counts = device(pts, feats, labels, dl, return_inverse=True, return_counts=True)
    assert_same((P, F, C), host(pts, feats, labels, dl))
    assert inverse.dtype == np.int64 and counts.dtype == np.int64
    assert np.array_equal(inverse, inv.reshape(-1)) and np.array_equal(counts, cnt) and counts.sum() == n
    only_counts = device(pts, None, None, dl, return_counts=True)
    assert len(only_counts) == 2 and np.array_equal(only_counts[1], cnt)


def test_layout_and_errors():
    pts, feats, labels = cloud(500, 4)
    only = S.compute_device(_up(pts), sampleDl=0.7)
    assert isinstance(only, torch.Tensor) and np.array_equal(only.cpu().numpy(), S.compute(pts, sampleDl=0.7))
    assert_same(device(pts, feats, None, 0.7), host(pts, feats, None, 0.7))
    p, c = device(pts, None, labels[:, 0], 0.7)
    assert c.ndim == 1
    assert_same((p, c), host(pts, None, labels[:, 0], 0.7))
    got = S.grid_subsampling_device(_up(pts), _up(feats), _up(labels), sampleDl=0.7)
    assert_same(tuple(t.cpu().numpy() for t in got), S.grid_subsampling(pts, feats, labels, sampleDl=0.7))
    wide = np.random.default_rng(9).random((500, 11), dtype=f32)                # more float columns than one pass sums
    assert_same(device(pts, wide, labels, 0.7), host(pts, wide, labels, 0.7))
    assert_same(device(pts[:1], feats[:1], labels[:1], 0.7), host(pts[:1], feats[:1], labels[:1], 0.7))
    e = S.compute_device(_up(pts[:0]), features=_up(feats[:0]), classes=_up(labels[:0]), sampleDl=0.7, return_inverse=True)
    assert [tuple(t.shape) for t in e] == [(0, 3), (0, 3), (0, 1), (0,)] and all(t.is_cuda for t in e)
    dp, df = _up(pts), _up(feats)
    with pytest.raises(ValueError):
        S.compute_device(torch.from_numpy(pts), sampleDl=0.7)
    with pytest.raises(ValueError):
        S.compute_device(dp.double(), sampleDl=0.7)
    with pytest.raises(ValueError):
        S.compute_device(dp, sampleDl=0.0)
    with pytest.raises(ValueError):
        S.compute_device(dp, features=df[:-1], sampleDl=0.7)
    with pytest.raises(ValueError):
        S.compute_device(dp, classes=_up(labels).long(), sampleDl=0.7)
    bad = pts.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        S.compute_device(_up(bad), sampleDl=0.7)
    bad[17, 1] = np.inf
    with pytest.raises(ValueError, match="finite"):
        S.compute_device(_up(bad), sampleDl=0.7)
    with pytest.raises(ValueError, match="cells"):
        S.compute_device(_up(pts * f32(1e6)), sampleDl=1e-15)
    # nothing is kept between calls: other inputs on a side stream, then the first ones again
    pts2, feats2, labels2 = cloud(1300, 6)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got2 = device(pts2, feats2, labels2, 0.3)
    assert_same(got2, host(pts2, feats2, labels2, 0.3))
    assert_same(device(pts, feats, labels, 0.7), host(pts, feats, labels, 0.7))


def _write_area(root, area, rooms):
    for room, objects in rooms.items():
        ann = os.path.join(root, "Stanford3dDataset_v1.2", area, room, "Annotations")
        os.makedirs(ann, exist_ok=True)
        for name, rows in objects.items():
            np.savetxt(os.path.join(ann, name + ".txt"), np.asarray(rows, dtype=np.float64), fmt="%.3f")


def test_load_areas_on_the_device(tmp_path, monkeypatch):
    from cloud_transformers_amd.data import s3dis_kpconv as K
    rng = np.random.default_rng(8)
    obj = lambda n, lo: np.concatenate([rng.uniform(lo, lo + 1.0, (n, 3)), rng.integers(0, 256, (n, 3))], 1)   # noqa: E731
    _write_area(str(tmp_path), "Area_3", {"office_1": {"chair_1": obj(300, 0.0), "wall_1": obj(250, 0.5), "stairs_1": obj(200, 0.3)},
                                          "hallway_1": {"floor_1": obj(350, 0.2), "board_2": obj(200, 0.8)}})
    calls = []
    real = K.grid_subsampling_device
    monkeypatch.setattr(K, "grid_subsampling_device", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    fields = ("points", "colors", "labels", "sub_points", "sub_colors", "sub_labels")
    monkeypatch.delenv("CLOUDCT_GRID_SUBSAMPLE", raising=False)
    h, = K.load_areas(str(tmp_path), [3], sampleDl=0.25, cache_dir=str(tmp_path / "host"))
    assert not calls
    d, = K.load_areas(str(tmp_path), [3], sampleDl=0.25, cache_dir=str(tmp_path / "dev"), device="cuda")
    assert len(calls) == 1 and 0 < len(d.sub_points) < 1300
    monkeypatch.setenv("CLOUDCT_GRID_SUBSAMPLE", "host")
    e, = K.load_areas(str(tmp_path), [3], sampleDl=0.25, device=torch.device("cuda"))
    assert len(calls) == 1                                         # the switch is read where load_areas runs
    for f in fields:
        a = getattr(h, f)
        for other in (d, e):
            b = getattr(other, f)
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f
    with np.load(str(tmp_path / "host" / "Area_3_0.250.npz")) as zh, np.load(str(tmp_path / "dev" / "Area_3_0.250.npz")) as zd:
        assert sorted(zh.files) == sorted(zd.files) == sorted(fields)
        for f in fields:
            assert zh[f].dtype == zd[f].dtype and zh[f].tobytes() == zd[f].tobytes(), f
