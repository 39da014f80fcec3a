"""The device voxel-grid subsampling without a GPU: ct_voxel_bounds / ct_voxel_keys / ct_voxel_reduce and the workspace queries
(include/cloudct.h, csrc/ct_voxel.hip) are declared, exported and bound, the workspace queries are host arithmetic, the calls
refuse bad arguments before touching a device, `compute_device` raises its documented ValueErrors on CPU tensors, and
`load_areas(device=None)` is the host path it always was."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cloud_transformers_amd.data import subsampling as S

EINVAL, EWORKSPACE = -1, -3
SYMBOLS = ("ct_voxel_bounds_workspace_bytes", "ct_voxel_bounds", "ct_voxel_keys", "ct_voxel_reduce_workspace_bytes", "ct_voxel_reduce")


@pytest.fixture(scope="module")
def lib():
    from cloud_transformers_amd import _lib
    _lib.build()
    return _lib.load()


def _buf(n=4096):
    b = ctypes.create_string_buffer(n + 64)
    a = ctypes.addressof(b)
    return b, ctypes.c_void_p((a + 63) & ~63)                      # 64-byte aligned inside b


def test_symbols_are_declared_exported_and_bound(lib):
    from cloud_transformers_amd import _lib
    with open(os.path.join(_lib.INCLUDE, "cloudct.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"^(int|size_t) %s\(" % name, header, re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "ct_voxel.hip" in _lib.HIP_SOURCES and _lib.ABI_VERSION == 3       # additive: no bump
    assert "grid_subsampling.cpp:4-104" in header and "datasets/s3dis_closer.py:13-31" in header


def test_workspace_bytes_is_host_arithmetic(lib):
    q = lib.ct_voxel_reduce_workspace_bytes
    assert q(0) == 0 and q(-1) == 0 and q(2 ** 31) == 0 and q(2 ** 40) == 0
    sizes = [1, 2, 63, 64, 4095, 4096, 4097, 10 ** 6, 44 * 10 ** 6, 2 ** 31 - 1]
    got = [q(n) for n in sizes]
    assert all(g > 0 for g in got) and got == sorted(got) and got[0] < got[-1]
    assert all(g >= 8 * n for g, n in zip(got, sizes))             # a row number and a run start per point, at least
    assert got[-1] < 9 * 2 ** 31


def test_bounds_rejects_bad_arguments(lib):
    keep, p = _buf(1 << 15)
    q = lib.ct_voxel_bounds_workspace_bytes
    assert q(0) == 0 and q(-1) == 0 and q(2 ** 31) == 0
    assert q(1) == 24 and q(256) == 24 and q(257) == 48 and q(10 ** 6) == q(2 ** 31 - 1) == 1024 * 24     # 6 floats per workgroup
    need = q(1000)

    def call(*, points=p, N=1000, bounds=p, ws=p, ws_bytes=need):
        return lib.ct_voxel_bounds(points, N, bounds, ws, ws_bytes, None)

    assert call(points=None) == EINVAL and call(bounds=None) == EINVAL
    assert call(N=0) == EINVAL and call(N=-1) == EINVAL and call(N=2 ** 31) == EINVAL
    assert call(ws=None) == EWORKSPACE and call(ws_bytes=need - 1) == EWORKSPACE
    assert call(ws=ctypes.c_void_p(p.value + 2)) == EWORKSPACE
    del keep


def test_keys_rejects_bad_arguments(lib):
    keep, p = _buf()

    def call(*, points=p, N=100, dl=0.04, bounds=p, grid=p, keys=p):
        return lib.ct_voxel_keys(points, N, dl, bounds, grid, keys, None)

    assert call(points=None) == EINVAL and call(bounds=None) == EINVAL and call(grid=None) == EINVAL and call(keys=None) == EINVAL
    assert call(N=0) == EINVAL and call(N=-3) == EINVAL and call(N=2 ** 31) == EINVAL
    assert call(dl=0.0) == EINVAL and call(dl=-0.04) == EINVAL and call(dl=float("nan")) == EINVAL and call(dl=float("inf")) == EINVAL
    assert call(grid=ctypes.c_void_p(p.value + 4)) == EINVAL       # the record holds i64 fields
    del keep


def test_reduce_rejects_bad_arguments(lib):
    keep, p = _buf()
    need = lib.ct_voxel_reduce_workspace_bytes(100)

    def call(*, ks=p, order=p, points=p, features=p, classes=p, N=100, F=3, L=1, out_p=p, out_f=p, out_c=p, inverse=None, counts=None,
             M=p, ws=p, ws_bytes=need):
        return lib.ct_voxel_reduce(ks, order, points, features, classes, N, F, L, out_p, out_f, out_c, inverse, counts, M, ws, ws_bytes,
                                   None)

    for name in ("ks", "order", "points", "features", "classes", "out_p", "out_f", "out_c", "M"):
        assert call(**{name: None}) == EINVAL, name
    assert call(N=0) == EINVAL and call(N=-1) == EINVAL and call(N=2 ** 31) == EINVAL
    assert call(F=-1) == EINVAL and call(L=-1) == EINVAL
    assert call(ws=None) == EWORKSPACE and call(ws_bytes=need - 1) == EWORKSPACE and call(ws_bytes=0) == EWORKSPACE
    assert call(ws=None, N=0) == EINVAL                            # arguments are judged before the workspace
    del keep


def test_compute_device_refuses_cpu_tensors_and_bad_arguments():
    pts = torch.zeros(8, 3)
    with pytest.raises(ValueError, match="HIP device"):
        S.compute_device(pts, sampleDl=0.1)
    with pytest.raises(ValueError):
        S.compute_device(np.zeros((8, 3), np.float32), sampleDl=0.1)
    with pytest.raises(ValueError):
        S.grid_subsampling_device(pts, torch.zeros(8, 3), torch.zeros(8, 1, dtype=torch.int32), sampleDl=0.1)
    with pytest.raises(ValueError):
        S.compute_device(pts, sampleDl=0.0)


def _write_area(root, area, rooms):
    for room, objects in rooms.items():
        ann = os.path.join(root, "Stanford3dDataset_v1.2", area, room, "Annotations")
        os.makedirs(ann, exist_ok=True)
        for name, rows in objects.items():
            np.savetxt(os.path.join(ann, name + ".txt"), np.asarray(rows, dtype=np.float64), fmt="%.3f")


def test_load_areas_without_a_device_is_the_host_path(tmp_path, monkeypatch):
    from cloud_transformers_amd.data import s3dis_kpconv as K
    rng = np.random.default_rng(3)
    obj = lambda n, lo: np.concatenate([rng.uniform(lo, lo + 1.0, (n, 3)), rng.integers(0, 256, (n, 3))], 1)   # noqa: E731
    _write_area(str(tmp_path), "Area_2", {"office_1": {"chair_1": obj(120, 0.0), "wall_1": obj(90, 0.5)},
                                          "hallway_2": {"floor_1": obj(150, 0.2)}})

    def never(*a, **k):
        raise AssertionError("the device path ran without a device")

    monkeypatch.setattr(K, "grid_subsampling_device", never)
    cache = str(tmp_path / "cache")
    a, = K.load_areas(str(tmp_path), [2], sampleDl=0.25, cache_dir=cache)
    b, = K.load_areas(str(tmp_path), [2], sampleDl=0.25, device=None)
    sp, sc, sl = S.grid_subsampling(a.points, features=a.colors, labels=a.labels[:, None], sampleDl=0.25)
    assert 0 < len(sp) < 360
    for area in (a, b):
        assert area.sub_points.tobytes() == sp.tobytes() and area.sub_colors.tobytes() == (sc / np.float32(255)).tobytes()
        assert area.sub_labels.tobytes() == sl[:, 0].tobytes()
    with np.load(os.path.join(cache, "Area_2_0.250.npz")) as z:
        assert sorted(z.files) == ["colors", "labels", "points", "sub_colors", "sub_labels", "sub_points"]
        assert z["sub_points"].tobytes() == sp.tobytes()
