"""Neighbour search and the S3DIS KPConv loader without a GPU: the ct_nbr_* entry points reject bad arguments before
touching the device, their workspace query is host arithmetic, and load_areas reads the Stanford3dDataset_v1.2 layout."""
import ctypes
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from cloud_transformers_amd import _lib
    _lib.build()
    return _lib.load()


def _buf(n=256):
    b = ctypes.create_string_buffer(n)
    return ctypes.cast(b, ctypes.c_void_p), b


def test_index_build_rejects_bad_arguments(lib):
    from cloud_transformers_amd import _lib
    p, keep = _buf()
    o, d = _lib.float_array([0, 0, 0]), _lib.int_array([4, 4, 4])
    ws = 1 << 20
    assert lib.ct_nbr_index_build(None, 8, o, 0.5, d, p, p, p, p, ws, None) == -1          # null points
    assert lib.ct_nbr_index_build(p, 8, o, 0.5, d, None, p, p, p, ws, None) == -1          # null cell_start
    assert lib.ct_nbr_index_build(p, 8, o, 0.0, d, p, p, p, p, ws, None) == -1             # h <= 0
    assert lib.ct_nbr_index_build(p, 8, o, -1.0, d, p, p, p, p, ws, None) == -1
    assert lib.ct_nbr_index_build(p, 8, o, float("nan"), d, p, p, p, p, ws, None) == -1
    assert lib.ct_nbr_index_build(p, 0, o, 0.5, d, p, p, p, p, ws, None) == -1             # M = 0
    assert lib.ct_nbr_index_build(p, 1 << 31, o, 0.5, d, p, p, p, p, ws, None) == -1       # M >= 2^31
    big = _lib.int_array([1024, 1024, 65])                                                 # > 2^26 cells
    assert lib.ct_nbr_index_build(p, 8, o, 0.5, big, p, p, p, p, ws, None) == -1
    assert lib.ct_nbr_index_build(p, 8, o, 0.5, _lib.int_array([0, 4, 4]), p, p, p, p, ws, None) == -1
    assert lib.ct_nbr_index_build(p, 8, None, 0.5, d, p, p, p, p, ws, None) == -1
    assert lib.ct_nbr_index_build(p, 8, o, 0.5, d, p, p, p, p, 4, None) == -3              # workspace too small
    del keep


def test_queries_reject_bad_arguments(lib):
    from cloud_transformers_amd import _lib
    p, keep = _buf()
    o, d = _lib.float_array([0, 0, 0]), _lib.int_array([4, 4, 4])
    assert lib.ct_nbr_radius(p, p, o, 0.5, d, p, 1, 1.0, 16385, p, p, p, None) == -1       # K > 16384
    assert lib.ct_nbr_radius(p, p, o, 0.5, d, p, 1, 1.0, 0, p, p, p, None) == -1           # K < 1
    assert lib.ct_nbr_radius(p, p, o, 0.5, d, p, 1, -0.1, 8, p, p, p, None) == -1          # r < 0
    assert lib.ct_nbr_radius(p, p, o, 0.5, d, p, 1, float("nan"), 8, p, p, p, None) == -1
    assert lib.ct_nbr_radius(None, p, o, 0.5, d, p, 1, 1.0, 8, p, p, p, None) == -1
    assert lib.ct_nbr_radius(p, p, o, 0.5, d, None, 1, 1.0, 8, p, p, p, None) == -1
    assert lib.ct_nbr_radius(p, p, o, 0.0, d, p, 1, 1.0, 8, p, p, p, None) == -1           # h <= 0
    assert lib.ct_nbr_radius(p, p, o, 0.5, _lib.int_array([1 << 13, 1 << 13, 2]), p, 1, 1.0, 8, p, p, p, None) == -1
    assert lib.ct_nbr_radius(p, p, o, 0.5, d, p, 0, 1.0, 8, p, p, p, None) == -1           # Q < 1
    assert lib.ct_nbr_nearest(None, p, o, 0.5, d, p, 4, p, p, None) == -1
    assert lib.ct_nbr_nearest(p, p, o, 0.5, d, p, 4, None, p, None) == -1
    assert lib.ct_nbr_nearest(p, p, o, -0.5, d, p, 4, p, p, None) == -1
    assert lib.ct_nbr_nearest(p, p, o, 0.5, _lib.int_array([1 << 26, 2, 1]), p, 4, p, p, None) == -1
    assert lib.ct_nbr_nearest(p, p, o, 0.5, d, p, 0, p, p, None) == -1
    del keep


def test_index_workspace_is_host_arithmetic(lib):
    from cloud_transformers_amd import _lib
    d = _lib.int_array([10, 20, 30])
    # two int32 per point (cell, slot in cell) + one per 4096-cell scan block, each 256-byte aligned
    nb = (10 * 20 * 30 + 1 + 4095) // 4096
    assert lib.ct_nbr_index_workspace_bytes(1000, d) == 2 * 4096 + ((nb * 4 + 255) // 256) * 256
    assert lib.ct_nbr_index_workspace_bytes(1 << 20, d) == 2 * (4 << 20) + 256
    assert lib.ct_nbr_index_workspace_bytes(0, d) == 0
    assert lib.ct_nbr_index_workspace_bytes(10, _lib.int_array([1 << 14, 1 << 13, 1])) == 0    # > 2^26 cells


def test_grid_index_refuses_cpu_tensors():
    import torch
    from cloud_transformers_amd.neighbors import GridIndex
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GridIndex(torch.zeros(4, 3))


def _write_area(root, area, rooms):
    for room, objects in rooms.items():
        ann = os.path.join(root, "Stanford3dDataset_v1.2", area, room, "Annotations")
        os.makedirs(ann, exist_ok=True)
        for name, rows in objects.items():
            np.savetxt(os.path.join(ann, name + ".txt"), np.asarray(rows, dtype=np.float64), fmt="%.3f")
        with open(os.path.join(root, "Stanford3dDataset_v1.2", area, room, room + ".txt"), "w") as f:
            f.write("0 0 0 0 0 0\n")       # the room's unlabelled whole-room file: not read


def test_load_areas_tiny_tree(tmp_path):
    from cloud_transformers_amd.data.s3dis_kpconv import load_areas, NAME_TO_LABEL
    rng = np.random.default_rng(0)

    def obj(n, lo):
        xyz = rng.uniform(lo, lo + 1.0, (n, 3))
        rgb = rng.integers(0, 256, (n, 3))
        return np.concatenate([xyz, rgb], 1)

    rooms = {"office_1": {"chair_1": obj(30, 0.0), "stairs_1": obj(20, 2.0), "wall_2": obj(25, 4.0)},
             "hallway_1": {"clutter_3": obj(15, 6.0), "board_1": obj(10, 8.0)}}
    _write_area(str(tmp_path), "Area_5", rooms)
    cache = str(tmp_path / "cache")
    a, = load_areas(str(tmp_path), [5], sampleDl=0.25, cache_dir=cache)
    assert a.name == "Area_5"
    assert a.points.shape == (100, 3) and a.points.dtype == np.float32
    assert a.colors.dtype == np.float32 and a.colors.max() <= 255 and a.colors.min() >= 0
    # rooms and objects in name order: hallway_1 (board, clutter) then office_1 (chair, stairs, wall)
    want = ([NAME_TO_LABEL["board"]] * 10 + [NAME_TO_LABEL["clutter"]] * 15 + [NAME_TO_LABEL["chair"]] * 30 +
            [NAME_TO_LABEL["clutter"]] * 20 + [NAME_TO_LABEL["wall"]] * 25)
    np.testing.assert_array_equal(a.labels, np.asarray(want, np.int32))
    first = np.loadtxt(str(tmp_path / "Stanford3dDataset_v1.2" / "Area_5" / "hallway_1" / "Annotations" / "board_1.txt"))
    np.testing.assert_array_equal(a.points[:10], first[:, :3].astype(np.float32))
    np.testing.assert_array_equal(a.colors[:10], first[:, 3:6].astype(np.uint8).astype(np.float32))
    # subsampled: colours / 255, labels squeezed and drawn from the input's
    assert a.sub_points.ndim == 2 and 0 < a.sub_points.shape[0] <= 100
    assert a.sub_colors.max() <= 1.0 and a.sub_labels.ndim == 1 and a.sub_labels.shape[0] == a.sub_points.shape[0]
    assert set(a.sub_labels.tolist()) <= set(want)
    from cloud_transformers_amd.data.subsampling import grid_subsampling
    sp, sc, sl = grid_subsampling(a.points, features=a.colors, labels=a.labels[:, None], sampleDl=0.25)
    np.testing.assert_array_equal(a.sub_points, sp)
    np.testing.assert_array_equal(a.sub_colors, sc / np.float32(255))
    np.testing.assert_array_equal(a.sub_labels, sl[:, 0])
    # the cache holds arrays, and reading it back gives the same Area
    assert os.path.exists(os.path.join(cache, "Area_5_0.250.npz"))
    b, = load_areas(str(tmp_path / "nowhere"), ["Area_5"], sampleDl=0.25, cache_dir=cache)
    for f in ("points", "colors", "labels", "sub_points", "sub_colors", "sub_labels"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f))


def test_load_areas_rejects_unknown_objects(tmp_path):
    from cloud_transformers_amd.data.s3dis_kpconv import load_areas
    _write_area(str(tmp_path), "Area_1", {"room_1": {"unicorn_1": [[0, 0, 0, 1, 2, 3]]}})
    with pytest.raises(ValueError, match="Unknown object name"):
        load_areas(str(tmp_path / "Stanford3dDataset_v1.2"), ["Area_1"])


def test_sorted_records_must_be_16_byte_aligned(lib):
    """`sorted` is read and written as float4 records: a misaligned pointer is refused before any launch."""
    from cloud_transformers_amd import _lib
    p, keep = _buf(1 << 12)
    base = p.value + (-p.value % 16)
    al, mis = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    o, d = _lib.float_array([0, 0, 0]), _lib.int_array([4, 4, 4])
    assert lib.ct_nbr_index_build(al, 8, o, 0.5, d, al, al, mis, al, 1 << 20, None) == -1
    assert lib.ct_nbr_radius(al, mis, o, 0.5, d, al, 1, 1.0, 8, al, al, al, None) == -1
    assert lib.ct_nbr_nearest(al, mis, o, 0.5, d, al, 4, al, al, None) == -1
    del keep


def test_nearest_query_count_fits_one_launch(lib):
    from cloud_transformers_amd import _lib
    p, keep = _buf()
    o, d = _lib.float_array([0, 0, 0]), _lib.int_array([4, 4, 4])
    assert lib.ct_nbr_nearest(p, p, o, 0.5, d, p, 1 << 31, p, p, None) == -1            # Q >= 2^31: split into calls
    assert lib.ct_nbr_nearest(p, p, o, 0.5, d, p, 1 << 40, p, p, None) == -1
    del keep
