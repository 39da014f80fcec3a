"""Barycentre voxel-grid subsampling (KPConv-style).  On the host: numpy front end of ct_grid_subsample
(include/cloudct_host.h, csrc/host/grid_subsampling.cpp).  On a HIP device: `compute_device` / `grid_subsampling_device`
(ct_voxel_bounds, ct_voxel_keys, torch's stable sort, ct_voxel_reduce: csrc/ct_voxel.hip), the same rows in the same order with the same
bits.  Mirrors the reference's call surface:
`datasets/s3dis_closer.py:13-31` `grid_subsampling(points, features, labels, sampleDl, verbose)` and the extension function
behind it, `cpp_wrappers.cpp_subsampling.grid_subsampling.compute(points, features=, classes=, sampleDl=, verbose=)`
(cpp_wrappers/cpp_subsampling/wrapper.cpp)."""
import ctypes

import numpy as np
import torch

from .. import _lib


def compute(points, features=None, classes=None, sampleDl=0.1, verbose=0):
    """points f32[N,3] (+ features f32[N,F], classes i32[N] or [N,L]) -> subsampled points (, features) (, classes):
    the tuple layout of the reference's extension — one array when only points are given, else a tuple in this order."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points must be [N, 3]")
    N = pts.shape[0]
    feats = cls = None
    fdim = ldim = 0
    if features is not None:
        feats = np.ascontiguousarray(features, dtype=np.float32)
        if feats.ndim != 2 or feats.shape[0] != N:
            raise ValueError("features must be [N, F]")
        fdim = feats.shape[1]
    cls_1d = False
    if classes is not None:
        cls = np.ascontiguousarray(classes, dtype=np.int32)
        cls_1d = cls.ndim == 1
        if cls_1d:
            cls = cls[:, None]
        if cls.ndim != 2 or cls.shape[0] != N:
            raise ValueError("classes must be [N] or [N, L]")
        cls = np.ascontiguousarray(cls)
        ldim = cls.shape[1]
    out_p = np.empty((N, 3), np.float32)
    out_f = np.empty((N, fdim), np.float32) if fdim else None
    out_c = np.empty((N, ldim), np.int32) if ldim else None
    f32p, i32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)      # noqa: E731
    M = _lib.load_host().ct_grid_subsample(ptr(pts, f32p), ptr(feats, f32p), ptr(cls, i32p), N, fdim, ldim, float(sampleDl),
                                           ptr(out_p, f32p), ptr(out_f, f32p), ptr(out_c, i32p))
    if M < 0:
        raise ValueError("ct_grid_subsample: bad argument (sampleDl must be > 0)")
    res = [out_p[:M].copy()]
    if fdim:
        res.append(out_f[:M].copy())
    if ldim:
        c = out_c[:M].copy()
        res.append(c[:, 0] if cls_1d else c)
    return res[0] if len(res) == 1 else tuple(res)


def grid_subsampling(points, features=None, labels=None, sampleDl=0.1, verbose=0):
    """datasets/s3dis_closer.py:13-31"""
    return compute(points, features=features, classes=labels, sampleDl=sampleDl, verbose=verbose)


def _device_tensor(t, name, dtype, dev):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or (dev is not None and t.device != dev):
        raise ValueError("%s must be a tensor on %s" % (name, "a HIP device" if dev is None else "the points' device"))
    if t.dtype != dtype:
        raise ValueError("%s must be %s" % (name, dtype))
    return t.contiguous()


def compute_device(points, features=None, classes=None, sampleDl=0.1, return_inverse=False, return_counts=False):
    """`compute` for tensors on a HIP device: points f32[N,3] (+ features f32[N,F], classes i32[N] or [N,L]) -> the same
    tuple layout in tensors on that device, then `inverse` i64[N] (each point's output row) and `counts` i64[M] when asked
    for.  Equal to `compute` array for array, rows in the same order.  Work on the current stream; the host reads back the
    grid record and M in one copy.  ValueError: a wrong shape, dtype or device, sampleDl <= 0, non-finite points, a grid of
    2^62 cells or more."""
    pts = _device_tensor(points, "points", torch.float32, None)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points must be [N, 3]")
    dev, N = pts.device, pts.shape[0]
    if N >= 1 << 31:
        raise ValueError("points: N must be below 2^31")
    feats = cls = None
    fdim = ldim = 0
    if features is not None:
        feats = _device_tensor(features, "features", torch.float32, dev)
        if feats.ndim != 2 or feats.shape[0] != N:
            raise ValueError("features must be [N, F]")
        fdim = feats.shape[1]
    cls_1d = False
    if classes is not None:
        cls = _device_tensor(classes, "classes", torch.int32, dev)
        cls_1d = cls.ndim == 1
        if cls_1d:
            cls = cls[:, None]
        if cls.ndim != 2 or cls.shape[0] != N:
            raise ValueError("classes must be [N] or [N, L]")
        ldim = cls.shape[1]
    dl = float(np.float32(sampleDl))
    if not (dl > 0.0 and np.isfinite(dl)):
        raise ValueError("sampleDl must be > 0")
    with torch.cuda.device(dev):
        i64 = dict(dtype=torch.int64, device=dev)
        out_p = torch.empty((N, 3), dtype=torch.float32, device=dev)
        out_f = torch.empty((N, fdim), dtype=torch.float32, device=dev) if fdim else None
        out_c = torch.empty((N, ldim), dtype=torch.int32, device=dev) if ldim else None
        inverse = torch.empty(N, **i64) if return_inverse else None
        counts = torch.empty(N, **i64) if return_counts else None
        M = 0
        if N > 0:
            lib = _lib.load()
            stream = torch.cuda.current_stream().cuda_stream
            ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
            bounds = torch.empty(6, dtype=torch.float32, device=dev)
            ws = torch.empty(lib.ct_voxel_bounds_workspace_bytes(N), dtype=torch.uint8, device=dev)
            _lib.check(lib.ct_voxel_bounds(pts.data_ptr(), N, bounds.data_ptr(), ws.data_ptr(), ws.numel(), stream), "ct_voxel_bounds")
            record = torch.zeros(_lib.VOXEL_GRID_BYTES // 8 + 1, **i64)          # the grid record, then M
            keys = torch.empty(N, **i64)
            _lib.check(lib.ct_voxel_keys(pts.data_ptr(), N, dl, bounds.data_ptr(), record.data_ptr(), keys.data_ptr(), stream),
                       "ct_voxel_keys")
            keys_sorted, order = torch.sort(keys, stable=True)
            del keys
            ws = torch.empty(lib.ct_voxel_reduce_workspace_bytes(N), dtype=torch.uint8, device=dev)
            _lib.check(lib.ct_voxel_reduce(keys_sorted.data_ptr(), order.data_ptr(), pts.data_ptr(), ptr(feats), ptr(cls), N, fdim, ldim,
                                           out_p.data_ptr(), ptr(out_f), ptr(out_c), ptr(inverse), ptr(counts),
                                           record.data_ptr() + _lib.VOXEL_GRID_BYTES, ws.data_ptr(), ws.numel(), stream),
                       "ct_voxel_reduce")
            rec = record.cpu().numpy()
            if rec[:2].view(np.int32)[3] != 0:
                raise ValueError("points must be finite")
            if int(rec[2]) * int(rec[3]) * int(rec[4]) >= _lib.VOXEL_MAX_CELLS:
                raise ValueError("a grid of %d x %d x %d cells: sampleDl is too small for the points' extent"
                                 % (int(rec[2]), int(rec[3]), int(rec[4])))
            M = int(rec[5])
    res = [out_p[:M].clone()]
    if fdim:
        res.append(out_f[:M].clone())
    if ldim:
        c = out_c[:M].clone()
        res.append(c[:, 0] if cls_1d else c)
    if return_inverse:
        res.append(inverse)
    if return_counts:
        res.append(counts[:M].clone())
    return res[0] if len(res) == 1 else tuple(res)


def grid_subsampling_device(points, features=None, labels=None, sampleDl=0.1):
    """datasets/s3dis_closer.py:13-31 on a HIP device"""
    return compute_device(points, features=features, classes=labels, sampleDl=sampleDl)
