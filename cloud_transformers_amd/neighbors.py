"""Neighbour search on the GPU (csrc/ct_nbr.hip, include/cloudct.h `ct_nbr_*`): what the S3DIS KPConv protocol asks of
sklearn's CPU KDTree (datasets/s3dis_closer.py:204 `KDTree(sub_points)`, :262-265,319-322 `query_radius(..., sort_results=True)`
cut to num_points, :290 `query(points)`).  A uniform grid of cells, counting-sorted on the device; no CPU path.

Distances are squared, ((dx*dx) + (dy*dy)) + (dz*dz) with d = p - c in float32: numpy float32 computes the same bits, so a
brute force in numpy reproduces every output exactly (ties: the lower index first)."""
import math

import numpy as np
import torch

from . import _lib
from .ops import _dev, _on, _stream

# default cell: aim at ~6 points per occupied cell (4-8 is the target band)
_TARGET_PER_CELL = 6.0
NEAREST_CHUNK = 1 << 24      # queries per ct_nbr_nearest / ct_nbr_knn launch


def _knn_k(k):
    k = int(k)
    if not 1 <= k <= _lib.NBR_KNN_K_MAX:
        raise ValueError("query_knn: k must be in [1, %d]" % _lib.NBR_KNN_K_MAX)
    return k


def _knn_tensor(x, device, name, dtype, what, ok):
    """The k-nearest methods' argument check: ValueError for a wrong dtype or shape, then for a tensor that is not on `device`
    (a CPU tensor included)."""
    if not torch.is_tensor(x) or x.dtype != dtype or not ok(x):
        raise ValueError("%s must be %s" % (name, what))
    if not x.is_cuda or x.device != device:
        raise ValueError("%s must be on %s; there is no CPU fallback" % (name, device))
    return x.contiguous()


def _knn_queries(x, device):
    return _knn_tensor(x, device, "queries", torch.float32, "float32 [Q, 3]", lambda t: t.dim() == 2 and t.shape[1] == 3)


def _dims_for(lo, hi, h):
    return [int(math.floor((hi[a] - lo[a]) / h)) + 1 for a in range(3)]


class GridIndex:
    """Uniform-grid index of a HIP f32[M, 3] cloud (1 <= M < 2^31).

    The box is read from the device once at build time.  `cell` (the cell edge) defaults to the edge, out of a ladder
    of candidates, whose occupied cells hold closest to ~6 points each (one more device-to-host read: the candidates'
    occupied-cell counts, computed together); every candidate respects the cap of 2^26 cells."""

    def __init__(self, points, cell=None):
        _dev(points)
        if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
            raise ValueError("GridIndex needs float32 points of shape [M, 3]")
        M = points.shape[0]
        if not 1 <= M < 2 ** 31:
            raise ValueError("GridIndex needs 1 <= M < 2^31 points, got %d" % M)
        self.points = points.contiguous()
        self.device = points.device
        self.M = M
        box = torch.cat(torch.aminmax(self.points, dim=0)).cpu().numpy()       # the one read of the box
        lo, hi = [float(v) for v in box[:3]], [float(v) for v in box[3:]]
        if not all(math.isfinite(v) for v in lo + hi):
            raise ValueError("GridIndex: points must be finite")
        h = self._default_cell(lo, hi) if cell is None else float(cell)
        h = float(np.float32(h))                                              # the kernels' h, exactly
        if not (h > 0 and math.isfinite(h)):
            raise ValueError("GridIndex: cell must be > 0")
        dims = _dims_for(lo, hi, h)
        if math.prod(dims) > _lib.NBR_MAX_CELLS:
            raise ValueError("GridIndex: cell %g gives %d cells, more than 2^26" % (h, math.prod(dims)))
        self.origin, self.h, self.dims = [float(np.float32(v)) for v in lo], h, dims
        self._origin_c, self._dims_c = _lib.float_array(self.origin), _lib.int_array(dims)
        ncells = math.prod(dims)
        dev = self.device
        self.cell_start = torch.empty(ncells + 1, dtype=torch.int32, device=dev)
        self.order = torch.empty(M, dtype=torch.int32, device=dev)
        self.sorted = torch.empty(M, 4, dtype=torch.float32, device=dev)
        lib = _lib.load()
        ws = torch.empty(lib.ct_nbr_index_workspace_bytes(M, self._dims_c), dtype=torch.uint8, device=dev)
        with _on(dev):
            _lib.check(lib.ct_nbr_index_build(self.points.data_ptr(), M, self._origin_c, h, self._dims_c, self.cell_start.data_ptr(),
                                              self.order.data_ptr(), self.sorted.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)),
                       "ct_nbr_index_build")

    def _default_cell(self, lo, hi):
        ext = [max(hi[a] - lo[a], 0.0) for a in range(3)]
        span = [e for e in ext if e > 0]
        if self.M == 1 or not span:
            return 1.0
        # the edge at which the cloud, filling its box, would put the target count in every cell; surfaces occupy fewer
        # cells (larger edges), dense clusters more (smaller ones): a ladder of edges a factor sqrt(2) apart around it
        h0 = (math.prod(span) * _TARGET_PER_CELL / self.M) ** (1.0 / len(span))
        h_cap = h0 / 8.0
        while math.prod(_dims_for(lo, hi, h_cap)) > _lib.NBR_MAX_CELLS:
            h_cap *= 1.25
        cands = sorted(set(max(h_cap, h0 * 2.0 ** (i / 2.0)) for i in range(-6, 9)))
        lo_t = torch.tensor(lo, dtype=torch.float32, device=self.device)
        occ = []
        for h in cands:
            nx, ny, nz = _dims_for(lo, hi, h)
            c = torch.floor((self.points - lo_t) / h).long()
            c[:, 0].clamp_(0, nx - 1), c[:, 1].clamp_(0, ny - 1), c[:, 2].clamp_(0, nz - 1)
            ids = torch.sort((c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]).values
            occ.append((ids[1:] != ids[:-1]).sum() + 1)
        occ = torch.stack(occ).cpu().numpy()
        per = self.M / occ
        score = np.abs(np.log(per / _TARGET_PER_CELL))
        return cands[int(np.argmin(score))]

    def _query_tensor(self, x, name):
        _dev(x)
        if x.device != self.device:
            raise ValueError("%s must be on %s" % (name, self.device))
        if x.dim() != 2 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise ValueError("%s must be float32 [Q, 3]" % name)
        return x.contiguous()

    def query_radius(self, centres, r, k):
        """KDTree.query_radius(centres, r, sort_results=True) cut to the first k: (idx i64[Q,k], d2 f32[Q,k], count i64[Q]).
        count is the full number of points with d2 <= r^2; slots past min(count, k) hold -1 / +inf."""
        c = self._query_tensor(centres, "centres")
        k = int(k)
        if not 1 <= k <= _lib.NBR_K_MAX:
            raise ValueError("query_radius: k must be in [1, %d]" % _lib.NBR_K_MAX)
        if not float(r) >= 0:
            raise ValueError("query_radius: r must be >= 0")
        Q = c.shape[0]
        dev = self.device
        idx = torch.empty(Q, k, dtype=torch.int64, device=dev)
        d2 = torch.empty(Q, k, dtype=torch.float32, device=dev)
        count = torch.empty(Q, dtype=torch.int64, device=dev)
        if Q == 0:
            return idx, d2, count
        with _on(dev):
            _lib.check(_lib.load().ct_nbr_radius(self.cell_start.data_ptr(), self.sorted.data_ptr(), self._origin_c, self.h, self._dims_c,
                                                 c.data_ptr(), Q, float(r), k, idx.data_ptr(), d2.data_ptr(), count.data_ptr(),
                                                 _stream(dev)), "ct_nbr_radius")
        return idx, d2, count

    def nearest(self, queries):
        """KDTree.query(queries, k=1): (idx i64[Q], d2 f32[Q]); the lowest index wins a tie.  Any query position is exact,
        outside the grid's box included; launched in chunks of NEAREST_CHUNK queries (no workspace)."""
        q = self._query_tensor(queries, "queries")
        Q = q.shape[0]
        dev = self.device
        idx = torch.empty(Q, dtype=torch.int64, device=dev)
        d2 = torch.empty(Q, dtype=torch.float32, device=dev)
        lib = _lib.load()
        with _on(dev):
            st = _stream(dev)
            for a in range(0, Q, NEAREST_CHUNK):
                n = min(NEAREST_CHUNK, Q - a)
                _lib.check(lib.ct_nbr_nearest(self.cell_start.data_ptr(), self.sorted.data_ptr(), self._origin_c, self.h, self._dims_c,
                                              q[a:].data_ptr(), n, idx[a:].data_ptr(), d2[a:].data_ptr(), st), "ct_nbr_nearest")
        return idx, d2

    def query_knn(self, queries, k):
        """KDTree.query(queries, k), 1 <= k <= 64: (idx i64[Q,k], d2 f32[Q,k]), the k nearest points by (d2, index)
        ascending (the order of `query_radius`, the tie rule of `nearest`); a cloud of fewer than k points leaves -1 / +inf
        in the tail, and so does a query with a non-finite coordinate in every slot.  Any query position is exact; one
        wavefront per query, launched in chunks of NEAREST_CHUNK queries (no workspace).  For finite queries k = 1 gives `nearest`'s bits."""
        k = _knn_k(k)
        q = _knn_queries(queries, self.device)
        Q = q.shape[0]
        dev = self.device
        idx = torch.empty(Q, k, dtype=torch.int64, device=dev)
        d2 = torch.empty(Q, k, dtype=torch.float32, device=dev)
        lib = _lib.load()
        with _on(dev):
            st = _stream(dev)
            for a in range(0, Q, NEAREST_CHUNK):
                n = min(NEAREST_CHUNK, Q - a)
                _lib.check(lib.ct_nbr_knn(self.cell_start.data_ptr(), self.sorted.data_ptr(), self._origin_c, self.h, self._dims_c,
                                          q[a:].data_ptr(), n, k, idx[a:].data_ptr(), d2[a:].data_ptr(), st), "ct_nbr_knn")
        return idx, d2

    def interpolate(self, values, queries, k=3, eps=1e-8):
        """Inverse-distance interpolation of `values` f32[M,C] (one row per indexed point) at `queries`: f32[Q,C], the mean of
        each query's k nearest rows weighted by 1 / (d2 + eps).  `query_knn` followed by ct_nbr_interp, in float32 in the
        order include/cloudct.h states; the gathered rows [Q,k,C] are never formed.  A query with a non-finite
        coordinate has no neighbour and gets NaN."""
        k = _knn_k(k)
        eps = float(eps)
        if not eps >= 0:
            raise ValueError("interpolate: eps must be >= 0")
        values = _knn_tensor(values, self.device, "values", torch.float32, "float32 [%d, C] with C >= 1" % self.M,
                             lambda t: t.dim() == 2 and t.shape[0] == self.M and t.shape[1] >= 1)
        idx, d2 = self.query_knn(queries, k)
        return _interp(idx, d2, values, eps)


def _interp(idx, d2, values, eps):
    """ct_nbr_interp over a finished table, in chunks of NEAREST_CHUNK queries."""
    Q, k = idx.shape
    M, C = values.shape
    dev = values.device
    out = torch.empty(Q, C, dtype=torch.float32, device=dev)
    lib = _lib.load()
    with _on(dev):
        st = _stream(dev)
        for a in range(0, Q, NEAREST_CHUNK):
            n = min(NEAREST_CHUNK, Q - a)
            _lib.check(lib.ct_nbr_interp(idx[a:].data_ptr(), d2[a:].data_ptr(), n, k, values.data_ptr(), M, C, eps,
                                         out[a:].data_ptr(), st), "ct_nbr_interp")
    return out


class GridIndexTable:
    """The grids of several `GridIndex`es in one device-resident table (include/cloudct.h `ct_nbr_table_*`), so that a query
    takes each centre's cloud from a device tensor and nothing is read back to choose an index.  `offsets[c]` is cloud c's
    first row in the concatenated clouds (default: the clouds back to back).  The table keeps the indices alive; it is
    filled on the host and uploaded once, here."""

    def __init__(self, indices, offsets=None):
        self.indices = list(indices)
        n = len(self.indices)
        if n < 1:
            raise ValueError("GridIndexTable needs at least one GridIndex")
        self.device = self.indices[0].device
        if any(ix.device != self.device for ix in self.indices):
            raise ValueError("GridIndexTable: every GridIndex must be on %s" % self.device)
        if offsets is None:
            offsets = [0] + list(np.cumsum([ix.M for ix in self.indices])[:-1])
        self.offsets = [int(o) for o in offsets]
        if len(self.offsets) != n:
            raise ValueError("GridIndexTable: one offset per GridIndex")
        self.n_clouds = n
        self.max_points = max(ix.M for ix in self.indices)
        lib = _lib.load()
        host = torch.zeros(lib.ct_nbr_table_bytes(n), dtype=torch.uint8)
        for i, (ix, off) in enumerate(zip(self.indices, self.offsets)):
            _lib.check(lib.ct_nbr_table_set(host.data_ptr(), n, i, ix.cell_start.data_ptr(), ix.sorted.data_ptr(), ix._origin_c, ix.h,
                                            ix._dims_c, ix.M, off), "ct_nbr_table_set")
        self.table = host.to(self.device)

    def query_radius(self, cloud, centres, r, k):
        """`GridIndex.query_radius` of centre q in cloud[q] (i64[Q], on the device), all Q in one launch: the same
        (idx i64[Q,k], d2 f32[Q,k], count i64[Q])."""
        c = self.indices[0]._query_tensor(centres, "centres")
        _dev(cloud)
        if cloud.device != self.device or cloud.dtype != torch.int64 or cloud.dim() != 1 or cloud.shape[0] != c.shape[0]:
            raise ValueError("query_radius: cloud must be int64 [Q] on %s" % self.device)
        cloud = cloud.contiguous()
        k = int(k)
        if not 1 <= k <= _lib.NBR_K_MAX:
            raise ValueError("query_radius: k must be in [1, %d]" % _lib.NBR_K_MAX)
        if not float(r) >= 0:
            raise ValueError("query_radius: r must be >= 0")
        Q = c.shape[0]
        dev = self.device
        idx = torch.empty(Q, k, dtype=torch.int64, device=dev)
        d2 = torch.empty(Q, k, dtype=torch.float32, device=dev)
        count = torch.empty(Q, dtype=torch.int64, device=dev)
        if Q == 0:
            return idx, d2, count
        with _on(dev):
            _lib.check(_lib.load().ct_nbr_radius_multi(self.table.data_ptr(), self.n_clouds, cloud.data_ptr(), c.data_ptr(), Q, float(r),
                                                       k, idx.data_ptr(), d2.data_ptr(), count.data_ptr(), _stream(dev)),
                       "ct_nbr_radius_multi")
        return idx, d2, count

    def query_knn(self, cloud, queries, k):
        """`GridIndex.query_knn` of query q in cloud[q] (i64[Q], on the device; ids outside the table are clamped into it):
        the same (idx i64[Q,k], d2 f32[Q,k]), idx counting inside the query's own cloud."""
        k = _knn_k(k)
        q = _knn_queries(queries, self.device)
        cloud = _knn_tensor(cloud, self.device, "cloud", torch.int64, "int64 [Q]", lambda t: t.dim() == 1 and t.shape[0] == q.shape[0])
        Q = q.shape[0]
        dev = self.device
        idx = torch.empty(Q, k, dtype=torch.int64, device=dev)
        d2 = torch.empty(Q, k, dtype=torch.float32, device=dev)
        lib = _lib.load()
        with _on(dev):
            st = _stream(dev)
            for a in range(0, Q, NEAREST_CHUNK):
                n = min(NEAREST_CHUNK, Q - a)
                _lib.check(lib.ct_nbr_knn_multi(self.table.data_ptr(), self.n_clouds, cloud[a:].data_ptr(), q[a:].data_ptr(), n, k,
                                                idx[a:].data_ptr(), d2[a:].data_ptr(), st), "ct_nbr_knn_multi")
        return idx, d2
