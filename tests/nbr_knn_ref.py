"""Numpy restatement of the k-nearest query and its interpolation (include/cloudct.h ct_nbr_knn / ct_nbr_interp): the same
float32 operations in the same order, so the device results must match bit for bit."""
import numpy as np


def d2_all(P, x):
    """((dx*dx) + (dy*dy)) + (dz*dz), d = p - x, in float32: the d2 of every point of P f32[M,3] to one query x f32[3]."""
    with np.errstate(over="ignore", invalid="ignore"):
        d = P - x[None, :]
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def knn_ref(P, X, k):
    """(idx i64[Q,k], d2 f32[Q,k]): the k nearest points of P to each row of X by (d2, index) ascending, the tail -1 / +inf;
    a row of X with a non-finite coordinate has no neighbour."""
    P, X = np.ascontiguousarray(P, np.float32), np.ascontiguousarray(X, np.float32)
    Q = X.shape[0]
    idx = np.full((Q, k), -1, np.int64)
    d2 = np.full((Q, k), np.inf, np.float32)
    ids = np.arange(P.shape[0])
    for q in range(Q):
        if not np.isfinite(X[q]).all():
            continue
        dd = d2_all(P, X[q])
        o = np.lexsort((ids, dd))[:k]
        idx[q, :o.size] = o
        d2[q, :o.size] = dd[o]
    return idx, d2


def interp_ref(idx, d2, values, eps):
    """w_j = 1 / (d2_j + eps) over the slots with idx_j >= 0, s = ((w_0 + w_1) + ...), out = ((w_0 / s) * v_0 + (w_1 / s) * v_1)
    + ..., all float32 in slot order; a row without a usable slot is NaN."""
    values = np.ascontiguousarray(values, np.float32)
    eps = np.float32(eps)
    one = np.float32(1.0)
    Q, K = idx.shape
    out = np.full((Q, values.shape[1]), np.nan, np.float32)
    with np.errstate(all="ignore"):
        for q in range(Q):
            slots = [j for j in range(K) if idx[q, j] >= 0]
            if not slots:
                continue
            w = [one / (np.float32(d2[q, j]) + eps) for j in slots]
            s = w[0]
            for wj in w[1:]:
                s = np.float32(s + wj)
            acc = None
            for wj, j in zip(w, slots):
                term = np.float32(wj / s) * values[idx[q, j]]
                acc = term if acc is None else acc + term
            out[q] = acc
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
