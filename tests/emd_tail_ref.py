"""One cloud's auction (oracle/emd_ref.c, which ct_emd_fwd / ct_emd_fwd_counts / ct_emd_fwd_tail reproduce bit for bit) restated
in numpy, operation by operation, with what ct_emd_fwd_tail reports beside the result: the bidder count of every iteration.
The value is evaluated in double and rounded once, d2 in float32 by two fused multiply-adds (_fma)."""
import numpy as np


def _fma(a, b, c):
    """float32 fma(a, b, c) with one rounding: the product of two float32 numbers is exact in a 64-bit mantissa, and so is its
    sum with c except far below the float32 rounding point."""
    return (a.astype(np.longdouble) * b.astype(np.longdouble) + c.astype(np.longdouble)).astype(np.float32)


def auction(xyz1, xyz2, eps, iters):
    """xyz1, xyz2 f32[n,3] -> (dist f32[n], assignment i32[n], bidders: list of the bidder count of iterations 0 .. iters - 1).
    info of ct_emd_fwd_tail for this cloud is first_empty(bidders, iters), bidders[-1]."""
    p1 = np.ascontiguousarray(xyz1, dtype=np.float32)
    p2 = np.ascontiguousarray(xyz2, dtype=np.float32)
    n = p1.shape[0]
    eps = np.float32(eps)
    ass = np.full(n, -1, np.int32)
    ass_inv = np.full(n, -1, np.int32)
    price = np.zeros(n, np.float32)
    bidders = []
    for it in range(iters):
        last = it == iters - 1
        un = np.nonzero(ass == -1)[0]
        bidders.append(int(un.size))
        if un.size == 0:
            continue
        # Bid: every bidder against every target
        x2 = p2[None, :, 0] - p1[un, None, 0]
        y2 = p2[None, :, 1] - p1[un, None, 1]
        z2 = p2[None, :, 2] - p1[un, None, 2]
        d2 = _fma(z2, z2, _fma(y2, y2, x2 * x2))
        val = (3.0 - np.sqrt(d2).astype(np.float64) - price[None, :].astype(np.float64)).astype(np.float32)
        best_i = np.argmax(val, axis=1)                              # the first of equal maxima: the lowest index
        best = val[np.arange(un.size), best_i]
        if n > 1:
            masked = val.copy()
            masked[np.arange(un.size), best_i] = -np.inf
            better = np.maximum(masked.max(axis=1), np.float32(-1e9))
        else:
            better = np.full(un.size, -1e9, np.float32)
        inc = (best - better).astype(np.float32) + eps
        assert inc.dtype == np.float32
        # GetMax: per target the largest increment, then the highest bidder index inside the +-1e-6 window (in double)
        max_inc = np.full(n, -np.inf, np.float32)
        np.maximum.at(max_inc, best_i, inc)
        mi = max_inc[best_i].astype(np.float64)
        bi = inc.astype(np.float64)
        inside = (bi - 1e-6 <= mi) & (mi <= bi + 1e-6)
        max_idx = np.full(n, -1, np.int64)
        np.maximum.at(max_idx, best_i[inside], un[inside])
        # Assign
        if last:
            ass[un] = best_i
        else:
            win = max_idx[best_i] == un
            wj, wt = un[win], best_i[win]
            prev = ass_inv[wt]
            ass[prev[prev != -1]] = -1
            ass_inv[wt] = wj
            ass[wj] = wt
            price[wt] = price[wt] + inc[win]
    k = ass.astype(np.int64)
    dx, dy, dz = p1[:, 0] - p2[k, 0], p1[:, 1] - p2[k, 1], p1[:, 2] - p2[k, 2]
    dist = (dx * dx + dy * dy) + dz * dz
    assert dist.dtype == np.float32
    return dist, ass, bidders


def first_empty(bidders, iters):
    """info[:, 0]: the first iteration that began without a bidder, or iters."""
    for it, u in enumerate(bidders):
        if u == 0:
            return it
    return iters


def uniform_pair(n, seed, B=1):
    """The clouds of the issue's measurements: x1 drawn first, x2 after it, from one generator."""
    rng = np.random.default_rng(seed)
    x1 = rng.random((B, n, 3), dtype=np.float32)
    x2 = rng.random((B, n, 3), dtype=np.float32)
    return x1, x2
