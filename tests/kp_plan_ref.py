"""The contract of ct_kp_plan (include/cloudct.h) restated in numpy float32, operation by operation: a brute-force ball in
the (d2, index) order of ct_nbr_radius, the lowest index among the minima, one rounding per operation."""
import numpy as np


def ball(points, centre, r, K):
    """ct_nbr_radius of one centre: (the first min(count, K) indices by (d2, index), their float32 d2, count)."""
    d = points - centre[None, :]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2.dtype == np.float32
    r = np.float32(r)
    sel = np.nonzero(d2 <= r * r)[0]
    o = sel[np.lexsort((sel, d2[sel]))][:K]
    return o, d2[o], sel.size


def plan(points, potentials, noise, r, K):
    """n = len(noise) picks over the clouds `points` (list of f32[M,3]) from the initial `potentials` (list of f32[M]) and the
    scaled noise f32[n,3]; r a Python float.  Returns (cloud i64[n], point i64[n], picks f32[n,3], final potentials,
    final min_potentials f32[clouds])."""
    pots = [np.array(p, dtype=np.float32) for p in potentials]
    noise = np.asarray(noise, dtype=np.float32)
    mins = np.array([p.min() for p in pots], dtype=np.float32)
    args = [int(np.argmin(p)) for p in pots]                       # numpy's argmin: the first of equal minima
    inv = np.float32(1.0) / np.float32(r * r)                       # r * r in double, rounded once, then the fp32 reciprocal
    n = noise.shape[0]
    cloud, point, picks = np.empty(n, np.int64), np.empty(n, np.int64), np.empty((n, 3), np.float32)
    for i in range(n):
        c = int(np.argmin(mins))
        p = args[c]
        pick = points[c][p] + noise[i]
        assert pick.dtype == np.float32
        idx, d2, _ = ball(points[c], pick, r, K)
        t = np.float32(1.0) - d2 * inv
        pots[c][idx] = pots[c][idx] + t * t
        assert t.dtype == np.float32
        mins[c], args[c] = pots[c].min(), int(np.argmin(pots[c]))
        cloud[i], point[i], picks[i] = c, p, pick
    return cloud, point, picks, pots, mins
