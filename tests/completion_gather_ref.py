"""The contract of ct_completion_gather (include/cloudct.h), restated in numpy from explicit draws, float32 throughout; and
helpers shared by the CPU and GPU tests of the resident completion path."""
import numpy as np


def restrict(perm_row, length):
    """The entries of a permutation row that are below `length`, in order: a permutation of `length`."""
    perm_row = np.asarray(perm_row)
    return perm_row[(perm_row >= 0) & (perm_row < length)]


def mirror_signs(u):
    """(sx, sz) of RandomMirrorPoints for the draw u; None: no mirror."""
    if u is None:
        return np.float32(1), np.float32(1)
    u = np.float32(u)
    sx = np.float32(-1) if u <= np.float32(0.5) else np.float32(1)
    sz = np.float32(-1) if (u <= np.float32(0.25) or np.float32(0.5) < u <= np.float32(0.75)) else np.float32(1)
    return sx, sz


def _sample(cloud, perm_row, cap, n):
    """RandomSamplePoints on a passed-in permutation of `cap`: (rows f32[min(n, L), 3], L)."""
    L = min(max(cloud.shape[0], 0), cap)
    if perm_row is None:
        return cloud[:min(n, L)], L
    return cloud[restrict(perm_row, L)[:n]], L


def reference_gather(partial_points, partial_offsets, gt_points, gt_offsets, R, p_cap, g_cap, item, rendering, perm_in, perm_gt,
                     u_mirror, gt_scale, n_in, n_out):
    """-> (out_partial f32[B, n_in, 3], out_gt f32[B, n_out, 3]).  Rows past the cloud's length are +0; the mirror is a product
    with +-1 (a sign flip), gt then takes one float32 multiply by gt_scale."""
    partial_points, gt_points = np.asarray(partial_points, np.float32), np.asarray(gt_points, np.float32)
    M = len(gt_offsets) - 1
    B = len(item)
    out_partial = np.zeros((B, n_in, 3), np.float32)
    out_gt = np.zeros((B, n_out, 3), np.float32)
    for b in range(B):
        m = int(np.clip(item[b], 0, M - 1))
        r = int(np.clip(rendering[b], 0, R - 1))
        c = m * R + r
        sx, sz = mirror_signs(None if u_mirror is None else u_mirror[b])
        sign = np.array([sx, 1, sz], np.float32)
        rows, _ = _sample(partial_points[partial_offsets[c]:partial_offsets[c + 1]], perm_in[b], p_cap, n_in)
        out_partial[b, :len(rows)] = rows * sign
        rows, _ = _sample(gt_points[gt_offsets[m]:gt_offsets[m + 1]], None if perm_gt is None else perm_gt[b], g_cap, n_out)
        out_gt[b, :len(rows)] = np.float32(gt_scale) * (rows * sign)
    return out_partial, out_gt


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def synthetic_split(lengths_partial, lengths_gt, R, seed=0, zero_rows=True):
    """Host arrays of a split with the given cloud lengths (partial: M * R of them, gt: M): distinct non-zero rows, and, with
    `zero_rows`, the second row of every cloud of at least three rows exactly (0, 0, 0)."""
    rng = np.random.default_rng(seed)

    def clouds(lengths):
        out = []
        for n in lengths:
            p = rng.uniform(0.05, 1.0, (n, 3)).astype(np.float32) * rng.choice(np.array([-1, 1], np.float32), (n, 3))
            if zero_rows and n >= 3:
                p[1] = 0.0
            out.append(p)
        return np.concatenate(out), np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)

    assert len(lengths_partial) == len(lengths_gt) * R
    pp, po = clouds(lengths_partial)
    gp, go = clouds(lengths_gt)
    return pp, po, gp, go
