"""Helper of the ct_scan_items tests (not a test): the entry point's contract (include/cloudct.h) restated in numpy, float32
throughout, operation for operation — every product, sum, min and max below is one fp32 rounding, in the header's order."""
import numpy as np

F = np.float32


def scan_items_reference(data, mask, label, item, perm, rot, jit, N, sigma=0.01, clip=0.05):
    """data f32[M, P, 3], mask u8[M, P], label i64[M], item i64[B], perm i64[B, P] | None, rot f32[B, 2] | None,
    jit f32[B, N, 3] | None -> (points f32[B, 3, N], mask f32[B, N], label i64[B])."""
    data, mask, label = np.asarray(data, F), np.asarray(mask, np.uint8), np.asarray(label, np.int64)
    M, P, _ = data.shape
    B = len(item)
    assert (rot is None) == (jit is None) and 1 <= N <= P
    g = np.clip(np.asarray(item, np.int64), 0, M - 1)
    src = np.broadcast_to(np.arange(N), (B, N)) if perm is None else np.clip(np.asarray(perm, np.int64)[:, :N], 0, P - 1)
    q = data[g[:, None], src]                                              # [B, N, 3]
    out_mask = mask[g[:, None], src].astype(F)
    if jit is not None:
        sigma, clip = F(sigma), F(clip)
        d = np.minimum(np.maximum(sigma * np.asarray(jit, F), -clip), clip)
        q = q + d
        c, s = np.asarray(rot, F)[:, 0, None], np.asarray(rot, F)[:, 1, None]
        x = (q[..., 0] * c) - (q[..., 2] * s)
        z = (q[..., 0] * s) + (q[..., 2] * c)
        q = np.stack([x, q[..., 1], z], axis=-1)
        assert q.dtype == F
    return np.ascontiguousarray(q.transpose(0, 2, 1), dtype=F), out_mask, label[g]


def golden_draws(gold, name):
    """The arguments of the contract for the golden file's items "sub" (subsample 64) or "full" (all points), from its replayed
    draws cast to float32: item = 0..M-1; perm = the choice followed by the points it left out (None for "full"); jit = the
    randn rows at the chosen points; rot = (cos, sin) of 2 pi * uniform, taken in float64 as upstream does, then cast.
    -> (item, perm, rot, jit, N)"""
    M, P, _ = gold["data"].shape
    angle = gold["uniform"] * 2 * np.pi
    rot = np.stack([np.cos(angle), np.sin(angle)], axis=1).astype(F)
    item = np.arange(M, dtype=np.int64)
    if name == "full":
        return item, None, rot, gold["randn"].astype(F), P
    choice = gold["choice"]
    perm = np.stack([np.concatenate([choice[i], np.setdiff1d(np.arange(P), choice[i])]) for i in range(M)]).astype(np.int64)
    jit = np.stack([gold["randn"][i][choice[i]] for i in range(M)]).astype(F)
    return item, perm, rot, jit, choice.shape[1]
