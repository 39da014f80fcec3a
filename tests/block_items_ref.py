"""Helper of the ct_block_items / ct_seg_confusion tests (not a test): the entry points' contracts (include/cloudct.h) restated
in numpy, float32 throughout, operation for operation — every product, sum, quotient, min and max below is one fp32 rounding, in
the header's order — and the replay of the host loader's draws (data.datasets.Indoor3DSemSeg) into the contract's arguments."""
import random

import numpy as np

F = np.float32


def _order_key(a):
    """uint32 keys with the floats' order (-0 below +0), as the kernel reduces them."""
    u = np.ascontiguousarray(a, F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _order_unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(F)


def _rem1(x):
    """np.remainder(x, 1) spelt as the header spells it: x - trunc(x), + 1 when that is negative."""
    m = x - np.trunc(x)
    m = np.where(m != 0, np.where(m < 0, m + F(1), m), F(0)).astype(F)
    return m


def _clip01(v):
    return np.minimum(np.maximum(v, F(0)), F(1))


def block_items_reference(data, label, item, perm, aug, jit, cjit, N, sigma=0.01, clip=0.05, cstd=0.05):
    """data f32[M, P, 6], label u8[M, P], item i64[B], perm i64[B, N] | None, aug f32[B, 16] | None, jit, cjit f32[B, N, 3] | None
    -> (out f32[B, 6, N], out_label i64[B, N])."""
    data, label = np.asarray(data, F), np.asarray(label, np.uint8)
    M, P, six = data.shape
    B = len(item)
    assert six == 6 and 1 <= N <= P and (aug is None) == (jit is None) == (cjit is None)
    g = np.clip(np.asarray(item, np.int64), 0, M - 1)
    src = np.broadcast_to(np.arange(N), (B, N)) if perm is None else np.clip(np.asarray(perm, np.int64), 0, N - 1)
    v = data[g[:, None], src].copy()                                       # [B, N, 6]
    out_label = label[g[:, None], src].astype(np.int64)
    if aug is not None:
        A = np.asarray(aug, F)
        sigma, clip, cstd = F(sigma), F(clip), F(cstd)
        col = lambda k: A[:, k, None]                                      # noqa: E731  ([B, 1]: one draw per block)
        # 1. rotation about z
        c, s = col(0), col(1)
        x = (v[..., 0] * c) - (v[..., 1] * s)
        y = (v[..., 0] * s) + (v[..., 1] * c)
        p = np.stack([x, y, v[..., 2]], axis=-1)
        # 2. scale (the mirror's sign rides on x), 3. jitter
        p = p * A[:, None, 2:5]
        p = p + np.minimum(np.maximum(sigma * np.asarray(jit, F), -clip), clip)
        rgb = v[..., 3:6].copy()
        # 4. auto-contrast over the block's pool: its first N points
        for b in range(B):
            w = A[b, 5]
            if not w >= 0:
                continue
            pool = data[g[b], :N, 3:6]
            lo = _order_unkey(_order_key(pool).min(axis=0))
            hi = _order_unkey(_order_key(pool).max(axis=0))
            for i in range(3):
                if hi[i] != lo[i]:
                    st = (rgb[b, :, i] - lo[i]) * (F(1) / (hi[i] - lo[i]))
                    rgb[b, :, i] = ((F(1) - w) * rgb[b, :, i]) + (w * st)
        # 5. translation, 6. colour jitter
        shifted = _clip01(A[:, None, 6:9] + rgb)
        rgb = np.where(col(9)[..., None] != 0, shifted, rgb)
        jittered = _clip01((np.asarray(cjit, F) * cstd) + rgb)
        rgb = np.where(col(10)[..., None] != 0, jittered, rgb)
        # 7. hue / saturation through HSV on the 0..255 scale
        with np.errstate(invalid="ignore", divide="ignore"):
            f = rgb * F(255)
            r, gg, bb = f[..., 0], f[..., 1], f[..., 2]
            mx, mn = np.maximum(np.maximum(r, gg), bb), np.minimum(np.minimum(r, gg), bb)
            span = mx - mn
            grey = span == 0
            rc, gc, bc = (mx - r) / span, (mx - gg) / span, (mx - bb) / span
            h = np.where(r == mx, bc - gc, np.where(gg == mx, (F(2) + rc) - bc, (F(4) + gc) - rc))
            h = np.where(grey, F(0), h)
            sat = np.where(grey, F(0), span / np.where(mx == 0, F(1), mx))
        h = _rem1(h / F(6))
        h = _rem1((col(11) + h) + F(1))
        sat = _clip01(col(12) * sat)
        h6 = h * F(6)
        sector = np.trunc(h6).astype(np.int64)
        fr = h6 - sector.astype(F)
        pp, q, t = mx * (F(1) - sat), mx * (F(1) - (sat * fr)), mx * (F(1) - (sat * (F(1) - fr)))
        sector = sector % 6
        cond = [sat == 0, sector == 1, sector == 2, sector == 3, sector == 4, sector == 5]
        R = np.select(cond, [mx, q, pp, pp, t, mx], default=mx)
        G = np.select(cond, [mx, mx, mx, q, pp, pp], default=t)
        Bl = np.select(cond, [mx, pp, t, mx, mx, q], default=pp)
        # 8. the 8-bit levels
        rgb = np.trunc(np.minimum(np.maximum(np.stack([R, G, Bl], axis=-1), F(0)), F(255))) / F(255)
        assert p.dtype == F and rgb.dtype == F and h.dtype == F and sat.dtype == F and pp.dtype == F and fr.dtype == F
        v = np.concatenate([p, rgb], axis=-1)
    return np.ascontiguousarray(v.transpose(0, 2, 1), dtype=F), out_label


def seg_confusion_reference(pred, labels, conf=None):
    """pred f32[B, C, N], labels i64[B, N] -> conf i64[C, C] (rows truth, columns np.argmax's prediction), added into `conf`."""
    pred, labels = np.asarray(pred, F), np.asarray(labels, np.int64)
    C = pred.shape[1]
    conf = np.zeros((C, C), np.int64) if conf is None else conf.copy()
    arg = np.argmax(pred, axis=1)
    keep = (labels >= 0) & (labels < C)
    np.add.at(conf, (labels[keep], arg[keep]), 1)
    return conf


def replay_loader_draws(N, ratio=0.1, hue_max=0.5, sat_max=0.2):
    """Consume numpy's and python's global generators exactly as one `Indoor3DSemSeg(aug=True)[i]` does (data.datasets: shuffle;
    uniform() angle; uniform(0.8, 1.2, 3); uniform() mirror; randn(N, 3); random() [random() w]; random() [rand(1, 3)]; random()
    [randn(N, 3)]; random(), random()) and return them as the contract's arguments for one row: (perm i64[N], aug f32[16],
    jit f32[N, 3], cjit f32[N, 3], stages (contrast, translation, colour jitter))."""
    perm = np.arange(0, N)
    np.random.shuffle(perm)
    angle = np.random.uniform() * 2 * np.pi
    scale = np.random.uniform(0.8, 1.2, size=3)
    sign = np.round(np.random.uniform()) * 2 - 1
    jit = np.random.randn(N, 3)
    aug = np.zeros(16, np.float64)
    aug[0], aug[1] = np.cos(angle), np.sin(angle)
    aug[2:5] = scale * np.asarray([sign, 1, 1], dtype=np.float32)
    contrast = random.random() < 0.2
    aug[5] = random.random() if contrast else -1.0
    translation = random.random() < 0.95
    if translation:
        aug[6:9] = (np.random.rand(1, 3)[0] - 0.5) * 2 * ratio
    aug[9] = float(translation)
    colour = random.random() < 0.95
    cjit = np.random.randn(N, 3) if colour else np.zeros((N, 3))
    aug[10] = float(colour)
    aug[11] = (random.random() - 0.5) * 2 * hue_max
    aug[12] = 1 + (random.random() - 0.5) * 2 * sat_max
    return perm.astype(np.int64), aug.astype(F), jit.astype(F), cjit.astype(F), (contrast, translation, colour)
