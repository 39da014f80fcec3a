"""The contract of ct_image_items (include/cloudct.h) restated in numpy, independent of the package's own table builder:
Pillow's 8-bit BILINEAR resample as two integer passes with their coefficient tables, the fp32 ToTensor / Normalize stage, and
`resample_pcd` on explicit draws.  tests/test_image_items_cpu.py settles its agreement with Pillow itself (live, and through
tests/golden/image_items.npz); tests/test_image_items_gpu.py holds the kernel to it bit for bit."""
import math

import numpy as np

IMAGENET_MEAN = [0.485, 0.456, 0.406]
IMAGENET_STD = [0.229, 0.224, 0.225]
PRECISION_BITS = 32 - 8 - 2

# (H, W, OH, OW): the shapes the restatement was checked on against Pillow
SHAPES = [(224, 224, 128, 128), (137, 137, 128, 128), (7, 5, 3, 4), (5, 9, 8, 16), (64, 64, 128, 128), (128, 128, 128, 128),
          (224, 160, 128, 91), (9, 224, 5, 128), (300, 300, 16, 16)]


def axis_tables(n_in, n_out):
    """(k i32[n_out, ksize], bounds i32[n_out, 2] = (min, taps)) of one axis, everything in float64 as Pillow's precompute_coeffs."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs                                         # the bilinear filter's support is 1
    ksize = 2 * int(math.ceil(support)) + 1
    k = np.zeros((n_out, ksize), np.int32)
    bounds = np.zeros((n_out, 2), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        taps = min(int(center + support + 0.5), n_in) - xmin
        w = np.zeros(taps, np.float64)
        for x in range(taps):
            w[x] = max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs))
        total = 0.0
        for x in range(taps):
            total += w[x]
        for x in range(taps):
            if total != 0.0:
                w[x] /= total
            k[xx, x] = int(-0.5 + w[x] * (1 << PRECISION_BITS)) if w[x] < 0 else int(0.5 + w[x] * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, taps)
    return k, bounds


def _clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resample_axis0(img, k, bounds):
    """One pass along axis 0 of img u8[n_in, ...] -> u8[n_out, ...], 32-bit integer accumulation."""
    out = np.empty((k.shape[0],) + img.shape[1:], np.uint8)
    for i in range(k.shape[0]):
        lo, taps = int(bounds[i, 0]), int(bounds[i, 1])
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), np.int32)
        for x in range(taps):
            acc = acc + img[lo + x].astype(np.int32) * np.int32(k[i, x])
        out[i] = _clip8(acc)
    return out


def resize_bilinear(img, OH, OW):
    """Pillow's Image.fromarray(img).resize((OW, OH), BILINEAR) for img u8[H, W, 3]: the horizontal pass into 8-bit
    intermediates, then the vertical pass."""
    H, W, _ = img.shape
    kx, bx = axis_tables(W, OW)
    ky, by = axis_tables(H, OH)
    mid = resample_axis0(np.ascontiguousarray(img.transpose(1, 0, 2)), kx, bx).transpose(1, 0, 2)
    return resample_axis0(np.ascontiguousarray(mid), ky, by)


def float_stage(img8):
    """ToTensor and Normalize of img8 u8[OH, OW, 3] -> f32[3, OH, OW]: ((float)byte / 255.0f - mean) / std, one fp32 rounding each."""
    mean = np.asarray(IMAGENET_MEAN, np.float32).reshape(3, 1, 1)
    std = np.asarray(IMAGENET_STD, np.float32).reshape(3, 1, 1)
    v = img8.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    return ((v - mean) / std).astype(np.float32)


def image_reference(images, item, OH, OW):
    """out_img f32[B, 3, OH, OW] for images u8[M, H, W, 3] and item [B]."""
    done = {}
    for g in set(int(i) for i in item):
        done[g] = float_stage(resize_bilinear(images[g], OH, OW))
    return np.stack([done[int(i)] for i in item])


def pcd_reference(points, offsets, item, perm, u_dup, n):
    """out_pcd f32[B, 3, n]: slot j < min(n, P) takes the j-th entry of perm[b] below P; slot j >= P takes point
    min(int(fp32(u_dup[b, j] * P)), P - 1)."""
    out = np.zeros((len(item), 3, n), np.float32)
    for b, g in enumerate(item):
        cloud = points[int(offsets[g]):int(offsets[g + 1])]
        P = cloud.shape[0]
        kept = perm[b][perm[b] < P]
        idx = np.empty(n, np.int64)
        m = min(n, P)
        idx[:m] = kept[:m]
        if n > P:
            f = (u_dup[b, P:].astype(np.float32) * np.float32(P)).astype(np.float32)
            idx[P:] = np.minimum(f.astype(np.int64), P - 1)
        out[b] = cloud[idx].T
    return out
