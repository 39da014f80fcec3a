"""Tile staging of the hot-shape kernels (csrc/ct_raster_hot.h: stage_tile_ci, stage_tile_pairs) at the edges of its batches.

A lane stages ITEMS of 4 consecutive cells (one 16-byte load per row, four 16-byte LDS words), two items per batch, the
second one predicated — so the shapes here are chosen for the item counts, not for size: fewer items than threads, a ragged
last batch, exactly one full batch, several batches and several chunks, and planes with exact ties, where Splat(max)
backward stages a tied group's pairs a second time.

Every case forces the hot family (DEBUG_FORCE_HOT), asserts the launch tags of the staged passes, and compares z, out, g_z,
g_feat and g_keys with the CPU oracle at the bars of test_headline_gpu.py (z of Splat(max) bit-exact, 1e-4 of the tensor's
max elsewhere) and with the generic kernels (DEBUG_NO_HOT) at 1e-5."""
import pytest
import torch

from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

NAMES = ("z", "out", "g_z", "g_feat", "g_keys")

CASES = [
    # B, H, C, N, W, pad, duplicated points
    (1, 2, 4, 256, (8, 8), False, False),        # i:   32 pair items / 16 interleaved items for 512 threads
    (2, 2, 12, 516, (16, 24), True, False),      # ii:  576 pair items = 4.5 per 4 threads: the second item of the batch is ragged
    (2, 3, 8, 1024, (32, 32), False, False),     # iii: 1024 pair items = exactly one full batch of 2 x 512
    (1, 1, 32, 4096, (48, 40), False, False),    # iv:  several batches, several chunks, whole-CU LDS
    (1, 1, 20, 2048, (16, 16), True, False),     # v:   pad mask, odd chunk count
    (1, 2, 8, 256, (8, 8), False, True),         # vi:  exact ties, small
    (1, 2, 16, 4096, (32, 32), False, True),     # vii: exact ties at the headline tile size: the tied-group redo re-stages a tile
    (2, 2, 16, 1024, (16, 16, 16), False, False),    # viii: 3D, several batches
    (2, 2, 12, 516, (6, 8, 10), True, False),        # ix:   3D, pad mask, 120 items per row group: ragged everywhere
]


def _lib():
    from cloud_transformers_amd import _lib
    return _lib, _lib.load()


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(1e-30, float(b.abs().max())))


def hip_chain(keys, feat, cot, W, H, dim, reduce, pad):
    """The four passes one by one (the backward of each op on its own, so that each leaves its own launch tag)."""
    from cloud_transformers_amd import ops
    _, lib = _lib()
    tags = {}
    k = keys.clone().requires_grad_(True)
    f = feat.clone().requires_grad_(True)
    z = ops.splat_keys(k, f, pad, W, H, dim, reduce)
    tags["splat_fwd"] = lib.ct_debug_last_launch().decode()
    zl = z.detach().requires_grad_(True)
    o = ops.slice_keys(k, zl, pad, W, H, dim)
    tags["slice_fwd"] = lib.ct_debug_last_launch().decode()
    g_z, gk_slice = torch.autograd.grad(o, (zl, k), cot)
    tags["slice_bwd"] = lib.ct_debug_last_launch().decode()
    g_f, gk_splat = torch.autograd.grad(z, (f, k), g_z)
    tags["splat_bwd"] = lib.ct_debug_last_launch().decode()
    return (z.detach(), o.detach(), g_z, g_f, gk_slice + gk_splat), tags


def oracle_chain(keys, feat, cot, W, H, dim, reduce, pad):
    k = keys.clone().requires_grad_(True)
    f = feat.clone().requires_grad_(True)
    lc, idx = R.positions(k, W, H, dim)
    z = R.splat(lc, idx, f, pad, W, H, dim, reduce)
    z.retain_grad()
    o = R.slice_(lc, idx, z, pad, W, H, dim)
    o.backward(cot)
    return z.detach(), o.detach(), z.grad, f.grad, k.grad


@pytest.fixture
def flags():
    mod, lib = _lib()
    yield lambda v: lib.ct_debug_set_flags(v)
    lib.ct_debug_set_flags(0)


def _compare(got, ref, bar, copies_summed, what):
    """All five tensors within `bar` of the reference's max; with duplicated points (copies_summed: half the cloud's length)
    which of two identical points wins a cell is unspecified, so g_feat and g_keys are compared as the sum over the copies."""
    for name, a, r in zip(NAMES, got, ref):
        a, r = a.cpu(), r.cpu()
        if copies_summed and name in ("g_feat", "g_keys"):
            h = copies_summed
            a, r = a[..., :h] + a[..., h:], r[..., :h] + r[..., h:]
        e = relerr(a, r)
        print("%s %s: %.3e (bar %.0e)" % (what, name, e, bar))
        assert e <= bar, "%s %s: %.2e" % (what, name, e)


@pytest.mark.parametrize("reduce", ["max", "sum"])
@pytest.mark.parametrize("cfg", CASES, ids=[str(c) for c in CASES])
def test_staged_tiles_against_oracle_and_generic_kernels(cfg, reduce, flags):
    mod, lib = _lib()
    B, H, C, N, W, use_pad, dup = cfg
    dim = len(W)
    g = torch.Generator().manual_seed(B * 131 + C * 7 + N + len(W))
    keys = torch.tanh(torch.randn(B, H * dim, N, generator=g))
    feat = torch.randn(B, H * C, N, generator=g)
    if dup:
        keys = keys[..., : N // 2].repeat(1, 1, 2)
        feat = feat[..., : N // 2].repeat(1, 1, 2)
    cot = torch.randn(B, H * C, N, generator=g)
    pad = (torch.rand(B, N, generator=g) > 0.2).float() if use_pad else None
    ref = oracle_chain(keys, feat, cot, list(W), H, dim, reduce, pad)
    dev = [t.cuda() for t in (keys, feat, cot)] + [None if pad is None else pad.cuda()]

    flags(mod.DEBUG_FORCE_HOT)
    got, tags = hip_chain(dev[0], dev[1], dev[2], list(W), H, dim, reduce, dev[3])
    flags(0)
    print("tags", tags)
    sfx = "" if dim == 2 else "3"
    assert tags["slice_fwd"] == "gather_ci" + sfx, tags
    assert tags["slice_bwd"].startswith(("slice_bwd_fused" + sfx, "slice_bwd_sorted")), tags
    if reduce == "max":
        assert tags["splat_bwd"].startswith("splat_max_bwd_hot" + sfx), tags
    elif dim == 2:
        # one pass with the plane's whole g_grid tile in LDS where it fits a CU's (160 KiB - 512), else the staged gather
        # for g_feat and the generic key cotangent
        G = W[0] * W[1]
        assert tags["splat_bwd"] == ("splat_sum_bwd_hot" if C * G * 4 <= 160 * 1024 - 512 else "gather_ci+gather_gw_quad"), tags

    # exact ties only exist under max: a sum has no winner to choose
    halves = N // 2 if (dup and reduce == "max") else 0
    if reduce == "max":
        assert torch.equal(got[0].cpu(), ref[0]), "z is not bit-exact"
    _compare(got, ref, 1e-4, halves, "oracle")

    flags(mod.DEBUG_NO_HOT)
    gen, gtags = hip_chain(dev[0], dev[1], dev[2], list(W), H, dim, reduce, dev[3])
    flags(0)
    assert gtags["slice_fwd"] in ("gather_quad", "gather_generic"), gtags
    assert not gtags["splat_bwd"].startswith(("splat_max_bwd_hot", "splat_sum_bwd_hot")), gtags
    _compare(got, gen, 1e-5, halves, "generic")
