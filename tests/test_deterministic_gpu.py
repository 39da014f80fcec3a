"""Deterministic mode on the GPU (include/cloudct.h: ct_set_deterministic).

Splat(max) backward: the winner of a (cell, channel) is the LOWEST POINT INDEX among the contributions whose product is positive
and bit-equal to z, on every shape and under every family flag (the mode routes every call to ONE kernel family, splat_max_bwd_det*,
except the banded C = 4 kernels where CT_DEBUG_FORCE_BAND selects them: two families name the winners); g_keys is summed in a fixed order.  Chamfer backward: every
destination row is its own term first, then its sources in ascending index.  Grouped-conv weight gradient and the lattice
parameter cotangents: ordered sums (workspaces always passed), CT_EPRECOND from the library for a NULL workspace.
Bars: 1e-5 x sum|terms| for g_feat, 1e-4 relative for g_keys (tests/test_tie_rule_gpu.py); run-to-run: torch.equal."""
import math

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu


def _mod():
    from cloud_transformers_amd import _lib
    return _lib, _lib.load()


@pytest.fixture(autouse=True)
def _library_state():
    """every test leaves the switches as it found them"""
    mod, lib = _mod()
    yield
    lib.ct_debug_set_flags(0)
    lib.ct_debug_set_nseg(0)
    lib.ct_set_deterministic(0)


def _splat_bwd(keys, feat, gz, pad, Ws, H, dim, flags=0, nseg=0, det=True, lc_form=False):
    """(z, g_feat, g_keys, tag) of ops.splat_keys (or, lc_form, (z, g_feat, g_lc, tag) of ops.splat_lc) on the GPU"""
    import cloud_transformers_amd as ct
    from cloud_transformers_amd import ops
    mod, lib = _mod()
    fd = feat.cuda().requires_grad_(True)
    padd = None if pad is None else pad.cuda()
    lib.ct_debug_set_flags(flags)
    lib.ct_debug_set_nseg(nseg)
    try:
        with ct.deterministic(det):
            if lc_form:
                lc, idx = R.positions(keys, Ws, H, dim)
                pd = lc.cuda().requires_grad_(True)
                z = ops.splat_lc(pd, idx.cuda(), fd, padd, Ws, H, dim, "max")
            else:
                pd = keys.cuda().requires_grad_(True)
                z = ops.splat_keys(pd, fd, padd, Ws, H, dim, "max")
            z.backward(gz.cuda())
            torch.cuda.synchronize()
            tag = lib.ct_debug_last_launch().decode()
    finally:
        lib.ct_debug_set_flags(0)
        lib.ct_debug_set_nseg(0)
    return z.detach().cpu(), fd.grad.cpu(), pd.grad.cpu(), tag


def _reference(keys, feat, gz, pad, z, Ws, H, dim):
    """The lowest-index rule on the CPU from oracle.ref_cpu.positions: (g_feat, sum|terms| of g_feat, g_keys).
    winner of (cell, channel) = lowest n whose fp32 product (f * pad) * w is positive and bit-equal to the GPU's forward z."""
    B, HC, N = feat.shape
    C, G, V = HC // H, math.prod(Ws), 1 << dim
    k = keys.clone().requires_grad_(True)
    lc, idx = R.positions(k, Ws, H, dim)                                   # (B, H, V, N)
    w = lc.detach()
    f = feat.reshape(B, H, C, N)
    p = None if pad is None else pad.to(torch.float32)[:, None, None, :]
    if p is not None:
        f = f * p
    prod = f[:, :, :, None, :] * w[:, :, None]                             # (B, H, C, V, N), fp32
    cells = idx[:, :, None].expand(B, H, C, V, N).reshape(B, H, C, V * N)
    zv = z.reshape(B, H, C, G).gather(3, cells).reshape(B, H, C, V, N)
    match = (prod == zv) & (prod > 0)
    n_of = torch.arange(N).expand(B, H, C, V, N)
    owner = torch.full((B, H, C, G), N, dtype=torch.int64)
    owner.scatter_reduce_(3, cells, torch.where(match, n_of, torch.full_like(n_of, N)).reshape(B, H, C, V * N), "amin")
    win = match & (owner.gather(3, cells).reshape(B, H, C, V, N) == n_of)
    gzv = gz.reshape(B, H, C, G).gather(3, cells).reshape(B, H, C, V, N) * win
    terms = gzv * w[:, :, None]
    g_feat, scale = terms.sum(3), terms.abs().sum(3)
    if p is not None:
        g_feat, scale = g_feat * p, scale * p
    g_lc = (gzv * f[:, :, :, None, :]).sum(2)                              # (B, H, V, N)
    lc.backward(g_lc)
    return g_feat.reshape(B, HC, N), scale.reshape(B, HC, N), k.grad, g_lc


def _duplicated(B, H, C, N, dim, seed, pad_dtype=None):
    """points N/2 .. N-1 are exact copies of 0 .. N/2-1 (keys, features, mask); features in [0.5, 1.5)"""
    g = torch.Generator().manual_seed(seed)
    h = N // 2
    keys = torch.tanh(torch.randn(B, H * dim, N, generator=g))
    feat = torch.rand(B, H * C, N, generator=g) + 0.5
    keys[:, :, h:] = keys[:, :, :h]
    feat[:, :, h:] = feat[:, :, :h]
    pad = None
    if pad_dtype is not None:
        pad = (torch.rand(B, N, generator=g) > 0.15).to(pad_dtype)
        pad[:, h:] = pad[:, :h]
    return keys, feat, pad, g


# name, dim, W, C, N, B, H, nseg, mask dtype, tag of the deterministic kernel
DUP_CASES = [
    ("2d_register_form", 2, 32, 8, 1024, 2, 16, 0, None, "splat_max_bwd_det"),
    ("2d_through_memory", 2, 32, 8, 8192, 2, 16, 0, None, "splat_max_bwd_det"),
    ("3d", 3, 8, 8, 1024, 2, 16, 0, None, "splat_max_bwd_det"),
    ("3d_ragged", 3, 8, 8, 1000, 2, 16, 0, None, "splat_max_bwd_det"),
    ("2d_segments_tickets", 2, 16, 16, 4096, 2, 4, 4, None, "splat_max_bwd_det"),
    ("2d_claims_in_workspace", 2, 256, 1, 1024, 1, 2, 0, None, "splat_max_bwd_det_global"),
    ("3d_claim_tile_alone_in_lds", 3, 32, 2, 1024, 1, 2, 0, None, "splat_max_bwd_det"),
    ("2d_mask_f32", 2, 32, 8, 1024, 2, 16, 0, torch.float32, "splat_max_bwd_det"),
    ("3d_ragged_mask_i32", 3, 8, 8, 1000, 2, 16, 0, torch.int32, "splat_max_bwd_det"),
    ("2d_four_channels_banded", 2, 32, 4, 1024, 2, 16, 0, None, "splat_max_bwd_det"),
]
FAMILIES = ["FORCE_HOT", "NO_HOT", "FORCE_BAND"]
_refs = {}


def _dup_case(case):
    """inputs, the forward's z and the CPU reference of a case: computed once, shared by the families, never modified"""
    name, dim, W, C, N, B, H, nseg, pad_dtype, _ = case
    if name not in _refs:
        Ws = [W] * dim
        keys, feat, pad, g = _duplicated(B, H, C, N, dim, 100 + len(name), pad_dtype)
        gz = torch.randn(B, H * C, *Ws, generator=g)
        z, _, _, _ = _splat_bwd(keys, feat, gz, pad, Ws, H, dim, det=False)
        _refs[name] = (keys, feat, pad, gz, z) + _reference(keys, feat, gz, pad, z, Ws, H, dim)
    return _refs[name]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", DUP_CASES, ids=[c[0] for c in DUP_CASES])
def test_mass_duplicates_go_to_the_lowest_index_in_every_family(case, family):
    mod, lib = _mod()
    name, dim, W, C, N, B, H, nseg, pad_dtype, det_tag = case
    Ws, h = [W] * dim, N // 2
    keys, feat, pad, gz, z_ref, gf_ref, scale, gk_ref, _ = _dup_case(case)
    runs = [_splat_bwd(keys, feat, gz, pad, Ws, H, dim, getattr(mod, "DEBUG_" + family), nseg) for _ in range(2)]
    z, gf, gk, tag = runs[0]
    banded = family == "FORCE_BAND" and C == 4
    print("%s/%s: tag %s" % (name, family, tag))
    if banded:
        assert "band_splat_bwd" in tag and "det" not in tag, tag       # the banded kernels follow the rule already
    else:
        assert tag.startswith(det_tag) and "hot" not in tag and "generic" not in tag and "segments" not in tag, tag
    assert torch.equal(z, z_ref)
    # the copies lose every cell and channel: exact zeros
    assert float(gf[:, :, h:].abs().max()) == 0.0, (name, family, tag)
    assert float(gk[:, :, h:].abs().max()) == 0.0, (name, family, tag)
    err = (gf - gf_ref).abs()
    print("  g_feat: max err / (1e-5 sum|terms|) = %.3g" % float((err / (1e-5 * scale + 1e-30))[scale > 0].max()))
    assert bool((err <= 1e-5 * scale).all()), (name, family, tag, float(err.max()))
    rel = float((gk - gk_ref).abs().max()) / float(gk_ref.abs().max())
    print("  g_keys: max err relative to max|g_keys| = %.3g" % rel)
    assert rel <= 1e-4, (name, family, tag, rel)
    # run to run
    assert runs[1][3] == tag
    assert torch.equal(runs[1][1], gf) and torch.equal(runs[1][2], gk), (name, family, tag)


def test_default_mode_keeps_its_kernels():
    """With the mode off the launch tags of tests/test_tie_rule_gpu.py's cases are what they were: no `det`."""
    mod, lib = _mod()
    cases = [("FORCE_HOT", 2, 32, 8, 1024, "hot"), ("FORCE_HOT", 2, 32, 8, 8192, "hot"), ("FORCE_HOT", 3, 8, 8, 1024, "hot"),
             ("NO_HOT", 2, 32, 8, 1024, "splat_max_bwd_"), ("NO_HOT", 3, 8, 8, 1000, "splat_max_bwd_"),
             ("FORCE_BAND", 2, 32, 4, 1024, "band")]
    for flag, dim, W, C, N, want in cases:
        keys, feat, pad, g = _duplicated(2, 16, C, N, dim, 5)
        gz = torch.randn(2, 16 * C, *([W] * dim), generator=g)
        tag = _splat_bwd(keys, feat, gz, None, [W] * dim, 16, dim, getattr(mod, "DEBUG_" + flag), det=False)[3]
        assert "det" not in tag and want in tag, (flag, dim, W, C, N, tag)
    assert lib.ct_get_deterministic() == 0


def _node_keys(W, count):
    """float32 keys whose scaled coordinate (key + 1) * ((W - 1) / 2), rounded as ct_axis rounds it, is an exact integer j >= 2:
    a point there sits on a grid node and three of its four corner weights are exactly 0 (tests/test_tie_rule_gpu.py: _node_key)"""
    hw = np.float32((W - 1) / 2.0)
    out = []
    for j in range(2, W - 2):
        k = np.float32(2.0 * j / (W - 1) - 1.0)
        for _ in range(8):
            s = np.float32(np.float32(k + np.float32(1.0)) * hw)
            if float(s) == float(j):
                out.append((float(k), j))
                break
            k = np.nextafter(k, np.float32(1.0 if s < j else -1.0), dtype=np.float32)
        if len(out) == count:
            return out
    raise AssertionError("no %d node keys for W = %d" % (count, W))


@pytest.mark.parametrize("family", ["FORCE_HOT", "NO_HOT"])
def test_chance_ties_between_different_points(family):
    """Three points on one node tie pairwise in two channels, two more on a second node of the same plane tie in a third: more
    than one tie in a plane (the hot kernels' redo in the default mode).  The lower index keeps each award, the others get
    exactly nothing from that cell: the launch equals, bit for bit, the one with the losers' tied features removed."""
    mod, lib = _mod()
    W, C, N, B, H, dim = 32, 8, 1024, 2, 16, 2
    g = torch.Generator().manual_seed(23)
    (ka, ja), (kb, jb) = _node_keys(W, 2)
    keys = torch.tanh(torch.randn(B, H * dim, N, generator=g))
    feat = torch.randn(B, H * C, N, generator=g)
    gz = torch.randn(B, H * C, W, W, generator=g)
    b0, h0 = 1, 5
    p0, p1, p2, q0, q1 = 37, 300, N - 5, 70, 801
    c0, c1, c2 = 1, 6, 3
    for pts, kk in (((p0, p1, p2), ka), ((q0, q1), kb)):
        for p in pts:
            keys[b0, h0 * dim:(h0 + 1) * dim, p] = kk
            feat[b0, h0 * C:(h0 + 1) * C, p] = -1.0                   # never above the zero floor, except:
    feat[b0, h0 * C + c0, p0] = 100.0
    feat[b0, h0 * C + c1, p1] = 90.0
    feat[b0, h0 * C + c2, q0] = 80.0
    untied = feat.clone()
    feat[b0, h0 * C + c0, p1] = 100.0                                   # p0 == p1 in c0
    feat[b0, h0 * C + c1, p2] = 90.0                                    # p1 == p2 in c1
    feat[b0, h0 * C + c2, q1] = 80.0                                    # q0 == q1 in c2, on the second node
    flags = getattr(mod, "DEBUG_" + family)
    z, gf, gk, tag = _splat_bwd(keys, feat, gz, None, [W, W], H, dim, flags)
    z0, gf0, gk0, tag0 = _splat_bwd(keys, untied, gz, None, [W, W], H, dim, flags)
    assert "det" in tag and tag == tag0 and torch.equal(z, z0), (tag, tag0)
    cell_a, cell_b = ja * W + ja, jb * W + jb
    for c, cell, winner, loser in ((c0, cell_a, p0, p1), (c1, cell_a, p1, p2), (c2, cell_b, q0, q1)):
        assert float(z[b0, h0 * C + c].reshape(-1)[cell]) == float(feat[b0, h0 * C + c, winner])
        assert float(gf[b0, h0 * C + c, winner]) == float(gz[b0, h0 * C + c].reshape(-1)[cell]), (family, c)
        assert float(gf[b0, h0 * C + c, loser]) == 0.0, (family, c)
    assert float(gk[b0, h0 * dim:(h0 + 1) * dim, p2].abs().max()) == 0.0 and float(gk[b0, h0 * dim:(h0 + 1) * dim, q1].abs().max()) == 0.0
    assert torch.equal(gf, gf0) and torch.equal(gk, gk0), family


def test_lc_entry_point_follows_the_rule_and_repeats():
    """ct_splat_lc_bwd (SplatLcFn): explicit corner weights and cells, the cotangent of the weights instead of the keys"""
    case = DUP_CASES[3]                                                 # 3D, ragged N
    name, dim, W, C, N, B, H, nseg, pad_dtype, _ = case
    keys, feat, pad, gz, z_ref, gf_ref, scale, _, g_lc_ref = _dup_case(case)
    runs = [_splat_bwd(keys, feat, gz, pad, [W] * dim, H, dim, lc_form=True) for _ in range(2)]
    z, gf, g_lc, tag = runs[0]
    assert "det" in tag, tag
    assert torch.equal(z, z_ref)
    assert float(gf[:, :, N // 2:].abs().max()) == 0.0 and float(g_lc[:, :, :, N // 2:].abs().max()) == 0.0
    assert bool(((gf - gf_ref).abs() <= 1e-5 * scale).all())
    assert float((g_lc - g_lc_ref).abs().max()) <= 1e-4 * float(g_lc_ref.abs().max())
    assert torch.equal(runs[1][1], gf) and torch.equal(runs[1][2], g_lc)


def test_channel_chunk_groups_sum_g_keys_in_a_fixed_order():
    """B8 H16 8^3 C32 N4096: a plane's channel chunks go to several workgroups; their g_keys partials are added in group
    order (the default mode's generic kernel adds them with float atomics where it has no workspace)"""
    B, H, C, N, W, dim = 8, 16, 32, 4096, 8, 3
    keys, feat, pad, g = _duplicated(B, H, C, N, dim, 77)
    gz = torch.randn(B, H * C, W, W, W, generator=g)
    a = _splat_bwd(keys, feat, gz, None, [W] * dim, H, dim)
    b = _splat_bwd(keys, feat, gz, None, [W] * dim, H, dim)
    assert a[3] == b[3] and a[3].startswith("splat_max_bwd_det_groups"), a[3]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert float(a[1][:, :, N // 2:].abs().max()) == 0.0 and float(a[2][:, :, N // 2:].abs().max()) == 0.0


def test_accumulate_keys_and_keys_add_through_the_abi():
    """ct_splat_bwd_ex with CT_BWD_ACCUMULATE_KEYS (g_keys += result) and ct_splat_bwd_tk with a separate g_keys_add: the
    deterministic result plus the incoming cotangent, the same bits twice."""
    from cloud_transformers_amd.ops import _ptr, _stream
    mod, lib = _mod()
    case = DUP_CASES[0]
    name, dim, W, C, N, B, H, nseg, pad_dtype, _ = case
    keys, feat, pad, gz, z, gf_ref, scale, gk_ref, _ = _dup_case(case)
    Wa = mod.int_array([W] * dim)
    kd, fd, zd, gzd = keys.cuda(), feat.cuda(), z.cuda(), gz.cuda()
    add = torch.randn(B, H * dim, N, generator=torch.Generator().manual_seed(3))
    tickets = torch.zeros(mod.TICKETS_BYTES // 4, device="cuda", dtype=torch.int32)
    lib.ct_set_deterministic(1)
    try:
        nws = lib.ct_splat_bwd_ex_workspace_bytes(B, H, C, N, dim, Wa, 0, 1)
        ws = torch.empty(max(nws, 16), device="cuda", dtype=torch.uint8)
        outs = []
        for form in ("ex", "tk", "ex", "tk"):
            g_feat = torch.full_like(fd, float("nan"))
            if form == "ex":
                g_keys = add.cuda()
                mod.check(lib.ct_splat_bwd_ex(_ptr(kd), _ptr(fd), None, 0, _ptr(zd), _ptr(gzd), _ptr(g_feat), _ptr(g_keys), _ptr(ws), nws,
                                              B, H, C, N, dim, Wa, 0, 1, _stream()), "ct_splat_bwd_ex")
            else:
                g_keys, addd = torch.full_like(kd, float("nan")), add.cuda()
                mod.check(lib.ct_splat_bwd_tk(_ptr(kd), _ptr(fd), None, 0, _ptr(zd), _ptr(gzd), _ptr(g_feat), _ptr(addd), _ptr(g_keys),
                                              _ptr(ws), nws, _ptr(tickets), B, H, C, N, dim, Wa, 0, _stream()), "ct_splat_bwd_tk")
            torch.cuda.synchronize()
            assert "det" in lib.ct_debug_last_launch().decode()
            outs.append((g_feat.cpu(), g_keys.cpu()))
    finally:
        lib.ct_set_deterministic(0)
    for gf, gk in outs:
        assert bool(((gf - gf_ref).abs() <= 1e-5 * scale).all())
        assert float((gk - (gk_ref + add)).abs().max()) <= 1e-4 * float((gk_ref + add).abs().max())
        assert torch.equal(gk[:, :, N // 2:], add[:, :, N // 2:])      # the copies add exactly nothing
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])
    assert torch.equal(outs[1][0], outs[3][0]) and torch.equal(outs[1][1], outs[3][1])
    assert int(tickets.abs().sum()) == 0


def test_gather_side_key_cotangents_are_not_summed_with_atomics():
    """Slice backward in the lc form and Splat(sum) backward take the generic corner-cotangent kernel, which deals a plane's
    channel chunks to groups of workgroups and adds their g_keys with float atomics where planes are few: in the mode one
    workgroup adds the chunks of its points in order.  B1 H2 C32 16^2: 32 single-channel chunks."""
    import cloud_transformers_amd as ct
    from cloud_transformers_amd import ops
    mod, lib = _mod()
    B, H, C, N, W, dim = 1, 2, 32, 1024, 16, 2
    g = torch.Generator().manual_seed(31)
    keys = torch.tanh(torch.randn(B, H * dim, N, generator=g))
    grid = torch.randn(B, H * C, W, W, generator=g)
    feat = torch.randn(B, H * C, N, generator=g)
    cot_n = torch.randn(B, H * C, N, generator=g)
    cot_g = torch.randn(B, H * C, W, W, generator=g)
    lc, idx = R.positions(keys, [W, W], H, dim)

    def run(det):
        outs = []
        with ct.deterministic(det):
            l1 = lc.cuda().requires_grad_(True)
            ops.slice_lc(l1, idx.cuda(), grid.cuda(), None, [W, W], H, dim).backward(cot_n.cuda())
            outs.append(l1.grad.cpu())
            l2 = lc.cuda().requires_grad_(True)
            ops.splat_lc(l2, idx.cuda(), feat.cuda(), None, [W, W], H, dim, "sum").backward(cot_g.cuda())
            outs.append(l2.grad.cpu())
            k = keys.cuda().requires_grad_(True)
            ops.splat_keys(k, feat.cuda(), None, [W, W], H, dim, "sum").backward(cot_g.cuda())
            outs.append(k.grad.cpu())
        torch.cuda.synchronize()
        return outs

    a, b, ref = run(True), run(True), run(False)
    for u, v, r in zip(a, b, ref):
        assert torch.equal(u, v)
        assert float((u - r).abs().max()) <= 1e-5 * float(r.abs().max())


# ---------------------------------------------------------------------------
# Chamfer
# ---------------------------------------------------------------------------
def _chamfer_grads(a, b, g1, g2):
    import cloud_transformers_amd as ct
    from cloud_transformers_amd.chamfer import chamfer_with_indices
    ac, bc = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    with ct.deterministic():
        d1, d2, i1, i2 = chamfer_with_indices(ac, bc)
        ((d1 * g1.cuda()).sum() + (d2 * g2.cuda()).sum()).backward()
    torch.cuda.synchronize()
    return ac.grad.cpu(), bc.grad.cpu(), i1.cpu(), i2.cpu()


def _chamfer_ref64(a, b, g1, g2, i1, i2):
    """chamfer.cu:155-174 in float64 on the GPU's indices: (g_xyz1, g_xyz2) and, per element, the sum of the |terms| it adds up"""
    a, b, g1, g2 = a.double(), b.double(), g1.double(), g2.double()
    ga, gb, sa, sb = torch.zeros_like(a), torch.zeros_like(b), torch.zeros_like(a), torch.zeros_like(b)
    for k in range(a.shape[0]):
        t = 2 * g1[k][:, None] * (a[k] - b[k][i1[k].long()])
        ga[k] += t
        sa[k] += t.abs()
        gb[k].index_add_(0, i1[k].long(), -t)
        sb[k].index_add_(0, i1[k].long(), t.abs())
        t = 2 * g2[k][:, None] * (b[k] - a[k][i2[k].long()])
        gb[k] += t
        sb[k] += t.abs()
        ga[k].index_add_(0, i2[k].long(), -t)
        sa[k].index_add_(0, i2[k].long(), t.abs())
    return ga, gb, sa, sb


@pytest.mark.parametrize("B,n,m", [(2, 4096, 8), (2, 1000, 1536)], ids=["fan_in_512", "general"])
def test_chamfer_backward_is_ordered(B, n, m):
    """Cotangents in [0, 1) as in tests/test_chamfer_gpu.py, unscaled; the reference is the CPU formula in float64 on the GPU's
    indices.  General case: that test's own bar, atol 1e-5.  Fan-in case (512 fp32 terms per row of cloud 2, sums of a few
    hundred): an absolute 1e-5 is below the rounding of ANY order of that sum (eps x sum|terms| ~ 6e-8 x 500), so the bar is
    relative, 1e-5 x sum|terms| per element — 1/100 of one typical term, which a wrong or dropped term cannot pass."""
    g = torch.Generator().manual_seed(n + m)
    a, b = torch.rand(B, n, 3, generator=g), torch.rand(B, m, 3, generator=g)
    g1, g2 = torch.rand(B, n, generator=g), torch.rand(B, m, generator=g)
    ga, gb, i1, i2 = _chamfer_grads(a, b, g1, g2)
    ra, rb, sa, sb = _chamfer_ref64(a, b, g1, g2, i1, i2)

    def check(got, ref, scale, what):
        err = (got.double() - ref).abs()
        print("%s n=%d m=%d: max err %.3g, max err / sum|terms| %.3g" % (what, n, m, float(err.max()), float((err / (scale + 1e-300)).max())))
        if m == 8:
            assert bool((err <= 1e-5 * scale).all()), what
        else:
            assert float(err.max()) <= 1e-5, what
            assert bool((err <= 1e-5 * scale).all()), what

    if m == 8:
        assert int(torch.bincount(i1[0].long(), minlength=m).max()) >= 512      # the fan-in the case is about
    check(ga, ra, sa, "g_xyz1")
    check(gb, rb, sb, "g_xyz2")
    # run to run
    ga2, gb2, _, _ = _chamfer_grads(a, b, g1, g2)
    assert torch.equal(ga, ga2) and torch.equal(gb, gb2)
    # cloud 1 reversed: g_xyz1's rows keep their bits (own term, then cloud 2's sources in ascending index); g_xyz2 adds its
    # sources in the reversed order: to the same bars
    gar, gbr, _, _ = _chamfer_grads(a.flip(1).contiguous(), b, g1.flip(1).contiguous(), g2)
    assert torch.equal(gar.flip(1), ga)
    check(gbr, rb, sb, "g_xyz2, cloud 1 reversed")


# ---------------------------------------------------------------------------
# Routing: grouped-conv weight gradient, lattice
# ---------------------------------------------------------------------------
def test_gconv_weight_gradient_and_lattice_repeat_and_refuse_a_null_workspace():
    import cloud_transformers_amd as ct
    from cloud_transformers_amd import ops
    from cloud_transformers_amd.layers.gconv import GroupedConv2d
    from cloud_transformers_amd.ops import _ptr, _stream
    mod, lib = _mod()
    g = torch.Generator().manual_seed(9)
    B, groups, Cg, W = 8, 16, 16, 16
    conv = GroupedConv2d(groups * Cg, groups * Cg, 3, padding=1, groups=groups).cuda()
    x = torch.randn(B, groups * Cg, W, W, generator=g).cuda()
    gy = torch.randn(B, groups * Cg, W, W, generator=g).cuda()
    grads = []
    with ct.deterministic():
        for _ in range(2):
            conv.zero_grad(set_to_none=True)
            conv(x).backward(gy)
            assert "atomics" not in lib.ct_debug_last_launch().decode()
            grads.append((conv.weight.grad.clone(), conv.bias.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    # the direct call with a NULL workspace: refused in the mode, the atomic form outside it
    g_w, g_b = torch.empty_like(conv.weight), torch.empty_like(conv.bias)
    Wa = mod.int_array([W, W])
    args = (_ptr(x), _ptr(gy), _ptr(g_w), _ptr(g_b), None, 0, B, groups, Cg, Cg, 2, Wa, _stream())
    lib.ct_set_deterministic(1)
    try:
        assert lib.ct_gconv_bwd_weight(*args) == mod.CT_EPRECOND
    finally:
        lib.ct_set_deterministic(0)
    assert lib.ct_gconv_bwd_weight(*args) == 0 and "atomics" in lib.ct_debug_last_launch().decode()
    torch.cuda.synchronize()

    Bl, H, N, dim = 8, 16, 1024, 3
    xyz = torch.rand(Bl, 3, N, generator=g).cuda() * 2 - 1
    outs = []
    for _ in range(2):
        res = (torch.randn(Bl, H * 3, N, generator=torch.Generator().manual_seed(1)) * 0.1).cuda().requires_grad_(True)
        Rm = torch.linalg.qr(torch.randn(H, 3, 3, generator=torch.Generator().manual_seed(2)))[0].cuda().requires_grad_(True)
        shift = torch.zeros(H, 3).cuda().requires_grad_(True)
        scales = torch.ones(H, dim).cuda().requires_grad_(True)
        with ct.deterministic():
            keys, lattice = ops.lattice(xyz, res, Rm, shift, scales, None, dim)
            cot = torch.randn(keys.shape, generator=torch.Generator().manual_seed(4)).cuda()
            (lattice * cot).sum().backward()
        outs.append((res.grad.clone(), Rm.grad.clone(), shift.grad.clone(), scales.grad.clone()))
    for u, v in zip(*outs):
        assert torch.equal(u, v)
    lat = lattice.detach()
    g_xyz, g_res = torch.empty_like(xyz), torch.empty_like(res)
    g_R, g_shift, g_scales = torch.empty(H, 3, 3).cuda(), torch.empty(H, 3).cuda(), torch.empty(H, dim).cuda()
    largs = (_ptr(xyz), _ptr(res.detach()), _ptr(Rm.detach()), _ptr(shift.detach()), _ptr(scales.detach()), None, _ptr(lat), _ptr(cot),
             None, _ptr(g_xyz), _ptr(g_res), _ptr(g_R), _ptr(g_shift), _ptr(g_scales), None, None, 0, Bl, H, N, dim, _stream())
    lib.ct_set_deterministic(1)
    try:
        assert lib.ct_lattice_bwd(*largs) == mod.CT_EPRECOND
    finally:
        lib.ct_set_deterministic(0)
    assert lib.ct_lattice_bwd(*largs) == 0
    torch.cuda.synchronize()


def test_scatter_add_onto_a_grid_beyond_lds_is_refused_or_warned():
    """A grid whose single-channel tile exceeds a CU's LDS (256^2) takes the global float-atomic scatter-add for Splat(sum)
    forward and for the g_grid half of Slice backward: no ordered form, so the library returns CT_EPRECOND in the mode (nothing
    written), the ops raise naming the entry point, and under torch's warn_only they warn and give the ordinary result."""
    import cloud_transformers_amd as ct
    from cloud_transformers_amd import ops
    from cloud_transformers_amd.ops import _ptr, _stream
    mod, lib = _mod()
    B, H, C, N, W, dim = 1, 2, 1, 1024, 256, 2
    g = torch.Generator().manual_seed(5)
    keys = torch.tanh(torch.randn(B, H * dim, N, generator=g)).cuda()
    feat = torch.randn(B, H * C, N, generator=g).cuda()
    grid = torch.randn(B, H * C, W, W, generator=g).cuda()
    cot = torch.randn(B, H * C, N, generator=g).cuda()

    def slice_grads():
        k, z = keys.clone().requires_grad_(True), grid.clone().requires_grad_(True)
        ops.slice_keys(k, z, None, [W, W], H, dim).backward(cot)
        return k.grad, z.grad

    ref_k, ref_z = slice_grads()
    assert lib.ct_debug_last_launch().decode().startswith("scatter_global_atomics")
    ref_sum = ops.splat_keys(keys, feat, None, [W, W], H, dim, "sum")
    out = torch.full_like(grid, 7.0)
    Wa = mod.int_array([W, W])
    lib.ct_set_deterministic(1)
    try:
        rc = lib.ct_splat_fwd(_ptr(keys), _ptr(feat), None, 0, _ptr(out), B, H, C, N, dim, Wa, 1, _stream())
        rc_max = lib.ct_splat_fwd(_ptr(keys), _ptr(feat), None, 0, _ptr(torch.empty_like(grid)), B, H, C, N, dim, Wa, 0, _stream())
    finally:
        lib.ct_set_deterministic(0)
    torch.cuda.synchronize()
    assert rc == mod.CT_EPRECOND and rc_max == 0 and float((out - 7.0).abs().max()) == 0.0
    with ct.deterministic():
        with pytest.raises(RuntimeError, match="ct_splat_fwd .* does not have a deterministic implementation"):
            ops.splat_keys(keys, feat, None, [W, W], H, dim, "sum")
        with pytest.raises(RuntimeError, match="ct_slice_bwd_tk .* does not have a deterministic implementation"):
            slice_grads()
        ops.splat_keys(keys, feat, None, [W, W], H, dim, "max")                  # an atomic max: no order to fix
        prev = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
        torch.use_deterministic_algorithms(prev[0], warn_only=True)
        try:
            with pytest.warns(UserWarning, match="ct_splat_fwd"):
                got_sum = ops.splat_keys(keys, feat, None, [W, W], H, dim, "sum")
            with pytest.warns(UserWarning, match="ct_slice_bwd_tk"):
                got_k, got_z = slice_grads()
            assert lib.ct_get_deterministic() == 1                              # the override was this call's alone
        finally:
            torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
    for got, ref in ((got_sum, ref_sum), (got_k, ref_k), (got_z, ref_z)):
        assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_gconv_rows_off_the_float4_grid_are_refused_or_warned():
    """Rows that are not a multiple of 4 floats take the tile kernel, which sums with float atomics only: a RuntimeError naming
    the op in deterministic mode, a warning (and the ordinary result) under torch's warn_only."""
    import cloud_transformers_amd as ct
    from cloud_transformers_amd.layers.gconv import GroupedConv2d
    conv = GroupedConv2d(4 * 8, 4 * 8, 3, padding=1, groups=4).cuda()
    x = torch.randn(2, 32, 6, 6).cuda()
    y = conv(x)
    with ct.deterministic():
        with pytest.raises(RuntimeError, match="ct_gconv_bwd_weight .* does not have a deterministic implementation"):
            y.backward(torch.ones_like(y), retain_graph=True)
        prev = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
        torch.use_deterministic_algorithms(prev[0], warn_only=True)
        try:
            with pytest.warns(UserWarning, match="ct_gconv_bwd_weight"):
                y.backward(torch.ones_like(y), retain_graph=True)
        finally:
            torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
    warned = conv.weight.grad.clone()
    conv.zero_grad(set_to_none=True)
    y.backward(torch.ones_like(y))
    assert float((warned - conv.weight.grad).abs().max()) <= 1e-4 * float(conv.weight.grad.abs().max())


# ---------------------------------------------------------------------------
# One block, and the harness
# ---------------------------------------------------------------------------
def test_one_block_end_to_end_repeats_every_parameter_gradient():
    """MultiHead (2D, 16^2, H16, C8) on B2 N1024 with the second half of the cloud duplicated, loss_chamfer of the reshaped
    output against a fixed cloud: two fresh runs from one seed give torch.equal parameter gradients."""
    import cloud_transformers_amd as ct
    from cloud_transformers_amd.chamfer import loss_chamfer
    from cloud_transformers_amd.layers.multihead_ct import MultiHead
    B, N, D, C, H = 2, 1024, 16, 8, 16

    def run():
        torch.manual_seed(11)
        blk = MultiHead(D, C, D, 16, 2, H).cuda().train()
        x = torch.randn(B, D, N)
        pcd = torch.rand(B, 3, N) * 2 - 1
        x[:, :, N // 2:] = x[:, :, :N // 2]
        pcd[:, :, N // 2:] = pcd[:, :, :N // 2]
        target = torch.rand(B, 3, 1, 2048)
        with ct.deterministic():
            out, _ = blk(x.cuda(), pcd.cuda())
            assert out.shape == (B, H * C, N)
            cloud = out[:, :126].reshape(B, 3, 1, 42 * N)
            loss_chamfer(cloud, target.cuda()).backward()
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in blk.named_parameters() if p.grad is not None}

    a, b = run(), run()
    assert len(a) >= 8 and a.keys() == b.keys()
    for k in a:
        assert torch.isfinite(a[k]).all() and torch.equal(a[k], b[k]), k


HARNESS_CONFIG = '''
experiment:
    root: '{root}/exp'
    writer_root: '{root}/runs'
data:
    batch_size: 2
    num_workers: 0
    num_points: 512
model:
    generator: '{root}/segmenter.py'
    n_classes: 13
train:
    num_epochs: 1
    save_each: 100000
    deterministic: true
    optimizer:
        type: 'Adam'
        lr: !!float 1e-3
        betas: [!!float 0.9, !!float 0.999]
        weight_decay: !!float 0.0
    scheduler:
        type: 'StepLR'
        gamma: !!float 0.7
        step_size: 25000
'''


def test_train_deterministic_gives_one_loss_history(tmp_path):
    """`train.deterministic: true` through harness.Trainer (tests/test_harness_gpu.py's segmenter config): three steps, twice."""
    import cloud_transformers_amd as ct
    from cloud_transformers_amd import harness as H
    (tmp_path / "segmenter.py").write_text("from tests.test_zoo_gpu import Segmenter as Model\n")
    cfg_path = tmp_path / "s3dis.yaml"
    cfg_path.write_text(HARNESS_CONFIG.format(root=str(tmp_path)))
    hists, before = [], ct.is_deterministic()
    for i in range(2):
        torch.manual_seed(0)
        tr = H.Trainer(H.load_config(cfg_path), "segmentation", n_classes=13, device=torch.device("cuda", 0), dataset_length=8,
                       channels=6, exp_name="run%d" % i)
        hists.append(tr.fit(max_iters=3))
        assert ct.is_deterministic() is before                           # the scope ended with the fit
    assert len(hists[0]) == 3 and all(v == v for v in hists[0])
    assert hists[0] == hists[1], hists
