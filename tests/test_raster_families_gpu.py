"""Every Splat / Slice kernel family (tests/raster_families.py) on the GPU: the launch tag of each row, and its outputs against a
float64 reference of the same operation.

The reference takes the fp32 corner weights and cells of oracle.ref_cpu.positions (the kernels' weights are pinned bit-identical to
them by tests/test_raster_gpu.py::test_positions_golden), forms the products in float64 and scatters (scatter_add / amax with the
zero floor) or gathers them; key cotangents come from float64 autograd through the same expression (the GradientBalancing rule:
d s / d key = 1 inside the clamp, 0 outside).  Bars:
- Splat(max) z: bit-exact against the fp32 oracle (the kernels form (src * pad) * w exactly as it does);
- Splat(sum) z and Slice backward g_grid: per channel, within 1e-4 of that channel's own max (the fixed-point scatter's quantum is
  per channel; the global-atomics form adds floats);
- Slice forward out, Splat backward g_feat: per channel within 1e-4 of the channel's max (a sum of 2^dim products per element);
- g_keys / g_lc: within 1e-4 of their max (the sum over all channels of a head: its small channels are below fp32 resolution).
Splat(max) backward routes a cell's cotangent to the single contribution equal to its (fp32) maximum, the lowest point index on an
exact tie, and nothing where the maximum is the zero floor (include/cloudct.h, the deliberate deviation).

Every row's inputs carry the edges where these kernels go wrong: a channel whose values are all negative, channels whose
magnitudes span 1e-4 .. 1e4 (10^8), keys exactly at -1 / +1 and on cell edges, three quarters of the cloud clustered around one
cell (thousands of contributions to a cell), and, with a padding mask, padded points that carry values of 1e6."""
import zlib

import pytest
import torch

from oracle import ref_cpu as R
from tests import raster_families as F

pytestmark = pytest.mark.gpu

BAR = 1e-4


def _lib():
    from cloud_transformers_amd import _lib
    return _lib, _lib.load()


@pytest.fixture
def flags():
    mod, lib = _lib()
    yield lambda v, nseg=0: (lib.ct_debug_set_flags(v), lib.ct_debug_set_nseg(nseg))
    lib.ct_debug_set_flags(0)
    lib.ct_debug_set_nseg(0)


def per_channel_err(a, b, HC):
    """max over (batch, channel) of max|a - b| / max|b| within that channel"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    B = a.shape[0]
    a, b = a.reshape(B, HC, -1), b.reshape(B, HC, -1)
    return float(((a - b).abs().amax(dim=2) / b.abs().amax(dim=2).clamp_min(1e-30)).max())


def relerr(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(1e-30, float(b.abs().max())))


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def edge_keys(B, H, N, W, g):
    """tanh cloud, three quarters of it clustered around one cell, and (in every plane) keys exactly at -1 / +1 and on cell edges"""
    dim = len(W)
    keys = torch.tanh(torch.randn(B, H * dim, N, generator=g))
    nc = 3 * N // 4
    keys[..., :nc] = (0.31 + 0.01 * torch.randn(B, H * dim, nc, generator=g)).clamp(-1, 1)
    # keys whose scaled coordinate (k + 1) * (W - 1) / 2 is an integer in fp32: points on cell edges
    edges = []
    for j in range(dim):
        hw = torch.tensor((W[j] - 1) * 0.5, dtype=torch.float32)
        cand = (torch.arange(W[j], dtype=torch.float32) / hw - 1.0).float()
        ok = ((cand + 1.0) * hw) == ((cand + 1.0) * hw).floor()
        edges.append(cand[ok & (cand.abs() < 1)])
    special = N - nc
    n0 = nc                                     # the special points sit in the unclustered part
    k = min(special, 16)
    for h in range(H):
        for j in range(dim):
            e = edges[j]
            vals = torch.cat([torch.tensor([-1.0, 1.0]), e[torch.arange(k - 2) % max(1, len(e))] if len(e) else torch.zeros(k - 2)])
            keys[:, h * dim + j, n0:n0 + k] = vals[torch.randperm(k, generator=g)][:k]
    return keys.contiguous()


def channel_scales(C):
    """channel 0 all negative (handled by the caller), the others spanning 1e-4 .. 1e4"""
    return 10.0 ** torch.linspace(-4, 4, C)


def scaled(shape_bhc, rest, C, H, g, negative_first=True):
    B = shape_bhc
    x = torch.randn(B, H, C, *rest, generator=g) * channel_scales(C).reshape(1, 1, C, *([1] * len(rest)))
    if negative_first:
        x[:, :, 0] = -x[:, :, 0].abs() - 1e-3
    return x.reshape(B, H * C, *rest).contiguous()


def make_pad(B, N, pad, g):
    if pad is None:
        return None, None
    p = (torch.rand(B, N, generator=g) > 0.25).float()
    return p, (p if pad == "f32" else p.to(torch.int32))


def inputs(B, H, C, N, W, pad, seed):
    g = torch.Generator().manual_seed(seed)
    keys = edge_keys(B, H, N, W, g)
    p32, pdev = make_pad(B, N, pad, g)
    feat = scaled(B, (N,), C, H, g)
    if p32 is not None:                          # padded points carry large values
        feat = torch.where(p32[:, None, :] > 0, feat, torch.full_like(feat, 1e6) * torch.sign(torch.randn(feat.shape, generator=g)))
    grid = scaled(B, tuple(W), C, H, g)
    cot = scaled(B, (N,), C, H, g, negative_first=False)
    gz = scaled(B, tuple(W), C, H, g, negative_first=False)
    return dict(keys=keys, feat=feat, grid=grid, cot=cot, gz=gz, p32=p32, pdev=pdev,
                keys_add=torch.randn(B, H * len(W), N, generator=g))


# ---------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------------
def weights64(keys, W, H):
    """(lc32 [B,H,V,N] fp32, idx [B,H,V,N], lc64 float64 with autograd to keys64, keys64 leaf): lc64's VALUES are lc32's, its
    gradient the derivative of the bi/tri-linear weights w.r.t. the keys (unscaled, masked by the clamp) in float64"""
    dim = len(W)
    B, _, N = keys.shape
    lc32, idx = R.positions(keys, list(W), H, dim)
    eps = 1e-7
    k32 = keys.reshape(B * H, dim, N)
    kc = k32.clamp(-1 + eps, 1 - eps)
    inside = (k32 >= kc) & (k32 <= kc)          # = the clamp's pass-through mask (torch: bounds included)
    hw = ((torch.tensor(W, dtype=torch.float32) - 1) * 0.5)[None, :, None]
    s32 = (kc + 1.0) * hw
    f = s32.floor().double()
    k64 = keys.double().requires_grad_(True)
    kk = k64.reshape(B * H, dim, N)
    s = s32.double() + (kk - kk.detach()) * inside.double()
    w1, w0 = s - f, (f + 1) - s
    ws = []
    for v in range(1 << dim):
        wv = None
        for j in range(dim):
            wj = w1[:, j] if (v >> j) & 1 else w0[:, j]
            wv = wj if wv is None else wv * wj
        ws.append(wv)
    lc_grad = torch.stack(ws, 1).reshape(B, H, 1 << dim, N)
    lc64 = lc32.double() + (lc_grad - lc_grad.detach())
    return lc32, idx, lc64, k64


def _index(idx, C):
    B, H, V, N = idx.shape
    return idx[:, :, None].reshape(B, H, 1, V * N).expand(B, H, C, V * N)


def ref_scatter(pre, idx, C, G, amax):
    """pre [B,H,C,V,N] -> [B,H,C,G] (zero floor for amax)"""
    B, H = pre.shape[:2]
    z0 = torch.zeros(B, H, C, G, dtype=pre.dtype)
    src = pre.reshape(B, H, C, -1)
    if amax:
        return z0.scatter_reduce(3, _index(idx, C), src, reduce="amax", include_self=True)
    return z0.scatter_add(3, _index(idx, C), src)


def ref_gather(grid, idx, C):
    """grid [B,H*C,*W] -> [B,H,C,V,N]"""
    B, H, V, N = idx.shape
    return torch.gather(grid.reshape(B, H, C, -1), 3, _index(idx, C)).reshape(B, H, C, V, N)


def max_winners(pre32, z32, idx, C):
    """[B,H,C,V,N] bool: the contribution each cell's cotangent goes to — equal to the cell's fp32 maximum, the maximum above the
    zero floor, the lowest point index on an exact tie"""
    B, H, _, V, N = pre32.shape
    zg = ref_gather(z32, idx, C)
    cand = (pre32 == zg) & (zg > 0)
    # lowest point index per (b,h,c,cell) among the candidates
    order = torch.arange(N).expand(B, H, C, V, N)
    big = torch.full_like(order, N)
    first = torch.full((B, H, C, z32[0, 0].numel()), N, dtype=torch.long)
    first = first.scatter_reduce(3, _index(idx, C), torch.where(cand, order, big).reshape(B, H, C, -1), reduce="amin",
                                 include_self=True)
    return cand & (torch.gather(first, 3, _index(idx, C)).reshape(B, H, C, V, N) == order)


def reference(api, reduce, inp, B, H, C, N, W):
    """float64 outputs of the row's operation (and the fp32 oracle's z for Splat(max))"""
    dim, G = len(W), 1
    for w in W:
        G *= w
    lc_form = "_lc_" in api
    lc32, idx, lc64, k64 = weights64(inp["keys"], W, H)
    if lc_form:
        lc64 = lc32.double().requires_grad_(True)
    p = inp["p32"]
    pad64 = p.double()[:, None, None, None, :] if p is not None else None
    which = api.replace("_lc", "")[3:12]
    out = {}
    if which == "splat_fwd":
        f = inp["feat"].double().reshape(B, H, C, 1, N)
        if pad64 is not None:
            f = f * pad64
        pre = f * lc32.double()[:, :, None]
        out["z"] = ref_scatter(pre, idx, C, G, reduce == "max").reshape(B, H * C, *W)
        if reduce == "max":
            out["z32"] = R.splat(lc32, idx, inp["feat"], p, list(W), H, dim, "max")
    elif which == "splat_bwd":
        f64 = inp["feat"].double().requires_grad_(True)
        f = f64.reshape(B, H, C, 1, N)
        if pad64 is not None:
            f = f * pad64
        gzg = ref_gather(inp["gz"].double(), idx, C)
        if reduce == "max":
            z32 = R.splat(lc32, idx, inp["feat"], p, list(W), H, dim, "max")
            f32 = inp["feat"].reshape(B, H, C, 1, N)
            if p is not None:
                f32 = f32 * p[:, None, None, None, :]
            pre32 = f32 * lc32[:, :, None]
            win = max_winners(pre32, z32, idx, C)
            out["z32"] = z32
            loss = (f * lc64[:, :, None] * gzg * win.double()).sum()
        else:
            loss = (f * lc64[:, :, None] * gzg).sum()
        loss.backward()
        out["g_feat"] = f64.grad
        out["g_keys"] = lc64.grad if lc_form else k64.grad
    elif which == "slice_fwd":
        o = (ref_gather(inp["grid"].double(), idx, C) * lc32.double()[:, :, None]).sum(3)
        if pad64 is not None:
            o = o * pad64[:, :, :, 0]
        out["out"] = o.reshape(B, H * C, N)
    else:                                      # slice_bwd
        cot = inp["cot"].double().reshape(B, H, C, 1, N)
        if pad64 is not None:
            cot = cot * pad64
        out["g_grid"] = ref_scatter(cot * lc32.double()[:, :, None], idx, C, G, False).reshape(B, H * C, *W)
        (ref_gather(inp["grid"].double(), idx, C) * lc64[:, :, None] * cot).sum().backward()
        out["g_keys"] = lc64.grad if lc_form else k64.grad
    out["lc32"], out["idx"] = lc32, idx
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the call, straight through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
def place(t, off):
    """t on the GPU, 4 bytes past a 16-byte boundary when off"""
    if not off:
        return t.contiguous().cuda()
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    v = buf[1:1 + t.numel()]
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


def empty_like_on(t_shape, off, fill=float("nan")):
    return place(torch.full(t_shape, fill), off)


def run(api, reduce, inp, ref, B, H, C, N, W, *, ws=False, tickets=False, offset4=(), accumulate=False, keys_add=False, pad=None):
    """-> ({output name: tensor}, tag of the call, tag of the preparatory call)"""
    from cloud_transformers_amd.ops import _ptr, _stream
    mod, lib = _lib()
    dim = len(W)
    Wa = mod.int_array(list(W))
    st = _stream()
    lc_form = "_lc_" in api
    which = api.replace("_lc", "")[3:12]
    off = lambda name: name in offset4                                               # noqa: E731
    pd = None if pad is None else place(inp["pdev"], off("pad"))
    pdt = {None: mod.PAD_NONE, "f32": mod.PAD_F32, "i32": mod.PAD_I32}[pad]
    if lc_form:                                  # (the device tensors are held until the call has run)
        held = (place(ref["lc32"], off("lc")), place(ref["idx"], off("idx")))
        gk_shape = (B, H, 1 << dim, N)
    else:
        held = (place(inp["keys"], off("keys")),)
        gk_shape = (B, H * dim, N)
    pos = tuple(_ptr(t) for t in held)
    red = mod.REDUCE.get(reduce, 0)
    keep = [held]

    def buf(nbytes):
        if not nbytes:
            return None, 0
        b = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        keep.append(b)
        return b, nbytes

    tk = torch.zeros(mod.TICKETS_BYTES // 4, dtype=torch.int32, device="cuda") if tickets else None
    setup_tag, outs = None, {}
    if which == "splat_fwd":
        feat = place(inp["feat"], off("feat"))
        z = empty_like_on((B, H * C, *W), off("z"))
        fn = getattr(lib, api)
        mod.check(fn(*pos, _ptr(feat), _ptr(pd), pdt, _ptr(z), B, H, C, N, dim, Wa, red, st), api)
        outs["z"] = z
    elif which == "slice_fwd":
        grid = place(inp["grid"], off("grid"))
        o = empty_like_on((B, H * C, N), off("out"))
        mod.check(getattr(lib, api)(*pos, _ptr(grid), _ptr(pd), pdt, _ptr(o), B, H, C, N, dim, Wa, st), api)
        outs["out"] = o
    elif which == "splat_bwd":
        feat = place(inp["feat"], off("feat"))
        zin = place(ref["z32"], off("z")) if reduce == "max" else None
        gz = place(inp["gz"], off("g_z"))
        g_feat = empty_like_on((B, H * C, N), off("g_feat"))
        if accumulate:
            g_keys = place(inp["keys_add"], off("g_keys"))
        else:
            g_keys = empty_like_on(gk_shape, off("g_keys"))
        if api == "ct_splat_bwd_ex" or api == "ct_splat_bwd_tk":
            fl = mod.BWD_ACCUMULATE_KEYS if (accumulate or keys_add) else 0
            wsb = lib.ct_splat_bwd_ex_workspace_bytes(B, H, C, N, dim, Wa, red, fl)
        else:
            wsb = lib.ct_splat_bwd_workspace_bytes(B, H, C, N, dim, Wa, red)
        w, wsb = buf(wsb) if ws else (None, 0)
        head = (_ptr(feat), _ptr(pd), pdt, _ptr(zin), _ptr(gz), _ptr(g_feat))
        if api == "ct_splat_bwd_tk":
            add = place(inp["keys_add"], off("g_keys_add")) if keys_add else None
            mod.check(lib.ct_splat_bwd_tk(*pos, *head, _ptr(add), _ptr(g_keys), _ptr(w), wsb, _ptr(tk), B, H, C, N, dim, Wa, red, st),
                      api)
        elif api == "ct_splat_bwd_ex":
            mod.check(lib.ct_splat_bwd_ex(*pos, *head, _ptr(g_keys), _ptr(w), wsb, B, H, C, N, dim, Wa, red,
                                          mod.BWD_ACCUMULATE_KEYS if accumulate else 0, st), api)
        else:
            mod.check(getattr(lib, api)(*pos, *head, _ptr(g_keys), _ptr(w), wsb, B, H, C, N, dim, Wa, red, st), api)
        outs["g_feat"], outs["g_keys"] = g_feat, g_keys
    else:
        grid = place(inp["grid"], off("grid"))
        cot = place(inp["cot"], off("cot"))
        g_grid = empty_like_on((B, H * C, *W), off("g_grid"))
        g_keys = empty_like_on(gk_shape, off("g_keys"))
        head = (_ptr(grid), _ptr(pd), pdt, _ptr(cot), _ptr(g_grid), _ptr(g_keys))
        if api in ("ct_slice_bwd", "ct_slice_lc_bwd"):
            mod.check(getattr(lib, api)(*pos, *head, B, H, C, N, dim, Wa, st), api)
        else:
            w, wsb = buf(lib.ct_slice_bwd_workspace_bytes(B, H, C, N, dim, Wa)) if ws else (None, 0)
            if api == "ct_slice_bwd_ws":
                mod.check(lib.ct_slice_bwd_ws(*pos, *head, _ptr(w), wsb, B, H, C, N, dim, Wa, st), api)
            elif api == "ct_slice_bwd_tk":
                mod.check(lib.ct_slice_bwd_tk(*pos, *head, _ptr(w), wsb, _ptr(tk), B, H, C, N, dim, Wa, st), api)
            else:
                srt, sb = buf(lib.ct_plane_sort_bytes(B, H, N, dim, Wa))
                assert sb > 0, "no sorted form for this layout"
                mod.check(lib.ct_plane_sort(pos[0], _ptr(srt), sb, B, H, N, dim, Wa, st), "ct_plane_sort")
                setup_tag = lib.ct_debug_last_launch().decode()
                mod.check(lib.ct_slice_bwd_ps(*pos, *head, _ptr(w), wsb, _ptr(tk), _ptr(srt), B, H, C, N, dim, Wa, st), api)
        outs["g_grid"], outs["g_keys"] = g_grid, g_keys
    tag = lib.ct_debug_last_launch().decode()
    torch.cuda.synchronize()
    if tickets:
        assert int(tk.abs().sum()) == 0, "the arrival tickets were not handed back as zeros"
    return {k: v.cpu() for k, v in outs.items()}, tag, setup_tag


def fx_resolution(inp, ref, H, C):
    """[B, H*C] resolution of a fixed-point scatter-add per element: a cell takes at most K contributions, each rounded to the
    channel's quantum q = 2^(ceil(log2(max|g_out| * K)) - 30) (csrc/ct_raster_hot.h: fx_quantum; K taken 4x the plane's true
    maximum, which the kernels bound from above); K independent roundings of at most q / 2 add up to ~ sqrt(K) q / 2, and the
    bar allows 4 sqrt(K) q."""
    idx = ref["idx"]
    B = idx.shape[0]
    k = max(int(torch.bincount(idx[b, h].reshape(-1)).max()) for b in range(B) for h in range(H))
    cot = inp["cot"] if inp["p32"] is None else inp["cot"] * inp["p32"][:, None, :]
    m = cot.abs().amax(dim=2).double() * 4 * k
    return 4 * k ** 0.5 * torch.exp2(torch.ceil(torch.log2(m)) - 30)


def grid_allowed(inp, ref, H, C):
    """[B, H*C] the g_grid bar with fx_bound: the larger of 1e-4 of the channel's max and fx_resolution"""
    B = ref["g_grid"].shape[0]
    return torch.maximum(BAR * ref["g_grid"].abs().reshape(B, H * C, -1).amax(dim=2), fx_resolution(inp, ref, H, C))


def grid_err(a, b, allowed):
    """max per-channel |a - b| in units of `allowed`, times BAR (so that <= BAR passes)"""
    B, HC = allowed.shape
    d = (a.double() - b.double()).abs().reshape(B, HC, -1).amax(dim=2)
    return float((d / allowed).max()) * BAR


def check(api, reduce, got, ref, inp, H, C, keys_add=False, accumulate=False, fx_bound=False):
    """the bars of the module docstring; returns {output: error} for the report.  fx_bound: Slice backward's g_grid may also
    reach the fixed-point scatter's own resolution (fx_resolution) where that exceeds 1e-4 of the channel's max"""
    HC = H * C
    errs = {}
    which = api.replace("_lc", "")[3:12]
    if which == "splat_fwd":
        if reduce == "max":
            assert torch.equal(got["z"], ref["z32"]), "Splat(max) z differs from the fp32 oracle (max |d| %.3e)" % float(
                (got["z"] - ref["z32"]).abs().max())
            errs["z"] = per_channel_err(got["z"], ref["z"], HC)
        else:
            errs["z"] = per_channel_err(got["z"], ref["z"], HC)
    elif which == "slice_fwd":
        errs["out"] = per_channel_err(got["out"], ref["out"], HC)
    elif which == "splat_bwd":
        errs["g_feat"] = per_channel_err(got["g_feat"], ref["g_feat"], HC)
        gk = ref["g_keys"]
        if keys_add or accumulate:
            gk = gk + inp["keys_add"].double()
        errs["g_keys"] = relerr(got["g_keys"], gk)
    else:
        if fx_bound:
            errs["g_grid"] = grid_err(got["g_grid"], ref["g_grid"], grid_allowed(inp, ref, H, C))
        else:
            errs["g_grid"] = per_channel_err(got["g_grid"], ref["g_grid"], HC)
        errs["g_keys"] = relerr(got["g_keys"], ref["g_keys"])
    for k, v in errs.items():
        assert v <= BAR, (k, v, errs)
    return errs


@pytest.mark.parametrize("r", F.ROWS, ids=lambda r: r.id)
def test_family_tag_and_float64_reference(r, flags):
    torch.manual_seed(0)
    inp = inputs(r.B, r.H, r.C, r.N, r.W, r.pad, seed=zlib.crc32(r.id.encode()))
    ref = reference(r.api, r.reduce, inp, r.B, r.H, r.C, r.N, r.W)
    flags(r.flags, r.nseg)
    got, tag, setup_tag = run(r.api, r.reduce, inp, ref, r.B, r.H, r.C, r.N, r.W, ws=r.ws, tickets=r.tickets, offset4=r.offset4,
                              accumulate=r.accumulate, keys_add=r.keys_add, pad=r.pad)
    flags(0)
    assert tag == r.tag, (tag, r.tag)
    assert setup_tag == r.setup_tag, (setup_tag, r.setup_tag)
    check(r.api, r.reduce, got, ref, inp, r.H, r.C, keys_add=r.keys_add, accumulate=r.accumulate)


@pytest.mark.parametrize("w", F.WIDE_CASES, ids=lambda w: w.id)
def test_wide_and_narrow_launches_agree(w, flags):
    """The 1024-thread WIDE launches against the 512-thread ones (CT_DEBUG_NO_WIDE), both against the float64 reference.

    g_grid (Slice backward) is bit-equal between the two where both cut the plane's points the same way: the fixed-point
    scatter-add rounds every product to a per-channel quantum and adds integers, so the thread count cannot change a bit.  Where
    the wide form holds 8192 points per segment and the narrow one 4096 (64^2 N8192: one segment against two; 16^3 N16384: two
    against four), each segment's quantum comes from ITS points' maximum and the partial tiles are added in float: the two runs
    then legitimately differ in the last bits and are held to twice the float64 bar instead.  g_keys agree within the bar; Splat(max)
    g_feat, a routing of single cotangents, is bit-equal.

    These clouds put thousands of points into one cell (3/4 of N = 4096 .. 16384): the fixed-point scatter's quantum grows with
    that count (q ~ max|g_out| * K * 2^-30), and measured against float64 its per-channel error reaches a few 1e-4 of the
    channel's max — the resolution of the format, not a wrong sum.  g_grid is held to the larger of 1e-4 of the channel's max and
    that resolution (fx_resolution); the rows of the table, with at most ~800 contributions per cell, keep the plain 1e-4."""
    inp = inputs(w.B, w.H, w.C, w.N, w.W, w.pad, seed=zlib.crc32(w.id.encode()))
    ref = reference(w.api, w.reduce, inp, w.B, w.H, w.C, w.N, w.W)
    res = {}
    for name, fl in (("wide", F.FORCE_HOT), ("narrow", F.FORCE_HOT | F.NO_WIDE)):
        flags(fl)
        got, tag, _ = run(w.api, w.reduce, inp, ref, w.B, w.H, w.C, w.N, w.W, ws=True, pad=w.pad)
        flags(0)
        assert tag == (w.tag if name == "wide" else w.narrow_tag), (name, tag)
        check(w.api, w.reduce, got, ref, inp, w.H, w.C, fx_bound=True)
        res[name] = got
    a, b = res["wide"], res["narrow"]
    if w.api.startswith("ct_slice"):
        if w.same_cut:
            assert torch.equal(a["g_grid"], b["g_grid"]), "g_grid of the wide and the narrow launch differ"
        else:
            assert grid_err(a["g_grid"], b["g_grid"], 2 * grid_allowed(inp, ref, w.H, w.C)) <= BAR
    else:
        assert torch.equal(a["g_feat"], b["g_feat"]), "g_feat of the wide and the narrow launch differ"
    assert relerr(a["g_keys"], b["g_keys"]) <= BAR
