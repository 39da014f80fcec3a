"""ct_slice_splat_bwd (csrc/ct_raster_bwd_fused.h): Slice backward and Splat(max) backward of a plane in one kernel.

Every parity case calls the fused entry and ct_slice_bwd_tk followed by ct_splat_bwd_tk(add = Slice's key cotangent) on the same
device inputs under CT_DEBUG_FORCE_HOT and compares g_z, g_feat, g_keys and (where requested) g_keys_slice with torch.equal: the
fused kernel has to write the two calls' bits.  Outputs start as NaN, so an element nobody wrote shows; refused calls must leave
them so.

The reference's forms.  The fused kernel keeps the summation orders of the forms the headline runs: the sorted Slice backward and
the hot Splat(max) backward with ONE workgroup per plane.  On a few planes the two calls pick other forms — the scatter form of
Slice backward rounds every product to the fixed-point quantum where the sorted form rounds an item's sum, and both deal a plane's
channel groups to several workgroups whose partial key cotangents are added afterwards — whose bits differ from the
one-workgroup forms' by construction.  The two calls therefore run on the case's clouds REPEATED along the batch to 256 planes
(and under CT_DEBUG_FORCE_SORTED beside CT_DEBUG_FORCE_HOT), where they take the headline's forms (the tags are pinned), and the
first copy is compared: the same inputs per plane, the same calls, every bit required.

Exact ties: a tied group is redone with single-winner claims, in the fused kernel as in splat_max_bwd_hot_kernel.  Between two
contributions of ONE thread the lower point index wins in both (a thread walks its quad in order); between threads the claim
goes to whichever comes first, which no comparison of bits can pin.  The tie cases here therefore keep a tied pair inside one quad
of four consecutive points, where both kernels are deterministic."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TAG = "slice_splat_bwd_fused"
EINVAL = -1


def _lib():
    from cloud_transformers_amd import _lib
    return _lib, _lib.load()


FLAGS = [0]      # what the running test has set (two_calls puts it back behind its own)


@pytest.fixture
def flags():
    mod, lib = _lib()

    def set_flags(v):
        FLAGS[0] = v
        lib.ct_debug_set_flags(v)

    yield set_flags
    set_flags(0)
    lib.ct_set_deterministic(0)


def make(B, H, C, N, W, seed=0, dup=False, pad=False):
    g = torch.Generator().manual_seed(seed + B * 131 + C * 7 + N)
    keys = torch.tanh(torch.randn(B, H * 2, N, generator=g))
    feat = torch.randn(B, H * C, N, generator=g)
    cot = torch.randn(B, H * C, N, generator=g)
    if dup:               # every point twice, the copies side by side (one quad holds two pairs)
        keys = keys[..., : N // 2].repeat_interleave(2, dim=-1)
        feat = feat[..., : N // 2].repeat_interleave(2, dim=-1)
    p = (torch.rand(B, N, generator=g) > 0.2).float() if pad else None
    return keys, feat, cot, p


def _pad(mod, pad):
    from cloud_transformers_amd.ops import _ptr
    return (None, mod.PAD_NONE) if pad is None else (_ptr(pad), mod.PAD_F32)


def supported(B, H, C, N, W, reduce="max", pad_dtype=0):
    mod, lib = _lib()
    return lib.ct_slice_splat_bwd_supported(B, H, C, N, len(W), mod.int_array(list(W)), mod.REDUCE[reduce], pad_dtype)


def forward_z(keys, feat, pad, H, W):
    from cloud_transformers_amd.ops import _ptr, _stream
    mod, lib = _lib()
    B, HC, N = feat.shape
    z = torch.full((B, HC, *W), float("nan"), device="cuda")
    pp, pd = _pad(mod, pad)
    mod.check(lib.ct_splat_fwd(_ptr(keys), _ptr(feat), pp, pd, _ptr(z), B, H, HC // H, N, len(W), mod.int_array(list(W)), 0,
                               _stream()), "ct_splat_fwd")
    return z


def outputs(B, HC, HD, N, W):
    nan = float("nan")
    return {"g_z": torch.full((B, HC, *W), nan, device="cuda"), "g_feat": torch.full((B, HC, N), nan, device="cuda"),
            "g_keys_slice": torch.full((B, HD, N), nan, device="cuda"), "g_keys": torch.full((B, HD, N), nan, device="cuda")}


def two_calls(keys, feat, cot, pad, z, H, W):
    """ct_slice_bwd_tk, then ct_splat_bwd_tk(add = Slice's key cotangent), on the clouds repeated to >= 256 planes (module
    docstring); returns the first copy's outputs"""
    from cloud_transformers_amd.ops import _ptr, _stream
    mod, lib = _lib()
    B0 = feat.shape[0]
    rep = -(-256 // (B0 * H))
    keys, feat, cot, z = (t.repeat(rep, *([1] * (t.dim() - 1))).contiguous() for t in (keys, feat, cot, z))
    pad = None if pad is None else pad.repeat(rep, 1).contiguous()
    B, HC, N = feat.shape
    C, dim, Wa = HC // H, len(W), mod.int_array(list(W))
    o = outputs(B, HC, H * dim, N, W)
    pp, pd = _pad(mod, pad)
    n1 = lib.ct_slice_bwd_workspace_bytes(B, H, C, N, dim, Wa)
    n2 = lib.ct_splat_bwd_ex_workspace_bytes(B, H, C, N, dim, Wa, 0, mod.BWD_ACCUMULATE_KEYS)
    ws1 = torch.empty(max(n1, 16), device="cuda", dtype=torch.uint8)
    ws2 = torch.empty(max(n2, 16), device="cuda", dtype=torch.uint8)
    tk = torch.zeros(mod.TICKETS_BYTES // 4, device="cuda", dtype=torch.int32)
    before = FLAGS[0]
    lib.ct_debug_set_flags(mod.DEBUG_FORCE_HOT | mod.DEBUG_FORCE_SORTED)
    mod.check(lib.ct_slice_bwd_tk(_ptr(keys), _ptr(z), pp, pd, _ptr(cot), _ptr(o["g_z"]), _ptr(o["g_keys_slice"]),
                                  _ptr(ws1) if n1 else None, n1, _ptr(tk), B, H, C, N, dim, Wa, _stream()), "ct_slice_bwd_tk")
    tag1 = lib.ct_debug_last_launch().decode()
    mod.check(lib.ct_splat_bwd_tk(_ptr(keys), _ptr(feat), pp, pd, _ptr(z), _ptr(o["g_z"]), _ptr(o["g_feat"]),
                                  _ptr(o["g_keys_slice"]), _ptr(o["g_keys"]), _ptr(ws2) if n2 else None, n2, _ptr(tk),
                                  B, H, C, N, dim, Wa, 0, _stream()), "ct_splat_bwd_tk")
    tag2 = lib.ct_debug_last_launch().decode()
    lib.ct_debug_set_flags(before)
    torch.cuda.synchronize()
    assert tag1 == "slice_bwd_sorted" and tag2 == "splat_max_bwd_hot", (tag1, tag2)      # one workgroup per plane, both
    for t in o.values():                                                                  # every copy of a plane: the same bits
        assert torch.equal(t[:B0].view(torch.int32), t[B - B0:].view(torch.int32))
    return {k: t[:B0].contiguous() for k, t in o.items()}


def fused_status(keys, feat, cot, pad, z, H, W, o, reduce="max", with_slice=True):
    from cloud_transformers_amd.ops import _ptr, _stream
    mod, lib = _lib()
    B, HC, N = feat.shape
    pp, pd = _pad(mod, pad)
    return lib.ct_slice_splat_bwd(_ptr(keys), _ptr(feat), pp, pd, _ptr(z), _ptr(cot), _ptr(o["g_z"]), _ptr(o["g_feat"]),
                                  _ptr(o["g_keys_slice"]) if with_slice else None, _ptr(o["g_keys"]),
                                  B, H, HC // H, N, len(W), mod.int_array(list(W)), mod.REDUCE[reduce], _stream())


def assert_parity(keys, feat, cot, pad, H, W, with_slice=True):
    """the fused call against the two calls on the same inputs (host tensors in, z from ct_splat_fwd); returns the fused outputs"""
    mod, lib = _lib()
    keys, feat, cot = keys.cuda(), feat.cuda(), cot.cuda()
    pad = None if pad is None else pad.cuda()
    z = forward_z(keys, feat, pad, H, W)
    ref = two_calls(keys, feat, cot, pad, z, H, W)
    B, HC, N = feat.shape
    o = outputs(B, HC, H * 2, N, W)
    mod.check(fused_status(keys, feat, cot, pad, z, H, W, o, with_slice=with_slice), "ct_slice_splat_bwd")
    tag = lib.ct_debug_last_launch().decode()
    torch.cuda.synchronize()
    assert tag == TAG, tag
    names = ("g_z", "g_feat", "g_keys") + (("g_keys_slice",) if with_slice else ())
    diff = {}
    for n in names:
        same = (o[n].view(torch.int32) == ref[n].view(torch.int32))
        diff[n] = int((~same).sum())
        print("%s: %d of %d words differ" % (n, diff[n], o[n].numel()))
    assert all(d == 0 for d in diff.values()), diff
    if not with_slice:
        assert bool(torch.isnan(o["g_keys_slice"]).all())
    return o, z


# B, H, C, N, W, duplicated points, padding mask, Slice's own cotangent requested
PARITY = [
    (1, 1, 4, 4, (8, 8), False, False, True),          # one group, one quad, almost every cell empty
    (1, 2, 8, 256, (8, 8), True, False, True),         # every point twice: every group of every plane tied
    (1, 2, 8, 2052, (32, 32), False, False, False),    # a ragged last wave
    (2, 3, 12, 516, (16, 24), False, False, True),     # non-square general grid, three groups (with a mask: refused, below)
    (1, 2, 16, 4096, (32, 32), False, False, True),    # the <false, 32, 4096, 16> instance
]


@pytest.mark.parametrize("cfg", PARITY, ids=[str(c) for c in PARITY])
def test_fused_backward_writes_the_two_calls_bits(cfg, flags):
    mod, lib = _lib()
    B, H, C, N, W, dup, pad, with_slice = cfg
    keys, feat, cot, p = make(B, H, C, N, W, dup=dup, pad=pad)
    flags(mod.DEBUG_FORCE_HOT)
    assert supported(B, H, C, N, W, pad_dtype=mod.PAD_F32 if pad else 0) == 1
    assert_parity(keys, feat, cot, p, H, W, with_slice)


def test_a_padding_mask_is_refused(flags):
    """The HAS_PAD instance of the kernel spills in its group loop and is not built: the query answers 0 for either mask type,
    the call CT_EINVAL, and nothing is written."""
    mod, lib = _lib()
    B, H, C, N, W = 2, 3, 12, 516, (16, 24)
    keys, feat, cot, p = make(B, H, C, N, W, pad=True)
    keys, feat, cot, p = keys.cuda(), feat.cuda(), cot.cuda(), p.cuda()
    z = forward_z(keys, feat, p, H, W)
    flags(mod.DEBUG_FORCE_HOT)
    assert supported(B, H, C, N, W, pad_dtype=mod.PAD_F32) == 0 and supported(B, H, C, N, W, pad_dtype=mod.PAD_I32) == 0
    assert supported(B, H, C, N, W) == 1
    o = outputs(B, H * C, H * 2, N, W)
    assert fused_status(keys, feat, cot, p, z, H, W, o) == EINVAL
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in o.values())


def _node_key(W):
    """as tests/test_tie_rule_gpu.py: a key that sits exactly on a grid node (three corner weights exactly 0)"""
    import numpy as np
    hw = np.float32((W - 1) / 2.0)
    for j in range(2, W - 2):
        k = np.float32(2.0 * j / (W - 1) - 1.0)
        for _ in range(8):
            s = np.float32(np.float32(k + np.float32(1.0)) * hw)
            if float(s) == float(j):
                return float(k), j
            k = np.nextafter(k, np.float32(1.0 if s < j else -1.0), dtype=np.float32)
    raise AssertionError("no node key for W = %d" % W)


def test_one_crafted_tie_in_one_group_of_one_plane(flags):
    """Two points on one grid node, equal and dominant in ONE channel: one surplus match in one group of one plane."""
    mod, lib = _lib()
    B, H, C, N, W = 1, 2, 8, 256, (8, 8)
    keys, feat, cot, _ = make(B, H, C, N, W, seed=5)
    k_node, _ = _node_key(W[0])
    p0, p1, h0, c0 = 36, 37, 1, 6                       # one quad; the second group of plane 1
    keys[0, h0 * 2:(h0 + 1) * 2, p0] = k_node
    keys[0, h0 * 2:(h0 + 1) * 2, p1] = k_node
    feat[0, h0 * C:(h0 + 1) * C, p1] = -1.0
    feat[0, h0 * C + c0, p0] = 100.0
    feat[0, h0 * C + c0, p1] = 100.0
    flags(mod.DEBUG_FORCE_HOT)
    o, _ = assert_parity(keys, feat, cot, None, H, W)
    a0, a1 = float(o["g_feat"][0, h0 * C + c0, p0]), float(o["g_feat"][0, h0 * C + c0, p1])
    assert a0 != 0.0 and a1 == 0.0, (a0, a1)          # one winner: the lower index of the quad


def test_all_negative_features_give_no_matches(flags):
    mod, lib = _lib()
    B, H, C, N, W = 1, 2, 8, 256, (8, 8)
    keys, feat, cot, _ = make(B, H, C, N, W, seed=2)
    feat = -feat.abs() - 0.1
    flags(mod.DEBUG_FORCE_HOT)
    o, z = assert_parity(keys, feat, cot, None, H, W)
    assert int(z.view(torch.int32).count_nonzero()) == 0
    assert int(o["g_feat"].view(torch.int32).count_nonzero()) == 0          # +0.0 everywhere, by its bits


def test_an_infinite_cotangent_takes_the_float_path(flags):
    mod, lib = _lib()
    B, H, C, N, W = 1, 2, 8, 256, (8, 8)
    keys, feat, cot, _ = make(B, H, C, N, W, seed=3)
    cot[0, C + 5, 17] = float("inf")                    # plane 1, second group
    flags(mod.DEBUG_FORCE_HOT)
    o, _ = assert_parity(keys, feat, cot, None, H, W)
    assert bool(torch.isinf(o["g_z"][0, C + 5]).any())


def test_a_zero_cotangent(flags):
    mod, lib = _lib()
    B, H, C, N, W = 1, 2, 8, 256, (8, 8)
    keys, feat, cot, _ = make(B, H, C, N, W, seed=4)
    flags(mod.DEBUG_FORCE_HOT)
    o, _ = assert_parity(keys, feat, torch.zeros_like(cot), None, H, W)
    assert int(o["g_z"].count_nonzero()) == 0 and int(o["g_feat"].count_nonzero()) == 0 and int(o["g_keys"].count_nonzero()) == 0


def test_keys_on_cell_boundaries_and_at_the_ends(flags):
    """Keys of exactly -1 and 1, beyond them, and on grid lines (extent 17: every multiple of 1/8 is a line): zero weights, edge
    cells, cotangents the clamp does not pass."""
    mod, lib = _lib()
    B, H, C, N, W = 1, 2, 8, 512, (17, 12)
    g = torch.Generator().manual_seed(23)
    menu = torch.cat([torch.arange(-8, 9).float() / 8, torch.tensor([-1.5, 1.5, -0.99999994, 0.99999994])])
    keys = menu[torch.randint(0, menu.numel(), (B, H * 2, N), generator=g)]
    rnd = torch.rand(B, H * 2, N, generator=g) < 0.25
    keys = torch.where(rnd, torch.tanh(torch.randn(B, H * 2, N, generator=g)), keys)
    # (grid-line points share cells and weights: distinct feature magnitudes keep their products apart)
    feat = torch.randn(B, H * C, N, generator=g) + torch.arange(N).float() * 1e-3
    cot = torch.randn(B, H * C, N, generator=g)
    flags(mod.DEBUG_FORCE_HOT)
    assert_parity(keys, feat, cot, None, H, W)


REFUSED = [
    # id, B, H, C, N, W, reduce, flags, deterministic
    ("dim3", 1, 2, 8, 1024, (8, 8, 8), "max", "FORCE_HOT", 0),
    ("sum", 1, 2, 8, 1024, (32, 32), "sum", "FORCE_HOT", 0),
    ("n8192", 1, 2, 4, 8192, (32, 32), "max", "FORCE_HOT", 0),
    ("c6", 1, 2, 6, 1024, (32, 32), "max", "FORCE_HOT", 0),
    ("deterministic", 1, 2, 8, 1024, (32, 32), "max", "FORCE_HOT", 1),
    ("no_hot", 1, 2, 8, 1024, (32, 32), "max", "NO_HOT", 0),
    ("no_sorted", 1, 2, 8, 1024, (32, 32), "max", "NO_SORTED", 0),
    ("few_planes_no_flags", 1, 2, 8, 1024, (32, 32), "max", None, 0),
]


@pytest.mark.parametrize("cfg", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_calls_answer_zero_and_einval_and_write_nothing(cfg, flags):
    mod, lib = _lib()
    _, B, H, C, N, W, reduce, fl, det = cfg
    g = torch.Generator().manual_seed(1)
    dim = len(W)
    keys = torch.tanh(torch.randn(B, H * dim, N, generator=g)).cuda()
    feat, cot = torch.randn(B, H * C, N, generator=g).cuda(), torch.randn(B, H * C, N, generator=g).cuda()
    z = torch.rand(B, H * C, *W, generator=g).cuda()
    o = outputs(B, H * C, H * dim, N, W)
    flags(0 if fl is None else getattr(mod, "DEBUG_" + fl))
    lib.ct_set_deterministic(det)
    assert supported(B, H, C, N, W, reduce) == 0
    assert fused_status(keys, feat, cot, None, z, H, W, o, reduce) == EINVAL
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in o.values())


def test_null_misaligned_and_aliased_pointers_are_refused(flags):
    mod, lib = _lib()
    B, H, C, N, W = 1, 2, 8, 1024, (32, 32)
    keys, feat, cot, _ = make(B, H, C, N, W)
    keys, feat, cot = keys.cuda(), feat.cuda(), cot.cuda()
    z = forward_z(keys, feat, None, H, W)
    flags(mod.DEBUG_FORCE_HOT)
    assert supported(B, H, C, N, W) == 1
    o = outputs(B, H * C, H * 2, N, W)
    buf = torch.full((cot.numel() + 1,), 0.5, device="cuda")
    off4 = buf[1:].view(cot.shape)
    assert off4.data_ptr() % 16 == 4
    assert fused_status(keys, feat, off4, None, z, H, W, o) == EINVAL
    assert fused_status(keys, feat, cot, None, z, H, W, dict(o, g_keys=keys)) == EINVAL            # g_keys aliasing an input
    assert fused_status(keys, feat, cot, None, z, H, W, dict(o, g_keys=o["g_keys_slice"])) == EINVAL
    from cloud_transformers_amd.ops import _ptr, _stream
    Wa = mod.int_array(list(W))
    assert lib.ct_slice_splat_bwd(_ptr(keys), None, None, 0, _ptr(z), _ptr(cot), _ptr(o["g_z"]), _ptr(o["g_feat"]), None,
                                  _ptr(o["g_keys"]), B, H, C, N, 2, Wa, 0, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in o.values())


def _step_inputs(B, H, C, N, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.tanh(torch.randn(B, H * 2, N, generator=g)).cuda(), torch.randn(B, H * C, N, generator=g).cuda(),
            torch.randn(B, H * C, N, generator=g).cuda())


def test_step_graph_replays_with_the_fused_backward(flags):
    """SplatSliceStep.run() captured at (B2, H4, C16, N4096, 32 x 32) and replayed three times on fresh inputs copied into its
    static tensors: every replay equals an eager two-call step on that data."""
    from cloud_transformers_amd.step import SplatSliceStep
    mod, lib = _lib()
    B, H, C, N, W = 2, 4, 16, 4096, 32
    flags(mod.DEBUG_FORCE_HOT)
    keys, feat, cot = _step_inputs(B, H, C, N, 11)
    step = SplatSliceStep(keys, feat, cot, W, H, 2, "max")
    assert step.fused_bwd
    step.run()                                   # eager warm-up (sets the LDS attributes before capture)
    torch.cuda.synchronize()
    assert step.backward_tag() == TAG, step.backward_tag()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step.run()
    for seed in (12, 13, 14):
        k, f, c = _step_inputs(B, H, C, N, seed)
        z = forward_z(k, f, None, H, (W, W))
        ref = two_calls(k, f, c, None, z, H, (W, W))
        step.keys.copy_(k)
        step.feat.copy_(f)
        step.cot.copy_(c)
        for t in (step.g_z, step.g_feat, step.g_keys()):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(step.z, z), seed
        assert torch.equal(step.g_z, ref["g_z"]), seed
        assert torch.equal(step.g_feat, ref["g_feat"]), seed
        assert torch.equal(step.g_keys(), ref["g_keys"]), seed


def test_backward_tag_reports_what_run_launched(flags, monkeypatch):
    from cloud_transformers_amd.step import SplatSliceStep
    mod, lib = _lib()
    B, H, C, N, W = 1, 2, 8, 1024, 32
    flags(mod.DEBUG_FORCE_HOT)
    keys, feat, cot = _step_inputs(B, H, C, N, 7)
    a = SplatSliceStep(keys, feat, cot, W, H, 2, "max")
    assert a.fused_bwd and a.backward_tag() is None
    a.run()
    assert a.backward_tag() == TAG, a.backward_tag()
    monkeypatch.setenv("CLOUDCT_FUSED_BWD", "0")
    b = SplatSliceStep(keys, feat, cot, W, H, 2, "max")
    assert not b.fused_bwd
    b.run()
    torch.cuda.synchronize()
    # (a call's tag may itself join several notes with "+": the Slice call's come first, then the Splat call's)
    old = b.backward_tag()
    assert old.startswith("slice_bwd") and "+splat_max_bwd" in old and TAG not in old, old
    assert torch.equal(a.z, b.z) and torch.equal(a.out, b.out)
    ref = two_calls(keys, feat, cot, None, a.z, H, (W, W))
    assert torch.equal(a.g_z, ref["g_z"]) and torch.equal(a.g_feat, ref["g_feat"]) and torch.equal(a.g_keys(), ref["g_keys"])
    # (the two-call step on two planes: other forms — the same values to rounding)
    assert float((a.g_feat - b.g_feat).abs().max()) <= 1e-4 * float(b.g_feat.abs().max())
    assert float((a.g_keys() - b.g_keys()).abs().max()) <= 1e-4 * float(b.g_keys().abs().max())
    c = SplatSliceStep(keys, feat, cot, W, H, 2, "max", plane_sort=True)      # a plane-sort record: the two calls
    assert not c.fused_bwd or c.sorted is None
