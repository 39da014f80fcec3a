"""ct_splat_slice_fwd (csrc/ct_raster_fwd_fused.h): Splat(max) forward and Slice forward of a plane in one kernel.

Every parity case calls the fused entry and ct_splat_fwd + ct_slice_fwd on the same inputs under the same flags and compares z
and out with torch.equal — the fused kernel has to write the two calls' bits, not values close to them.  Outputs start as NaN, so
an element nobody wrote shows.  The parity cases pin the launch tag; the refused cases pin the query's 0 and the call's CT_EINVAL
with the outputs untouched.  Few-plane shapes take the kernel under CT_DEBUG_FORCE_HOT, as the other hot families' tests do."""
import pytest
import torch

from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

TAG = "splat_slice_fwd_fused"
EINVAL = -1


def _lib():
    from cloud_transformers_amd import _lib
    return _lib, _lib.load()


@pytest.fixture
def flags():
    mod, lib = _lib()
    yield lambda v: lib.ct_debug_set_flags(v)
    lib.ct_debug_set_flags(0)


def make(B, H, C, N, W, seed=0, dup=False, pad=None):
    g = torch.Generator().manual_seed(seed + B * 131 + C * 7 + N)
    dim = len(W)
    keys = torch.tanh(torch.randn(B, H * dim, N, generator=g))
    feat = torch.randn(B, H * C, N, generator=g)
    if dup:
        keys = keys[..., : N // 2].repeat(1, 1, 2)
        feat = feat[..., : N // 2].repeat(1, 1, 2)
    p = None
    if pad == "f32":
        p = (torch.rand(B, N, generator=g) > 0.2).float()
    elif pad == "i32":
        p = (torch.rand(B, N, generator=g) > 0.2).int()
    return keys, feat, p


def pad_args(mod, pad):
    from cloud_transformers_amd.ops import _ptr
    if pad is None:
        return None, mod.PAD_NONE
    return _ptr(pad), (mod.PAD_F32 if pad.dtype == torch.float32 else mod.PAD_I32)


def supported(B, H, C, N, W, reduce="max", pad_dtype=0):
    mod, lib = _lib()
    return lib.ct_splat_slice_fwd_supported(B, H, C, N, len(W), mod.int_array(list(W)), mod.REDUCE[reduce], pad_dtype)


def two_calls(keys, feat, pad, H, W):
    """(z, out) of ct_splat_fwd followed by ct_slice_fwd, both pre-filled with NaN; device tensors"""
    from cloud_transformers_amd.ops import _ptr, _stream
    mod, lib = _lib()
    B, HC, N = feat.shape
    C, dim, Wa = HC // H, len(W), mod.int_array(list(W))
    z = torch.full((B, HC, *W), float("nan"), device="cuda")
    out = torch.full((B, HC, N), float("nan"), device="cuda")
    pp, pd = pad_args(mod, pad)
    mod.check(lib.ct_splat_fwd(_ptr(keys), _ptr(feat), pp, pd, _ptr(z), B, H, C, N, dim, Wa, 0, _stream()), "ct_splat_fwd")
    mod.check(lib.ct_slice_fwd(_ptr(keys), _ptr(z), pp, pd, _ptr(out), B, H, C, N, dim, Wa, _stream()), "ct_slice_fwd")
    return z, out


def fused_status(keys, feat, pad, H, W, z, out, reduce="max"):
    from cloud_transformers_amd.ops import _ptr, _stream
    mod, lib = _lib()
    B, HC, N = feat.shape
    pp, pd = pad_args(mod, pad)
    return lib.ct_splat_slice_fwd(_ptr(keys), _ptr(feat), pp, pd, _ptr(z), _ptr(out), B, H, HC // H, N, len(W),
                                  mod.int_array(list(W)), mod.REDUCE[reduce], _stream())


def fused(keys, feat, pad, H, W):
    mod, lib = _lib()
    B, HC, N = feat.shape
    z = torch.full((B, HC, *W), float("nan"), device="cuda")
    out = torch.full((B, HC, N), float("nan"), device="cuda")
    mod.check(fused_status(keys, feat, pad, H, W, z, out), "ct_splat_slice_fwd")
    return z, out, lib.ct_debug_last_launch().decode()


def assert_parity(keys, feat, pad, H, W):
    """the fused call against the two calls on the same device inputs, under whatever flags are set; returns the fused (z, out)"""
    z_ref, out_ref = two_calls(keys, feat, pad, H, W)
    z, out, tag = fused(keys, feat, pad, H, W)
    torch.cuda.synchronize()
    assert tag == TAG, tag
    assert not bool(torch.isnan(z).any()) and not bool(torch.isnan(out).any())
    assert torch.equal(z, z_ref), "z: %d words differ" % int((z != z_ref).sum())
    assert torch.equal(out, out_ref), "out: %d words differ" % int((out != out_ref).sum())
    return z, out


# B, H, C, N, W, duplicated points, padding mask
PARITY = [
    (1, 2, 8, 1024, (32, 32), False, None),       # one chunk, one quad per thread
    (1, 2, 16, 4096, (32, 32), False, None),      # the headline's plane: every thread of the workgroup busy
    (2, 3, 12, 516, (16, 24), False, None),       # general-grid form, threads without a quad, a 12-channel plane, non-square
    (3, 3, 8, 1024, (32, 32), False, None),       # nine planes: not a multiple of the eight XCDs
    (1, 1, 32, 2048, (16, 16), False, None),      # the most channels per plane here: more than two chunks where a plane is chunked
    (1, 2, 8, 256, (8, 8), True, None),           # every point twice: heavy contention on the atomics, exact ties
    (2, 2, 12, 516, (16, 24), False, "f32"),      # padding masks: the HAS_PAD form of both halves
    (1, 2, 8, 1024, (32, 32), False, "i32"),
]


@pytest.mark.parametrize("cfg", PARITY, ids=[str(c) for c in PARITY])
def test_fused_forward_writes_the_two_calls_bits(cfg, flags):
    mod, lib = _lib()
    B, H, C, N, W, dup, pad = cfg
    keys, feat, p = make(B, H, C, N, W, dup=dup, pad=pad)
    flags(mod.DEBUG_FORCE_HOT)
    assert supported(B, H, C, N, W, pad_dtype={None: 0, "f32": mod.PAD_F32, "i32": mod.PAD_I32}[pad]) == 1
    assert_parity(keys.cuda(), feat.cuda(), None if p is None else p.cuda(), H, W)


@pytest.mark.parametrize("cfg", PARITY[:2], ids=[str(c) for c in PARITY[:2]])
def test_fused_forward_against_the_oracle(cfg, flags):
    """z bit-exact (a max of products formed in the reference's order), out within 1e-4 of the tensor's max"""
    mod, lib = _lib()
    B, H, C, N, W, dup, pad = cfg
    keys, feat, _ = make(B, H, C, N, W)
    lc, idx = R.positions(keys, list(W), H, 2)
    z_ref = R.splat(lc, idx, feat, None, list(W), H, 2, "max")
    out_ref = R.slice_(lc, idx, z_ref, None, list(W), H, 2)
    flags(mod.DEBUG_FORCE_HOT)
    z, out, tag = fused(keys.cuda(), feat.cuda(), None, H, W)
    assert tag == TAG, tag
    assert torch.equal(z.cpu(), z_ref)
    err = float((out.cpu().double() - out_ref.double()).abs().max() / out_ref.double().abs().max())
    print("out against the oracle: %.3e" % err)
    assert err <= 1e-4, err


def test_edge_keys_boundary_points_and_signed_zero_products(flags):
    """Keys of exactly -1, 0 and 1 and points exactly on cell boundaries (x extent 17: half-width 8, so every multiple of 1/8 lands
    on a grid line and one corner weight is exactly 0), features of exactly +0 and -0: edge cells, zero weights, +-0 products against
    the zero floor — the same bits as the two calls, on the general grid and on the folded 32 x 32 one."""
    mod, lib = _lib()
    flags(mod.DEBUG_FORCE_HOT)
    for W in ((17, 12), (32, 32)):
        B, H, C, N = 1, 2, 8, 1024
        g = torch.Generator().manual_seed(17 + W[0])
        menu = torch.cat([torch.arange(-8, 9).float() / 8, torch.tensor([-1.5, 1.5, -0.99999994, 0.99999994])])
        pick = torch.randint(0, menu.numel(), (B, H * 2, N), generator=g)
        keys = menu[pick]
        rnd = torch.rand(B, H * 2, N, generator=g) < 0.25             # a quarter of the coordinates stay off the lines
        keys = torch.where(rnd, torch.tanh(torch.randn(B, H * 2, N, generator=g)), keys)
        feat = torch.randn(B, H * C, N, generator=g)
        feat[..., ::7] = 0.0
        feat[..., 3::7] = -0.0
        lc, _ = R.positions(keys, list(W), H, 2)
        if W[0] == 17:
            assert int((lc == 0).sum()) > N // 4                       # the case is what it says: exact zero weights
        z, out = assert_parity(keys.cuda(), feat.cuda(), None, H, W)
        assert bool((z >= 0).all())


def test_all_negative_channel_stays_at_the_floor(flags):
    mod, lib = _lib()
    B, H, C, N, W = 1, 2, 8, 1024, (32, 32)
    keys, feat, _ = make(B, H, C, N, W, seed=3)
    feat[:, 5] = -feat[:, 5].abs() - 0.1           # head 0, channel 5
    feat[:, C + 2] = -feat[:, C + 2].abs() - 0.1   # head 1, channel 2
    flags(mod.DEBUG_FORCE_HOT)
    z, out = assert_parity(keys.cuda(), feat.cuda(), None, H, W)
    for ch in (5, C + 2):
        assert int(z[:, ch].view(torch.int32).count_nonzero()) == 0        # +0.0 in every cell, by its bits
        assert int(out[:, ch].count_nonzero()) == 0


REFUSED = [
    # id, B, H, C, N, W, reduce, flags
    ("n8192", 1, 2, 4, 8192, (32, 32), "max", "FORCE_HOT"),
    ("dim3", 1, 2, 8, 1024, (8, 8, 8), "max", "FORCE_HOT"),
    ("sum", 1, 2, 8, 1024, (32, 32), "sum", "FORCE_HOT"),
    ("no_hot", 1, 2, 8, 1024, (32, 32), "max", "NO_HOT"),
    ("few_planes_no_flags", 1, 2, 8, 1024, (32, 32), "max", None),
]


@pytest.mark.parametrize("cfg", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_shapes_answer_zero_and_einval_and_write_nothing(cfg, flags):
    mod, lib = _lib()
    _, B, H, C, N, W, reduce, fl = cfg
    keys, feat, _ = make(B, H, C, N, W)
    keys, feat = keys.cuda(), feat.cuda()
    z = torch.full((B, H * C, *W), float("nan"), device="cuda")
    out = torch.full((B, H * C, N), float("nan"), device="cuda")
    flags(0 if fl is None else getattr(mod, "DEBUG_" + fl))
    assert supported(B, H, C, N, W, reduce) == 0
    assert fused_status(keys, feat, None, H, W, z, out, reduce) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(z).all()) and bool(torch.isnan(out).all())


@pytest.mark.parametrize("which", ["keys", "feat", "z", "out"])
def test_misaligned_pointer_is_refused_by_the_call(which, flags):
    """The query sees no pointers (it answers for the shape: 1); the call plans with their low bits and refuses."""
    mod, lib = _lib()
    B, H, C, N, W = 1, 2, 8, 1024, (32, 32)
    keys, feat, _ = make(B, H, C, N, W)

    def off4(t):          # the same values 4 bytes past a 16-byte boundary
        buf = torch.empty(t.numel() + 1, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    t = {"keys": keys.cuda(), "feat": feat.cuda(), "z": torch.full((B, H * C, *W), float("nan"), device="cuda"),
         "out": torch.full((B, H * C, N), float("nan"), device="cuda")}
    t[which] = off4(t[which])
    flags(mod.DEBUG_FORCE_HOT)
    assert supported(B, H, C, N, W) == 1
    assert fused_status(t["keys"], t["feat"], None, H, W, t["z"], t["out"]) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(t["z"]).all()) and bool(torch.isnan(t["out"]).all())


def _step_inputs(B, H, C, N, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.tanh(torch.randn(B, H * 2, N, generator=g)).cuda(), torch.randn(B, H * C, N, generator=g).cuda(),
            torch.randn(B, H * C, N, generator=g).cuda())


def test_step_on_a_refused_shape_runs_the_four_calls(flags):
    from cloud_transformers_amd.step import SplatSliceStep
    mod, lib = _lib()
    B, H, C, N, W = 1, 2, 4, 8192, 32
    keys, feat, cot = _step_inputs(B, H, C, N, 5)
    flags(mod.DEBUG_FORCE_HOT)
    a = SplatSliceStep(keys, feat, cot, W, H, 2, "max")
    assert not a.fused_fwd
    a.run()
    assert a.forward_tag() == "scatter_quad_max+gather_ci", a.forward_tag()
    b = SplatSliceStep(keys, feat, cot, W, H, 2, "max")
    for name in b.PASSES:
        getattr(b, name)()
    torch.cuda.synchronize()
    for name in ("z", "out", "g_z", "g_feat"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    gk_a, gk_b = a.g_keys().double(), b.g_keys().double()
    assert float((gk_a - gk_b).abs().max()) <= 1e-6 * float(gk_b.abs().max())


def test_step_graph_replays_with_the_fused_forward(flags):
    """SplatSliceStep.run() captured at (B2, H4, C16, N4096, 32 x 32) and replayed twice on fresh inputs copied into its static
    buffers: each replay's z and out are the eager two calls' bits for that data."""
    from cloud_transformers_amd.step import SplatSliceStep
    mod, lib = _lib()
    B, H, C, N, W = 2, 4, 16, 4096, 32
    flags(mod.DEBUG_FORCE_HOT)
    keys, feat, cot = _step_inputs(B, H, C, N, 11)
    step = SplatSliceStep(keys, feat, cot, W, H, 2, "max")
    assert step.fused_fwd
    step.run()                                   # eager warm-up (sets the LDS attributes before capture)
    torch.cuda.synchronize()
    assert step.forward_tag() == TAG, step.forward_tag()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step.run()
    for seed in (12, 13):
        k, f, c = _step_inputs(B, H, C, N, seed)
        z_ref, out_ref = two_calls(k, f, None, H, (W, W))
        step.keys.copy_(k)
        step.feat.copy_(f)
        step.cot.copy_(c)
        step.z.fill_(float("nan"))
        step.out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(step.z, z_ref), seed
        assert torch.equal(step.out, out_ref), seed
    assert step.forward_tag() == TAG
