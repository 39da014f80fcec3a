"""ct_slice_splat_bwd (csrc/ct_raster_bwd_fused.h): where the Splat half's per-point set-up and its counts come from.

The fused backward takes a point's base cell, weights and clamp flags from the plane sort (parked cells, the entries' weights, the
rank flags) instead of recomputing them from the keys per four-channel group, and tests a group for ties by counting matches and
non-zero cells wave by wave.  The cases here sit where that can go wrong: a single (peeled) group, an odd number of groups on a
grid whose cell indices need more than eight bits, waves with one and with 33 point-owning lanes, clamp flags without a Slice
cotangent beside them, one cell holding the whole plane, and a tie whose two points are counted by different waves.

Every case is bit parity with ct_slice_bwd_tk followed by ct_splat_bwd_tk under CT_DEBUG_FORCE_HOT (assert_parity of
tests/test_slice_splat_bwd_fused_gpu.py, whose docstring says how the two calls are brought to the same forms), except the
two-wave tie, whose winner no comparison of bits can pin: that test says what it asserts instead."""
import pytest
import torch

from tests import test_slice_splat_bwd_fused_gpu as F
from tests.test_slice_splat_bwd_fused_gpu import flags  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

KEY_HI = 0.99999988          # CT_KEY_HI of csrc/ct_common.h: the clamp passes a cotangent only inside [-KEY_HI, KEY_HI]


def test_a_single_group_on_the_headline_grid(flags):
    """C = 4: the group loop's peeled last group alone, N 4096 on 32 x 32."""
    mod, lib = F._lib()
    B, H, C, N, W = 1, 2, 4, 4096, (32, 32)
    keys, feat, cot, _ = F.make(B, H, C, N, W, seed=31)
    flags(mod.DEBUG_FORCE_HOT)
    assert F.supported(B, H, C, N, W) == 1
    F.assert_parity(keys, feat, cot, None, H, W)


def test_five_groups_on_a_grid_with_cells_beyond_255(flags):
    """C = 20: an odd group count for the alternating tie words; 16 x 24 = 384 cells: a parked base cell needs its nine bits."""
    mod, lib = F._lib()
    B, H, C, N, W = 1, 2, 20, 512, (16, 24)
    keys, feat, cot, _ = F.make(B, H, C, N, W, seed=32)
    flags(mod.DEBUG_FORCE_HOT)
    assert F.supported(B, H, C, N, W) == 1
    F.assert_parity(keys, feat, cot, None, H, W)


@pytest.mark.parametrize("N", [132, 260])
def test_a_wave_with_one_and_with_33_point_owners(N, flags):
    """33 and 65 point-owning threads: the last wave counts the matches of one lane (N = 260) or of 33 (N = 132), and they must be
    the right ones — the last quad's features are positive and dominant (its points apart from each other), so each of them wins
    cells in every channel: its g_feat is non-zero in every word."""
    mod, lib = F._lib()
    B, H, C, W = 1, 2, 8, (8, 8)
    keys, feat, cot, _ = F.make(B, H, C, N, W, seed=33)
    quad = torch.tensor([[-0.6, 0.6, -0.6, 0.6], [-0.6, -0.6, 0.6, 0.6]])       # (x, y) of the four points: four different cells
    for h in range(H):
        keys[0, 2 * h:2 * h + 2, N - 4:] = quad + 0.01 * h
    feat[:, :, N - 4:] = 100.0 + torch.arange(H * C * 4).float().view(H * C, 4)
    flags(mod.DEBUG_FORCE_HOT)
    assert F.supported(B, H, C, N, W) == 1
    o, _ = F.assert_parity(keys, feat, cot, None, H, W)
    last = o["g_feat"][:, :, N - 4:]
    assert int((last != 0).sum()) == last.numel(), last


def test_clamp_flags_without_a_slice_cotangent(flags):
    """The key menu of test_keys_on_cell_boundaries_and_at_the_ends, out-of-range keys in the first and the last quad, no
    g_keys_slice requested: g_keys' clamp mask comes from the rank flags alone.  An out-of-range coordinate's g_keys is a zero."""
    mod, lib = F._lib()
    B, H, C, N, W = 1, 2, 8, 512, (17, 12)
    g = torch.Generator().manual_seed(29)
    menu = torch.cat([torch.arange(-8, 9).float() / 8, torch.tensor([-1.5, 1.5, -0.99999994, 0.99999994])])
    keys = menu[torch.randint(0, menu.numel(), (B, H * 2, N), generator=g)]
    rnd = torch.rand(B, H * 2, N, generator=g) < 0.25
    keys = torch.where(rnd, torch.tanh(torch.randn(B, H * 2, N, generator=g)), keys)
    keys[0, :, 0:4] = torch.tensor([-1.5, 1.5, 1.0, -1.0])
    keys[0, :, N - 4:] = torch.tensor([1.5, 0.25, -1.5, 0.99999994])
    keys[0, 1, 1] = 0.5                     # (mixed inside one point: x out, y in, and the reverse)
    keys[0, 2, N - 2] = -0.375
    feat = torch.randn(B, H * C, N, generator=g) + torch.arange(N).float() * 1e-3
    cot = torch.randn(B, H * C, N, generator=g)
    flags(mod.DEBUG_FORCE_HOT)
    o, _ = F.assert_parity(keys, feat, cot, None, H, W, with_slice=False)
    hi = torch.tensor(KEY_HI, dtype=torch.float32)
    outside = ((keys < -hi) | (keys > hi)).cuda()
    assert int(outside[0, :, 0:4].sum()) >= 8 and int(outside[0, :, N - 4:].sum()) >= 8
    gk = o["g_keys"]
    assert bool((gk[outside] == 0.0).all())                      # +0.0 or -0.0, nothing else
    assert int((gk[~outside] != 0.0).sum()) > 0


def test_the_whole_plane_in_one_base_cell(flags):
    """All 4096 points of a plane based at one cell of 32 x 32: equal parked cells, 1024 items of one cell, K at its maximum."""
    mod, lib = F._lib()
    B, H, C, N, W = 1, 2, 8, 4096, (32, 32)
    g = torch.Generator().manual_seed(37)
    cellx, celly = 10, 21
    u = 0.05 + 0.9 * torch.rand(B, H * 2, N, generator=g)
    first = torch.tensor([cellx, celly] * H).float().view(1, H * 2, 1)
    keys = (first + u) * (2.0 / (W[0] - 1)) - 1.0
    feat = torch.randn(B, H * C, N, generator=g) + torch.arange(N).float() * 1e-3
    cot = torch.randn(B, H * C, N, generator=g)
    s = (keys + 1.0) * ((W[0] - 1) / 2.0)
    assert bool((s.floor() == first).all())
    flags(mod.DEBUG_FORCE_HOT)
    o, z = F.assert_parity(keys, feat, cot, None, H, W)
    assert int(z.count_nonzero()) <= H * C * 4                   # four cells per plane and channel hold anything


def test_one_crafted_tie_between_two_waves(flags):
    """Two points on one grid node, equal and dominant in one channel, owned by threads of DIFFERENT waves (points 36 and 292):
    one surplus match, counted by two waves.  Which of the two wins is first come between threads, so: g_z and
    g_keys_slice are the two calls' bits, every g_feat word but the two tied ones is (and every g_keys word but the two points'),
    exactly one of the two tied words is non-zero and it is the reference pair's non-zero one.  A count that loses a wave's
    matches sees no tie and lets both through."""
    mod, lib = F._lib()
    B, H, C, N, W = 1, 2, 8, 512, (8, 8)
    keys, feat, cot, _ = F.make(B, H, C, N, W, seed=5)
    k_node, _ = F._node_key(W[0])
    p0, p1, h0, c0 = 36, 36 + 256, 1, 6
    keys[0, h0 * 2:(h0 + 1) * 2, p0] = k_node
    keys[0, h0 * 2:(h0 + 1) * 2, p1] = k_node
    feat[0, h0 * C:(h0 + 1) * C, p1] = -1.0
    feat[0, h0 * C + c0, p0] = 100.0
    feat[0, h0 * C + c0, p1] = 100.0
    flags(mod.DEBUG_FORCE_HOT)
    keys, feat, cot = keys.cuda(), feat.cuda(), cot.cuda()
    z = F.forward_z(keys, feat, None, H, W)
    ref = F.two_calls(keys, feat, cot, None, z, H, W)
    o = F.outputs(B, H * C, H * 2, N, W)
    mod.check(F.fused_status(keys, feat, cot, None, z, H, W, o), "ct_slice_splat_bwd")
    assert lib.ct_debug_last_launch().decode() == F.TAG
    torch.cuda.synchronize()

    def bits(t):
        return t.view(torch.int32)

    assert torch.equal(bits(o["g_z"]), bits(ref["g_z"]))
    assert torch.equal(bits(o["g_keys_slice"]), bits(ref["g_keys_slice"]))
    row = h0 * C + c0
    same = bits(o["g_feat"]) == bits(ref["g_feat"])
    same[0, row, p0] = same[0, row, p1] = True
    assert bool(same.all()), int((~same).sum())
    same = bits(o["g_keys"]) == bits(ref["g_keys"])
    same[0, h0 * 2:(h0 + 1) * 2, p0] = True
    same[0, h0 * 2:(h0 + 1) * 2, p1] = True
    assert bool(same.all()), int((~same).sum())
    got = [float(o["g_feat"][0, row, p]) for p in (p0, p1)]
    want = [float(ref["g_feat"][0, row, p]) for p in (p0, p1)]
    print("tied g_feat words: fused", got, "two calls", want)
    assert sum(v != 0.0 for v in want) == 1, want
    assert sum(v != 0.0 for v in got) == 1, got
    assert max(got, key=abs) == max(want, key=abs), (got, want)
