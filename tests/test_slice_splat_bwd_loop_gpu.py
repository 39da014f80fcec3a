"""The group loop of ct_slice_splat_bwd (csrc/ct_raster_bwd_fused.h) at the sizes where its layout can go wrong.

The loop keeps its pair tile {z, z, g_z, g_z} over the stage area (dead between the items and the next group's staging), clears a
cell's accumulator words in the thread that converted them, takes the convert phase's quanta from the items' and hands the row
results of its reductions to LDS from four lanes a wave.  What that can break, and the case that shows it:
  * the zero entry Sg[N], which padded item slots read, lies under the pair tile whenever N < 2 G: it has to be whole again in
    every later group (N < 2 G with two and three groups; N = 2 G exactly; N just above);
  * the redo of a tied group stages its pairs over the tile area after the loop used the stage area (every point twice; one
    crafted tie in the LAST group, N < 2 G);
  * the float path writes a group's accumulators as floats: the next group has to start from integer zeros and its own quanta;
  * rows of a wave without a valid point or a cell, ragged last waves, threads with a cell and no quad and the reverse;
  * the tie counters' parity is used again in a third group; a one-group launch runs the last-group body only.
Every case is tests/test_slice_splat_bwd_fused_gpu.py's comparison: the fused call against ct_slice_bwd_tk + ct_splat_bwd_tk on the
case's planes repeated to 256, under CT_DEBUG_FORCE_HOT, torch.equal on g_z, g_feat, g_keys and Slice's key cotangent."""
import pytest
import torch

from tests.test_slice_splat_bwd_fused_gpu import _lib, _node_key, assert_parity, flags, make, supported  # noqa: F401

pytestmark = pytest.mark.gpu

# B, H, C, N, W, duplicated points
CASES = [
    (1, 2, 8, 64, (8, 8), False),          # N < 2 G, two groups: Sg[N] under the pair tile
    (1, 1, 12, 4, (8, 8), False),          # N < 2 G, three groups, one quad
    (1, 2, 8, 2048, (32, 32), False),      # N = 2 G exactly: the zero entry is the first word behind the pair tile
    (1, 2, 8, 2052, (32, 32), False),      # just above; a ragged last wave, a row of lanes with one valid quad
    (1, 2, 4, 1024, (32, 32), False),      # one group: only the last-group body runs
    (1, 2, 12, 1024, (32, 32), False),     # three groups: the tie counters' first parity is used again
    (1, 2, 8, 256, (8, 8), True),          # every point twice: every group tied, the redo stages over the tile area
    (1, 2, 8, 40, (8, 8), False),          # 10 quads, 64 cells: threads with a cell and no quad, rows without a point
    (2, 3, 12, 516, (16, 24), False),      # the general-grid instance
    (1, 2, 16, 4096, (32, 32), False),     # the headline instance
]


@pytest.mark.parametrize("cfg", CASES, ids=[str(c) for c in CASES])
def test_group_loop_writes_the_two_calls_bits(cfg, flags):
    mod, lib = _lib()
    B, H, C, N, W, dup = cfg
    keys, feat, cot, _ = make(B, H, C, N, W, seed=9, dup=dup)
    flags(mod.DEBUG_FORCE_HOT)
    assert supported(B, H, C, N, W) == 1
    assert_parity(keys, feat, cot, None, H, W, with_slice=True)


def test_the_group_behind_a_float_path_group_is_clean(flags):
    """An infinite cotangent in one channel of the SECOND of three groups: that group's accumulators hold floats; the third group's
    g_z is finite and the two calls' bits, so the clear and the third group's quanta are its own."""
    mod, lib = _lib()
    B, H, C, N, W = 1, 2, 12, 256, (8, 8)
    keys, feat, cot, _ = make(B, H, C, N, W, seed=3)
    cot[0, C + 5, 17] = float("inf")                    # plane 1, second group
    flags(mod.DEBUG_FORCE_HOT)
    o, _ = assert_parity(keys, feat, cot, None, H, W)
    assert bool(torch.isinf(o["g_z"][0, C + 5]).any())
    assert bool(torch.isfinite(o["g_z"][0, C + 8:2 * C]).all()) and int(o["g_z"][0, C + 8:2 * C].count_nonzero()) > 0


def test_all_negative_features_leave_the_counters_at_zero(flags):
    """No match and no non-zero cell in any row of any wave (and rows without a point: N = 40): no group is redone, g_feat is +0."""
    mod, lib = _lib()
    B, H, C, N, W = 1, 2, 8, 40, (8, 8)
    keys, feat, cot, _ = make(B, H, C, N, W, seed=2)
    feat = -feat.abs() - 0.1
    flags(mod.DEBUG_FORCE_HOT)
    o, z = assert_parity(keys, feat, cot, None, H, W)
    assert int(z.view(torch.int32).count_nonzero()) == 0
    assert int(o["g_feat"].view(torch.int32).count_nonzero()) == 0


def test_one_crafted_tie_in_the_last_group(flags):
    """Two points of one quad on one grid node, equal and dominant in one channel of the LAST of three groups, N < 2 G: the loop
    used the stage area for its pairs, the redo behind it stages that group over the tile area."""
    mod, lib = _lib()
    B, H, C, N, W = 1, 2, 12, 64, (8, 8)
    keys, feat, cot, _ = make(B, H, C, N, W, seed=5)
    k_node, _ = _node_key(W[0])
    p0, p1, h0, c0 = 36, 37, 1, 10
    keys[0, h0 * 2:(h0 + 1) * 2, p0] = k_node
    keys[0, h0 * 2:(h0 + 1) * 2, p1] = k_node
    feat[0, h0 * C:(h0 + 1) * C, p1] = -1.0
    feat[0, h0 * C + c0, p0] = 100.0
    feat[0, h0 * C + c0, p1] = 100.0
    flags(mod.DEBUG_FORCE_HOT)
    o, _ = assert_parity(keys, feat, cot, None, H, W)
    a0, a1 = float(o["g_feat"][0, h0 * C + c0, p0]), float(o["g_feat"][0, h0 * C + c0, p1])
    assert a0 != 0.0 and a1 == 0.0, (a0, a1)          # one winner: the lower index of the quad
