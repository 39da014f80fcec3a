"""Every kernel family of Splat / Slice (csrc/ct_raster.hip and the ct_raster_*.h headers), one row per launch tag.

A host-side planner picks the kernels of each Splat / Slice call from the shape, the (b,h) plane count, N % 4, 16-byte pointer
alignment, the padding dtype, the LDS budget and the CT_DEBUG_* flags; each family names itself through note(), which
ct_debug_last_launch() returns ("+"-joined when a call launches several).  This module is plain data, importable without a GPU:

- tests/test_raster_families_cpu.py checks that the tags the rows name (plus UNREACHABLE) are exactly the literals passed to note()
  in csrc/ct_raster.hip, so a new family cannot come without a case and a removed one cannot leave a stale row;
- tests/test_raster_families_gpu.py runs every row on the GPU, asserts its tag and compares its outputs with a float64 reference.

Row fields:
  api      the C entry point, called straight through the ABI: ct_splat_fwd / ct_splat_bwd / ct_splat_bwd_ex / ct_splat_bwd_tk /
           ct_slice_fwd / ct_slice_bwd / ct_slice_bwd_ws / ct_slice_bwd_tk / ct_slice_bwd_ps (keys form: corners from the keys)
           or ct_splat_lc_fwd / ct_splat_lc_bwd / ct_slice_lc_fwd / ct_slice_lc_bwd (lc form: explicit local_coord / flat_idx)
  reduce   "max" / "sum" for Splat, None for Slice
  ws       pass the workspace the library asks for (ct_*_workspace_bytes under the row's flags), else NULL / 0
  tickets  pass a zeroed CT_TICKETS_BYTES arrival-ticket buffer (ct_*_tk / ct_slice_bwd_ps)
  B, H, C, N, W   sizes (dim = len(W))
  pad      None, "f32" or "i32" (the (B,N) padding mask's dtype)
  offset4  names of the tensors passed as views 4 bytes past a 16-byte boundary (empty: everything aligned)
  flags    the ct_debug_set_flags value;  nseg: the ct_debug_set_nseg value (0: automatic)
  accumulate  ct_splat_bwd_ex with CT_BWD_ACCUMULATE_KEYS (g_keys += result)
  keys_add    ct_splat_bwd_tk with a separate incoming key cotangent (g_keys = g_keys_add + result)
  tag      the expected ct_debug_last_launch() string of the call, exactly
  setup_tag   the tag of a preparatory call (ct_plane_sort for the presorted rows), or None
"""
from collections import namedtuple

# mirrors of include/cloudct.h's CT_DEBUG_* bits (tests/test_abi_cpu.py pins _lib's copies against the header)
NO_HOT, FORCE_HOT, NO_BAND, FORCE_BAND = 1, 2, 4, 8
NO_SORTED, FORCE_SORTED, FORCE_SORTED_SEG, NO_WIDE = 16, 32, 64, 128

Row = namedtuple("Row", "id api reduce ws tickets B H C N W pad offset4 flags nseg accumulate keys_add tag setup_tag")


def row(id, api, tag, B, H, C, N, W, reduce=None, ws=False, tickets=False, pad=None, offset4=(), flags=0, nseg=0,
        accumulate=False, keys_add=False, setup_tag=None):
    return Row(id, api, reduce, ws, tickets, B, H, C, N, tuple(W), pad, tuple(offset4), flags, nseg, accumulate, keys_add, tag,
               setup_tag)


def entry(r):
    """'splat_fwd' / 'splat_bwd' / 'slice_fwd' / 'slice_bwd'"""
    return r.api.replace("_lc", "")[3:12]


def lc_form(r):
    return "_lc_" in r.api


S32, S16, S64, S256 = (32, 32), (16, 16), (64, 64), (256, 256)
C8, C16, C36 = (8, 8, 8), (16, 16, 16), (36, 36, 36)

ROWS = [
    # ---- Splat forward (run_scatter) ----
    row("splat_max_quad", "ct_splat_fwd", "scatter_quad_max", 2, 2, 8, 1024, S32, reduce="max", pad="f32"),
    row("splat_max_generic_lc", "ct_splat_lc_fwd", "scatter_generic_max", 1, 2, 6, 999, (10, 12), reduce="max", pad="i32"),
    row("splat_max_global_256sq", "ct_splat_fwd", "scatter_global_atomics", 1, 1, 3, 2048, S256, reduce="max", pad="f32"),
    row("splat_sum_global_36cube", "ct_splat_fwd", "scatter_global_atomics", 1, 1, 3, 1024, C36, reduce="sum"),
    row("splat_sum_fx_reg", "ct_splat_fwd", "scatter_add_fx_reg", 1, 2, 8, 1024, S16, reduce="sum", pad="f32", flags=NO_HOT),
    row("splat_sum_fx_unaligned", "ct_splat_fwd", "scatter_add_fx", 1, 2, 8, 1024, S32, reduce="sum",
        offset4=("keys", "feat", "z")),
    row("splat_sum_sorted", "ct_splat_fwd", "scatter_add_sorted", 1, 2, 8, 1024, S32, reduce="sum",
        flags=FORCE_SORTED | FORCE_HOT),
    row("splat_sum_fused", "ct_splat_fwd", "scatter_add_fused", 1, 2, 8, 1024, S32, reduce="sum", pad="i32",
        flags=FORCE_HOT | NO_SORTED),
    row("splat_sum_sorted3", "ct_splat_fwd", "scatter_add_sorted3", 1, 2, 8, 1024, C8, reduce="sum", flags=FORCE_SORTED | FORCE_HOT),

    # ---- Slice forward (run_gather) ----
    row("slice_fwd_ci", "ct_slice_fwd", "gather_ci", 1, 2, 8, 1024, S32, pad="f32", flags=FORCE_HOT),
    row("slice_fwd_ci3", "ct_slice_fwd", "gather_ci3", 1, 2, 8, 1024, C8, pad="i32", flags=FORCE_HOT),
    row("slice_fwd_quad", "ct_slice_fwd", "gather_quad", 1, 2, 8, 1024, S32, flags=NO_HOT),
    row("slice_fwd_generic_lc", "ct_slice_lc_fwd", "gather_generic", 1, 2, 5, 777, (10, 12), pad="i32"),
    row("slice_fwd_global_256sq", "ct_slice_fwd", "gather_generic", 1, 1, 3, 2048, S256, pad="f32"),

    # ---- Splat(sum) backward ----
    row("splat_sum_bwd_hot", "ct_splat_bwd", "splat_sum_bwd_hot", 1, 2, 8, 1024, S32, reduce="sum", pad="f32", flags=FORCE_HOT),
    row("splat_sum_bwd_quad", "ct_splat_bwd", "gather_quad+gather_gw_quad", 1, 2, 8, 1024, S32, reduce="sum", flags=NO_HOT),
    row("splat_sum_bwd_generic_lc3", "ct_splat_lc_bwd", "gather_generic+gather_gw_generic", 1, 2, 6, 500, (6, 6, 5),
        reduce="sum", pad="i32"),
    row("splat_sum_bwd_global_256sq", "ct_splat_bwd", "gather_generic+gather_gw_generic", 1, 1, 3, 2048, S256, reduce="sum"),
    row("splat_sum_bwd_accumulate", "ct_splat_bwd_ex", "gather_quad+gather_gw_quad+add_inplace", 1, 2, 8, 1024, S32,
        reduce="sum", ws=True, flags=NO_HOT, accumulate=True),

    # ---- Splat(max) backward ----
    row("splat_max_bwd_hot", "ct_splat_bwd", "splat_max_bwd_hot", 1, 2, 4, 1024, S32, reduce="max", ws=True, pad="f32",
        flags=FORCE_HOT),
    row("splat_max_bwd_hot_groups", "ct_splat_bwd", "splat_max_bwd_hot_groups", 1, 2, 8, 1024, S32, reduce="max", ws=True,
        flags=FORCE_HOT),
    row("splat_max_bwd_hot_segments", "ct_splat_bwd_tk", "splat_max_bwd_hot_segments", 1, 2, 4, 2048, S16, reduce="max",
        ws=True, tickets=True, pad="i32", flags=FORCE_HOT, nseg=2, keys_add=True),
    row("splat_max_bwd_hot3", "ct_splat_bwd", "splat_max_bwd_hot3", 1, 2, 4, 1024, C8, reduce="max", ws=True, flags=FORCE_HOT),
    row("splat_max_bwd_hot3_groups", "ct_splat_bwd_tk", "splat_max_bwd_hot3_groups+folded", 1, 2, 8, 1024, C8, reduce="max",
        ws=True, tickets=True, pad="f32", flags=FORCE_HOT),
    row("splat_max_bwd_hot3_segments", "ct_splat_bwd_tk", "splat_max_bwd_hot3_segments", 1, 2, 4, 2048, C8, reduce="max",
        ws=True, tickets=True, flags=FORCE_HOT, nseg=2, keys_add=True),
    row("splat_max_bwd_band", "ct_splat_bwd", "band_splat_bwd", 1, 2, 4, 1024, S32, reduce="max", pad="f32", flags=FORCE_BAND),
    row("splat_max_bwd_band3_36cube", "ct_splat_bwd", "band_splat_bwd3", 1, 1, 4, 2048, C36, reduce="max"),
    row("splat_max_bwd_global_256sq", "ct_splat_bwd", "splat_max_bwd_global", 1, 1, 3, 2048, S256, reduce="max", ws=True,
        pad="i32"),
    row("splat_max_bwd_global_36cube", "ct_splat_bwd", "splat_max_bwd_global", 1, 1, 2, 1024, C36, reduce="max", ws=True),
    row("splat_max_bwd_whole_head", "ct_splat_bwd", "splat_max_bwd_whole_head", 16, 16, 12, 256, S32, reduce="max", ws=True,
        flags=NO_HOT),
    row("splat_max_bwd_quad", "ct_splat_bwd", "splat_max_bwd_quad", 1, 2, 8, 1024, S32, reduce="max", ws=True, pad="i32",
        flags=NO_HOT),
    row("splat_max_bwd_generic_lc", "ct_splat_lc_bwd", "splat_max_bwd_generic", 1, 2, 6, 999, (10, 12), reduce="max", ws=True,
        pad="f32"),

    # ---- Slice backward: two-kernel form (gather + statistics, then the fixed-point scatter) ----
    row("slice_bwd_gw_stats", "ct_slice_bwd", "slice_bwd_gw_stats+scatter_quad_add", 1, 2, 8, 512, S32, pad="f32", flags=NO_HOT),
    row("slice_bwd_gw_stats_parts", "ct_slice_bwd_ws", "slice_bwd_gw_stats_parts+scatter_quad_add", 1, 2, 8, 2048, S32,
        ws=True, flags=NO_HOT),
    row("slice_bwd_gw_stats_nsplit", "ct_slice_bwd", "slice_bwd_gw_stats_nsplit+scatter_quad_add", 1, 2, 8, 2048, S32,
        pad="i32", flags=NO_HOT),
    row("slice_bwd_fx_stream", "ct_slice_bwd_ws", "slice_bwd_gw_stats_parts+scatter_add_fx_stream", 1, 2, 8, 2048, S32,
        ws=True, offset4=("g_grid",)),
    # ---- Slice backward: the generic pair (scatter-add, then gather of g_keys) ----
    row("slice_bwd_pair_fx_reg", "ct_slice_bwd", "scatter_add_fx_reg+gather_gw_generic", 1, 2, 8, 1024, S32,
        offset4=("g_keys",)),
    row("slice_bwd_pair_lc", "ct_slice_lc_bwd", "scatter_add_fx+gather_gw_generic", 1, 2, 6, 777, (10, 12), pad="f32"),
    row("slice_bwd_global_256sq", "ct_slice_bwd", "scatter_global_atomics+gather_gw_generic", 1, 1, 3, 2048, S256, pad="f32"),
    row("slice_bwd_global_36cube", "ct_slice_bwd_ws", "scatter_global_atomics+gather_gw_generic", 1, 1, 3, 1024, C36, ws=True),
    # ---- Slice backward: banded four-channel kernels ----
    row("slice_bwd_band", "ct_slice_bwd", "band_slice_bwd", 1, 2, 4, 1024, S32, pad="i32", flags=FORCE_BAND),
    row("slice_bwd_band3_36cube", "ct_slice_bwd", "band_slice_bwd3", 1, 1, 4, 2048, C36, pad="f32"),
    # ---- Slice backward: fused hot kernels ----
    row("slice_bwd_fused", "ct_slice_bwd_ws", "slice_bwd_fused", 1, 2, 4, 1024, S32, ws=True, pad="f32",
        flags=FORCE_HOT | NO_SORTED),
    row("slice_bwd_fused_groups", "ct_slice_bwd_ws", "slice_bwd_fused_groups", 1, 2, 8, 1024, S32, ws=True,
        flags=FORCE_HOT | NO_SORTED),
    row("slice_bwd_fused_segments", "ct_slice_bwd_tk", "slice_bwd_fused_segments+folded", 1, 2, 4, 8192, S16, ws=True,
        tickets=True, pad="i32", flags=FORCE_HOT | NO_SORTED),
    row("slice_bwd_fused3", "ct_slice_bwd_ws", "slice_bwd_fused3", 1, 2, 4, 1024, C8, ws=True, flags=FORCE_HOT | NO_SORTED),
    row("slice_bwd_fused3_groups", "ct_slice_bwd_ws", "slice_bwd_fused3_groups", 1, 2, 8, 1024, C8, ws=True, pad="f32",
        flags=FORCE_HOT | NO_SORTED),
    row("slice_bwd_fused3_segments", "ct_slice_bwd_ws", "slice_bwd_fused3_segments", 1, 2, 4, 8192, C8, ws=True,
        flags=FORCE_HOT | NO_SORTED),
    # ---- Slice backward: sorted planes (ct_raster_sorted.h) ----
    row("slice_bwd_sorted", "ct_slice_bwd", "slice_bwd_sorted", 1, 2, 4, 1024, S32, pad="f32", flags=FORCE_SORTED | FORCE_HOT),
    row("slice_bwd_sorted_groups", "ct_slice_bwd_ws", "slice_bwd_sorted_groups", 1, 2, 8, 1024, S32, ws=True,
        flags=FORCE_SORTED | FORCE_HOT),
    row("slice_bwd_presorted", "ct_slice_bwd_ps", "slice_bwd_presorted", 1, 2, 4, 1024, S32, ws=True,
        flags=FORCE_SORTED | FORCE_HOT, setup_tag="plane_sort"),
    row("slice_bwd_presorted_groups", "ct_slice_bwd_ps", "slice_bwd_presorted_groups", 1, 2, 8, 1024, S32, ws=True, pad="i32",
        flags=FORCE_SORTED | FORCE_HOT, setup_tag="plane_sort"),
    # ---- Slice backward: sorted segments (ct_raster_sorted3d.h; 3D, and its 2D form) ----
    row("slice_bwd_sorted3", "ct_slice_bwd", "slice_bwd_sorted3", 1, 2, 4, 1024, C8, pad="i32", flags=FORCE_SORTED | FORCE_HOT),
    row("slice_bwd_sorted3_groups", "ct_slice_bwd_ws", "slice_bwd_sorted3_groups", 1, 2, 8, 1024, C8, ws=True,
        flags=FORCE_SORTED | FORCE_HOT),
    row("slice_bwd_sorted3_segments", "ct_slice_bwd_ws", "slice_bwd_sorted3_segments", 1, 2, 4, 4096, C8, ws=True, pad="f32",
        flags=FORCE_SORTED | FORCE_HOT),
    row("slice_bwd_sorted2s", "ct_slice_bwd", "slice_bwd_sorted2s", 1, 2, 4, 1024, S16, flags=FORCE_SORTED_SEG | FORCE_HOT),
    row("slice_bwd_sorted2s_groups", "ct_slice_bwd_ws", "slice_bwd_sorted2s_groups", 1, 2, 8, 1024, S16, ws=True, pad="f32",
        flags=FORCE_SORTED_SEG | FORCE_HOT),
    row("slice_bwd_sorted2s_segments", "ct_slice_bwd_ws", "slice_bwd_sorted2s_segments", 1, 2, 4, 4096, S16, ws=True,
        flags=FORCE_SORTED_SEG | FORCE_HOT),
]

# The 1024-thread WIDE launches of the hot backward kernels (hot_wide / slice_bwd_wide_shape in csrc/ct_raster.hip): each case runs
# with FORCE_HOT (B2 x H4 is too few planes for the hot kernels by themselves) and again with FORCE_HOT | NO_WIDE.
# (id, api, reduce, B, H, C, N, W, pad, tag, tag under NO_WIDE, launch form of the wide run, both runs cut the points alike)
WideCase = namedtuple("WideCase", "id api reduce B H C N W pad tag narrow_tag form same_cut")
WIDE_CASES = [
    WideCase("slice64sq_n4096", "ct_slice_bwd_ws", None, 2, 4, 16, 4096, S64, "f32",
             "slice_bwd_fused_groups+wide", "slice_bwd_fused_groups", "QPT=1", True),
    WideCase("slice64sq_n8192", "ct_slice_bwd_ws", None, 2, 4, 16, 8192, S64, "f32",
             "slice_bwd_fused_groups+wide", "slice_bwd_fused_segments", "QPT=2, one 8192-point segment (narrow: two)", False),
    WideCase("slice16cube_n4096", "ct_slice_bwd_ws", None, 2, 4, 16, 4096, C16, None,
             "slice_bwd_fused3_groups+wide", "slice_bwd_fused3_groups", "QPT=1", True),
    WideCase("slice16cube_n16384", "ct_slice_bwd_ws", None, 2, 4, 16, 16384, C16, None,
             "slice_bwd_fused3_segments+wide", "slice_bwd_fused3_segments", "QPT=2, two segments (narrow: four)", False),
    WideCase("splat64sq_n4096", "ct_splat_bwd", "max", 2, 4, 16, 4096, S64, "f32",
             "splat_max_bwd_hot_groups+wide", "splat_max_bwd_hot_groups", "QPT=1", True),
    WideCase("splat64sq_n8192", "ct_splat_bwd", "max", 2, 4, 16, 8192, S64, "f32",
             "splat_max_bwd_hot_groups+wide", "splat_max_bwd_hot_groups", "loop (QPT=0)", True),
    WideCase("splat16cube_n4096", "ct_splat_bwd", "max", 2, 4, 16, 4096, C16, None,
             "splat_max_bwd_hot3_groups+wide", "splat_max_bwd_hot3_groups", "loop (QPT=0)", True),
    # two workgroups fit a CU here: the wide form is not taken (csrc/ct_raster.hip, the comment above wide_enabled)
    WideCase("slice8cube_c32", "ct_slice_bwd_ws", None, 2, 4, 32, 4096, C8, None,
             "slice_bwd_fused3_groups", "slice_bwd_fused3_groups", "narrow", True),
    WideCase("splat8cube_c32", "ct_splat_bwd", "max", 2, 4, 32, 4096, C8, None,
             "splat_max_bwd_hot3_groups", "splat_max_bwd_hot3_groups", "narrow", True),
]

# tags no legal call reaches, with the reason from the planner's code
UNREACHABLE = {}


def covered_tags():
    """every note() literal the rows and wide cases name, plus UNREACHABLE's"""
    out = set(UNREACHABLE)
    for r in ROWS:
        out.update(r.tag.split("+"))
        if r.setup_tag:
            out.update(r.setup_tag.split("+"))
    for w in WIDE_CASES:
        out.update(w.tag.split("+"))
        out.update(w.narrow_tag.split("+"))
    return out
