"""Every kernel family of the grouped convolution (csrc/ct_gconv.hip), one row per launch tag and variant.

The host planner in the second half of csrc/ct_gconv.hip (plan_fwd -> FwdPlan for ct_gconv_fwd / ct_gconv_fwd_norm /
ct_gconv_bwd_data, wrw_candidate -> WrwCand for ct_gconv_bwd_weight) picks the kernels from the channel counts per group, the row
length modulo 4 / 8 / 16, the volume and the batch (how many workgroups exist), four LDS budgets, 16-byte alignment of
x / y / g_y / w, the workspace and the ct_debug_set_gconv bits; the one launch function of the family it settles on names itself
through note(), which ct_debug_last_launch() returns: one tag per kernel, followed by the tags of the host-side choices that change its code
path, all joined with '+'.  This module is plain data, importable without a GPU:

- tests/test_gconv_families_cpu.py checks that the tags the rows name (plus UNREACHABLE) are exactly the literals passed to note()
  in csrc/ct_gconv.hip, so a new family cannot come without a row and a removed one cannot leave a stale row;
- tests/test_gconv_families_gpu.py runs every row on the GPU straight through the C ABI, asserts its tag and return code and
  compares its outputs with a float64 reference.

The tags:
  bwd_data             prefix of every ct_gconv_bwd_data call: the forward kernels with the bank read transposed and flipped
  dense2d / dense3d    2^d volumes, gconv_tiny_kernel
  c4_mfma3             four-channel 3D groups on the matrix cores, gconv_c4_mfma3_kernel
  c4_valu              four-channel groups on the vector ALU, gconv_c4_kernel
  ksplit_{one,tiled}_{dma,elem}   gconv_fwd4k_kernel: pass 0 (one tile covers the volume) or pass 1 (tiled); bank slices staged by
                       LDS-DMA or element-wise;  + ksplit_items{1,2,4} (the MAXI template variant: items a wave keeps in registers)
                       + ksplit_msplit (several workgroups share a tile and split its 16-row output blocks)
  quad_256 / quad_1024 gconv_fwd4_kernel at 256 or 1024 threads;  + quad_msplit
  onepos               gconv_fwd_kernel (any row length, any alignment);  + onepos_msplit
  wrw_small_mfma_ksplit + wrw_reduce   small-volume weight gradient on the matrix cores, batch split over workgroups through the workspace
  wrw_small_mfma       ... one workgroup per channel block (ksplit == 1, or no workspace)
  wrw_small_valu       small-volume weight gradient on the vector ALU
  wrw_c4_mfma3 + wrw_c4_reduce         four-channel 3D weight gradient on the matrix cores
  wrw_c4_ring + wrw_c4_reduce          four-channel ring kernel (vector-ALU engine)
  wrw_ring_ws + wrw_reduce             16-channel ring kernel, chunk sums through the workspace
  wrw_ring_atomics     16-channel ring kernel, float atomics into g_w
  wrw_tiles            tile kernel (rows off the 16-byte grid), float atomics
  bias_grad            the separate bias-gradient kernel (the ring / small-volume kernels with a workspace produce g_bias themselves)

What has no tag of its own: the ring kernels (wrw_ring_*, wrw_c4_ring) stage x / g_y by 16-byte or by 4-byte LDS-DMA pieces after
a flag the KERNEL computes from the pointers (`vec`), not the host planner; the rows with x or g_y offset (wrw_c4_x_offset,
wrw_c4_g_y_offset, wrw_ring_x_offset) run the 4-byte staging under the same tag.  Likewise the halo staging of the one-position form.

Row fields:
  api      ct_gconv_fwd / ct_gconv_bwd_data / ct_gconv_bwd_weight
  B, G, Cin, Cout, W   sizes (channels per group; dim = len(W))
  bias     pass bias (forward) / g_bias (weight gradient); ignored by backward-data
  ws       weight gradient only: "query" = the workspace ct_gconv_bwd_weight_workspace_bytes asks for (NULL where it asks for none),
           None = NULL, "short" = half of what it asks for
  offset4  names among x, w, y, g_y, g_x passed as views 4 bytes past a 16-byte boundary
  flags    the ct_debug_set_gconv value
  tag      the expected ct_debug_last_launch() string, exactly
  rc       the expected return code
"""
from collections import namedtuple

CT_OK, CT_EINVAL, CT_EWORKSPACE = 0, -1, -3
# ct_debug_set_gconv bits (include/cloudct.h)
WRW_VALU, C4_NO_MFMA, C4_FORCE_MFMA = 1, 2, 4


def ksplit_from(cin):
    """bits 8..15: input channels per group from which forward / backward-data take the K-split kernel"""
    return cin << 8


Row = namedtuple("Row", "id api B G Cin Cout W bias ws offset4 flags tag rc")
FWD, BWD, WRW = "ct_gconv_fwd", "ct_gconv_bwd_data", "ct_gconv_bwd_weight"


def row(id, api, tag, B, G, Cin, Cout, W, bias=True, ws="query", offset4=(), flags=0, rc=CT_OK):
    return Row(id, api, B, G, Cin, Cout, tuple(W), bias, ws if api == WRW else None, tuple(offset4), flags, tag, rc)


NOPLAN = (2, 2, 38, 22, (6, 10, 64))      # ct_gconv_supported == 0: the one-position form has no tile plan
NOPLAN_WRW = (1, 1, 3, 3, (2, 1001))      # ct_gconv_supported == 0: the weight gradient has no plan (no ring: W % 4 != 0; no tile of 16
                                          # planes of three 1001-float rows fits LDS); not a row: only its return code is checked

ROWS = [
    # ---- dense 2^d (plan_dense: cob = 64 / B output channels per workgroup, at least 4, at most Cout) ----
    row("dense3d_ragged_channels", FWD, "dense3d", 2, 3, 40, 24, (2, 2, 2), bias=False),
    row("dense3d_cout_not_multiple_of_cob", FWD, "dense3d", 2, 3, 24, 40, (2, 2, 2)),                 # cob 32: blocks of 32 + 8
    row("dense2d", FWD, "dense2d", 3, 2, 5, 7, (2, 2)),
    row("dense3d_b70", FWD, "dense3d", 70, 1, 8, 6, (2, 2, 2)),                                        # cob 4: blocks of 4 + 2
    row("dense3d_bwd", BWD, "bwd_data+dense3d", 2, 3, 40, 24, (2, 2, 2)),
    row("dense2d_bwd", BWD, "bwd_data+dense2d", 3, 2, 5, 7, (2, 2)),
    row("dense2d_y_offset_refused", FWD, "onepos", 3, 2, 5, 7, (2, 2), offset4=("y",)),
    # ---- four-channel 3D groups on the matrix cores ----
    row("c4_mfma3_by_size", FWD, "c4_mfma3", 4, 16, 4, 4, (32, 32, 32)),                               # 2 M positions: the threshold
    row("c4_mfma3_below_size", FWD, "c4_valu", 1, 3, 4, 4, (5, 7, 16)),
    row("c4_mfma3_ragged_5x7x16", FWD, "c4_mfma3", 1, 3, 4, 4, (5, 7, 16), flags=C4_FORCE_MFMA),
    row("c4_mfma3_ragged_9x33x48", FWD, "c4_mfma3", 2, 2, 4, 4, (9, 33, 48), bias=False, flags=C4_FORCE_MFMA),
    row("c4_mfma3_depth_segments", FWD, "c4_mfma3", 1, 2, 4, 4, (16, 8, 16), flags=C4_FORCE_MFMA),   # nZ = 4 segments of 4 slices
    row("c4_mfma3_suppressed", FWD, "c4_valu", 1, 3, 4, 4, (5, 7, 16), flags=C4_NO_MFMA | C4_FORCE_MFMA),   # "never" wins over "always"
    row("c4_mfma3_bwd_suppressed", BWD, "bwd_data+c4_valu", 1, 3, 4, 4, (5, 7, 16), flags=C4_NO_MFMA | C4_FORCE_MFMA),
    row("c4_mfma3_bwd", BWD, "bwd_data+c4_mfma3", 1, 3, 4, 4, (5, 7, 16), flags=C4_FORCE_MFMA),
    # ---- four-channel groups on the vector ALU ----
    row("c4_valu_16sq", FWD, "c4_valu", 2, 4, 4, 4, (16, 16)),
    row("c4_valu_128sq_tiles", FWD, "c4_valu", 1, 2, 4, 4, (128, 128)),                                # TH 14: ten tiles, the last of 2 rows
    row("c4_valu_8cube", FWD, "c4_valu", 2, 2, 4, 4, (8, 8, 8), bias=False),
    row("c4_valu_rows12", FWD, "c4_valu", 1, 2, 4, 4, (7, 12)),
    row("c4_valu_ragged_tile", FWD, "c4_valu", 1, 1, 4, 4, (100, 64)),                                 # TH 30: 30 + 30 + 30 + 10
    row("c4_valu_3d_ragged_tile", FWD, "c4_valu", 1, 2, 4, 4, (5, 37, 12)),
    row("c4_valu_bwd", BWD, "bwd_data+c4_valu", 2, 2, 4, 4, (8, 8, 8)),
    # ---- K-split (>= 32 input channels per group) ----
    row("ksplit_one_64_8cube", FWD, "ksplit_one_dma+ksplit_items1+ksplit_msplit", 1, 2, 64, 64, (8, 8, 8)),
    row("ksplit_one_no_msplit", FWD, "ksplit_one_dma+ksplit_items1", 1, 2, 64, 64, (4, 4, 4), bias=False),
    row("ksplit_tiled_16cube", FWD, "ksplit_tiled_dma+ksplit_items1+ksplit_msplit", 1, 2, 64, 64, (16, 16, 16)),
    row("ksplit_elem_48_40", FWD, "ksplit_one_elem+ksplit_items1+ksplit_msplit", 3, 2, 48, 40, (4, 8, 8)),
    row("ksplit_elem_w_offset", FWD, "ksplit_one_elem+ksplit_items1+ksplit_msplit", 1, 2, 64, 64, (8, 8, 8), offset4=("w",)),
    row("ksplit_items2", FWD, "ksplit_one_dma+ksplit_items2", 1, 2, 32, 16, (40, 32)),
    row("ksplit_items4_tiled", FWD, "ksplit_tiled_dma+ksplit_items4+ksplit_msplit", 1, 1, 64, 64, (64, 64), bias=False),
    row("ksplit_threshold_cin20", FWD, "ksplit_one_elem+ksplit_items1", 1, 2, 20, 24, (8, 8), flags=ksplit_from(20)),
    row("ksplit_threshold_default", FWD, "quad_256+quad_msplit", 1, 2, 20, 24, (8, 8)),
    row("ksplit_bwd_elem", BWD, "bwd_data+ksplit_one_elem+ksplit_items1+ksplit_msplit", 3, 2, 48, 40, (4, 8, 8)),
    row("ksplit_bwd_tiled", BWD, "bwd_data+ksplit_tiled_dma+ksplit_items1+ksplit_msplit", 1, 2, 64, 64, (16, 16, 16)),
    row("ksplit_bwd_items2", BWD, "bwd_data+ksplit_one_dma+ksplit_items2", 1, 2, 16, 32, (40, 32)),
    # ---- quad ----
    row("quad_16_32sq", FWD, "quad_256", 2, 3, 16, 16, (32, 32)),
    row("quad_msplit_16_48", FWD, "quad_256+quad_msplit", 1, 3, 16, 48, (8, 8)),
    row("quad_1024_threads", FWD, "quad_1024", 1, 2, 16, 16, (8, 256), bias=False),                   # rows of 256: no tile under 48 KiB
    row("quad_ragged_th", FWD, "quad_256", 1, 1, 16, 16, (101, 32)),                                   # 101 rows: no tile height divides them
    row("quad_3d_depth_tiles", FWD, "quad_1024", 1, 2, 16, 16, (16, 16, 16)),
    row("quad_w_offset", FWD, "quad_256", 2, 3, 16, 16, (32, 32), offset4=("w",)),
    row("quad_bwd", BWD, "bwd_data+quad_256", 2, 3, 16, 16, (32, 32)),
    row("quad_bwd_widening", BWD, "bwd_data+quad_256+quad_msplit", 1, 3, 48, 16, (8, 8)),
    # ---- one-position ----
    row("onepos_5_7_9x11", FWD, "onepos", 1, 1, 5, 7, (9, 11)),
    row("onepos_3d_6x5x7", FWD, "onepos", 1, 2, 5, 7, (6, 5, 7), bias=False),
    row("onepos_row18", FWD, "onepos", 1, 2, 8, 8, (9, 18)),                                            # W >= 16: the depth-first tile policy
    row("onepos_x_offset", FWD, "onepos", 2, 3, 16, 16, (32, 32), offset4=("x",)),
    row("onepos_msplit", FWD, "onepos+onepos_msplit", 1, 1, 5, 40, (9, 11)),
    row("onepos_bwd", BWD, "bwd_data+onepos", 1, 1, 5, 7, (9, 11)),
    row("onepos_bwd_g_x_offset", BWD, "bwd_data+onepos", 2, 3, 16, 16, (32, 32), offset4=("g_x",)),
    # ---- weight gradient: small volumes on the matrix cores ----
    row("wrw_mfma_ksplit", WRW, "wrw_small_mfma_ksplit+wrw_reduce", 2, 2, 64, 64, (8, 8, 8)),
    row("wrw_mfma_no_workspace", WRW, "wrw_small_mfma", 2, 2, 64, 64, (8, 8, 8), ws=None),
    row("wrw_mfma_ksplit1", WRW, "wrw_small_mfma", 1, 2, 64, 64, (4, 4, 4)),                            # B 1: nothing to split
    row("wrw_mfma_tz_lt_d", WRW, "wrw_small_mfma_ksplit+wrw_reduce", 2, 1, 32, 32, (8, 4, 16)),       # 10 x 4 x 4 staging units > 128
    row("wrw_mfma_2d_rows8", WRW, "wrw_small_mfma_ksplit+wrw_reduce", 2, 3, 32, 64, (8, 8), bias=False),
    row("wrw_mfma_2d_rows4", WRW, "wrw_small_mfma_ksplit+wrw_reduce", 5, 2, 64, 32, (4, 4)),
    row("wrw_mfma_3d_rows16", WRW, "wrw_small_mfma_ksplit+wrw_reduce", 2, 1, 32, 32, (4, 8, 16)),
    row("wrw_mfma_ragged_blocks", WRW, "wrw_small_mfma_ksplit+wrw_reduce", 3, 5, 48, 40, (4, 8, 8)),
    # ---- weight gradient: small volumes on the vector ALU ----
    row("wrw_valu_flag", WRW, "wrw_small_valu", 2, 2, 64, 64, (8, 8, 8), flags=WRW_VALU),
    row("wrw_valu_rows2", WRW, "wrw_small_valu", 2, 3, 40, 24, (2, 2, 2), ws=None),           # rows of 2: no workspace form
    row("wrw_valu_g_y_offset", WRW, "wrw_small_valu", 2, 2, 64, 64, (8, 8, 8), offset4=("g_y",)),
    # ---- weight gradient: four-channel groups ----
    row("wrw_c4_mfma3", WRW, "wrw_c4_mfma3+wrw_c4_reduce", 1, 3, 4, 4, (5, 7, 16)),
    row("wrw_c4_mfma3_suppressed", WRW, "wrw_c4_ring+wrw_c4_reduce", 1, 3, 4, 4, (5, 7, 16), flags=C4_NO_MFMA),
    row("wrw_c4_ring_2d", WRW, "wrw_c4_ring+wrw_c4_reduce", 1, 2, 4, 4, (16, 16)),
    row("wrw_c4_ring_3d_rows12", WRW, "wrw_c4_ring+wrw_c4_reduce", 1, 2, 4, 4, (5, 6, 12), bias=False),
    row("wrw_c4_no_workspace", WRW, "wrw_ring_atomics+bias_grad", 1, 2, 4, 4, (16, 16), ws=None),
    row("wrw_c4_x_offset", WRW, "wrw_c4_ring+wrw_c4_reduce", 1, 2, 4, 4, (16, 16), offset4=("x",)),
    row("wrw_c4_g_y_offset", WRW, "wrw_c4_ring+wrw_c4_reduce", 1, 2, 4, 4, (16, 16), offset4=("g_y",)),
    row("wrw_c4_3d_g_y_offset", WRW, "wrw_c4_ring+wrw_c4_reduce", 1, 2, 4, 4, (8, 8, 8), offset4=("g_y",)),   # aligned: wrw_c4_mfma3
    # ---- weight gradient: 16-channel ring ----
    row("wrw_ring_one_chunk", WRW, "wrw_ring_ws+wrw_reduce", 1, 2, 16, 16, (16, 16)),
    row("wrw_ring_many_chunks", WRW, "wrw_ring_ws+wrw_reduce", 2, 2, 16, 16, (8, 16, 16)),
    row("wrw_ring_ragged_blocks", WRW, "wrw_ring_ws+wrw_reduce", 2, 3, 20, 12, (12, 20), bias=False),
    row("wrw_ring_atomics", WRW, "wrw_ring_atomics+bias_grad", 2, 3, 16, 16, (32, 32), ws=None),
    row("wrw_ring_atomics_no_bias", WRW, "wrw_ring_atomics", 2, 3, 16, 16, (32, 32), ws=None, bias=False),
    row("wrw_ring_x_offset", WRW, "wrw_ring_ws+wrw_reduce", 2, 3, 16, 16, (32, 32), offset4=("x",)),
    row("wrw_ring_short_workspace", WRW, "", 2, 3, 16, 16, (32, 32), ws="short", rc=CT_EWORKSPACE),
    # ---- weight gradient: tiles ----
    row("wrw_tiles_rows9", WRW, "wrw_tiles+bias_grad", 1, 1, 5, 7, (9, 9), ws=None),
    row("wrw_tiles_3d", WRW, "wrw_tiles", 2, 2, 5, 7, (6, 5, 7), bias=False, ws=None),
    # ---- the shape ct_gconv_supported refuses: aligned tensors still find a plan on the K-split / quad / ring kernels; tensors off
    # the 16-byte grid need the one-position form, whose filter bank and halo tile do not fit LDS ----
    row("noplan_fwd_aligned", FWD, "ksplit_tiled_elem+ksplit_items1+ksplit_msplit", *NOPLAN),
    row("noplan_fwd_x_offset", FWD, "", *NOPLAN, offset4=("x",), rc=CT_EINVAL),
    row("noplan_bwd_aligned", BWD, "bwd_data+quad_1024+quad_msplit", *NOPLAN),
    row("noplan_bwd_g_y_offset", BWD, "bwd_data+onepos+onepos_msplit", *NOPLAN, offset4=("g_y",)),
    row("noplan_wrw", WRW, "wrw_ring_ws+wrw_reduce", *NOPLAN),
]

# tags no legal call reaches, with the reason from the planner's code
UNREACHABLE = {}

# rows whose call accumulates with float atomics (order not fixed): held to the bounds, not to bitwise reproducibility
ATOMICS_TAGS = ("wrw_ring_atomics", "wrw_tiles")


def covered_tags():
    """every note() literal the rows name, plus UNREACHABLE's"""
    out = set(UNREACHABLE)
    for r in ROWS:
        out.update(t for t in r.tag.split("+") if t)
    return out


def shapes():
    """the distinct (B, G, Cin, Cout, W) of the table, in table order"""
    seen = []
    for r in ROWS:
        s = (r.B, r.G, r.Cin, r.Cout, r.W)
        if s not in seen:
            seen.append(s)
    return seen
