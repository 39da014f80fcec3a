"""Every kernel body of the norm kernels (csrc/ct_bnorm.hip, csrc/ct_adain.hip), one row per launch tag at the smallest shape that
reaches it, with rows on both sides of every threshold of the dispatch code.

The launch functions (bn_fwd_launch_table, bn_bwd_launch_table, the two eval launches, adain_fwd_launch_table,
adain_bwd_launch_table) name the body they picked through note(), which ct_debug_last_launch() returns.  This module is plain
data, importable without a GPU:

- tests/test_norm_families_cpu.py checks that the tags the rows name are exactly the literals passed to note() in the two
  sources (no tag is marked unreachable), and holds the bounds of tests/test_norm_families_gpu.py against an fp32 emulation of
  the kernels' algorithm and against six wrong variants of it;
- tests/test_norm_families_gpu.py runs every row on the GPU straight through the C ABI, asserts its tags and compares every
  output with a float64 reference.

The dispatch (the numbers are the sources' own):
  training BatchNorm, one workgroup of 1024 threads per channel, quads = B * N / 4:
    reg<NV>      N % 4 == 0, batch strides % 4 == 0, 16-byte aligned bases, quads <= 8192: NV = 1, 2, 4, 8 float4 per thread
                 (NV = the power of two >= ceil(quads / 1024))
    loop_vec     float4-addressable but quads > 8192
    loop_scalar  anything else (N % 4 != 0, or a base off the 16-byte grid; `vec_all` is a property of the LAUNCH)
  eval BatchNorm forward: bn_eval_vec / bn_eval_scalar by the same addressability; backward: one kernel, bn_eval_bwd
  AdaIN, one workgroup of 256 threads per (b, c) row, quads = N / 4:
    reg<NV>      N % 4 == 0, N <= 16384, aligned: NV = 1, 2, 4, 8, 16
    strided      anything else

Row fields:
  id       unique name
  entry    "bn_train"  ct_bn_group_fwd then ct_bn_group_bwd                           tags (forward, backward)
           "bn_phases" ct_bn_group_stats_fwd, _apply_fwd, _reduce_bwd, _apply_bwd     tags (forward, backward): both forward
                       phases report the first, both backward phases the second
           "bn_eval"   ct_bn_eval_group_fwd over norms of C and C + 2 channels        tags (forward,); `cut` = runs per channel
           "bn_eval_bwd" ct_bn_eval_group_bwd                                         tags (backward,)
           "adain"     ct_adain_group_fwd then ct_adain_group_bwd                     tags (forward, backward)
  B, C, N  sizes
  variant  "dense" contiguous tensors; "x_offset" x begins one float into its storage (4 bytes past a 16-byte boundary)
  tags     the expected ct_debug_last_launch() strings
  cut      bn_eval only: the runs a channel is cut into (1 = not cut)
"""
from collections import namedtuple

Row = namedtuple("Row", "id entry B C N variant tags cut")

BN_THREADS, ADAIN_THREADS = 1024, 256
BN_REG_MAX_QUADS = 8 * BN_THREADS
ADAIN_REG_MAX_N = 4 * ADAIN_THREADS * 16


def _pair(prefix, family):
    return ("%s_fwd_%s" % (prefix, family), "%s_bwd_%s" % (prefix, family))


def bn(id, B, C, N, family, variant="dense", entry="bn_train"):
    return Row(id, entry, B, C, N, variant, _pair("bn", family), 1)


def adain(id, B, C, N, family, variant="dense"):
    return Row(id, "adain", B, C, N, variant, _pair("adain", family), 1)


ROWS = [
    # ---- training BatchNorm: both sides of 1024 / 2048 / 4096 / 8192 quads ----
    bn("bn_reg1_one_quad", 1, 3, 4, "reg1"),
    bn("bn_reg1_1024_quads", 1, 4, 4096, "reg1"),
    bn("bn_reg2_1025_quads", 1, 5, 4100, "reg2"),
    bn("bn_reg2_2048_quads", 2, 3, 4096, "reg2"),
    bn("bn_reg4_2049_quads", 1, 4, 8196, "reg4"),
    bn("bn_reg4_4096_quads", 4, 3, 4096, "reg4"),
    bn("bn_reg8_4097_quads", 1, 5, 16388, "reg8"),
    bn("bn_reg8_8192_quads", 8, 3, 4096, "reg8"),
    bn("bn_loop_vec_8194_quads", 2, 4, 16388, "loop_vec"),
    bn("bn_loop_scalar_n1001", 3, 5, 1001, "loop_scalar"),
    bn("bn_loop_scalar_two_clouds_of_one", 2, 3, 1, "loop_scalar"),          # M = 2
    bn("bn_loop_scalar_one_cloud_of_two", 1, 4, 2, "loop_scalar"),           # M = 2
    bn("bn_loop_scalar_x_offset", 1, 3, 1024, "loop_scalar", variant="x_offset"),
    # ---- the four exchange phases: the same two launch functions ----
    bn("phases_reg", 2, 3, 1024, "reg1", entry="bn_phases"),
    bn("phases_loop_vec", 2, 4, 16388, "loop_vec", entry="bn_phases"),
    bn("phases_loop_scalar", 3, 5, 1001, "loop_scalar", entry="bn_phases"),
    # ---- eval BatchNorm (the cut cases are tests/test_bn_eval_gpu.py's CUT_CASES at 3 + 5 channels) ----
    Row("eval_vec_uncut", "bn_eval", 2, 3, 256, "dense", ("bn_eval_vec",), 1),
    Row("eval_vec_cut", "bn_eval", 3, 3, 5468, "dense", ("bn_eval_vec",), 2),
    Row("eval_scalar_uncut", "bn_eval", 3, 3, 101, "dense", ("bn_eval_scalar",), 1),
    Row("eval_scalar_cut", "bn_eval", 3, 3, 2731, "dense", ("bn_eval_scalar",), 4),
    Row("eval_bwd_vec", "bn_eval_bwd", 2, 4, 512, "dense", ("bn_eval_bwd",), 1),
    Row("eval_bwd_scalar", "bn_eval_bwd", 3, 5, 1001, "dense", ("bn_eval_bwd",), 1),
    # ---- AdaIN: both sides of 256 / 512 / 1024 / 2048 quads a row, the end of the register path, rows off the float4 grid ----
    adain("adain_reg1_n4", 3, 4, 4, "reg1"),
    adain("adain_reg1_n1024", 2, 5, 1024, "reg1"),
    adain("adain_reg2_n1028", 2, 3, 1028, "reg2"),
    adain("adain_reg2_n2048", 2, 4, 2048, "reg2"),
    adain("adain_reg4_n2052", 2, 3, 2052, "reg4"),
    adain("adain_reg4_n4096", 2, 3, 4096, "reg4"),
    adain("adain_reg8_n4100", 2, 3, 4100, "reg8"),
    adain("adain_reg8_n8192", 1, 4, 8192, "reg8"),
    adain("adain_reg16_n8196", 1, 3, 8196, "reg16"),
    adain("adain_reg16_n16384", 1, 3, 16384, "reg16"),
    adain("adain_strided_too_long", 1, 3, 16388, "strided"),
    adain("adain_strided_n1001", 2, 5, 1001, "strided"),
    adain("adain_strided_n1", 2, 5, 1, "strided"),                           # forward only: xhat = 0
    adain("adain_strided_x_offset", 2, 3, 1024, "strided", variant="x_offset"),
]

# the multi-rank emulation on one GPU (no process group): clouds per rank, N, and the family every rank's phases report
Ranks = namedtuple("Ranks", "id Bs C N families")
RANKS = [
    Ranks("world1", (2,), 3, 1024, ("reg1",)),
    Ranks("world2_reg", (1, 3), 4, 1024, ("reg1", "reg1")),
    Ranks("world3_reg", (2, 1, 5), 3, 1024, ("reg1", "reg1", "reg2")),
    Ranks("world3_scalar", (1, 4, 2), 5, 1001, ("loop_scalar",) * 3),
    Ranks("world2_two_values", (1, 1), 3, 2, ("loop_scalar",) * 2),
    Ranks("world2_loop_vec_on_second", (1, 3), 3, 16388, ("reg8", "loop_vec")),   # 4097 quads in registers, 12291 past them
]

# one row per kernel body for the exact-integer mask check and the rows of the slice / table checks
MASK_ROWS = ("bn_reg1_1024_quads", "bn_reg2_1025_quads", "bn_reg4_2049_quads", "bn_reg8_4097_quads", "bn_loop_vec_8194_quads",
             "bn_loop_scalar_n1001")
SLICE_ROWS = ("bn_reg2_1025_quads", "bn_loop_vec_8194_quads", "bn_loop_scalar_n1001")
TABLE_ROWS = SLICE_ROWS
ADAIN_SLICE_ROWS = ("adain_reg2_n1028", "adain_strided_n1001")
ADAIN_MASK_ROWS = ADAIN_SLICE_ROWS


def by_id(id):
    return next(r for r in ROWS if r.id == id)


def rows(entry):
    return [r for r in ROWS if r.entry == entry]


def covered_tags():
    """every note() literal the rows name"""
    out = set()
    for r in ROWS:
        out.update(r.tags)
    return out


def bn_family(B, N, aligned=True):
    """the body bn_*_launch_table picks for one aligned (or not) contiguous norm, restated from the dispatch code"""
    quads = B * (N // 4)
    if N % 4 or not aligned:
        return "loop_scalar"
    if quads > BN_REG_MAX_QUADS:
        return "loop_vec"
    per, nv = -(-quads // BN_THREADS), 1
    while nv < per:
        nv *= 2
    return "reg%d" % nv


def adain_family(N, aligned=True):
    if N % 4 or not aligned or N > ADAIN_REG_MAX_N:
        return "strided"
    per, nv = -(-(N // 4) // ADAIN_THREADS), 1
    while nv < per:
        nv *= 2
    return "reg%d" % nv
