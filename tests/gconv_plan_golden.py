"""The table behind tests/test_gconv_plan_golden_cpu.py: what the grouped convolution's planner answers without a GPU, over a sweep
of shapes, recorded from a library built from the commit BEFORE a change to the planner (csrc/ct_gconv.hip) and required of the
in-tree library afterwards.

    python -m tests.gconv_plan_golden /path/to/libcloudct.so      # rewrites tests/golden/gconv_plan_queries.json

The library is opened with plain ctypes, never through the package, so that the table cannot come from the tree under test by
accident.  Regenerate it only when an answer is MEANT to change, from a build of the parent commit plus that one change.

A row is [B, groups, Cin, Cout, W, answers]; `answers` in the order of QUERIES:
  supported         ct_gconv_supported
  norm              ct_gconv_fwd_norm_supported
  covers0, covers1  ct_gconv_precision_covers, forward and backward-data
  workspace         ct_gconv_bwd_weight_workspace_bytes
  norm_k20, covers0_k20, covers1_k20   the norm and precision queries again under ct_debug_set_gconv(ksplit_from(20))
"""
import ctypes
import itertools
import json
import os
import sys

from tests import gconv_families as F

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gconv_plan_queries.json")
QUERIES = ("supported", "norm", "covers0", "covers1", "workspace", "norm_k20", "covers0_k20", "covers1_k20")

# the grouped convolutions of the three zoo models (tools/gconv_model_shapes.py, profiles/r3_gconv_model_shapes.txt: groups 16 at
# batch 8 and 2; the Res blocks of DESIGN.md §4.15 are among them) and the rows of tools/gconv_bench.py
ZOO = [(4, 4, (32, 32, 32)), (16, 16, (16, 16, 16)), (16, 16, (64, 64)), (64, 64, (8, 8, 8)), (4, 4, (128, 128)), (64, 64, (4, 4, 4)),
       (32, 64, (8, 8, 8)), (64, 64, (4, 4)), (64, 64, (2, 2, 2)), (64, 64, (8, 8)), (32, 32, (16, 16)), (32, 64, (8, 8)),
       (16, 32, (16, 16)), (16, 16, (16, 16)), (32, 32, (8, 8, 8))]
BATCHES, GROUPS, CHANNELS = (1, 2, 8, 70), (1, 3, 16), (3, 4, 5, 16, 20, 32, 48, 64)
EXTENTS = [(2, 2), (4, 4), (5, 9), (8, 8), (9, 12), (16, 16), (12, 18), (32, 32), (64, 64), (128, 128), (8, 256), (256, 5), (2, 1001),
           (3, 4096), (2, 2, 2), (4, 4, 4), (5, 8, 9), (8, 8, 8), (4, 8, 16), (16, 16, 16), (9, 5, 12), (32, 32, 32), (2, 18, 64),
           (6, 10, 64), (5, 7, 16), (4, 4, 128)]
PER_COMBINATION = 4      # extents per (batch, groups, Cin, Cout): 768 combinations x 4 of the 26 extents, every pairing in turn


def sweep():
    """the shapes (B, groups, Cin, Cout, W), without repeats: the families table, the two shapes without a plan, the zoo, the grid"""
    out = list(F.shapes()) + [F.NOPLAN, F.NOPLAN_WRW]
    out += [(B, 16, ci, co, W) for B in (8, 2) for ci, co, W in ZOO] + [(8, 64, 16, 16, (32, 32))]
    for i, (B, G, ci, co) in enumerate(itertools.product(BATCHES, GROUPS, CHANNELS, CHANNELS)):
        out += [(B, G, ci, co, EXTENTS[(5 * i + 7 * j) % len(EXTENTS)]) for j in range(PER_COMBINATION)]
    return list(dict.fromkeys(out))


def answers(lib, shapes):
    """one list in the order of QUERIES per shape; `lib`: any handle with the five C functions (prototypes are set here where the handle has none)"""
    size = (ctypes.c_int,) * 5 + (ctypes.POINTER(ctypes.c_int),)
    for name, restype, argtypes in (("ct_gconv_supported", ctypes.c_int, size), ("ct_gconv_fwd_norm_supported", ctypes.c_int, size),
                                    ("ct_gconv_precision_covers", ctypes.c_int, (ctypes.c_int,) + size),
                                    ("ct_gconv_bwd_weight_workspace_bytes", ctypes.c_size_t, size),
                                    ("ct_debug_set_gconv", None, (ctypes.c_uint,))):
        fn = getattr(lib, name)
        if fn.argtypes is None:      # (a handle of the package comes with its prototypes: leave them as every other test sees them)
            fn.restype, fn.argtypes = restype, list(argtypes)
    rows = []
    for B, G, ci, co, W in shapes:
        a = (B, G, ci, co, len(W), (ctypes.c_int * len(W))(*W))

        def norm_and_covers():
            return [lib.ct_gconv_fwd_norm_supported(*a), lib.ct_gconv_precision_covers(0, *a), lib.ct_gconv_precision_covers(1, *a)]
        row = [lib.ct_gconv_supported(*a)] + norm_and_covers() + [lib.ct_gconv_bwd_weight_workspace_bytes(*a)]
        lib.ct_debug_set_gconv(F.ksplit_from(20))
        try:
            row += norm_and_covers()
        finally:
            lib.ct_debug_set_gconv(0)
        rows.append(row)
    return rows


def small_mfma_workspace(B, G, ci, co, W):
    """what the small-volume matrix-core weight gradient wants (its plan's batch split, csrc/ct_gconv.hip: plan_wrw_mfma), 0 where
    the kind does not apply by shape; only used to tell which rule of the workspace query a row of the table exercises"""
    P = 1
    for w in W:
        P *= w
    if W[-1] not in (4, 8, 16) or not 16 <= P <= 512 or max(ci, co) < 32:
        return 0
    blocks = ((ci + 15) // 16) * ((co + 15) // 16)
    ksplit = 1
    while blocks * G * ksplit < 256 and ksplit * 2 <= B:
        ksplit *= 2
    return 0 if ksplit == 1 else (ksplit * G * blocks * 3 ** len(W) * 256 + ksplit * G * ((co + 15) // 16) * 16) * 4


def load():
    with open(PATH) as f:
        table = json.load(f)
    assert table["queries"] == list(QUERIES)
    return [((B, G, ci, co, tuple(W)), row) for B, G, ci, co, W, row in table["rows"]]


if __name__ == "__main__":
    shapes = sweep()
    rows = answers(ctypes.CDLL(os.path.abspath(sys.argv[1])), shapes)
    with open(PATH, "w") as f:
        f.write('{"queries": %s,\n "rows": [\n' % json.dumps(list(QUERIES)))
        f.write(",\n".join(json.dumps([B, G, ci, co, list(W), row], separators=(",", ":")) for (B, G, ci, co, W), row in zip(shapes, rows)))
        f.write("\n]}\n")
    print(len(shapes), "shapes ->", PATH)
