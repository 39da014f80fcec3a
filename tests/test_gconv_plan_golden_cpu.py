"""What the grouped convolution's planner (csrc/ct_gconv.hip) answers without a GPU — ct_gconv_supported,
ct_gconv_fwd_norm_supported, ct_gconv_precision_covers and ct_gconv_bwd_weight_workspace_bytes — equals, shape by shape, the table
tests/golden/gconv_plan_queries.json, which tests/gconv_plan_golden.py recorded from a build of the commit before the planner became
a value (FwdPlan / WrwCand).  A change to the walk, a threshold, a budget or a workspace formula shows here as the rows it moves."""
from cloud_transformers_amd import _lib
from tests import gconv_families as F
from tests import gconv_plan_golden as G

TABLE = G.load()
COL = {q: i for i, q in enumerate(G.QUERIES)}


def test_the_table_covers_the_sweep_and_cannot_pass_vacuously():
    shapes = [s for s, _ in TABLE]
    assert len(shapes) == len(set(shapes)) and 2000 <= len(shapes) <= 5000
    assert set(G.sweep()) == set(shapes), "tests/gconv_plan_golden.py: sweep() and the recorded table differ"
    assert set(F.shapes()) | {F.NOPLAN, F.NOPLAN_WRW} <= set(shapes)
    by_shape = dict(TABLE)
    assert by_shape[F.NOPLAN][COL["supported"]] == 0 and by_shape[F.NOPLAN_WRW][COL["supported"]] == 0
    for q in G.QUERIES:
        values = {row[COL[q]] for _, row in TABLE}
        if q == "workspace":
            assert 0 in values and len(values) > 100, q
        else:
            assert values == {0, 1}, (q, values)
    # the three rules of the workspace query: four-channel groups (sized for the four-channel kinds only), the 16-channel ring
    # alone (the small-volume matrix-core kind does not apply by shape), and the small-volume kind's batch split
    rules = {"c4": 0, "ring": 0, "small_mfma": 0}
    for (B, Gr, ci, co, W), row in TABLE:
        ws, mfma = row[COL["workspace"]], G.small_mfma_workspace(B, Gr, ci, co, W)
        if ws and ci == 4 and co == 4:
            rules["c4"] += 1
        elif ws and not mfma:
            rules["ring"] += 1
        elif ws and ws == mfma:
            rules["small_mfma"] += 1
    assert min(rules.values()) >= 10, rules
    # the debug word moves answers: the second pass is not a copy of the first
    assert any(row[COL["norm"]] != row[COL["norm_k20"]] or row[COL["covers0"]] != row[COL["covers0_k20"]] for _, row in TABLE)


def test_the_planner_answers_what_it_answered_before():
    _lib.build()
    got = G.answers(_lib.load(), [s for s, _ in TABLE])
    wrong = [(s, dict(zip(G.QUERIES, want)), dict(zip(G.QUERIES, g))) for (s, want), g in zip(TABLE, got) if g != want]
    assert not wrong, "%d of %d shapes differ; the first: %s" % (len(wrong), len(TABLE), wrong[:3])
