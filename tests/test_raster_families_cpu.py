"""The table of Splat / Slice kernel families (tests/raster_families.py) names every launch tag of csrc/ct_raster.hip: the string
literals passed to note() — both arms of a ternary included — are exactly the tags its rows cover or mark unreachable."""
import os
import re

from tests import raster_families as F

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cloud_transformers_amd", "csrc", "ct_raster.hip")


def note_literals(text):
    """every string literal inside the argument list of a note(...) call (not the definition `void note(const char* tag)`)"""
    out = set()
    for m in re.finditer(r"(?<![\w.])note\(", text):
        depth, i = 1, m.end()
        while depth:
            ch = text[i]
            if ch == '"':
                j = text.index('"', i + 1)
                out.add(text[i + 1:j])
                i = j
            elif ch == "(":
                depth += 1
            elif ch == ")":
                depth -= 1
            i += 1
    return out


def test_note_parser_reads_ternaries_and_skips_the_definition():
    text = 'void note(const char* tag) {}\n  note(n > 1 ? "a_segments" : k > 1 ? "a_groups" : "a");\n  note("b"); x.note("c");'
    assert note_literals(text) == {"a_segments", "a_groups", "a", "b"}


def test_every_note_literal_has_a_row_and_every_row_a_literal():
    with open(SRC) as f:
        tags = note_literals(f.read())
    assert len(tags) > 40, sorted(tags)
    covered = F.covered_tags()
    assert not tags - covered, "launch tags without a row in tests/raster_families.py: %s" % sorted(tags - covered)
    assert not covered - tags, "rows naming tags csrc/ct_raster.hip no longer has: %s" % sorted(covered - tags)


def test_rows_are_well_formed():
    from cloud_transformers_amd import _lib
    assert (F.NO_HOT, F.FORCE_HOT, F.NO_BAND, F.FORCE_BAND, F.NO_SORTED, F.FORCE_SORTED, F.FORCE_SORTED_SEG, F.NO_WIDE) == (
        _lib.DEBUG_NO_HOT, _lib.DEBUG_FORCE_HOT, _lib.DEBUG_NO_BAND, _lib.DEBUG_FORCE_BAND, _lib.DEBUG_NO_SORTED,
        _lib.DEBUG_FORCE_SORTED, _lib.DEBUG_FORCE_SORTED_SEG, _lib.DEBUG_NO_WIDE)
    ids = [r.id for r in F.ROWS] + [w.id for w in F.WIDE_CASES]
    assert len(ids) == len(set(ids))
    for r in F.ROWS:
        assert r.api in _lib.SIGNATURES, r
        assert F.entry(r) in ("splat_fwd", "splat_bwd", "slice_fwd", "slice_bwd"), r
        assert (r.reduce in ("max", "sum")) == r.api.startswith(("ct_splat_", )), r
        assert r.pad in (None, "f32", "i32") and len(r.W) in (2, 3) and min(r.W) >= 2, r
        assert not r.tickets or r.api.endswith(("_tk", "_ps")), r
        assert not r.accumulate or r.api == "ct_splat_bwd_ex", r
        assert not r.keys_add or r.api == "ct_splat_bwd_tk", r
        assert r.C >= 2, "a row needs two channels at least for its all-negative and its 1e-4 .. 1e4 channels"
    for w in F.WIDE_CASES:
        assert "+wide" not in w.narrow_tag and w.tag.replace("+wide", "") .split("_")[0] == w.narrow_tag.split("_")[0]


def test_removing_a_row_or_adding_a_literal_is_caught():
    with open(SRC) as f:
        text = f.read()
    tags = note_literals(text)
    assert "x_new_family" not in tags
    assert note_literals(text + '\nvoid f() { note("x_new_family"); }') - F.covered_tags() == {"x_new_family"}
    for drop in ("scatter_global_atomics", "slice_bwd_gw_stats_nsplit", "band_splat_bwd3"):
        rest = set(F.UNREACHABLE)
        for r in F.ROWS:
            if drop not in r.tag.split("+"):
                rest.update(r.tag.split("+"))
                rest.update((r.setup_tag or "").split("+"))
        for w in F.WIDE_CASES:
            rest.update(w.tag.split("+") + w.narrow_tag.split("+"))
        assert drop in tags - rest
