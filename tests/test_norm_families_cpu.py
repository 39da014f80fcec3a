"""The table of norm kernel families (tests/norm_families.py) names every launch tag of csrc/ct_bnorm.hip and csrc/ct_adain.hip: the
string literals passed to note() are exactly the tags its rows cover (none is marked unreachable), and the rows name the body the
dispatch code picks.  And the two conditions on the bounds of tests/test_norm_families_gpu.py (the same bound functions):

1. an fp32 emulation of the kernels' algorithm — two passes, per-thread strided partial sums (float4 items where the kernel takes
   them), the xor-shuffle tree over the 64 lanes, the waves added in order, the ranks merged by the parallel-variance rule in
   fp32 — stays at or below 0.5 of every bound on every row of the table, both distributions, ReLU on and off;
2. six wrong variants of the emulation each exceed a bound on at least one row: the bounds can see the errors they are there for."""
import os
import re

import numpy as np
import pytest

from tests import norm_families as F
from tests import test_norm_families_gpu as T
from tests.test_raster_families_cpu import note_literals

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cloud_transformers_amd", "csrc")
SOURCES = [os.path.join(CSRC, "ct_bnorm.hip"), os.path.join(CSRC, "ct_adain.hip")]
f32, f64 = np.float32, np.float64


def _text():
    out = ""
    for p in SOURCES:
        with open(p) as f:
            out += f.read()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# tags
# ---------------------------------------------------------------------------------------------------------------------
def test_every_note_literal_has_a_row_and_every_row_a_literal():
    tags = note_literals(_text())
    assert len(tags) == 12 + 3 + 12, sorted(tags)
    covered = F.covered_tags()
    assert not tags - covered, "launch tags without a row in tests/norm_families.py: %s" % sorted(tags - covered)
    assert not covered - tags, "rows naming tags the sources no longer have: %s" % sorted(covered - tags)


def test_removing_a_row_or_adding_a_literal_is_caught():
    text = _text()
    tags = note_literals(text)
    assert "x_new" not in tags
    assert note_literals(text + '\nvoid f() { note("x_new"); }') - F.covered_tags() == {"x_new"}
    for drop in ("bn_fwd_reg4", "bn_bwd_loop_vec", "bn_eval_scalar", "bn_eval_bwd", "adain_fwd_reg16", "adain_bwd_strided"):
        rest = set()
        for r in F.ROWS:
            if drop not in r.tags:
                rest.update(r.tags)
        assert drop in tags - rest, drop


def test_every_launch_function_notes_a_tag_and_every_entry_point_resets():
    text = _text()
    for name in ("bn_fwd_launch_table", "bn_bwd_launch_table", "adain_fwd_launch_table", "adain_bwd_launch_table", "ct_bn_eval_group_fwd",
                 "ct_bn_eval_group_bwd"):
        body = text[text.index(" %s(" % name):]
        body = body[:body.index("\n}\n")]
        assert "hipLaunchKernelGGL" in body or "_DISPATCH(" in body, name
        assert re.search(r"(?<![\w.])note\(", body), name
    entries = re.findall(r'extern "C" int (ct_\w+)\(', text)
    launching = [e for e in entries if not e.endswith("_supported")]
    assert len(launching) == 10, launching
    for name in launching:
        body = text[text.index('extern "C" int %s(' % name):]
        body = body[body.index("{"):body.index("\n}\n")]
        assert body.lstrip("{ \n").startswith("note_reset();"), name


def test_rows_name_the_body_the_dispatch_picks():
    ids = [r.id for r in F.ROWS] + [r.id for r in F.RANKS]
    assert len(ids) == len(set(ids))
    for r in F.ROWS:
        assert 3 <= r.C <= 5 and r.B * r.C * r.N <= 135000, r
        aligned = r.variant == "dense"
        assert r.variant in ("dense", "x_offset"), r
        if r.entry in ("bn_train", "bn_phases"):
            assert r.B * r.N >= 2 and r.tags == F._pair("bn", F.bn_family(r.B, r.N, aligned)), r
        elif r.entry == "adain":
            assert r.tags == F._pair("adain", F.adain_family(r.N, aligned)), r
        elif r.entry == "bn_eval":
            assert r.tags == ("bn_eval_vec" if r.N % 4 == 0 else "bn_eval_scalar",), r
            assert T.eval_cut(r.B, r.N, 2 * r.C + 2) == r.cut, r
    assert {r.cut > 1 for r in F.rows("bn_eval")} == {True, False}
    # both sides of every threshold
    quads = sorted(r.B * r.N // 4 for r in F.rows("bn_train") if r.tags[0] not in ("bn_fwd_loop_scalar",))
    assert quads == [1, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8194], quads
    assert sorted(r.N for r in F.rows("adain") if r.variant == "dense") == [1, 4, 1001, 1024, 1028, 2048, 2052, 4096, 4100, 8192, 8196,
                                                                           16384, 16388]
    for k in F.RANKS:
        assert 3 <= k.C <= 5 and k.families == tuple(F.bn_family(B, k.N) for B in k.Bs), k
    assert len({B for k in F.RANKS for B in k.Bs if len(k.Bs) > 1}) > 2                 # unequal counts per rank
    for id in F.MASK_ROWS + F.SLICE_ROWS + F.ADAIN_SLICE_ROWS:
        assert F.by_id(id)
    assert {F.by_id(i).tags[0] for i in F.MASK_ROWS} == {"bn_fwd_" + k for k in ("reg1", "reg2", "reg4", "reg8", "loop_vec", "loop_scalar")}


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 emulation
# ---------------------------------------------------------------------------------------------------------------------
VARIANTS = ("one_pass", "var_m1", "rv_no_factor", "merge_no_term", "local_count", "drop_last")
_LANE = np.arange(64)


def emu_sum(vals, vec, threads, drop_last=False):
    """the workgroup's sum of a channel's fp32 values in channel order: items (float4: (x + y) + (z + w)) dealt to the threads with
    stride `threads` and added in loop order, the wave's xor-shuffle tree, the waves in order"""
    vals = np.asarray(vals, f32)
    if vec:
        q = vals.reshape(-1, 4)
        vals = (q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])
    if drop_last:
        vals = vals[:-1]
    K = -(-vals.size // threads)
    pad = np.zeros(K * threads, f32)
    pad[:vals.size] = vals
    acc = np.zeros(threads, f32)
    for row in pad.reshape(K, threads):
        acc = acc + row
    lanes = acc.reshape(threads // 64, 64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, _LANE ^ o]
    s = f32(0)
    for w in range(threads // 64):
        s = s + lanes[w, 0]
    return f32(s)


def _rsqrt(v):
    return f32(1.0 / np.sqrt(f64(v)))


def emulate(xs, gys, w, b, relu, rm=None, rv=None, vecs=None, threads=F.BN_THREADS, phases=False, adain=False, variant=None):
    """the kernels' arithmetic in fp32 (numpy), one norm over len(xs) ranks; returns `out` as T.compare() reads it.  phases: the
    four exchange phases (statistics merged in fp32, sums added in rank order); adain: the means by a multiplication with 1 / N.
    The backward's mask is the emulated forward's."""
    world, C = len(xs), xs[0].shape[1]
    eps, mom, one = f32(T.EPS), f32(T.MOMENTUM), f32(1)
    n = [f32(x.shape[0] * x.shape[2]) for x in xs]
    drop = variant == "drop_last"
    div = (lambda s, k: s * (one / k)) if adain else (lambda s, k: s / k)

    def chan(a, c):
        return a[:, c, :].ravel()

    mean, m2 = np.zeros((world, C), f32), np.zeros((world, C), f32)
    for r, x in enumerate(xs):
        for c in range(C):
            v = chan(x, c)
            mean[r, c] = div(emu_sum(v, vecs[r], threads, drop), n[r])
            if variant == "one_pass":
                m2[r, c] = emu_sum(v * v, vecs[r], threads) - n[r] * mean[r, c] * mean[r, c]
            else:
                d = v - mean[r, c]
                m2[r, c] = emu_sum(d * d, vecs[r], threads, drop)
    out = dict(y=[], save_mean=[], save_rstd=[], gx=[])
    if phases:
        out.update(local=[(mean[r], m2[r], n[r]) for r in range(world)], count_total=[], sums=[])
    if rm is not None:
        out.update(rm=[], rv=[])
    stats = []
    for r, x in enumerate(xs):
        if phases:                                             # merge_rank_stats, every rank for itself
            total, acc = f32(0), np.zeros(C, f32)
            for k in range(world):
                total = total + n[k]
                acc = acc + mean[k] * n[k]
            mu = acc / total
            s = np.zeros(C, f32)
            for k in range(world):
                d = mean[k] - mu
                s = s + (m2[k] if variant == "merge_no_term" else m2[k] + n[k] * d * d)
            var, M = s / total, total
            out["count_total"].append(M)
        else:
            mu, M = mean[r], n[r]
            var = div(m2[r], M)
        rs = _rsqrt((var * (M / (M - one)) if variant == "var_m1" else var) + eps)
        if rm is not None:
            unb = var if variant == "rv_no_factor" else var * (M / (M - one))
            out["rm"].append((one - mom) * rm + mom * mu)
            out["rv"].append((one - mom) * rv + mom * unb)
        g = w * rs
        y = (x - T._c(mu)) * T._c(g) + T._c(b)
        if relu:
            y = np.maximum(y, f32(0))
        out["y"].append(y)
        out["save_mean"].append(mu)
        out["save_rstd"].append(rs)
        stats.append((mu, rs, g, M))
    # backward
    s0, s1 = np.zeros((world, C), f32), np.zeros((world, C), f32)
    gps, xhs = [], []
    for r, x in enumerate(xs):
        mu, rs, g, M = stats[r]
        xh = (x - T._c(mu)) * T._c(rs)
        gp = np.where(out["y"][r] > 0, gys[r], f32(0)) if relu else gys[r]
        for c in range(C):
            s0[r, c] = emu_sum(chan(gp, c), vecs[r], threads, drop)
            s1[r, c] = emu_sum(chan(gp * xh, c), vecs[r], threads, drop)
        gps.append(gp)
        xhs.append(xh)
    t0, t1 = s0[0].copy(), s1[0].copy()
    for r in range(1, world):
        t0, t1 = t0 + s0[r], t1 + s1[r]
    for r in range(world):
        mu, rs, g, M = stats[r]
        if phases:
            out["sums"].append((s0[r], s1[r]))
            a0, a1 = t0, t1
            M = n[r] if variant == "local_count" else M
        else:
            a0, a1 = s0[r], s1[r]
        m0, m1 = div(a0, M), div(a1, M)
        out["gx"].append(T._c(g) * (gps[r] - T._c(m0) - xhs[r] * T._c(m1)))
    out["gb"] = s0.astype(f64).sum(0) if phases else s0[0]
    out["gw"] = s1.astype(f64).sum(0) if phases else s1[0]
    return out


def _worst(R):
    return max(R.worst.values())


def _bn_setup(key, Bs, C, N, dist, variant_layout="dense"):
    case = T.make_case(key, Bs, C, N, dist)
    vecs = T.bn_vecs(Bs, N, variant_layout == "dense")
    return case, vecs


def _bn_ratios(key, Bs, C, N, dist, relu, phases, layout="dense", variant=None):
    case, vecs = _bn_setup(key, Bs, C, N, dist, layout)
    with np.errstate(invalid="ignore"):                        # (a one-pass variance can come out negative)
        out = emulate(case["xs"], case["gys"], case["w"], case["b"], relu, case["rm"], case["rv"], vecs, phases=phases, variant=variant)
    f = T.forward_ref(case["xs"], case["w"], case["b"], relu, vecs, rm=case["rm"], rv=case["rv"])
    bw = T.backward_ref(f, case["gys"], [y > 0 for y in out["y"]] if relu else None)
    R = T.Ratios("%s %s relu=%d %s" % (key, dist, relu, variant or "emulation"), strict=variant is None)
    T.compare(R, f, bw, out)
    return R


def _adain_ratios(row, dist, relu):
    case, gamma, w64 = T.adain_case(row, dist)
    vec = row.tags[0] != "adain_fwd_strided"
    out = emulate(case["xs"], case["gys"], f32(gamma + f32(1)), case["b"], relu, vecs=[vec], threads=F.ADAIN_THREADS, adain=True)
    f = T.forward_ref(case["xs"], w64, case["b"], relu, [vec], threads=F.ADAIN_THREADS)
    if row.N == 1:
        out = {k: v for k, v in out.items() if k in ("y", "save_mean", "save_rstd")}
        bw = None
    else:
        bw = T.backward_ref(f, case["gys"], [out["y"][0] > 0] if relu else None)
    R = T.Ratios("%s %s relu=%d emulation" % (row.id, dist, relu))
    T.compare(R, f, bw, out)
    return R


BN_ROWS = F.rows("bn_train") + F.rows("bn_phases")


@pytest.mark.parametrize("dist", T.DISTS)
@pytest.mark.parametrize("row", BN_ROWS, ids=[r.id for r in BN_ROWS])
def test_emulation_is_within_half_of_every_bound_bn(row, dist):
    for relu in (False, True):
        _bn_ratios(row.id, (row.B,), row.C, row.N, dist, relu, row.entry == "bn_phases", row.variant).done(0.5)


@pytest.mark.parametrize("dist", T.DISTS)
@pytest.mark.parametrize("ranks", F.RANKS, ids=[r.id for r in F.RANKS])
def test_emulation_is_within_half_of_every_bound_multi_rank(ranks, dist):
    for relu in (False, True):
        _bn_ratios(ranks.id, ranks.Bs, ranks.C, ranks.N, dist, relu, True).done(0.5)


ADAIN_ROWS = F.rows("adain")


@pytest.mark.parametrize("dist", T.DISTS)
@pytest.mark.parametrize("row", ADAIN_ROWS, ids=[r.id for r in ADAIN_ROWS])
def test_emulation_is_within_half_of_every_bound_adain(row, dist):
    for relu in (False, True):
        _adain_ratios(row, dist, relu).done(0.5)


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_wrong_variant_exceeds_a_bound(variant):
    """every row the variant can show on is tried with both distributions; it must leave a bound on at least one, and the list of
    rows it leaves a bound on is printed with the factor"""
    multi = variant in ("merge_no_term", "local_count")
    hits = []
    cases = [(k.id, k.Bs, k.C, k.N, True, "dense") for k in F.RANKS if len(k.Bs) > 1]
    if not multi:
        cases = [(r.id, (r.B,), r.C, r.N, r.entry == "bn_phases", r.variant) for r in BN_ROWS] + cases
    for key, Bs, C, N, phases, layout in cases:
        for dist in T.DISTS:
            R = _bn_ratios(key, Bs, C, N, dist, False, phases, layout, variant)
            if _worst(R) > 1.0:
                hits.append((key, dist, max(R.worst, key=R.worst.get), _worst(R)))
    print("\n".join("%s: %s %s %s %.3g x the bound" % ((variant,) + h) for h in hits))
    assert hits, variant
    if variant in ("one_pass", "merge_no_term", "local_count"):
        assert max(h[3] for h in hits) > 50, hits
