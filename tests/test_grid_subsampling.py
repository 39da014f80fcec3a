"""csrc/host/grid_subsampling.cpp (ct_grid_subsample, include/cloudct_host.h) against the REFERENCE's own C++
(cpp_wrappers/cpp_subsampling/grid_subsampling/grid_subsampling.cpp:4-104: row counts and digests of its results in
tests/golden/grid_subsampling_reference.json, written by tests/golden/gen_grid_subsampling_golden.py) and against a numpy
restatement.  Rows are compared as sets (the reference's order is its hash map's): points and features BIT FOR BIT (same
float sums in input order), classes exactly."""
import hashlib
import json
import os

import numpy as np
import pytest

from cloud_transformers_amd.data import subsampling as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_subsampling_reference.json")
REF_CASES = [(20000, 0.04, 10), (5000, 0.3, 11), (4096, 1.5, 12)]
REF_VARIANTS = ((True, True), (True, False), (False, True), (False, False))


def numpy_restatement(points, features, classes, dl):
    pts = points.astype(np.float32)
    inv = np.float32(1) / np.float32(dl)
    org = np.floor(pts.min(0) * inv) * np.float32(dl)
    idx = np.floor((pts - org) / np.float32(dl)).astype(np.int64)
    span = np.floor((pts.max(0) - org) / np.float32(dl)).astype(np.int64) + 1
    key = idx[:, 0] + span[0] * idx[:, 1] + span[0] * span[1] * idx[:, 2]
    out = {}
    for i, k in enumerate(key):
        rec = out.setdefault(int(k), [np.zeros(3, np.float32), 0, None, None])
        rec[0] = rec[0] + pts[i]
        rec[1] += 1
        if features is not None:
            rec[2] = features[i].astype(np.float32) if rec[2] is None else rec[2] + features[i].astype(np.float32)
        if classes is not None:
            rec[3] = classes[i].copy() if rec[3] is None else np.maximum(rec[3], classes[i])
    keys = sorted(out)
    P = np.stack([out[k][0] * np.float32(1.0 / out[k][1]) for k in keys])
    F = None if features is None else np.stack([out[k][2] / np.float32(out[k][1]) for k in keys])
    C = None if classes is None else np.stack([out[k][3] for k in keys])
    return P, F, C


def as_sorted_rows(P, F, C):
    cols = [P] + ([F] if F is not None else []) + ([C.astype(np.float32)] if C is not None else [])
    rows = np.concatenate(cols, axis=1)
    return rows[np.lexsort(rows.T[::-1])]


def cloud(n, seed, lo=-3.0, hi=5.0):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    feats = rng.random((n, 3), dtype=np.float32)
    labels = rng.integers(0, 13, size=(n, 1)).astype(np.int32)
    return pts, feats, labels


@pytest.mark.parametrize("n,dl,seed", [(2000, 0.5, 0), (5000, 0.04, 1), (300, 2.0, 2), (1, 0.1, 3)])
def test_matches_numpy_restatement(n, dl, seed):
    pts, feats, labels = cloud(n, seed)
    P, F, C = S.compute(pts, features=feats, classes=labels, sampleDl=dl)
    Pn, Fn, Cn = numpy_restatement(pts, feats, labels, dl)
    assert P.shape == Pn.shape and np.array_equal(P, Pn) and np.array_equal(F, Fn) and np.array_equal(C, Cn)
    assert 0 < len(P) <= n


def test_return_layout_follows_the_reference_wrapper():
    pts, feats, labels = cloud(500, 4)
    only = S.compute(pts, sampleDl=0.7)
    assert isinstance(only, np.ndarray) and only.shape[1] == 3
    p, f = S.compute(pts, features=feats, sampleDl=0.7)
    p2, c = S.compute(pts, classes=labels[:, 0], sampleDl=0.7)
    assert c.ndim == 1 and np.array_equal(p, p2) and np.array_equal(p, only)
    p3, f3, c3 = S.grid_subsampling(pts, feats, labels, sampleDl=0.7)
    assert np.array_equal(f3, f) and c3.shape == (len(p3), 1)
    import cpp_wrappers.cpp_subsampling.grid_subsampling as ext          # the reference's import path
    assert np.array_equal(ext.compute(pts, sampleDl=0.7), only)
    with pytest.raises(ValueError):
        S.compute(pts, sampleDl=0.0)
    assert S.compute(np.zeros((0, 3), np.float32), sampleDl=0.1).shape == (0, 3)


def reference_cloud(n, seed):
    pts, feats, labels = cloud(n, seed)
    # clustered part: many points per cell, long float sums
    pts[: n // 2] = (pts[: n // 2] * 0.05).astype(np.float32)
    return pts, feats, labels


def golden_key(n, dl, seed, use_f, use_c):
    return "%d,%g,%d,features=%d,classes=%d" % (n, dl, seed, use_f, use_c)


def rows_digest(P, F, C):
    rows = np.ascontiguousarray(as_sorted_rows(P, F, C), np.float32)
    return {"rows": int(rows.shape[0]), "cols": int(rows.shape[1]), "sha256": hashlib.sha256(rows.tobytes()).hexdigest()}


@pytest.mark.parametrize("n,dl,seed", REF_CASES)
def test_matches_the_reference_cpp(n, dl, seed):
    with open(GOLDEN) as f:
        golden = json.load(f)
    pts, feats, labels = reference_cloud(n, seed)
    for use_f, use_c in REF_VARIANTS:
        f = feats if use_f else None
        c = labels if use_c else None
        got = S.compute(pts, features=f, classes=c, sampleDl=dl)
        got = (got,) if isinstance(got, np.ndarray) else got
        P = got[0]
        F = got[1] if use_f else None
        C = (got[2] if use_f else got[1]) if use_c else None
        assert rows_digest(P, F, C) == golden[golden_key(n, dl, seed, use_f, use_c)], (use_f, use_c)
