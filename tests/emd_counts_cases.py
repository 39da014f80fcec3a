"""Shared by the EMD-with-counts tests: the reference for a cloud whose size is no multiple of 1024.

oracle/emd_ref.c keeps the reference's precondition n % 1024 == 0, so a pair of clouds with c rows each is FAR-PADDED to the
next multiple of 1024: dummy row i = (1e6 + 16 i, 1e6, 1e6), the same in both clouds (exact in float32: ulp(1e6) = 1/16).  A
dummy target scores about 3 - 1.7e6 for a real bidder, far below every real target's value while prices stay below ~1e6, so
with at least two real targets it is never a real bidder's best or second best; a dummy bidder scores 3 - price on its own
dummy target and at most 3 - 16 elsewhere, so it takes its own target and touches no real price.  The real rows of the padded
run are therefore the auction on the real rows alone (tests/test_emd_counts_cpu.py checks this oracle against oracle where
it can be checked: c = 1024 padded to 2048).  Each reference is computed once per process and never modified."""
import functools

import numpy as np

from oracle import emd_ref


def uniform_pair(c, seed):
    rng = np.random.default_rng(seed)
    return rng.random((c, 3), dtype=np.float32), rng.random((c, 3), dtype=np.float32)


def collapsed_pair(c, seed):
    """tests/test_emd_gpu.py::_collapsed for one pair: a blob with every point twice against a sphere shell."""
    from tests.test_emd_gpu import _collapsed
    a, b = _collapsed(1, c, seed)
    return a[0], b[0]


def far_pad(x, rows):
    """x f32[c,3] -> f32[rows,3] with the dummy rows appended."""
    c = x.shape[0]
    i = np.arange(rows - c, dtype=np.float64)
    dummy = np.stack([1e6 + 16.0 * i, np.full_like(i, 1e6), np.full_like(i, 1e6)], axis=1).astype(np.float32)
    return np.concatenate([np.ascontiguousarray(x, dtype=np.float32), dummy], axis=0)


def oracle_far_padded(a, b, eps, iters, rows=None):
    """The auction of oracle/emd_ref.c on the pair a, b f32[c,3] (c >= 2), far-padded to `rows` (default: the next multiple
    of 1024) -> (dist f32[c], assignment i32[c]).  Asserts what the recipe rests on: real rows get real targets."""
    c = a.shape[0]
    assert c >= 2 and b.shape[0] == c
    rows = -(-c // 1024) * 1024 if rows is None else rows
    st, dist, ass = emd_ref.forward(far_pad(a, rows)[None], far_pad(b, rows)[None], eps, iters)
    assert st == 1
    assert ass[0, :c].min() >= 0 and ass[0, :c].max() < c
    assert np.array_equal(ass[0, c:], np.arange(c, rows, dtype=np.int32))      # every dummy on its own dummy
    return dist[0, :c].copy(), ass[0, :c].copy()


@functools.lru_cache(maxsize=None)
def _cached(kind, c, seed, eps, iters):
    a, b = (uniform_pair if kind == "uniform" else collapsed_pair)(c, seed)
    dist, ass = oracle_far_padded(a, b, eps, iters)
    for x in (a, b, dist, ass):
        x.setflags(write=False)
    return a, b, dist, ass


def case(c, seed, eps, iters, kind="uniform"):
    """(a f32[c,3], b f32[c,3], dist f32[c], assignment i32[c]) of a seeded pair and its far-padded oracle run; read-only,
    computed once."""
    return _cached(kind, int(c), int(seed), float(eps), int(iters))


def batch(n, counts, seed, eps, iters):
    """A ragged batch: cloud k has counts[k] rows of a seeded uniform pair, the rows at or beyond it are NaN in both clouds.
    -> (xyz1 f32[B,n,3], xyz2 f32[B,n,3], refs): refs[k] = (dist, assignment) of the far-padded oracle for counts[k] >= 2,
    None below."""
    B = len(counts)
    x1 = np.full((B, n, 3), np.nan, dtype=np.float32)
    x2 = np.full((B, n, 3), np.nan, dtype=np.float32)
    refs = []
    for k, c in enumerate(counts):
        if c >= 2:
            a, b, dist, ass = case(c, seed + k, eps, iters)
            refs.append((dist, ass))
        else:
            a, b = uniform_pair(c, seed + k)
            refs.append(None)
        x1[k, :c], x2[k, :c] = a, b
    return x1, x2, refs
