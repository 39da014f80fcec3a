"""ct_emd_fwd_tail without a GPU: the numpy restatement of one cloud's auction (tests/emd_tail_ref.py) held to oracle/emd_ref.c,
the facts the tail kernel rests on (the bidder count never grows; where a known auction ends), and the three new symbols."""
import os
import re

import numpy as np
import pytest

from tests import emd_tail_ref as R
from oracle import emd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(0.05, 2, 199), (0.05, 2, 250), (0.005, 0, 60), (0.004, 1, 1), (0.05, 0, 120), (1.0, 3, 80)]      # eps, seed, iters at n = 1024


@pytest.fixture(scope="module")
def runs():
    out = {}
    for eps, seed, iters in CASES:
        a, b = R.uniform_pair(1024, seed)
        out[(eps, seed, iters)] = (a, b) + R.auction(a[0], b[0], eps, iters)
    return out


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_the_oracle(runs, case):
    a, b, dist, ass, _ = runs[case]
    st, d_ref, a_ref = emd_ref.forward(a, b, case[0], case[2])
    assert st == 1
    assert np.array_equal(ass, a_ref[0])
    assert np.array_equal(dist.view(np.uint32), d_ref[0].view(np.uint32))


@pytest.mark.parametrize("case", CASES)
def test_bidder_counts_never_grow(runs, case):
    bidders = runs[case][4]
    assert len(bidders) == case[2] and bidders[0] == 1024
    assert all(x >= y for x, y in zip(bidders, bidders[1:]))


def test_the_known_auction_ends_at_iteration_199(runs):
    """n = 1024, eps 0.05, seed 2: iteration 199 is the first without a bidder — the oracle's assignment is a permutation at
    iters = 199 (the one bidder left is force-assigned to a free target) and not at 198."""
    a, b, _, _, bidders = runs[(0.05, 2, 250)]
    assert R.first_empty(bidders, 250) == 199 and bidders[198] == 1 and bidders[-1] == 0
    for iters, perm in ((199, True), (198, False)):
        st, _, ass = emd_ref.forward(a, b, 0.05, iters)
        assert st == 1 and (np.unique(ass[0]).size == 1024) == perm
    assert R.first_empty(runs[(0.05, 2, 199)][4], 199) == 199 and runs[(0.05, 2, 199)][4][-1] == 1


def test_the_new_symbols_are_declared_and_exported():
    from cloud_transformers_amd import _lib
    header = open(os.path.join(ROOT, "include", "cloudct.h")).read()
    lib = _lib.load()
    for name in ("ct_emd_tail_supported", "ct_emd_tail_workspace_bytes", "ct_emd_fwd_tail"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.ct_emd_tail_supported(1, 1) == 1 and lib.ct_emd_tail_supported(512, 16384) == 1
    assert lib.ct_emd_tail_supported(513, 1024) == 0 and lib.ct_emd_tail_supported(1, 16385) == 0 and lib.ct_emd_tail_supported(0, 8) == 0
    assert lib.ct_emd_tail_workspace_bytes(4, 8192) > lib.ct_emd_workspace_bytes(4, 8192) > 0
    assert lib.ct_emd_tail_workspace_bytes(0, 8) == 0
    assert lib.ct_emd_workspace_bytes(4, 8192) == 7 * 4 * 8192 * 4 + 256 + 256      # unchanged by this entry
    # refused before any launch (no device is touched: this test runs without one)
    assert lib.ct_emd_fwd_tail(None, None, None, None, None, None, None, 0, 1, 1024, 0.005, 5, -1, None) == -1       # CT_EINVAL
