"""CPU-side checks of the EMD for any cloud size and per-cloud counts: the far-padding recipe of tests/emd_counts_cases.py
(oracle against oracle), argument validation of the two new entry points without a device, their declarations, the Python
wrappers' errors and the routing between the dense and the counts autograd functions."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import emd_ref
from tests.emd_counts_cases import collapsed_pair, oracle_far_padded, uniform_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from cloud_transformers_amd import _lib
    _lib.build()
    return _lib.load()


@pytest.mark.parametrize("kind,eps,iters", [("uniform", 0.005, 50), ("collapsed", 0.005, 30)])
def test_far_padding_leaves_the_real_rows_alone(kind, eps, iters):
    """c = 1024 needs no padding, so the recipe can be held to the oracle itself: padded to 2048, the first 1024 rows are the
    unpadded run's assignment exactly and its distances bit for bit, and every dummy is assigned to a dummy."""
    a, b = uniform_pair(1024, 31) if kind == "uniform" else collapsed_pair(1024, 32)
    st, d0, a0 = emd_ref.forward(a[None], b[None], eps, iters)
    assert st == 1
    d1, a1 = oracle_far_padded(a, b, eps, iters, rows=2048)
    assert np.array_equal(a1, a0[0])
    assert np.array_equal(d1.view(np.uint32), d0[0].view(np.uint32))


def test_new_entry_points_validate_without_gpu(lib):
    """CT_EINVAL for null required pointers, B <= 0, n <= 0, iters < 1; CT_EPRECOND for B > 512; CT_EWORKSPACE for a short
    workspace — before anything touches the device.  The count may be null; n need not be a multiple of 1024."""
    p = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    big = 1 << 40
    # ct_emd_fwd_counts(xyz1, xyz2, count, dist, assignment, workspace, workspace_bytes, B, n, eps, iters, s)
    for hole in (0, 1, 3, 4, 5):
        args = [p] * 6
        args[hole] = None
        assert lib.ct_emd_fwd_counts(*args, big, 1, 1000, 0.005, 5, None) == -1, hole
    for B, n, iters in [(0, 1000, 5), (-1, 1000, 5), (1, 0, 5), (1, -7, 5), (1, 1000, 0), (1, 1000, -1)]:
        assert lib.ct_emd_fwd_counts(p, p, None, p, p, p, big, B, n, 0.005, iters, None) == -1, (B, n, iters)
    assert lib.ct_emd_fwd_counts(p, p, None, p, p, p, big, 513, 1000, 0.005, 5, None) == -4
    assert lib.ct_emd_fwd_counts(p, p, p, p, p, p, big, 513, 1024, 0.005, 5, None) == -4
    for B, n in [(1, 1000), (3, 1), (2, 1024)]:
        need = lib.ct_emd_workspace_bytes(B, n)
        assert need > 0
        assert lib.ct_emd_fwd_counts(p, p, None, p, p, p, need - 1, B, n, 0.005, 5, None) == -3, (B, n)
        assert lib.ct_emd_fwd_counts(p, p, p, p, p, p, 0, B, n, 0.005, 5, None) == -3, (B, n)
    # ct_emd_bwd_counts(xyz1, xyz2, count, g_dist, assignment, g_xyz1, B, n, s)
    for hole in (0, 1, 3, 4, 5):
        args = [p] * 6
        args[hole] = None
        assert lib.ct_emd_bwd_counts(*args, 1, 1000, None) == -1, hole
    for B, n in [(0, 1000), (-1, 1000), (1, 0), (1, -7)]:
        assert lib.ct_emd_bwd_counts(p, p, None, p, p, p, B, n, None) == -1, (B, n)


def test_header_and_table_declare_the_new_symbols():
    from cloud_transformers_amd import _lib
    text = open(os.path.join(ROOT, "include", "cloudct.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("ct_emd_fwd_counts", 12), ("ct_emd_bwd_counts", 9)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert len(m.group(1).split(",")) == n_args
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
    # ... and the version comment lists them among the additive symbols, after Chamfer's
    listing = [m for m in re.findall(r"/\*.*?\*/", text, flags=re.S) if "ct_voxel_bounds" in m and "ct_chamfer_fwd_counts" in m]
    assert len(listing) == 1 and "ct_emd_fwd_counts / ct_emd_bwd_counts" in listing[0]


def test_wrappers_refuse_cpu_tensors_and_bad_counts():
    from cloud_transformers_amd.emd import emd_distance, emd_with_counts, emdModule, loss_emd_counts
    a, b = torch.zeros(2, 5, 3), torch.zeros(2, 5, 3)
    c = torch.tensor([5, 2], dtype=torch.int32)
    for call in (lambda: emd_with_counts(a, b, 0.005, 5, c), lambda: emd_with_counts(a, b, 0.005, 5),
                 lambda: emdModule()(a, b, 0.005, 5, c), lambda: emd_distance(a, b, 0.005, 5, c),
                 lambda: emd_distance(a, b, 0.005, 5),
                 lambda: loss_emd_counts(a.permute(0, 2, 1)[:, :, None], b.permute(0, 2, 1)[:, :, None], 0.005, 5, c)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for bad in (c.long(), c.float(), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), [5, 2], 5):
        with pytest.raises(TypeError, match="int32"):
            emd_with_counts(a, b, 0.005, 5, bad)
    with pytest.raises(ValueError, match="count is on meta"):
        emd_with_counts(a, b, 0.005, 5, torch.zeros(2, dtype=torch.int32, device="meta"))


def test_routing_between_the_dense_and_the_counts_function(monkeypatch):
    """emd_distance takes emdFunction exactly when there is no count and n is a multiple of 1024; emdModule()(a, b, eps,
    iters) never takes the counts function (its asserts stay), and with a count it always does."""
    from cloud_transformers_amd import emd
    calls = []
    monkeypatch.setattr(emd.emdFunction, "apply", staticmethod(lambda *args: calls.append(("dense", len(args))) or ("d", "a")))
    monkeypatch.setattr(emd.EmdWithCountsFunction, "apply",
                        staticmethod(lambda *args: calls.append(("counts", len(args))) or ("d", "a")))
    c = torch.tensor([1], dtype=torch.int32)
    for n in (1, 63, 1000, 1023, 1024, 1025, 2048, 2500, 10000, 16384):
        x = torch.zeros(1, n, 3)
        del calls[:]
        emd.emd_distance(x, x, 0.005, 5)
        emd.emd_distance(x, x, 0.005, 5, c)
        emd.emdModule()(x, x, 0.005, 5)
        emd.emdModule()(x, x, 0.005, 5, c)
        emd.emdModule()(x, x, 0.005, 5, count=c)
        emd.emd_with_counts(x, x, 0.005, 5)
        first = ("dense", 4) if n % 1024 == 0 else ("counts", 5)
        assert calls == [first, ("counts", 5), ("dense", 4), ("counts", 5), ("counts", 5), ("counts", 5)], (n, calls)
