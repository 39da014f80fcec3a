"""The k-nearest query and its interpolation without a GPU: the three entry points are declared and bound alike, they refuse
bad arguments before touching the device, the Python methods refuse theirs with ValueError, and the numpy restatement the GPU
tests compare against (tests/nbr_knn_ref.py) agrees with sklearn's KDTree."""
import ctypes
import re

import numpy as np
import pytest
import torch

from tests.nbr_knn_ref import knn_ref

NAMES = ("ct_nbr_knn", "ct_nbr_knn_multi", "ct_nbr_interp")


@pytest.fixture(scope="module")
def lib():
    from cloud_transformers_amd import _lib
    _lib.build()
    return _lib.load()


def _buf(n=4096):
    """A host buffer no entry point may dereference (every call below is refused before any launch), 16-byte aligned."""
    b = ctypes.create_string_buffer(n)
    base = ctypes.addressof(b)
    return ctypes.c_void_p(base + (-base % 16)), b


def test_declared_and_bound_with_matching_argument_counts(lib):
    from cloud_transformers_amd import _lib
    header = open(_lib.INCLUDE + "/cloudct.h").read()
    for name in NAMES:
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M | re.S)
        assert m, name + " is not declared in include/cloudct.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int and hasattr(lib, name)
    assert _lib.NBR_KNN_K_MAX == 64 and re.search(r"#define CT_NBR_KNN_K_MAX 64\b", header)


def test_knn_rejects_bad_arguments(lib):
    from cloud_transformers_amd import _lib
    p, keep = _buf()
    mis = ctypes.c_void_p(p.value + 4)
    o, d = _lib.float_array([0, 0, 0]), _lib.int_array([4, 4, 4])
    knn = lib.ct_nbr_knn
    for at in (0, 1, 5, 8, 9):                                                             # each pointer argument null
        args = [p, p, o, 0.5, d, p, 4, 3, p, p, None]
        args[at] = None
        assert knn(*args) == -1, at
    assert knn(p, p, None, 0.5, d, p, 4, 3, p, p, None) == -1                              # no origin / no dims
    assert knn(p, p, o, 0.5, None, p, 4, 3, p, p, None) == -1
    for k in (0, -1, 65, 16384):
        assert knn(p, p, o, 0.5, d, p, 4, k, p, p, None) == -1                             # K outside [1, 64]
    for q in (0, -5, 1 << 31, 1 << 40):
        assert knn(p, p, o, 0.5, d, p, q, 3, p, p, None) == -1                             # Q < 1, Q >= 2^31
    for h in (0.0, -0.5, float("nan"), float("inf")):
        assert knn(p, p, o, h, d, p, 4, 3, p, p, None) == -1                               # a bad grid
    assert knn(p, p, o, 0.5, _lib.int_array([0, 4, 4]), p, 4, 3, p, p, None) == -1
    assert knn(p, p, o, 0.5, _lib.int_array([1 << 13, 1 << 13, 2]), p, 4, 3, p, p, None) == -1
    assert knn(p, p, _lib.float_array([0, float("nan"), 0]), 0.5, d, p, 4, 3, p, p, None) == -1
    assert knn(p, mis, o, 0.5, d, p, 4, 3, p, p, None) == -1                               # sorted off the 16-byte grid
    del keep


def test_knn_multi_rejects_bad_arguments(lib):
    p, keep = _buf()
    multi = lib.ct_nbr_knn_multi
    for at in (0, 2, 3, 6, 7):
        args = [p, 2, p, p, 4, 3, p, p, None]
        args[at] = None
        assert multi(*args) == -1, at
    assert multi(ctypes.c_void_p(p.value + 4), 2, p, p, 4, 3, p, p, None) == -1            # the table off its 8-byte grid
    assert multi(p, 0, p, p, 4, 3, p, p, None) == -1                                       # no cloud
    for k in (0, 65):
        assert multi(p, 2, p, p, 4, k, p, p, None) == -1
    for q in (0, 1 << 31):
        assert multi(p, 2, p, p, q, 3, p, p, None) == -1
    del keep


def test_interp_rejects_bad_arguments(lib):
    p, keep = _buf()
    interp = lib.ct_nbr_interp
    for at in (0, 1, 4, 8):
        args = [p, p, 4, 3, p, 10, 13, 1e-8, p, None]
        args[at] = None
        assert interp(*args) == -1, at
    for k in (0, 65):
        assert interp(p, p, 4, k, p, 10, 13, 1e-8, p, None) == -1
    for q in (0, -1, 1 << 31):
        assert interp(p, p, q, 3, p, 10, 13, 1e-8, p, None) == -1
    assert interp(p, p, 4, 3, p, 0, 13, 1e-8, p, None) == -1                               # M < 1
    assert interp(p, p, 4, 3, p, 10, 0, 1e-8, p, None) == -1                               # C < 1
    assert interp(p, p, 4, 3, p, 10, 13, -1e-8, p, None) == -1                             # eps negative
    assert interp(p, p, 4, 3, p, 10, 13, float("nan"), p, None) == -1                      # eps NaN
    del keep


def _index_without_device(M=10):
    """The argument checks run before anything touches the device: an index whose build was skipped is enough for them."""
    from cloud_transformers_amd.neighbors import GridIndex
    ix = GridIndex.__new__(GridIndex)
    ix.device, ix.M = torch.device("cuda", 0), M
    return ix


def test_python_methods_raise_value_error():
    from cloud_transformers_amd.neighbors import GridIndexTable
    ix = _index_without_device()
    q = torch.zeros(4, 3)
    for k in (0, 65):
        with pytest.raises(ValueError, match="k must be in"):
            ix.query_knn(q, k)
        with pytest.raises(ValueError, match="k must be in"):
            ix.interpolate(torch.zeros(10, 2), q, k)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ix.query_knn(q, 3)                                                                 # a CPU tensor
    for bad in (torch.zeros(4, 2), torch.zeros(4), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(2, 4, 3)):
        with pytest.raises(ValueError, match=r"float32 \[Q, 3\]"):
            ix.query_knn(bad, 3)
    with pytest.raises(ValueError, match="values must be on"):
        ix.interpolate(torch.zeros(10, 2), q)
    for bad in (torch.zeros(9, 2), torch.zeros(10), torch.zeros(10, 0), torch.zeros(10, 2, dtype=torch.float16)):
        with pytest.raises(ValueError, match="values must be float32"):
            ix.interpolate(bad, q)
    for eps in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="eps"):
            ix.interpolate(torch.zeros(10, 2), q, eps=eps)
    tb = GridIndexTable.__new__(GridIndexTable)
    tb.device, tb.indices, tb.n_clouds = ix.device, [ix], 1
    cloud = torch.zeros(4, dtype=torch.int64)
    for k in (0, 65):
        with pytest.raises(ValueError, match="k must be in"):
            tb.query_knn(cloud, q, k)
    with pytest.raises(ValueError, match="no CPU fallback"):
        tb.query_knn(cloud, q, 3)
    with pytest.raises(ValueError, match=r"float32 \[Q, 3\]"):
        tb.query_knn(cloud, torch.zeros(4, 4), 3)


def test_full_ious_k_defaults_to_the_reference_projection_and_is_checked():
    import inspect
    from cloud_transformers_amd.data.s3dis_kpconv import VoteEvaluator
    assert inspect.signature(VoteEvaluator.full_ious).parameters["k"].default == 1
    ev = VoteEvaluator.__new__(VoteEvaluator)                  # the check comes before any state is touched
    for k in (0, -3, 65):
        with pytest.raises(ValueError, match="k must be in"):
            ev.full_ious(k)


# seeds checked on the CPU: with them no query has two equal distances among its k + 1 nearest (see the assertion below)
@pytest.mark.parametrize("k,seed", [(1, 11), (3, 12), (16, 13), (64, 14)])
def test_restatement_against_sklearn_kdtree(k, seed):
    from sklearn.neighbors import KDTree
    rng = np.random.default_rng(seed)
    P = rng.uniform(-3, 3, (2000, 3)).astype(np.float32)
    X = rng.uniform(-3.5, 3.5, (300, 3)).astype(np.float32)
    tree = KDTree(P.astype(np.float64))
    # sklearn's tie order is unspecified: the comparison holds only without ties, and no query is left out
    near, _ = tree.query(X.astype(np.float64), k + 1)
    assert (np.diff(near, axis=1) > 0).all(), "a query has equal distances among its k + 1 nearest: choose another seed"
    idx32, d232 = knn_ref(P, X, k + 1)
    assert (np.diff(d232.astype(np.float64), axis=1) > 0).all(), "equal float32 distances among the k + 1 nearest"
    dist, ind = tree.query(X.astype(np.float64), k)
    idx, d2 = knn_ref(P, X, k)
    np.testing.assert_array_equal(idx, ind)
    want = dist.astype(np.float32)
    got = np.sqrt(d2)
    ulp = np.spacing(want)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= 4 * ulp.astype(np.float64)).all()
