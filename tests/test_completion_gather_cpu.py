"""The resident ShapeNet completion path without a GPU: ct_completion_gather (include/cloudct.h, csrc/ct_completion.hip) is
declared, exported and bound and refuses bad arguments before touching a device; its numpy restatement
(tests/completion_gather_ref.py) equals the project's host chain (Dataset.__getitem__, Compose, RandomSamplePoints,
RandomMirrorPoints, collate_fn) on the same draws for the train, val and test subsets; `decode_split` and its cache;
`DeviceCompletionBatches.epoch_order` is torch's DistributedSampler order; the harness knows the new data kind."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from tests.completion_gather_ref import mirror_signs, reference_gather, restrict
from tests.completion_tree import make_tree

EINVAL = -1
N_IN, N_OUT = 32, 64


@pytest.fixture(scope="module")
def lib():
    from cloud_transformers_amd import _lib
    _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from cloud_transformers_amd.data.completion import shapenet_loader
    root = tmp_path_factory.mktemp("gather_tree")
    keys = make_tree(root, N_IN, N_OUT)
    return {"root": root, "keys": keys, "loader": shapenet_loader(keys)}


def test_symbol_is_declared_exported_and_bound(lib):
    from cloud_transformers_amd import _lib
    with open(os.path.join(_lib.INCLUDE, "cloudct.h")) as f:
        header = f.read()
    assert re.search(r"^int ct_completion_gather\(", header, re.M)
    assert "ct_completion_gather" in _lib.SIGNATURES and hasattr(lib, "ct_completion_gather")
    assert len(_lib.SIGNATURES["ct_completion_gather"][1]) == 20
    assert _lib.ABI_VERSION == 3 and "#define CT_ABI_VERSION 3" in header            # additive: no bump
    version_comment = header[:header.index("#define CT_ABI_VERSION")]
    assert "ct_completion_gather" in version_comment


def test_gather_rejects_bad_arguments(lib):
    b = ctypes.create_string_buffer(256)
    p = ctypes.cast(b, ctypes.c_void_p)
    names = ("pp", "po", "gp", "go", "item", "rendering", "perm_in", "perm_gt", "u_mirror", "out_p", "out_g")

    def call(*, M=3, R=2, p_cap=20, g_cap=30, scale=2.0, B=2, n_in=16, n_out=32, **ptr):
        a = {k: ptr.get(k, p) for k in names}
        return lib.ct_completion_gather(a["pp"], a["po"], a["gp"], a["go"], M, R, p_cap, g_cap, a["item"], a["rendering"], a["perm_in"],
                                        a["perm_gt"], a["u_mirror"], scale, B, n_in, n_out, a["out_p"], a["out_g"], None)

    for name in names:
        if name not in ("perm_gt", "u_mirror"):                            # (those two are nullable)
            assert call(**{name: None}) == EINVAL, name
    assert call(B=0) == EINVAL and call(B=-1) == EINVAL and call(B=65536) == EINVAL
    assert call(n_in=0) == EINVAL and call(n_in=-2) == EINVAL and call(n_in=16385) == EINVAL
    assert call(n_out=0) == EINVAL and call(n_out=-2) == EINVAL and call(n_out=65537) == EINVAL
    assert call(p_cap=0) == EINVAL and call(p_cap=-1) == EINVAL and call(p_cap=65537) == EINVAL
    assert call(g_cap=0) == EINVAL and call(g_cap=-1) == EINVAL and call(g_cap=65537) == EINVAL
    assert call(R=0) == EINVAL and call(R=-1) == EINVAL
    assert call(M=0) == EINVAL and call(M=-5) == EINVAL and call(M=2 ** 62, R=4) == EINVAL
    for scale in (0.0, -0.0, float("inf"), -float("inf"), float("nan")):
        assert call(scale=scale) == EINVAL, scale
    del b


SUBSETS = ["TRAIN", "VAL", "TEST"]


@pytest.mark.parametrize("subset", SUBSETS)
def test_restatement_equals_the_host_chain(tree, subset, monkeypatch):
    """The host items of a batch with np.random.permutation, np.random.uniform and random.randint patched to hand out the
    restricted permutations, the mirror draw and the rendering of the same explicit draws the restatement takes."""
    from cloud_transformers_amd.data import completion as C
    ds = tree["loader"].get_dataset(getattr(C.DatasetSubset, subset))
    dec = C.decode_split(ds)
    train, sampled_gt = subset == "TRAIN", subset != "TEST"
    R, M = dec["R"], len(ds)
    assert R == (2 if train else 1) and M == 3
    p_cap = int(np.diff(dec["partial_offsets"]).max())
    g_cap = int(np.diff(dec["gt_offsets"]).max())
    n_out = N_OUT                                                            # (TEST stores gt clouds of exactly N_OUT rows)
    rng = np.random.default_rng(7)
    item = np.array([2, 0, 1, 0, 2], np.int64)
    B = len(item)
    rendering = np.array([1, 0, 1, 1, 0], np.int64) if train else np.zeros(B, np.int64)
    perm_in = np.stack([rng.permutation(p_cap) for _ in range(B)]).astype(np.int64)
    perm_gt = np.stack([rng.permutation(g_cap) for _ in range(B)]).astype(np.int64) if sampled_gt else None
    u_mirror = np.array([0.1, 0.3, 0.7, 0.9, 0.5], np.float32) if train else None

    state = {}

    def permutation(n):
        return restrict(state["perms"].pop(0), n)

    monkeypatch.setattr(np.random, "permutation", permutation)
    monkeypatch.setattr(np.random, "uniform", lambda lo, hi: float(state["u"]))
    monkeypatch.setattr(random, "randint", lambda lo, hi: int(state["r"]))
    samples = []
    for b in range(B):
        state["perms"] = [perm_in[b]] + ([perm_gt[b]] if sampled_gt else [])
        state["u"] = u_mirror[b] if train else 0.1                           # (a draw nobody may use outside TRAIN)
        state["r"] = rendering[b]
        samples.append(ds[int(item[b])])
        assert not state["perms"]
    tax, mids, data = C.collate_fn(samples)
    monkeypatch.undo()

    want_p, want_g = reference_gather(dec["partial_points"], dec["partial_offsets"], dec["gt_points"], dec["gt_offsets"], R, p_cap, g_cap,
                                      item, rendering, perm_in, perm_gt, u_mirror, 2.0, N_IN, n_out)
    host_p = data["partial_cloud"].numpy()
    host_g = (2 * data["gtcloud"]).numpy()                                 # CompletionBatches: gt = 2 * data['gtcloud']
    assert host_p.dtype == np.float32 and host_p.shape == (B, N_IN, 3) and host_g.shape == (B, n_out, 3)
    assert np.array_equal(host_p, want_p) and np.array_equal(host_g, want_g)
    assert tax == [dec["taxonomy_ids"][i] for i in item] and mids == [dec["model_ids"][i] for i in item]
    lengths = np.diff(dec["partial_offsets"])
    used = lengths[item * R + rendering]
    assert (used < N_IN).any() and (used > N_IN).any()                     # padded and cut clouds both occur
    for b in range(B):
        assert not want_p[b, min(used[b], N_IN):].any() and want_p[b, :min(used[b], N_IN)].any(axis=1).all()
    if train:
        assert len({mirror_signs(u) for u in u_mirror}) == 4                 # all four mirror cases occur


def test_decode_split_offsets_cache_and_key(tree, tmp_path):
    from cloud_transformers_amd.data import completion as C
    ds = tree["loader"].get_dataset(C.DatasetSubset.TRAIN)
    dec = C.decode_split(ds)
    assert not dec["cached"] and dec["R"] == 2
    assert dec["partial_points"].dtype == np.float32 and dec["gt_points"].dtype == np.float32
    assert dec["partial_offsets"].dtype == np.int64 and dec["partial_offsets"].shape == (3 * 2 + 1,) and dec["gt_offsets"].shape == (4,)
    assert dec["taxonomy_ids"] == ["02691156", "02691156", "03001627"] and dec["model_ids"] == ["a1", "a2", "c1"]
    # make_tree: model k's rendering r holds (N_IN // 2 + 3, N_IN + 40)[(k + r) % 2] rows, ascii and binary files alternate
    assert np.diff(dec["partial_offsets"]).tolist() == [(N_IN // 2 + 3, N_IN + 40)[(k + r) % 2] for k in range(3) for r in range(2)]
    assert np.diff(dec["gt_offsets"]).tolist() == [N_OUT + 76] * 3
    for m, sample in enumerate(ds.file_list):
        for r, path in enumerate(sample["partial_cloud_path"]):
            a, b = dec["partial_offsets"][m * 2 + r:m * 2 + r + 2]
            assert dec["partial_points"][a:b].tobytes() == C.read_pcd(path).tobytes()
        a, b = dec["gt_offsets"][m:m + 2]
        assert dec["gt_points"][a:b].tobytes() == C.read_pcd(sample["gtcloud_path"]).tobytes()

    cache = tmp_path / "cache"
    first = C.decode_split(ds, str(cache))
    again = C.decode_split(ds, str(cache))
    assert not first["cached"] and again["cached"] and again["key"] == first["key"] == dec["key"]
    assert len(os.listdir(str(cache))) == 1
    for k in ("partial_points", "partial_offsets", "gt_points", "gt_offsets"):
        assert again[k].dtype == dec[k].dtype and again[k].tobytes() == dec[k].tobytes(), k
    assert again["taxonomy_ids"] == dec["taxonomy_ids"] and again["model_ids"] == dec["model_ids"]

    tag = C._split_cache_key(ds)[0]
    path = ds.file_list[1]["partial_cloud_path"][1]
    st = os.stat(path)
    os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns + 10 ** 9))
    try:
        assert C._split_cache_key(ds)[1] != dec["key"] and C._split_cache_key(ds)[0] == tag
        touched = C.decode_split(ds, str(cache))
        assert not touched["cached"] and touched["key"] != dec["key"]      # never a stale hit
        assert len(os.listdir(str(cache))) == 1                            # the subset's file is replaced
    finally:
        os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert C._split_cache_key(ds)[1] == dec["key"]
    val = C.decode_split(tree["loader"].get_dataset(C.DatasetSubset.VAL), str(cache))
    assert val["R"] == 1 and val["key"] != dec["key"] and len(os.listdir(str(cache))) == 2


def _resident_cpu(tree, subset):
    from cloud_transformers_amd.data import completion as C
    return C.DeviceShapeNetCompletion(tree["loader"].get_dataset(getattr(C.DatasetSubset, subset)), "cpu")


def test_resident_split_sizes_and_refusals(tree):
    from cloud_transformers_amd.data import completion as C
    tr, te = _resident_cpu(tree, "TRAIN"), _resident_cpu(tree, "TEST")
    assert (tr.M, tr.R, tr.p_cap, tr.g_cap, tr.n_in, tr.n_out, tr.sampled_gt) == (3, 2, N_IN + 40, N_OUT + 76, N_IN, N_OUT, True)
    assert (te.M, te.R, te.g_cap, te.n_in, te.n_out, te.sampled_gt) == (3, 1, N_OUT, N_IN, N_OUT, False)
    assert tr.partial_points.dtype == torch.float32 and tr.partial_offsets.dtype == torch.int64 and len(tr) == 3
    pp = np.zeros((9, 3), np.float32)
    with pytest.raises(ValueError, match="holds 4 points where 5 are expected"):
        C.DeviceShapeNetCompletion.from_arrays(pp[:4], [0, 2, 4], pp, [0, 5, 9], 1, 4, None, "cpu", sampled_gt=False)
    with pytest.raises(ValueError):
        C.DeviceShapeNetCompletion.from_arrays(pp[:4], [0, 2, 4], pp, [0, 5, 9], 2, 4, 8, "cpu")      # partial_offsets is not [M * R + 1]
    with pytest.raises(ValueError, match="65536"):
        big = np.zeros((65537, 3), np.float32)
        C.DeviceShapeNetCompletion.from_arrays(big, [0, 65537], pp, [0, 9], 1, 4, 8, "cpu")


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("train", [False, True])
def test_epoch_order_is_the_distributed_samplers(world, drop_last, train):
    from torch.utils.data.distributed import DistributedSampler
    from cloud_transformers_amd.data import completion as C
    M, batch = 11, 4
    pts = np.ones((M, 3), np.float32)
    ds = C.DeviceShapeNetCompletion.from_arrays(pts, np.arange(M + 1), pts, np.arange(M + 1), 1, 4, 8, "cpu",
                                                taxonomy_ids=["t%d" % (i % 2) for i in range(M)], model_ids=["m%d" % i for i in range(M)])
    seen = []
    for rank in range(world):
        batches = C.DeviceCompletionBatches(ds, batch, train=train, seed=5, rank=rank, world=world, drop_last=drop_last)
        ref = DistributedSampler(range(M), num_replicas=world, rank=rank, shuffle=train, seed=5)
        for epoch in (0, 3):
            batches.set_epoch(epoch)
            ref.set_epoch(epoch)
            want = list(ref)
            n = len(want) // batch if drop_last else -(-len(want) // batch)
            assert len(batches) == n and batches.epoch_order() == want[:n * batch]
        seen.append(batches.epoch_order())
    if world == 2 and not drop_last:
        assert sorted(set(seen[0] + seen[1])) == list(range(M))
    if train:
        assert seen[0] != sorted(seen[0])


MODEL_FILE = "import torch\n\n\nclass Model(torch.nn.Module):\n    def __init__(self):\n        super().__init__()\n        self.w = torch.nn.Parameter(torch.zeros(1))\n"


def _config(tree, root, kind):
    keys = tree["keys"]
    return {"experiment": {"root": str(root / "exp"), "writer_root": str(root / "runs")},
            "data": {"kind": kind, "category_path": keys["category_path"], "partial_path": keys["partial_path"], "gt_path": keys["gt_path"],
                     "n_renders": 2, "input_size": N_IN, "gt_size": N_OUT, "batch_size": 2, "batch_size_val": 2, "seed": 3,
                     "cache_dir": str(root / "cache")},
            "model": {"generator": str(root / "model.py")},
            "train": {"num_epochs": 1, "optimizer": {"type": "Adam", "lr": 1e-4, "betas": [0.9, 0.999], "weight_decay": 0.0}}}


def test_harness_picks_the_device_kind(tree, tmp_path):
    from cloud_transformers_amd import harness as H
    from cloud_transformers_amd.data import completion as C
    from cloud_transformers_amd.train_completion import completion_config
    (tmp_path / "model.py").write_text(MODEL_FILE)
    cfg = completion_config(_config(tree, tmp_path, "shapenet_completion_device"))
    assert cfg["data"]["kind"] == "shapenet_completion_device"
    data = H.make_dataset(cfg, "completion", N_IN)
    assert isinstance(data, C.Dataset) and data.options["shuffle"] and data.options["n_renderings"] == 2
    assert not H.make_dataset(cfg, "completion", N_IN, train=False).options["shuffle"]
    tr = H.Trainer(cfg, "completion", N_IN, device=torch.device("cpu"), make_dirs=False)
    assert tr.protocol.shapenet and tr.protocol.shapenet_device and tr.sampler is None
    assert isinstance(tr.loader, C.DeviceCompletionBatches) and tr.loader.train and tr.loader.drop_last and len(tr.loader) == 1
    assert isinstance(tr.loader.ds, C.DeviceShapeNetCompletion) and (tr.loader.ds.n_in, tr.loader.ds.n_out) == (N_IN, N_OUT)
    assert os.listdir(str(tmp_path / "cache"))                             # data.cache_dir is used
    host = H.Trainer(completion_config(_config(tree, tmp_path, "shapenet_completion")), "completion", N_IN, device=torch.device("cpu"),
                     make_dirs=False)
    assert host.protocol.shapenet and not host.protocol.shapenet_device and isinstance(host.loader, C.CompletionBatches)


def test_unknown_kind_still_raises(tree, tmp_path):
    from cloud_transformers_amd import harness as H
    cfg = _config(tree, tmp_path, "shapenet_completion_resident")
    with pytest.raises(ValueError, match="shapenet_completion_device") as ex:
        H.make_dataset(cfg, "completion", N_IN)
    assert "shapenet_completion_resident" in str(ex.value) and "what3d_device" in str(ex.value)
