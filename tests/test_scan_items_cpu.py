"""The ScanObjectNN classification protocol without a GPU: the numpy restatement of ct_scan_items' contract
(tests/scan_items_ref.py) against the upstream loader's own items (tests/golden/scan_items_reference.npz, written by
tests/golden/gen_scan_items_golden.py); the header's prototype against the ctypes table; the entry point's argument checks;
ScanBatches' epoch order against torch's DistributedSampler; ClassificationMeter against the upstream numpy loop."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.scan_items_ref import golden_draws, scan_items_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scan_items_reference.npz")


@pytest.mark.parametrize("name", ["sub", "full"])
def test_restatement_equals_the_upstream_items(name):
    """The contract in fp32 on the upstream draws cast to fp32, against upstream's float64 arithmetic rounded once to fp32:
    within 1e-6 absolute; mask and label exactly.

    The bound is derived, not measured.  The clouds lie in the unit ball, |d| <= clip = 0.05, so |q| <= 1.05, and |c| + |s| <=
    sqrt(2).  With u = 2^-24 (half an ulp, relative): casting sigma and the draw and rounding sigma * g perturb d by at most
    3u * 0.05; the sum p + d rounds once, u * 1.05; so q carries at most 1.2u * 1.05 < 1.3u.  Through the rotation that error
    is multiplied by |c| + |s| <= 1.42: 1.85u; the casts of c and s add u * |q.x| |c| + u * |q.z| |s| <= 1.49u, the two
    products one rounding each, another 1.49u, the final sum u * 1.49, and upstream's own rounding to fp32 u * 1.49.  Total
    under 7.9u = 4.7e-7 < 5e-7 for x' and z'; y' = q.y has 1.3u + u.  1e-6 leaves a factor of two."""
    gold = np.load(GOLDEN)
    item, perm, rot, jit, N = golden_draws(gold, name)
    pts, mask, label = scan_items_reference(gold["data"], gold["mask"], gold["label"], item, perm, rot, jit, N)
    want = gold["pc_" + name]                                             # [M, N, 3] float32
    assert pts.dtype == np.float32 and pts.shape == (len(item), 3, N) and want.shape == (len(item), N, 3)
    assert np.abs(gold["data"]).max() <= 1.0 + 1e-6 and np.abs(want - gold["data"][:, :N]).max() > 1e-3      # (the items are augmented)
    err = np.abs(pts.transpose(0, 2, 1).astype(np.float64) - want.astype(np.float64)).max()
    print("restatement vs upstream (%s): max abs error %.3g" % (name, err))
    assert err <= 1e-6, err
    assert mask.dtype == np.float32 and np.array_equal(mask, gold["ma_" + name].astype(np.float32))
    assert set(np.unique(mask)) == {0.0, 1.0}
    assert label.dtype == np.int64 and np.array_equal(label, gold["label_" + name])


def test_restatement_without_augmentation_is_a_gather():
    gold = np.load(GOLDEN)
    item = np.array([5, 0, 5, 2], np.int64)
    _, perm, _, _, N = golden_draws(gold, "sub")
    pts, mask, label = scan_items_reference(gold["data"], gold["mask"], gold["label"], item, perm[item], None, None, N)
    for b, g in enumerate(item):
        assert np.array_equal(pts[b].T, gold["data"][g][perm[g, :N]]) and np.array_equal(mask[b], gold["mask"][g][perm[g, :N]])
    assert np.array_equal(label, gold["label"][item])


# ---------------------------------------------------------------------------------------------------------------------
# the boundary
_CTYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "ct_stream_t": ctypes.c_void_p}


def test_header_prototype_matches_the_ctypes_table():
    from cloud_transformers_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cloudct.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+ct_scan_items\s*\(([^)]*)\)\s*;", text)
    assert m, "ct_scan_items is not declared in include/cloudct.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    names = [re.sub(r".*[\s*]", "", p) for p in params]
    assert names == ["data", "mask", "label", "M", "P", "item", "perm", "rot", "jit", "sigma", "clip", "B", "N", "out_points",
                     "out_mask", "out_label", "s"]
    types = [ctypes.c_void_p if "*" in p else _CTYPES[p.rsplit(" ", 1)[0].replace("const ", "")] for p in params]
    res, args = _lib.SIGNATURES["ct_scan_items"]
    assert res is ctypes.c_int and [ctypes.sizeof(a) for a in args] == [ctypes.sizeof(t) for t in types]
    assert [a is ctypes.c_float for a in args] == [t is ctypes.c_float for t in types]
    assert [a is ctypes.c_void_p for a in args] == [t is ctypes.c_void_p for t in types]
    assert "ct_scanitems.hip" in _lib.HIP_SOURCES


def test_scan_items_rejects_bad_arguments():
    """Every CT_EINVAL case returns before anything touches the device (there is none here)."""
    from cloud_transformers_amd import _lib
    _lib.build()
    lib = _lib.load()
    b = ctypes.create_string_buffer(256)
    p = ctypes.cast(b, ctypes.c_void_p)

    def call(*, src=(p, p, p), M=4, P=16, item=p, perm=p, rot=p, jit=p, sigma=0.01, clip=0.05, B=2, N=8, outs=(p, p, p)):
        return lib.ct_scan_items(*src, M, P, item, perm, rot, jit, sigma, clip, B, N, *outs, None)

    for k in range(3):                                                     # every null source and output
        src, outs = [p] * 3, [p] * 3
        src[k] = None
        assert call(src=tuple(src)) == -1, k
        outs[k] = None
        assert call(outs=tuple(outs)) == -1, k
    assert call(item=None) == -1
    assert call(rot=None) == -1 and call(jit=None) == -1                   # half an augmentation
    assert call(N=17) == -1 and call(N=0) == -1 and call(N=-8) == -1       # N > P, N < 1
    assert call(P=_lib.SCAN_P_MAX + 1) == -1 and call(P=0, N=0) == -1
    assert call(B=0) == -1 and call(B=-1) == -1 and call(B=65536) == -1
    assert call(M=0) == -1 and call(M=-3) == -1
    for clip in (0.0, -0.05, float("nan")):
        assert call(clip=clip) == -1, clip
    for sigma in (float("inf"), -float("inf"), float("nan")):
        assert call(sigma=sigma) == -1, sigma
    del b


# ---------------------------------------------------------------------------------------------------------------------
# the epoch's order
class _Host(object):
    """The arrays of a data.datasets.ScanObjectNN."""

    def __init__(self, M, P, seed=0):
        rng = np.random.default_rng(seed)
        self.data = rng.normal(size=(M, P, 3)).astype(np.float32)
        self.mask = (rng.random((M, P)) > 0.5).astype(np.float64)
        self.label = rng.integers(0, 15, size=(M,)).astype(np.int64)


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("train", [False, True])
def test_scan_batches_order_is_the_distributed_samplers(world, drop_last, train):
    from torch.utils.data.distributed import DistributedSampler
    from cloud_transformers_amd.data.scanobjectnn import DeviceScanObjectNN, ScanBatches
    M, B, seed = 23, 4, 5
    ds = DeviceScanObjectNN(_Host(M, 8), "cpu")
    assert len(ds) == M and ds.num_points == 8 and ds.mask.dtype == torch.uint8 and ds.label.dtype == torch.int64
    seen = []
    for rank in range(world):
        batches = ScanBatches(ds, B, train=train, seed=seed, rank=rank, world=world, drop_last=drop_last)
        sampler = DistributedSampler(range(M), num_replicas=world, rank=rank, shuffle=train, seed=seed)
        for epoch in range(2):
            batches.set_epoch(epoch)
            sampler.set_epoch(epoch)
            want = list(sampler)
            shard = len(want)                                              # ceil(M / world): torch pads the shards to equal length
            assert shard == -(-M // world)
            assert len(batches) == (shard // B if drop_last else -(-shard // B))
            assert batches.epoch_order() == (want[:(shard // B) * B] if drop_last else want)
            if epoch == 0:
                seen += want
        if train and world == 1:
            a = batches.epoch_order()
            batches.set_epoch(0)
            assert batches.epoch_order() != a                              # set_epoch reshuffles
            assert drop_last or sorted(batches.epoch_order()) == sorted(a) == list(range(M))
    assert sorted(set(seen)) == list(range(M))                             # the ranks' shards cover the split


def test_device_dataset_refuses_to_launch_on_the_cpu():
    from cloud_transformers_amd.data.scanobjectnn import DeviceScanObjectNN, scan_items
    ds = DeviceScanObjectNN(_Host(4, 8), "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scan_items(ds, torch.zeros(2, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------------------------
# the accuracies
def _upstream_accuracies(batches, n_classes):
    """train_classification.py:162-166, 333-350 on one rank's batches, in numpy."""
    total_correct = total_seen = total_correct_seg = total_seen_seg = 0
    correct_per_label, total_per_label = np.zeros(n_classes), np.zeros(n_classes)
    for class_pred, mask_pred, labels, mask in batches:
        class_pred_np = np.argmax(class_pred.numpy(), axis=1)
        mask_pred_np = (torch.sigmoid(mask_pred[:, 0, 0]) > 0.5).numpy()
        labels_np, mask_np = labels.numpy(), mask.numpy()
        total_correct += np.sum(class_pred_np == labels_np)
        total_seen += labels_np.shape[0]
        for batch_id in range(labels_np.shape[0]):
            correct_per_label[labels_np[batch_id]] += class_pred_np[batch_id] == labels_np[batch_id]
            total_per_label[labels_np[batch_id]] += 1
        total_correct_seg += np.sum(mask_pred_np == mask_np)
        total_seen_seg += mask_np.shape[0] * mask_np.shape[-1]
    with np.errstate(invalid="ignore"):
        per = correct_per_label / total_per_label
    return total_correct / float(total_seen), total_correct_seg / float(total_seen_seg), np.mean(per), per


def _hand_made(n_classes, absent):
    g = torch.Generator().manual_seed(3)
    batches = []
    for B in (5, 3):
        labels = torch.randint(n_classes, (B,), generator=g)
        if absent is not None:
            labels[labels == absent] = (absent + 1) % n_classes
        class_pred = torch.randn(B, n_classes, generator=g)
        class_pred[0, labels[0]] += 10.0                                   # at least one hit per batch
        mask = (torch.rand(B, 7, generator=g) > 0.4).float()
        batches.append((class_pred, torch.randn(B, 1, 1, 7, generator=g), labels, mask))
    return batches


@pytest.mark.parametrize("absent", [None, 2])
def test_classification_meter_equals_the_upstream_loop(absent):
    from cloud_transformers_amd.data.scanobjectnn import ClassificationMeter
    n = 4
    batches = _hand_made(n, absent)
    meter = ClassificationMeter(n)
    for b in batches:
        meter.update(*b)
    got = meter.result()
    cls_acc, seg_acc, m_acc, per = _upstream_accuracies(batches, n)
    assert 0.0 < cls_acc < 1.0 and 0.0 < seg_acc < 1.0
    assert got["cls_acc"] == cls_acc and got["seg_acc"] == seg_acc
    assert len(got["class_acc"]) == n
    if absent is None:
        assert got["class_acc"] == per.tolist() and abs(got["m_acc"] - m_acc) <= 1e-15
    else:                                                                  # 0 / 0 -> NaN upstream, and so is the mean
        assert np.isnan(per[absent]) and np.isnan(m_acc)
        assert np.isnan(got["class_acc"][absent]) and np.isnan(got["m_acc"])
        assert [v for k, v in enumerate(got["class_acc"]) if k != absent] == [v for k, v in enumerate(per.tolist()) if k != absent]


def test_classification_config_fills_the_upstream_constants():
    from cloud_transformers_amd.train_classification import classification_config
    cfg = classification_config({"data": {"path": "a", "path_val": "b", "batch_size": 8}, "train": {"seg_weight": 0.25}})
    d, t = cfg["data"], cfg["train"]
    assert d["kind"] == "scanobjectnn_device" and d["n_classes"] == 15 and d["jitter_sigma"] == 0.01 and d["jitter_clip"] == 0.05
    assert d["seed"] == 0 and d["batch_size_val"] == 8 and "subsample" not in d
    assert t["seg_weight"] == 0.25 and t["val_step"] == 1
