"""The S3DIS block protocol without a GPU: the numpy restatement of ct_block_items' contract (tests/block_items_ref.py) against
the host loader's own items (data.datasets.Indoor3DSemSeg, which tests/golden/datasets_reference_items.npz pins to the upstream
loader) on the loader's replayed draws; the header's prototypes against the ctypes table; the entry points' argument checks;
SegmentationMeter against the upstream formulas; block_draws' reproducibility and stage frequencies; BlockBatches' epoch order
against torch's DistributedSampler."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

from tests.block_items_ref import block_items_reference, replay_loader_draws, seg_confusion_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_dataset(M, P, N, seed, aug=True):
    """A data.datasets.Indoor3DSemSeg over made-up blocks (no files): rows [x, y, z, r, g, b, 3 more], coordinates in
    [-0.5, 1.5], colours in [0, 1], as the stored blocks have them."""
    from cloud_transformers_amd.data import datasets as D
    rng = np.random.default_rng(seed)
    ds = D.Indoor3DSemSeg.__new__(D.Indoor3DSemSeg)
    ds.points = np.concatenate([rng.uniform(-0.5, 1.5, (M, P, 3)), rng.uniform(0.0, 1.0, (M, P, 3)), rng.uniform(0.0, 1.0, (M, P, 3))],
                               axis=2).astype(np.float32)
    ds.labels = rng.integers(0, 13, (M, P)).astype(np.uint8)
    ds.num_points, ds.aug, ds.train, ds.data_precent, ds.test_area = N, aug, True, 1.0, "Area_5"
    return ds


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against the host loader
@pytest.mark.parametrize("N,P,items,all_stages", [(96, 128, 300, True), (4096, 4096, 32, False)])
def test_restatement_equals_the_host_loader(N, P, items, all_stages):
    """Seed numpy's and python's generators, take the host item, restore the states, replay the loader's draws in its order
    and run the fp32 restatement on them.  Labels exactly; xyz within 1e-6 (the loader rotates and scales in float64 and rounds
    once, the contract rounds every operation: coordinates below 2 in magnitude, a handful of roundings of 2^-24 relative
    each); every colour element within 1e-6, or exactly one 8-bit level off — where the loader's float64 HSV round trip and the
    contract's fp32 one land on the two sides of a truncation — and those a share of at most 1e-4.

    Measured (seed 5): N 96: 2 of 86 400 colour elements one level off, none beyond; N 4096: 2 of 393 216, none beyond; xyz
    error <= 4.8e-7."""
    M = 20
    ds = _host_dataset(M, P, N, seed=N)
    np.random.seed(5)
    random.seed(5)
    stages = np.zeros((3, 2), np.int64)
    xyz_err, colour_n, level_off, beyond = 0.0, 0, 0, 0
    for k in range(items):
        idx = (k * 7) % M
        st_np, st_py = np.random.get_state(), random.getstate()
        pts, lab = ds[idx]
        after = (np.random.get_state()[1].copy(), np.random.get_state()[2], random.getstate())
        np.random.set_state(st_np)
        random.setstate(st_py)
        perm, aug, jit, cjit, taken = replay_loader_draws(N)
        assert np.array_equal(np.random.get_state()[1], after[0]) and np.random.get_state()[2] == after[1]      # every draw replayed
        assert random.getstate() == after[2]
        for s, t in enumerate(taken):
            stages[s, int(t)] += 1
        out, out_label = block_items_reference(ds.points[:, :, :6], ds.labels, np.array([idx]), perm[None], aug[None], jit[None],
                                               cjit[None], N)
        assert out.dtype == np.float32 and out.shape == (1, 6, N) and out_label.dtype == np.int64
        assert np.array_equal(out_label[0], lab.numpy())
        want = pts.numpy().astype(np.float64)                              # [N, 6]
        got = out[0].T.astype(np.float64)
        xyz_err = max(xyz_err, float(np.abs(got[:, :3] - want[:, :3]).max()))
        d = np.abs(got[:, 3:] - want[:, 3:])
        off = d > 1e-6
        colour_n += d.size
        level_off += int((off & (np.abs(d - 1 / 255) <= 1e-6)).sum())
        beyond += int((off & (np.abs(d - 1 / 255) > 1e-6)).sum())
    print("N %d: xyz error %.3g; %d of %d colour elements one level off, %d beyond; stages (skipped, taken) %s"
          % (N, xyz_err, level_off, colour_n, beyond, stages.tolist()))
    assert xyz_err <= 1e-6, xyz_err
    assert beyond == 0, beyond
    assert colour_n >= 80000 and level_off <= 1e-4 * colour_n, (level_off, colour_n)
    if all_stages:
        assert (stages > 0).all(), stages.tolist()


def test_restatement_without_augmentation_is_a_gather():
    ds = _host_dataset(4, 16, 12, seed=1)
    item = np.array([3, 0, 3], np.int64)
    perm = np.stack([np.random.default_rng(k).permutation(12) for k in range(3)])
    out, lab = block_items_reference(ds.points[:, :, :6], ds.labels, item, perm, None, None, None, 12)
    for b, g in enumerate(item):
        assert np.array_equal(out[b].T, ds.points[g, perm[b], :6]) and np.array_equal(lab[b], ds.labels[g, perm[b]])
    out, lab = block_items_reference(ds.points[:, :, :6], ds.labels, item, None, None, None, None, 12)
    assert np.array_equal(out[1].T, ds.points[0, :12, :6])


def test_restatement_leaves_a_constant_channel_alone():
    """hi == lo: the stage leaves the channel as it is (the loader divides by zero there); no NaN comes out."""
    ds = _host_dataset(2, 8, 8, seed=2)
    ds.points[0, :, 4] = 0.25
    aug = np.zeros((1, 16), np.float32)
    aug[0, :5], aug[0, 5], aug[0, 12] = [1, 0, 1, 1, 1], 0.5, 1.0
    z = np.zeros((1, 8, 3), np.float32)
    out, _ = block_items_reference(ds.points[:, :, :6], ds.labels, np.array([0]), None, aug, z, z, 8)
    assert np.isfinite(out).all() and np.array_equal(out[0, 4], np.full(8, np.float32(63) / np.float32(255)))


# ---------------------------------------------------------------------------------------------------------------------
# the boundary
_CTYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64, "ct_stream_t": ctypes.c_void_p}
_NAMES = {"ct_block_items": ["data", "label", "M", "P", "item", "perm", "aug", "jit", "cjit", "sigma", "clip", "cstd", "B", "N", "out",
                             "out_label", "s"],
          "ct_seg_confusion": ["pred", "labels", "B", "C", "N", "conf", "s"]}


@pytest.mark.parametrize("symbol", sorted(_NAMES))
def test_header_prototype_matches_the_ctypes_table(symbol):
    from cloud_transformers_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cloudct.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % symbol, text)
    assert m, "%s is not declared in include/cloudct.h" % symbol
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert [re.sub(r".*[\s*]", "", p) for p in params] == _NAMES[symbol]
    types = [ctypes.c_void_p if "*" in p else _CTYPES[p.rsplit(" ", 1)[0].replace("const ", "")] for p in params]
    res, args = _lib.SIGNATURES[symbol]
    assert res is ctypes.c_int and [ctypes.sizeof(a) for a in args] == [ctypes.sizeof(t) for t in types]
    assert [a is ctypes.c_float for a in args] == [t is ctypes.c_float for t in types]
    assert [a is ctypes.c_void_p for a in args] == [t is ctypes.c_void_p for t in types]
    assert "ct_blockitems.hip" in _lib.HIP_SOURCES and _lib.ABI_VERSION == 3


def test_entry_points_reject_bad_arguments():
    """Every CT_EINVAL case returns before anything touches the device (there is none here)."""
    from cloud_transformers_amd import _lib
    _lib.build()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(*, data=p, label=p, M=4, P=16, item=p, perm=p, aug=p, jit=p, cjit=p, sigma=0.01, clip=0.05, cstd=0.05, B=2, N=8, out=p,
             out_label=p):
        return lib.ct_block_items(data, label, M, P, item, perm, aug, jit, cjit, sigma, clip, cstd, B, N, out, out_label, None)

    for k in ("data", "label", "item", "out", "out_label"):
        assert call(**{k: None}) == -1, k
    for k in ("aug", "jit", "cjit"):                                       # a partial augmentation, one and two missing
        assert call(**{k: None}) == -1, k
        assert call(**{j: None for j in ("aug", "jit", "cjit") if j != k}) == -1, k
    assert call(N=17) == -1 and call(N=0) == -1 and call(N=-8) == -1       # N > P, N < 1
    assert call(P=_lib.BLOCK_P_MAX + 1) == -1 and call(P=0, N=0) == -1
    assert call(B=0) == -1 and call(B=-1) == -1 and call(B=65536) == -1
    assert call(M=0) == -1 and call(M=-3) == -1
    for clip in (0.0, -0.05, float("nan")):
        assert call(clip=clip) == -1, clip
    for bad in (float("inf"), -float("inf"), float("nan")):
        assert call(sigma=bad) == -1 and call(cstd=bad) == -1, bad

    def conf(*, pred=p, labels=p, B=2, C=13, N=8, out=p):
        return lib.ct_seg_confusion(pred, labels, B, C, N, out, None)

    assert conf(pred=None) == -1 and conf(labels=None) == -1 and conf(out=None) == -1
    assert conf(C=0) == -1 and conf(C=_lib.CONFUSION_C_MAX + 1) == -1 and conf(B=0) == -1 and conf(N=0) == -1
    assert conf(B=1 << 16, N=1 << 15) == -1                               # B * N = 2^31
    del buf


def test_device_dataset_refuses_to_launch_on_the_cpu():
    from cloud_transformers_amd.data.s3dis_blocks import DeviceS3DISBlocks, SegmentationMeter, block_items
    ds = DeviceS3DISBlocks(_host_dataset(4, 8, 8, seed=0), "cpu")
    assert len(ds) == 4 and ds.num_points == 8 and tuple(ds.data.shape) == (4, 8, 6) and ds.label.dtype == torch.uint8
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        block_items(ds, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SegmentationMeter(13).update(torch.zeros(1, 13, 4), torch.zeros(1, 4, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------------------------
# the metrics
def _upstream_metrics(matrix, names):
    """datasets/S3DIS_tools/iou_util_new.py return_metrics_dict on a float64 confusion matrix (rows truth, columns prediction),
    formula for formula."""
    n = matrix.shape[0]
    metrics = {}
    total = matrix.sum()
    metrics["overall_acc"] = float(np.trace(matrix)) / (total if total != 0 else 1)
    acc = 0
    for i in range(n):
        acc = acc + matrix[i][i] / max(1, np.sum(matrix[i, :]))
    metrics["mean_class_acc"] = acc / n
    ious = []
    for i in range(n):
        wrong_row = sum(matrix[i][j] for j in range(n) if j != i)
        wrong_col = sum(matrix[j][i] for j in range(n) if j != i)
        divisor = matrix[i][i] + wrong_row + wrong_col
        if matrix[i][i] == 0:
            divisor = 1
        ious.append(float(matrix[i][i]) / divisor)
    for i in range(n):
        metrics["iou_" + names[i]] = ious[i]
    seen = ((matrix.sum(1) + matrix.sum(0)) != 0).sum()
    metrics["mean_iou"] = sum(ious) / seen
    return metrics


def _matrices():
    rng = np.random.default_rng(7)
    full = rng.integers(0, 5000, (13, 13))
    absent = full.copy()
    absent[4, :] = 0
    absent[:, 4] = 0                                                       # class 4 neither labelled nor predicted
    never = full.copy()
    never[9, 9] = 0                                                        # class 9 present, never predicted correctly
    return {"random": full, "absent": absent, "never_correct": never}


@pytest.mark.parametrize("which", ["random", "absent", "never_correct"])
def test_segmentation_meter_equals_the_upstream_formulas(which):
    from cloud_transformers_amd.data.s3dis_blocks import CLASS_NAMES, SegmentationMeter
    assert CLASS_NAMES == ("ceiling", "floor", "wall", "beam", "column", "window", "door", "table", "chair", "sofa", "bookcase",
                           "board", "clutter")
    mat = _matrices()[which]
    meter = SegmentationMeter(13)
    meter.conf = torch.from_numpy(mat.astype(np.int64))
    got = meter.result()
    want = _upstream_metrics(mat.astype(np.float64), CLASS_NAMES)
    assert list(got) == list(want) and len(got) == 16
    for k in want:
        assert isinstance(got[k], float) and got[k] == float(want[k]), (k, got[k], want[k])
    if which == "absent":
        assert got["iou_column"] == 0.0 and abs(got["mean_iou"] - sum(got["iou_" + n] for n in CLASS_NAMES) / 12) < 1e-15
    if which == "never_correct":
        assert got["iou_sofa"] == 0.0
    assert 0.0 < got["overall_acc"] < 1.0 and 0.0 < got["mean_class_acc"] < 1.0


def test_segmentation_meter_names_other_class_counts_by_index():
    from cloud_transformers_amd.data.s3dis_blocks import SegmentationMeter
    meter = SegmentationMeter(3)
    assert meter.result()["overall_acc"] == 0.0 and np.isnan(meter.result()["mean_iou"])      # nothing counted yet
    meter.conf = torch.tensor([[2, 0, 0], [1, 1, 0], [0, 0, 0]])
    got = meter.result()
    assert list(got) == ["overall_acc", "mean_class_acc", "iou_0", "iou_1", "iou_2", "mean_iou"]
    assert got["overall_acc"] == 0.75 and got["iou_0"] == 2 / 3 and got["iou_1"] == 0.5 and got["mean_iou"] == (2 / 3 + 0.5) / 2


def test_confusion_restatement_counts_np_argmax():
    pred = np.array([[[0.5, np.nan, 1.0], [0.5, 2.0, 1.0], [0.1, np.nan, 0.0]]], np.float32)      # [1, 3, 3]: a tie, a NaN, a plain point
    conf = seg_confusion_reference(pred, np.array([[0, 2, 7]]))
    assert conf.tolist() == [[1, 0, 0], [0, 0, 0], [1, 0, 0]]              # the tie and the first NaN go to class 0; label 7 is dropped


# ---------------------------------------------------------------------------------------------------------------------
# the draws
def test_block_draws_are_reproducible_and_take_the_stages_at_the_loaders_rates():
    """Equal seeds, equal draws; over 20 000 blocks the auto-contrast is taken in 0.2 +- 0.02 of them, the translation and the
    colour jitter in 0.95 +- 0.01 (binomial standard deviations 0.0028 and 0.0015: the bands are 7 and 6.5 of them)."""
    from cloud_transformers_amd.data.s3dis_blocks import block_draws
    B, N = 20000, 2
    outs = [block_draws(B, N, True, True, "cpu", torch.Generator().manual_seed(4)) for _ in range(2)]
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    other = block_draws(B, N, True, True, "cpu", torch.Generator().manual_seed(5))
    assert not torch.equal(other[1], outs[0][1])
    perm, aug, jit, cjit = outs[0]
    assert perm.dtype == torch.int64 and tuple(perm.shape) == (B, N) and bool((perm.sort(dim=1).values == torch.arange(N)).all())
    assert aug.dtype == torch.float32 and tuple(aug.shape) == (B, 16) and tuple(jit.shape) == tuple(cjit.shape) == (B, N, 3)
    contrast, translation, colour = float((aug[:, 5] >= 0).float().mean()), float(aug[:, 9].mean()), float(aug[:, 10].mean())
    print("stage frequencies over %d draws: auto-contrast %.4f, translation %.4f, colour jitter %.4f" % (B, contrast, translation, colour))
    assert abs(contrast - 0.2) <= 0.02 and abs(translation - 0.95) <= 0.01 and abs(colour - 0.95) <= 0.01
    assert set(aug[:, 9].unique().tolist()) == {0.0, 1.0} and set(aug[:, 10].unique().tolist()) == {0.0, 1.0}
    # the layout of include/cloudct.h and the loader's ranges
    assert float((aug[:, 0] ** 2 + aug[:, 1] ** 2 - 1).abs().max()) < 1e-6
    assert float(aug[:, 2].abs().min()) >= 0.8 and float(aug[:, 2:5].abs().max()) <= 1.2 and float(aug[:, 3:5].min()) >= 0.8
    assert abs(float((aug[:, 2] < 0).float().mean()) - 0.5) < 0.02        # the mirror's sign rides on x
    w = aug[:, 5][aug[:, 5] >= 0]
    assert float(w.max()) < 1.0 and bool((aug[:, 5][aug[:, 5] < 0] == -1).all())
    assert float(aug[:, 6:9].abs().max()) <= 0.1 and bool((aug[:, 6:9][aug[:, 9] == 0] == 0).all())
    assert float(aug[:, 11].abs().max()) <= 0.5 and float((aug[:, 12] - 1).abs().max()) <= 0.2 + 1e-6
    assert bool((aug[:, 13:] == 0).all())
    # validation, or aug off: the shuffle alone, from the same first draw
    for train, use_aug in ((False, True), (True, False), (False, False)):
        p2, a2, j2, c2 = block_draws(B, N, train, use_aug, "cpu", torch.Generator().manual_seed(4))
        assert a2 is None and j2 is None and c2 is None and torch.equal(p2, perm)


# ---------------------------------------------------------------------------------------------------------------------
# the epoch's order
@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("train", [False, True])
def test_block_batches_order_is_the_distributed_samplers(world, drop_last, train):
    from torch.utils.data.distributed import DistributedSampler
    from cloud_transformers_amd.data.s3dis_blocks import BlockBatches, DeviceS3DISBlocks
    M, B, seed = 23, 4, 5
    ds = DeviceS3DISBlocks(_host_dataset(M, 8, 8, seed=3), "cpu")
    seen = []
    for rank in range(world):
        batches = BlockBatches(ds, B, train=train, seed=seed, rank=rank, world=world, drop_last=drop_last)
        sampler = DistributedSampler(range(M), num_replicas=world, rank=rank, shuffle=train, seed=seed)
        for epoch in range(2):
            batches.set_epoch(epoch)
            sampler.set_epoch(epoch)
            want = list(sampler)
            shard = len(want)
            assert shard == -(-M // world)
            assert len(batches) == (shard // B if drop_last else -(-shard // B))
            assert batches.epoch_order() == (want[:(shard // B) * B] if drop_last else want)
            if epoch == 0:
                seen += want
    assert sorted(set(seen)) == list(range(M))


def test_data_percent_cuts_the_epoch_as_the_host_dataset_does():
    from cloud_transformers_amd.data.s3dis_blocks import BlockBatches, DeviceS3DISBlocks
    host = _host_dataset(23, 8, 8, seed=3)
    host.data_precent = 0.5
    assert len(host) == 11
    ds = DeviceS3DISBlocks(host, "cpu")
    assert len(ds) == 23 and ds.length == 11
    assert sorted(BlockBatches(ds, 4, train=True).epoch_order()) == list(range(11))           # the host dataset's own cut
    assert sorted(BlockBatches(ds, 4, train=True, data_percent=0.3).epoch_order()) == list(range(6))     # int(23 * 0.3)
    assert len(BlockBatches(ds, 4, data_percent=1.0)) == 6


def test_segmentation_config_fills_the_upstream_constants():
    from cloud_transformers_amd.train_segmentation import segmentation_config
    cfg = segmentation_config({"data": {"path": "a", "batch_size": 8, "num_points": 4096, "data_percent": 0.5, "aug": True},
                               "train": {"val_step": 2}})
    d, t = cfg["data"], cfg["train"]
    assert d["kind"] == "s3dis_device" and d["n_classes"] == 13 and d["seed"] == 0 and d["jitter_sigma"] == 0.01 and d["jitter_clip"] == 0.05
    assert d["color_jitter_std"] == 0.05 and d["color_shift_ratio"] == 0.1 and d["hue_max"] == 0.5 and d["saturation_max"] == 0.2
    assert d["data_percent"] == 0.5 and d["aug"] is True and d["batch_size_val"] == 8 and d["test_area"] == "Area_5"
    assert t["val_step"] == 2 and "save_each" not in t
