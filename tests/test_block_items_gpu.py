"""ct_block_items and ct_seg_confusion on the device (cloud_transformers_amd.data.s3dis_blocks): equal, bit for bit, to the numpy
restatement of the entry points' contracts (tests/block_items_ref.py, whose agreement with the host loader's items is settled
in tests/test_block_items_cpu.py) over the sizes at which the kernels take another path; the argument checks; the public
functions without device-to-host synchronisation; the epoch's order; a training step, eager and from a HIP graph, a validation
and `train_segmentation --eval` on a tiny file set."""
import json
import os

import numpy as np
import pytest
import torch

from tests.block_items_ref import block_items_reference, seg_confusion_reference

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
M = 5


class Host(object):
    """The arrays of a data.datasets.Indoor3DSemSeg: M blocks of P points [x, y, z, r, g, b, 3 more], coordinates in [-0.5, 1.5],
    colours in [0, 1].  Block 2 has a constant green channel (inside its first point already: every pool sees it), block 0
    starts with a grey point, block 1 with a black one and, when there is room, ends its pool candidates with a white one."""

    def __init__(self, M, P, seed=0):
        rng = np.random.default_rng(seed)
        self.points = np.concatenate([rng.uniform(-0.5, 1.5, (M, P, 3)), rng.uniform(0.0, 1.0, (M, P, 6))], axis=2).astype(np.float32)
        self.points[2 % M, :, 4] = 0.375
        self.points[0, 0, 3:6] = 0.5
        self.points[1 % M, 0, 3:6] = 0.0
        if P > 1:
            self.points[1 % M, 1, 3:6] = 1.0
        self.labels = rng.integers(0, 13, (M, P)).astype(np.uint8)

    def __len__(self):
        return self.points.shape[0]


_DATASETS = {}


def dataset(M, P):
    """(host arrays, DeviceS3DISBlocks), made once per size and left unchanged."""
    from cloud_transformers_amd.data.s3dis_blocks import DeviceS3DISBlocks
    if (M, P) not in _DATASETS:
        host = Host(M, P, seed=P)
        _DATASETS[(M, P)] = (host, DeviceS3DISBlocks(host, DEV))
    return _DATASETS[(M, P)]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what):
    g, w = got[0].cpu().numpy(), want[0]
    assert g.shape == w.shape and g.dtype == np.float32, (what, g.shape, w.shape)
    bad = np.argwhere(bits(g) != bits(w))
    assert bad.size == 0, "%s: points differ at %d places, first %s: got %r want %r" % (
        what, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    assert got[1].dtype == torch.int64 and np.array_equal(got[1].cpu().numpy(), want[1]), (what, "labels")


def draws(B, N, with_perm, with_aug, seed):
    """Explicit draws in the loader's ranges.  Row b takes the three optional stages by the bits of (b + seed) % 8, so B = 8 has
    every combination and the smaller batches a few that move with the seed; every fifth jitter draw lies beyond clip / sigma."""
    rng = np.random.default_rng(seed)
    perm = np.stack([rng.permutation(N) for _ in range(B)]).astype(np.int64) if with_perm else None
    if not with_aug:
        return perm, None, None, None
    aug = np.zeros((B, 16), np.float64)
    angle = rng.uniform(0, 2 * np.pi, B)
    aug[:, 0], aug[:, 1] = np.cos(angle), np.sin(angle)
    aug[:, 2:5] = rng.uniform(0.8, 1.2, (B, 3))
    aug[:, 2] *= np.where(rng.random(B) < 0.5, -1.0, 1.0)
    combo = (np.arange(B) + seed) % 8
    aug[:, 5] = np.where(combo & 1, rng.random(B), -1.0)
    aug[:, 9] = (combo >> 1) & 1
    aug[:, 6:9] = (rng.random((B, 3)) - 0.5) * 0.2 * aug[:, 9:10]
    aug[:, 10] = (combo >> 2) & 1
    aug[:, 11] = (rng.random(B) - 0.5)
    aug[:, 12] = 1 + (rng.random(B) - 0.5) * 0.4
    jit = rng.normal(size=(B, N, 3)).astype(np.float32)
    jit.reshape(-1)[::5] *= 8.0                                           # beyond clip / sigma = 5: both clip branches
    cjit = rng.normal(size=(B, N, 3)).astype(np.float32)
    return perm, aug.astype(np.float32), jit, cjit


ITEMS = {1: [M - 1], 3: [0, M - 1, 0], 8: [0, M - 1, 2, 2, 1, 3, M - 1, 0]}      # repeats, the first and the last block
NS = [1, 3, 4, 5, 63, 64, 65, 257, 4096]
SHAPES = [(n, p) for n in NS for p in (n, n + 1)]


# ---------------------------------------------------------------------------------------------------------------------
# the contract over the shapes
@pytest.mark.parametrize("N,P", SHAPES)
def test_equals_the_contract_bit_for_bit(N, P):
    """B 1, 3 and 8; perm NULL and given; augmentation off and on, every optional stage taken and skipped (B 8: all eight
    combinations).  N % 4 == 0 takes the four-slot path, every other N one slot per work-item; N = 257 needs two workgroups per
    block on the scalar path, N = 4096 four on the vector path (each recomputes the auto-contrast's bounds).  Block 2 has a
    constant channel, N = 1 is one by construction; blocks 0 and 1 hold a grey, a black and a white point."""
    from cloud_transformers_amd.data.s3dis_blocks import block_items_from_draws
    host, ds = dataset(M, P)
    for B, item in ITEMS.items():
        item = np.asarray(item, np.int64)
        for with_perm in (False, True):
            for with_aug in (False, True):
                perm, aug, jit, cjit = draws(B, N, with_perm, with_aug, seed=N * 7 + P + B)
                want = block_items_reference(host.points[:, :, :6], host.labels, item, perm, aug, jit, cjit, N)
                got = block_items_from_draws(ds, dev(item), dev(perm), dev(aug), dev(jit), dev(cjit), N)
                assert_same(got, want, "N %d P %d B %d perm %d aug %d" % (N, P, B, with_perm, with_aug))
                if with_aug:
                    assert np.isfinite(want[0]).all()


@pytest.mark.parametrize("N,P", [(64, 64), (4096, 4096), (64, 65)])
@pytest.mark.parametrize("which", ["out", "labels", "jit", "cjit"])
def test_unaligned_buffers_take_the_scalar_path(N, P, which):
    """An output or a jitter that starts one float (the labels: one int64) past a 16-byte boundary: N % 4 == 0, but the rows are
    not 16-byte addressable, so the launch goes one slot per work-item — the same bits, and nothing around the views is
    touched."""
    from cloud_transformers_amd.data.s3dis_blocks import block_items_from_draws
    host, ds = dataset(M, P)
    B = 3
    item = np.asarray(ITEMS[B], np.int64)
    perm, aug, jit, cjit = draws(B, N, True, True, seed=N + P)
    want = block_items_reference(host.points[:, :, :6], host.labels, item, perm, aug, jit, cjit, N)
    big_o = torch.full((B * 6 * N + 8,), 7.0, device=DEV)
    big_l = torch.full((B * N + 8,), -7, dtype=torch.int64, device=DEV)
    big_j = torch.zeros(B * N * 3 + 8, device=DEV)
    big_c = torch.zeros(B * N * 3 + 8, device=DEV)
    oo, ol, oj, oc = (1 if which == w else 0 for w in ("out", "labels", "jit", "cjit"))
    assert all(t.data_ptr() % 16 == 0 for t in (big_o, big_l, big_j, big_c))
    out, labels = big_o[oo:oo + B * 6 * N].view(B, 6, N), big_l[ol:ol + B * N].view(B, N)
    j, c = big_j[oj:oj + B * N * 3].view(B, N, 3), big_c[oc:oc + B * N * 3].view(B, N, 3)
    j.copy_(dev(jit))
    c.copy_(dev(cjit))
    for t, name in ((out, "out"), (labels, "labels"), (j, "jit"), (c, "cjit")):
        assert (t.data_ptr() % 16 != 0) == (which == name)
    got = block_items_from_draws(ds, dev(item), dev(perm), dev(aug), j, c, N, out=(out, labels))
    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == labels.data_ptr()
    assert_same(got, want, "offset " + which)
    assert bool((torch.cat([big_o[:oo], big_o[oo + B * 6 * N:]]) == 7.0).all())
    assert bool((torch.cat([big_l[:ol], big_l[ol + B * N:]]) == -7).all())


def test_bad_arguments_launch_nothing():
    """A partial augmentation, N > P, clip <= 0 and each null pointer: CT_EINVAL, and the outputs keep their contents."""
    from cloud_transformers_amd import _lib
    from cloud_transformers_amd.data.s3dis_blocks import block_items_from_draws
    lib = _lib.load()
    host, ds = dataset(M, 64)
    B, N, P = 2, 32, 64
    item = dev(np.array([0, 1], np.int64))
    perm, aug, jit, cjit = (dev(a) for a in draws(B, N, True, True, seed=1))
    out = torch.full((B, 6, N), 7.0, device=DEV)
    labels = torch.full((B, N), -7, dtype=torch.int64, device=DEV)
    good = dict(data=ds.data.data_ptr(), label=ds.label.data_ptr(), M=M, P=P, item=item.data_ptr(), perm=perm.data_ptr(),
                aug=aug.data_ptr(), jit=jit.data_ptr(), cjit=cjit.data_ptr(), sigma=0.01, clip=0.05, cstd=0.05, B=B, N=N,
                out=out.data_ptr(), out_label=labels.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.ct_block_items(*[a[k] for k in good], None)

    for k in ("aug", "jit", "cjit"):
        assert call(**{k: None}) == -1, k
        assert call(**{j: None for j in ("aug", "jit", "cjit") if j != k}) == -1, k
    assert call(N=P + 1) == -1
    assert call(clip=0.0) == -1 and call(clip=-0.05) == -1
    for k in ("data", "label", "item", "out", "out_label"):
        assert call(**{k: None}) == -1, k
    conf = torch.full((13 * 13,), 5, dtype=torch.int64, device=DEV)
    pred, lab = torch.zeros(1, 13, 8, device=DEV), torch.zeros(1, 8, dtype=torch.int64, device=DEV)
    assert lib.ct_seg_confusion(None, lab.data_ptr(), 1, 13, 8, conf.data_ptr(), None) == -1
    assert lib.ct_seg_confusion(pred.data_ptr(), None, 1, 13, 8, conf.data_ptr(), None) == -1
    assert lib.ct_seg_confusion(pred.data_ptr(), lab.data_ptr(), 1, 13, 8, None, None) == -1
    assert lib.ct_seg_confusion(pred.data_ptr(), lab.data_ptr(), 1, 65, 8, conf.data_ptr(), None) == -1
    assert lib.ct_seg_confusion(pred.data_ptr(), lab.data_ptr(), 1, 0, 8, conf.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((labels == -7).all()) and bool((conf == 5).all())
    with pytest.raises(ValueError):
        block_items_from_draws(ds, item, perm, aug, None, cjit, N)
    assert call() == 0                                                     # and the same arguments unbroken do launch
    assert call(perm=None) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any()) and np.array_equal(labels.cpu().numpy(), host.labels[:2, :N].astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# the confusion matrix
@pytest.mark.parametrize("C", [1, 2, 13, 20, 64])
def test_confusion_equals_numpy(C):
    """B 1 and 3, N from one point to several workgroups; predictions on a grid of halves, so that ties occur (the first index
    wins); a class that is NaN at every other point, and class 0 NaN as well at a few (the first NaN wins); labels below and
    above the range are not counted; a second call adds into the same matrix."""
    from cloud_transformers_amd.data.s3dis_blocks import SegmentationMeter
    for B in (1, 3):
        for N in (1, 63, 64, 65, 257, 4096):
            rng = np.random.default_rng(C * 131 + B * 17 + N)
            calls, want = [], None
            for _ in range(2):
                pred = (np.round(rng.normal(size=(B, C, N)) * 2) / 2).astype(np.float32)
                pred[0, C // 2, ::2] = np.nan
                pred[B - 1, 0, ::7] = np.nan
                labels = rng.integers(0, C, (B, N)).astype(np.int64)
                labels.reshape(-1)[::11] = -1
                labels.reshape(-1)[5::13] = C
                labels.reshape(-1)[3::17] = 1 << 40
                want = seg_confusion_reference(pred, labels, want)
                calls.append((pred, labels))
            if C > 1 and N >= 63:
                top = np.sort(calls[0][0], axis=1)
                assert (top[:, -1] == top[:, -2]).any()                    # ties are present
            meter = SegmentationMeter(C)
            for pred, labels in calls:
                meter.update(dev(pred), dev(labels))
            got = meter.conf.cpu().numpy()
            assert got.dtype == np.int64 and np.array_equal(got, want), (B, C, N, np.argwhere(got != want)[:4].tolist())
            assert 0 < want.sum() < 2 * B * N or N == 1
    # the model's [B, C, 1, N] output is taken as it is
    meter4 = SegmentationMeter(C)
    meter4.update(dev(calls[0][0])[:, :, None], dev(calls[0][1]))
    assert np.array_equal(meter4.conf.cpu().numpy(), seg_confusion_reference(*calls[0]))


# ---------------------------------------------------------------------------------------------------------------------
# the public functions
def test_block_items_public_function():
    from cloud_transformers_amd.data.s3dis_blocks import block_items
    host, ds = dataset(M, 4096)
    idx = ITEMS[8]
    item = dev(np.asarray(idx, np.int64))
    for N in (4096, 1024):
        outs = [block_items(ds, item, N, True, True, torch.Generator(device=DEV).manual_seed(11)) for _ in range(2)]
        for a, b in zip(*outs):
            assert torch.equal(a, b)                                       # equally seeded generators: equal bits
        other = block_items(ds, item, N, True, True, torch.Generator(device=DEV).manual_seed(12))
        assert not torch.equal(other[0], outs[0][0])
        points, labels = outs[0]
        assert tuple(points.shape) == (8, 6, N) and tuple(labels.shape) == (8, N) and labels.dtype == torch.int64
        assert tuple(points[:, :, None].shape) == (8, 6, 1, N) and points[:, :, None].is_contiguous()
        assert bool(torch.isfinite(points).all()) and float(points[:, 3:].min()) >= 0.0 and float(points[:, 3:].max()) <= 1.0
        levels = points[:, 3:] * 255
        assert float((levels - levels.round()).abs().max()) < 1e-4         # colours come out on the 8-bit levels
        # validation: the block's first N points, shuffled, nothing else
        points, labels = block_items(ds, item, N, False, True, torch.Generator(device=DEV).manual_seed(0))
        for b, g in enumerate(idx[:3]):
            got = np.ascontiguousarray(points[b].t().cpu().numpy())
            rows = {r.tobytes(): k for k, r in enumerate(host.points[g, :N, :6])}
            picked = [rows[r.tobytes()] for r in got]
            assert sorted(picked) == list(range(N)) and picked != list(range(N))
            assert np.array_equal(labels[b].cpu().numpy(), host.labels[g][picked].astype(np.int64))


def test_items_and_an_epoch_do_not_synchronise():
    """No device-to-host synchronisation in block_items (draws, argsort, stage choices, launch), in a BlockBatches epoch nor in
    SegmentationMeter.update: under torch's sync debug mode set to "error" a synchronising call raises — checked first on
    `.item()`, so that the mode is known to be live."""
    from cloud_transformers_amd.data.s3dis_blocks import BlockBatches, SegmentationMeter, block_items
    host, ds = dataset(M, 4096)
    item = dev(np.asarray(ITEMS[8], np.int64))
    gen = torch.Generator(device=DEV).manual_seed(0)
    block_items(ds, item, 1024, True, True, gen)                           # (library load, allocator warm-up)
    batches = BlockBatches(ds, 2, num_points=1024, train=True, aug=True, seed=3)
    list(batches)
    meter = SegmentationMeter(13)
    pred = torch.randn(8, 13, 1, 1024, device=DEV)
    meter.update(pred, torch.zeros(8, 1024, dtype=torch.int64, device=DEV))
    probe = ds.data.sum()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        points, labels = block_items(ds, item, 1024, True, True, gen)
        meter.update(pred, labels)
        batches.set_epoch(1)
        epoch = [(p, l, batches.last_items) for p, l in batches]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(points.shape) == (8, 6, 1024) and int(meter.conf.sum()) == 2 * 8 * 1024
    assert len(epoch) == 3 and [tuple(e[0].shape) for e in epoch] == [(2, 6, 1, 1024), (2, 6, 1, 1024), (1, 6, 1, 1024)]
    assert all(e[0].is_cuda and e[1].dtype == torch.int64 and tuple(e[1].shape) == (e[0].shape[0], 1024) for e in epoch)


@pytest.mark.parametrize("world", [1, 2])
def test_an_epoch_visits_the_distributed_samplers_order(world):
    from torch.utils.data.distributed import DistributedSampler
    from cloud_transformers_amd.data.s3dis_blocks import BlockBatches, DeviceS3DISBlocks
    n = 22
    host = Host(n, 16, seed=9)
    host.labels[:] = np.arange(n, dtype=np.uint8)[:, None]                 # the label names the block
    ds = DeviceS3DISBlocks(host, DEV)
    for rank in range(world):
        batches = BlockBatches(ds, 4, train=True, aug=True, seed=2, rank=rank, world=world)
        sampler = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=True, seed=2)
        for epoch in range(2):
            batches.set_epoch(epoch)
            sampler.set_epoch(epoch)
            got, named = [], []
            for pcd, labels in batches:
                assert tuple(pcd.shape[1:]) == (6, 1, 16) and tuple(labels.shape) == (pcd.shape[0], 16)
                assert bool((labels == labels[:, :1]).all())
                got += batches.last_items.tolist()
                named += labels[:, 0].tolist()
            assert got == named == list(sampler)                           # torch's order, every index of the shard
            assert len(got) == n // world and len(set(got)) == len(got)    # ... once (22 blocks: no padding at world 1 and 2)


# ---------------------------------------------------------------------------------------------------------------------
# harness and entry point
CONFIG = '''
experiment:
    root: '{root}/exp'
    writer_root: '{root}/runs'
data:
    path: '{root}/blocks'
    batch_size: 2
    batch_size_val: 3
    num_workers: 0
    num_points: 128
    test_area: 'Area_5'
    data_percent: !!float 1.0
    aug: True
model:
    generator: '{root}/segmenter.py'
    n_classes: 13
train:
    num_epochs: 1
    save_each: 1000
    save_each_epoch: 10
    val_step: 1
    optimizer:
        type: 'Adam'
        lr: !!float 1e-3
        betas: [!!float 0.9, !!float 0.999]
        weight_decay: !!float 0
    scheduler:
        type: 'StepLR'
        gamma: !!float 0.7
        step_size: 2
{restore}
'''

MODEL = '''
import torch
from torch import nn


class Model(nn.Module):
    """A per-point stem and head: the segmenter's interface (cloud [B, 6, 1, N] -> (pred [B, n_classes, 1, N], lattice stats))."""

    def __init__(self, n_classes=13):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv1d(6, 16, kernel_size=1, bias=False), nn.ReLU(inplace=True))
        self.head = nn.Conv1d(16, n_classes, kernel_size=1)

    def forward(self, cloud):
        return self.head(self.stem(cloud.squeeze(2))).unsqueeze(2), []
'''


def write_blocks(root, P=128):
    """indoor3d_sem_seg_hdf5_data in miniature (the .npz twins of two shards): 10 blocks of P points, 6 of Area_1, 4 of Area_5."""
    d = os.path.join(str(root), "blocks")
    os.makedirs(d)
    rng = np.random.default_rng(0)
    rooms = ["Area_1_office_1"] * 3 + ["Area_5_hall_2"] * 2 + ["Area_1_office_2"] * 3 + ["Area_5_hall_3"] * 2
    with open(os.path.join(d, "all_files.txt"), "w") as f:
        f.write("indoor3d_sem_seg_hdf5_data/ply_data_all_0.h5\nindoor3d_sem_seg_hdf5_data/ply_data_all_1.h5\n")
    with open(os.path.join(d, "room_filelist.txt"), "w") as f:
        f.write("\n".join(rooms) + "\n")
    for k in range(2):
        label = rng.integers(0, 13, (5, P)).astype(np.uint8)
        data = np.concatenate([rng.uniform(-0.5, 1.5, (5, P, 3)), rng.uniform(0, 1, (5, P, 6))], axis=2).astype(np.float32)
        data[:, :, 3] = label / 13.0 * 0.8 + 0.2 * data[:, :, 3]          # the colour tells something about the label
        np.savez(os.path.join(d, "ply_data_all_%d.npz" % k), data=data, label=label)


def expected_loss(model, batch):
    with torch.no_grad():
        return float(torch.nn.functional.cross_entropy(model(batch[0])[0][:, :, 0], batch[1]))


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """A Trainer on the tiny file set after one eager step, one step through fit(), one HIP-graph step, a checkpoint and two
    validations (before the second the validation loader's generator state is kept, so that a test can replay its batches)."""
    from cloud_transformers_amd import harness as H
    root = tmp_path_factory.mktemp("blocks")
    write_blocks(root)
    (root / "segmenter.py").write_text(MODEL)
    cfg_path = root / "s3dis.yaml"
    cfg_path.write_text(CONFIG.format(root=str(root), restore=""))
    torch.manual_seed(0)
    cfg = H.load_config(cfg_path)
    cfg["data"]["kind"] = "s3dis_device"
    tr = H.Trainer(cfg, "segmentation", n_classes=13, device=DEV)          # (data.kind selects the task)
    res = {"root": root, "trainer": tr, "steps": []}
    it = iter(tr.loader)
    batch = next(it)
    want = expected_loss(tr.model, batch)
    res["steps"].append((float(tr._eager_step(batch)), want))
    res["conf_eager"] = (tr.protocol.train_meter.conf.clone(), tr.protocol.out.detach().clone(), batch[1].clone())
    res["hist"] = tr.fit(max_iters=1, hip_graph=False)
    tr._graphs = {}                                                        # (what fit(hip_graph=True) starts from)
    before = tr.protocol.train_meter.conf.clone()
    batch = next(it)
    want = expected_loss(tr.model, batch)
    res["steps"].append((float(tr._graph_step(batch)), want))
    (rec,) = tr._graphs.values()                                           # (the captured step's prediction is in its record)
    res["conf_graph"] = (tr.protocol.train_meter.conf - before, rec[4].detach().clone(), batch[1].clone())
    tr.save()
    tr.validate(epoch=0)
    res["val_state"] = tr.val_loader.generator.get_state()
    res["records"] = tr.validate(epoch=1)
    return res


def test_trainer_steps_eagerly_and_from_a_graph(trained):
    """The loss of a step is the CE of the batch it was given, recomputed in torch from the model before the step (the stem and
    the head run on the split-f16 pointwise kernel in both, so the two agree to fp32 rounding of the loss: 1e-5 relative); the
    train confusion matrix took the step's own predictions, from the graph's static tensors too."""
    from cloud_transformers_amd.data.s3dis_blocks import BlockBatches
    tr = trained["trainer"]
    assert tr.task == "segmentation_blocks" and isinstance(tr.loader, BlockBatches) and len(tr.loader) == 3      # 6 blocks, batch 2
    assert tr.loader.aug and tr.loader.N == 128 and tr.cfg["data"]["jitter_sigma"] == 0.01 and tr.cfg["data"]["seed"] == 0
    for (got, want), name in zip(trained["steps"], ("eager", "hip_graph")):
        print("%s step: loss %.7f, recomputed %.7f" % (name, got, want))
        assert np.isfinite(got) and abs(got - want) <= 1e-5 * abs(want), (name, got, want)
    assert trained["steps"][0][0] != trained["steps"][1][0]
    assert len(tr._graphs) == 1 and all(rec is not False for rec in tr._graphs.values())      # captured, not the eager way out
    assert len(trained["hist"]) == 1 and np.isfinite(trained["hist"][0])
    assert tr.scheduler.last_epoch == 1                                    # stepped per iteration (by fit)
    for name in ("conf_eager", "conf_graph"):
        conf, pred, labels = trained[name]
        want = seg_confusion_reference(pred[:, :, 0].cpu().numpy(), labels.cpu().numpy())
        assert int(conf.sum()) == 2 * 128 and np.array_equal(conf.cpu().numpy(), want), name
    assert (tr.exp_dir / ("generator_iter_%d.t7" % tr.iters)).exists() and (tr.exp_dir / ("g_opt_iter_%d.t7" % tr.iters)).exists()


def test_validation_record(trained):
    """The record against the same batches replayed (the loader's generator put back), metrics recomputed on the host from the
    model's outputs with the upstream formulas, the loss as the mean of the batches' CE."""
    from tests.test_block_items_cpu import _upstream_metrics
    from cloud_transformers_amd.data.s3dis_blocks import CLASS_NAMES
    tr, records = trained["trainer"], trained["records"]
    assert len(records) == 1
    rec = records[0]
    model = tr.model.eval()
    tr.val_loader.generator.set_state(trained["val_state"])
    tr.val_loader.set_epoch(1)
    conf, losses, blocks = np.zeros((13, 13), np.int64), [], 0
    with torch.no_grad():
        for pcd, labels in tr.val_loader:
            pred = model(pcd)[0][:, :, 0]
            losses.append(float(torch.nn.functional.cross_entropy(pred, labels)))
            conf = seg_confusion_reference(pred.cpu().numpy(), labels.cpu().numpy(), conf)
            blocks += pcd.shape[0]
    model.train()
    assert blocks == 4 and rec["batches"] == 2 and rec["epoch"] == 1 and conf.sum() == 4 * 128
    want = _upstream_metrics(conf.astype(np.float64), CLASS_NAMES)
    for k, v in want.items():
        assert rec[k] == float(v), (k, rec[k], v)
    assert abs(rec["loss"] - np.mean(losses)) <= 1e-6 * abs(np.mean(losses)), (rec["loss"], np.mean(losses))
    assert list(rec) == ["epoch", "iters", "batches", "loss"] + list(want)
    lines = (tr.exp_dir / "segmentation_val.jsonl").read_text().splitlines()
    assert len(lines) == 2 and json.loads(lines[1]) == json.loads(json.dumps(rec)) and json.loads(lines[0])["epoch"] == 0


def test_eval_entry_point_reproduces_the_record(trained, capsys):
    from cloud_transformers_amd import train_segmentation
    root, tr, rec = trained["root"], trained["trainer"], trained["records"][0]
    cfg_path = root / "s3dis_eval.yaml"
    restore = "restore:\n    generator: '%s'\n" % (tr.exp_dir / ("generator_iter_%d.t7" % tr.iters))
    cfg_path.write_text(CONFIG.format(root=str(root), restore=restore))   # (no data.kind: filled in)
    got = train_segmentation.main(["evalrun", "-c", str(cfg_path), "--eval"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["mean_iou"] == got["mean_iou"]
    assert got["epoch"] == "eval" and got["batches"] == rec["batches"]
    for k in rec:
        if k not in ("epoch", "iters", "loss"):
            assert got[k] == rec[k], k                                     # (the points' order differs: the counts do not)
    assert abs(got["loss"] - rec["loss"]) <= 1e-6 * abs(rec["loss"]), (got["loss"], rec["loss"])


def test_fit_reports_the_train_confusion_and_validates(tmp_path):
    """One epoch through fit() with train.hip_graph: three graph steps, the epoch's train metrics over all 6 * 128 points, one
    validation record and the per-iteration checkpoint."""
    from cloud_transformers_amd import harness as H
    write_blocks(tmp_path)
    (tmp_path / "segmenter.py").write_text(MODEL)
    cfg_path = tmp_path / "s3dis.yaml"
    cfg_path.write_text(CONFIG.format(root=str(tmp_path), restore="").replace("save_each: 1000", "save_each: 2\n    hip_graph: True"))
    tr = H.Trainer(H.load_config(cfg_path), "segmentation_blocks", n_classes=13, device=DEV)
    hist = tr.fit()
    assert len(hist) == 3 and np.isfinite(hist).all() and tr.iters == 3
    assert len(tr._graphs) == 1 and all(rec is not False for rec in tr._graphs.values())
    assert len(tr.protocol.train_records) == 1 and tr.protocol.train_records[0]["epoch"] == 0 and 0.0 <= tr.protocol.train_records[0]["overall_acc"] <= 1.0
    assert int(tr.protocol.train_meter.conf.sum()) == 0                             # started anew for the next epoch
    assert len(tr.val_records) == 1 and (tr.exp_dir / "segmentation_val.jsonl").exists()
    assert (tr.exp_dir / "generator_iter_2.t7").exists() and not (tr.exp_dir / "generator_iter_3.t7").exists()
