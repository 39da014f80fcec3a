"""ct_scan_items on the device (cloud_transformers_amd.data.scanobjectnn): equal, bit for bit, to the numpy restatement of
the entry point's contract (tests/scan_items_ref.py, whose agreement with the upstream loader's items is settled in
tests/test_scan_items_cpu.py) over the sizes at which the kernel takes another path; the argument checks; the upstream
loader's items on its own draws; the public functions without device-to-host synchronisation; a training step, eager and
from a HIP graph, a validation and `train_classification --eval` on a tiny file pair."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests.scan_items_ref import golden_draws, scan_items_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scan_items_reference.npz")
DEV = torch.device("cuda", 0)


class Host(object):
    """The arrays of a data.datasets.ScanObjectNN: M clouds of P distinct points in the unit ball."""

    def __init__(self, M, P, seed=0, n_classes=15):
        rng = np.random.default_rng(seed)
        d = rng.normal(size=(M, P, 3))
        self.data = (d / np.linalg.norm(d, axis=2, keepdims=True) * rng.uniform(0.05, 1.0, (M, P, 1))).astype(np.float32)
        self.mask = (rng.random((M, P)) > 0.4).astype(np.float64)
        self.label = (np.arange(M) % n_classes).astype(np.int64)


_DATASETS = {}


def dataset(M, P):
    """(host arrays, DeviceScanObjectNN), made once per size and left unchanged."""
    from cloud_transformers_amd.data.scanobjectnn import DeviceScanObjectNN
    if (M, P) not in _DATASETS:
        host = Host(M, P, seed=P)
        _DATASETS[(M, P)] = (host, DeviceScanObjectNN(host, DEV))
    return _DATASETS[(M, P)]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what):
    for name, g, w in zip(("points", "mask"), got[:2], want[:2]):
        g = g.cpu().numpy()
        assert g.shape == w.shape and g.dtype == np.float32, (what, name, g.shape, w.shape)
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, "%s: %s differs at %d places, first %s: got %r want %r" % (
            what, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    assert got[2].dtype == torch.int64 and got[2].cpu().tolist() == want[2].tolist(), (what, "label")


def draws(B, P, N, with_perm, with_aug, seed):
    rng = np.random.default_rng(seed)
    perm = np.stack([rng.permutation(P) for _ in range(B)]).astype(np.int64) if with_perm else None
    rot = jit = None
    if with_aug:
        a = rng.uniform(0, 2 * np.pi, B)
        rot = np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)
        jit = rng.normal(size=(B, N, 3)).astype(np.float32)
        jit.reshape(-1)[::5] *= 8.0                                       # draws beyond clip / sigma = 5: both clip branches
    return perm, rot, jit


M = 5
ITEMS = {1: [M - 1], 3: [0, M - 1, 0], 8: [0, M - 1, 2, 2, 1, 3, M - 1, 0]}      # repeats, the first and the last cloud
NS = [1, 3, 4, 5, 63, 64, 65, 257, 2048]
SHAPES = sorted({(n, p) for n in NS for p in (n, n + 1, 2048) if p >= n})


# ---------------------------------------------------------------------------------------------------------------------
# the contract over the shapes
@pytest.mark.parametrize("N,P", SHAPES)
def test_equals_the_contract_bit_for_bit(N, P):
    """B 1, 3 and 8; perm NULL and given; augmentation on and off.  N % 4 == 0 takes the four-slot path, with P % 4 == 0 and no
    perm the 16-byte source loads as well (P = N + 1: not); every other N one slot per work-item; N = 257 and 2048 span several
    workgroups."""
    from cloud_transformers_amd.data.scanobjectnn import scan_items_from_draws
    host, ds = dataset(M, P)
    for B, item in ITEMS.items():
        item = np.asarray(item, np.int64)
        for with_perm in (False, True):
            for with_aug in (False, True):
                perm, rot, jit = draws(B, P, N, with_perm, with_aug, seed=N * 7 + P + B)
                want = scan_items_reference(host.data, host.mask, host.label, item, perm, rot, jit, N)
                got = scan_items_from_draws(ds, dev(item), dev(perm), dev(rot), dev(jit), N)
                assert_same(got, want, "N %d P %d B %d perm %d aug %d" % (N, P, B, with_perm, with_aug))


@pytest.mark.parametrize("N,P", [(64, 64), (2048, 2048), (64, 65)])
@pytest.mark.parametrize("which", ["points", "mask", "jit"])
def test_unaligned_buffers_take_the_scalar_path(N, P, which):
    """An output (or the jitter) that starts one float past a 16-byte boundary: N % 4 == 0, but the rows are not 16-byte
    addressable, so the launch goes one slot per work-item — and must not touch the floats around the view."""
    from cloud_transformers_amd.data.scanobjectnn import scan_items_from_draws
    host, ds = dataset(M, P)
    B = 3
    item = np.asarray(ITEMS[B], np.int64)
    perm, rot, jit = draws(B, P, N, False, True, seed=N + P)
    want = scan_items_reference(host.data, host.mask, host.label, item, perm, rot, jit, N)
    big_p = torch.full((B * 3 * N + 8,), 7.0, device=DEV)
    big_m = torch.full((B * N + 8,), 7.0, device=DEV)
    big_j = torch.zeros(B * N * 3 + 8, device=DEV)
    op, om, oj = (1 if which == w else 0 for w in ("points", "mask", "jit"))
    assert big_p.data_ptr() % 16 == 0 and big_m.data_ptr() % 16 == 0 and big_j.data_ptr() % 16 == 0
    points, mask = big_p[op:op + B * 3 * N].view(B, 3, N), big_m[om:om + B * N].view(B, N)
    j = big_j[oj:oj + B * N * 3].view(B, N, 3)
    j.copy_(dev(jit))
    assert (points.data_ptr() % 16 != 0) == (which == "points") and (j.data_ptr() % 16 != 0) == (which == "jit")
    got = scan_items_from_draws(ds, dev(item), None, dev(rot), j, N, out=(points, mask, torch.empty(B, dtype=torch.int64, device=DEV)))
    assert got[0].data_ptr() == points.data_ptr()
    assert_same(got, want, "offset " + which)
    for big, o, n in ((big_p, op, B * 3 * N), (big_m, om, B * N)):
        rest = torch.cat([big[:o], big[o + n:]])
        assert bool((rest == 7.0).all())


def test_bad_arguments_launch_nothing():
    """Half an augmentation, N > P, clip <= 0 and a null pointer: CT_EINVAL, and the outputs keep their contents."""
    from cloud_transformers_amd import _lib
    lib = _lib.load()
    host, ds = dataset(M, 64)
    B, N, P = 2, 32, 64
    item = dev(np.array([0, 1], np.int64))
    perm, rot, jit = (dev(a) for a in draws(B, P, N, True, True, seed=1))
    points = torch.full((B, 3, N), 7.0, device=DEV)
    mask = torch.full((B, N), 7.0, device=DEV)
    label = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    good = dict(data=ds.data.data_ptr(), mask=ds.mask.data_ptr(), label=ds.label.data_ptr(), M=M, P=P, item=item.data_ptr(),
                perm=perm.data_ptr(), rot=rot.data_ptr(), jit=jit.data_ptr(), sigma=0.01, clip=0.05, B=B, N=N,
                out_points=points.data_ptr(), out_mask=mask.data_ptr(), out_label=label.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.ct_scan_items(*[a[k] for k in good], None)

    assert call(rot=None) == -1 and call(jit=None) == -1
    assert call(N=P + 1) == -1
    assert call(clip=0.0) == -1 and call(clip=-0.05) == -1
    for k in ("data", "mask", "label", "item", "out_points", "out_mask", "out_label"):
        assert call(**{k: None}) == -1, k
    torch.cuda.synchronize()
    assert bool((points == 7.0).all()) and bool((mask == 7.0).all()) and bool((label == -7).all())
    with pytest.raises(ValueError):
        from cloud_transformers_amd.data.scanobjectnn import scan_items_from_draws
        scan_items_from_draws(ds, item, perm, rot, None, N)
    assert call() == 0                                                     # and the same arguments unbroken do launch
    torch.cuda.synchronize()
    assert not bool((points == 7.0).any()) and label.tolist() == [0, 1]


@pytest.mark.parametrize("name", ["sub", "full"])
def test_the_upstream_items_on_their_own_draws(name):
    """The golden file's draws through the kernel: within the 1e-6 of the upstream items that tests/test_scan_items_cpu.py
    derives for the contract (the kernel is that contract bit for bit), mask and label exactly."""
    from cloud_transformers_amd.data.scanobjectnn import DeviceScanObjectNN, scan_items_from_draws
    gold = np.load(GOLDEN)

    class Stored(object):
        data, mask, label = gold["data"], gold["mask"], gold["label"]

    ds = DeviceScanObjectNN(Stored, DEV)
    item, perm, rot, jit, N = golden_draws(gold, name)
    got = scan_items_from_draws(ds, dev(item), dev(perm), dev(rot), dev(jit), N)
    assert_same(got, scan_items_reference(gold["data"], gold["mask"], gold["label"], item, perm, rot, jit, N), "golden " + name)
    err = np.abs(got[0].cpu().numpy().transpose(0, 2, 1).astype(np.float64) - gold["pc_" + name].astype(np.float64)).max()
    print("kernel vs upstream (%s): max abs error %.3g" % (name, err))
    assert err <= 1e-6, err
    assert np.array_equal(got[1].cpu().numpy(), gold["ma_" + name].astype(np.float32))
    assert np.array_equal(got[2].cpu().numpy(), gold["label_" + name])


# ---------------------------------------------------------------------------------------------------------------------
# the public functions
def test_scan_items_public_function():
    from cloud_transformers_amd.data.scanobjectnn import scan_items
    host, ds = dataset(M, 2048)
    item = dev(np.asarray(ITEMS[8], np.int64))
    for N in (2048, 1024):
        outs = [scan_items(ds, item, N, True, torch.Generator(device=DEV).manual_seed(11)) for _ in range(2)]
        for a, b in zip(*outs):
            assert torch.equal(a, b)                                       # equally seeded generators: equal bits
        other = scan_items(ds, item, N, True, torch.Generator(device=DEV).manual_seed(12))
        assert not torch.equal(other[0], outs[0][0]) and torch.equal(other[2], outs[0][2])
        points, mask, label = outs[0]
        assert tuple(points.shape) == (8, 3, N) and tuple(mask.shape) == (8, N) and label.tolist() == host.label[ITEMS[8]].tolist()
        assert tuple(points[:, :, None].shape) == (8, 3, 1, N) and points[:, :, None].is_contiguous()
        # the augmentation is a rotation about y of points moved by at most clip per coordinate
        src = torch.from_numpy(host.data[ITEMS[8]]).to(DEV)
        if N == 2048:
            assert float((points[:, 1] - src[:, :, 1]).abs().max()) <= 0.05 + 1e-6
            r_out, r_src = points[:, [0, 2]].norm(dim=1), src[:, :, [0, 2]].norm(dim=2)
            assert float((r_out - r_src).abs().max()) <= 0.05 * 2 ** 0.5 + 1e-5
            assert float((points[:, 1] - src[:, :, 1]).abs().max()) > 0.02


def test_eval_items_are_the_stored_points():
    """train=False: no draw touches the points.  N == P: the stored clouds, transposed; N < P: N distinct rows of them."""
    from cloud_transformers_amd.data.scanobjectnn import scan_items
    host, ds = dataset(M, 2048)
    idx = ITEMS[8]
    points, mask, label = scan_items(ds, dev(np.asarray(idx, np.int64)), None, False, torch.Generator(device=DEV).manual_seed(0))
    assert (bits(points.cpu().numpy()) == bits(host.data[idx].transpose(0, 2, 1))).all()
    assert np.array_equal(mask.cpu().numpy(), host.mask[idx].astype(np.float32)) and label.tolist() == host.label[idx].tolist()
    points, mask, _ = scan_items(ds, dev(np.asarray(idx, np.int64)), 100, False, torch.Generator(device=DEV).manual_seed(0))
    for b, g in enumerate(idx):
        rows = {r.tobytes(): k for k, r in enumerate(host.data[g])}
        picked = [rows[r.tobytes()] for r in np.ascontiguousarray(points[b].t().cpu().numpy())]
        assert len(set(picked)) == 100                                     # without replacement
        assert np.array_equal(mask[b].cpu().numpy(), host.mask[g][picked].astype(np.float32))


def test_items_and_an_epoch_do_not_synchronise():
    """No device-to-host synchronisation in scan_items (draws, argsort, cos / sin, launch) nor in a ScanBatches epoch: under
    torch's sync debug mode set to "error" a synchronising call raises — checked first on `.item()`, so that the mode is known
    to be live."""
    from cloud_transformers_amd.data.scanobjectnn import ScanBatches, scan_items
    host, ds = dataset(M, 2048)
    item = dev(np.asarray(ITEMS[8], np.int64))
    gen = torch.Generator(device=DEV).manual_seed(0)
    scan_items(ds, item, 1024, True, gen)                                  # (library load, allocator warm-up)
    batches = ScanBatches(ds, 2, train=True, seed=3, subsample=1024)
    list(batches)
    probe = ds.data.sum()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        points, mask, label = scan_items(ds, item, 1024, True, gen)
        batches.set_epoch(1)
        epoch = [(p, l, m, batches.last_items) for p, l, m in batches]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(points.shape) == (8, 3, 1024) and label.tolist() == host.label[ITEMS[8]].tolist()
    assert len(epoch) == 3 and [tuple(e[0].shape) for e in epoch] == [(2, 3, 1, 1024), (2, 3, 1, 1024), (1, 3, 1, 1024)]
    assert all(e[0].is_cuda and e[1].dtype == torch.int64 and e[2].dtype == torch.float32 for e in epoch)


@pytest.mark.parametrize("world", [1, 2])
def test_an_epoch_visits_every_index_of_the_shard_once(world):
    from torch.utils.data.distributed import DistributedSampler
    from cloud_transformers_amd.data.scanobjectnn import DeviceScanObjectNN, ScanBatches
    n = 22
    host = Host(n, 16, seed=9)
    host.label = np.arange(n, dtype=np.int64)                              # the label names the cloud
    ds = DeviceScanObjectNN(host, DEV)
    for rank in range(world):
        batches = ScanBatches(ds, 4, train=True, seed=2, rank=rank, world=world)
        sampler = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=True, seed=2)
        for epoch in range(2):
            batches.set_epoch(epoch)
            sampler.set_epoch(epoch)
            got, labels = [], []
            for pcd, label, mask in batches:
                assert tuple(pcd.shape[1:]) == (3, 1, 16) and tuple(mask.shape) == (pcd.shape[0], 16)
                got += batches.last_items.tolist()
                labels += label.tolist()
            assert got == labels == list(sampler)                          # torch's order, every index of the shard
            assert len(got) == n // world and len(set(got)) == len(got)    # ... once (22 clouds: no padding at world 1 and 2)


# ---------------------------------------------------------------------------------------------------------------------
# harness and entry point
CONFIG = '''
experiment:
    root: '{root}/exp'
    writer_root: '{root}/runs'
data:
    path: '{root}/train.h5'
    path_val: '{root}/val.h5'
    n_classes: 3
    batch_size: 4
    batch_size_val: 4
    normalize: True
    center: True
model:
    generator: '{root}/{model}.py'
    n_classes: 3
train:
    seg_weight: !!float 0.25
    num_epochs: 1
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
    """A per-point stem, a max-pooled class head and a per-point mask head: the classifier's outputs in miniature."""

    def __init__(self, n_classes=3, outputs=2):
        super().__init__()
        self.outputs = outputs
        self.stem = nn.Sequential(nn.Conv1d(3, 16, kernel_size=1, bias=False), nn.ReLU(inplace=True))
        self.class_head = nn.Linear(16, n_classes)
        self.mask_head = nn.Conv1d(32, 1, kernel_size=1)

    def forward(self, cloud):                       # [B, 3, 1, N]
        x = self.stem(cloud.squeeze(2))
        vect = x.max(dim=2).values
        mask = self.mask_head(torch.cat([x, vect[:, :, None].expand(-1, -1, x.size(-1))], dim=1)).unsqueeze(2)
        return (self.class_head(vect), mask) if self.outputs == 2 else (self.class_head(vect), mask, [])
'''


def write_pair(root, P=64):
    """train.npz (14 clouds) and val.npz (7 clouds, every class present) in the loader's form: raw points, -1 = background."""
    for name, n, seed in (("train", 14, 0), ("val", 7, 1)):
        rng = np.random.default_rng(seed)
        label = (np.arange(n) % 3).astype(np.int64)
        data = (rng.normal(size=(n, P, 3)) * (0.5 + label[:, None, None]) + 2.0).astype(np.float32)
        np.savez(os.path.join(str(root), name + ".npz"), data=data, label=label, mask=rng.integers(-1, 3, size=(n, P)).astype(np.float32))


def expected_loss(model, batch, w):
    pcd, label, mask = batch
    with torch.no_grad():
        out = model(pcd)
        return float((1 - w) * torch.nn.functional.cross_entropy(out[0], label)
                     + w * torch.nn.functional.binary_cross_entropy_with_logits(out[1][:, 0, 0], mask))


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """A Trainer on the tiny pair after one eager step, one HIP-graph step, one step through fit() and one validation."""
    from cloud_transformers_amd import harness as H
    root = tmp_path_factory.mktemp("scan")
    write_pair(root)
    (root / "classifier.py").write_text(MODEL)
    cfg_path = root / "scanobjectnn.yaml"
    cfg_path.write_text(CONFIG.format(root=str(root), model="classifier", restore=""))
    torch.manual_seed(0)
    cfg = H.load_config(cfg_path)
    cfg["data"]["kind"] = "scanobjectnn_device"
    tr = H.Trainer(cfg, "classification", n_classes=3, device=DEV)      # (data.kind selects the task)
    res = {"root": root, "trainer": tr, "steps": []}
    it = iter(tr.loader)
    batch = next(it)
    want = expected_loss(tr.model, batch, 0.25)
    res["steps"].append((float(tr._eager_step(batch)), want))
    res["hist"] = tr.fit(max_iters=1, hip_graph=False)
    tr._graphs = {}                                                        # (what fit(hip_graph=True) starts from)
    batch = next(it)
    want = expected_loss(tr.model, batch, 0.25)
    res["steps"].append((float(tr._graph_step(batch)), want))
    res["records"] = tr.validate(epoch=0)
    return res


def test_trainer_steps_eagerly_and_from_a_graph(trained):
    """The loss of a step is (1 - w) * CE + w * BCE of the batch it was given, recomputed in torch from the model before the step
    (the stem runs on the split-f16 pointwise kernel in both, so the two agree to fp32 rounding of the loss: 1e-5 relative)."""
    from cloud_transformers_amd.data.scanobjectnn import ScanBatches
    tr = trained["trainer"]
    assert tr.task == "classification_scanobjectnn" and isinstance(tr.loader, ScanBatches) and len(tr.loader) == 4     # 14 clouds, batch 4
    assert tr.cfg["data"]["jitter_sigma"] == 0.01 and tr.cfg["data"]["seed"] == 0
    for (got, want), name in zip(trained["steps"], ("eager", "hip_graph")):
        print("%s step: loss %.7f, recomputed %.7f" % (name, got, want))
        assert np.isfinite(got) and abs(got - want) <= 1e-5 * abs(want), (name, got, want)
    assert trained["steps"][0][0] != trained["steps"][1][0]
    assert len(tr._graphs) == 1 and all(rec is not False for rec in tr._graphs.values())      # captured, not the eager way out
    assert len(trained["hist"]) == 1 and np.isfinite(trained["hist"][0])
    assert tr.scheduler.last_epoch == 1                                    # stepped per iteration (by fit)


def test_validation_record_and_checkpoints(trained):
    from tests.test_scan_items_cpu import _upstream_accuracies
    tr, records = trained["trainer"], trained["records"]
    assert len(records) == 1
    rec = records[0]
    model = tr.model.eval()
    outs, losses = [], []
    with torch.no_grad():
        for pcd, label, mask in tr.val_loader:
            out = model(pcd)
            cls = torch.nn.functional.cross_entropy(out[0], label)
            seg = torch.nn.functional.binary_cross_entropy_with_logits(out[1][:, 0, 0], mask)
            losses.append([float(0.75 * cls + 0.25 * seg), float(cls), float(seg)])
            outs.append((out[0].cpu(), out[1].cpu(), label.cpu(), mask.cpu()))
    model.train()
    cls_acc, seg_acc, m_acc, per = _upstream_accuracies(outs, 3)
    assert rec["batches"] == 2 and rec["epoch"] == 0 and sum(len(o[2]) for o in outs) == 7
    assert rec["cls_acc"] == cls_acc and rec["seg_acc"] == seg_acc and rec["class_acc"] == per.tolist()
    assert abs(rec["m_acc"] - m_acc) <= 1e-15 and np.isfinite(m_acc)
    for k, v in zip(("loss", "loss_cls", "loss_seg"), np.mean(losses, axis=0)):
        assert abs(rec[k] - v) <= 1e-6 * abs(v), (k, rec[k], v)
    assert rec["best"] and rec["macc_best"]
    lines = (tr.exp_dir / "classification_val.jsonl").read_text().splitlines()
    assert len(lines) == 1 and json.loads(lines[0]) == json.loads(json.dumps(rec))
    for name in ("generator_best_0.t7", "g_opt_best_0.t7", "generator_macc_best_0.t7", "g_opt_macc_best_0.t7"):
        assert (tr.exp_dir / name).exists(), name


def test_eval_entry_point_reproduces_the_record(trained, capsys):
    from cloud_transformers_amd import train_classification
    root, tr, rec = trained["root"], trained["trainer"], trained["records"][0]
    cfg_path = root / "scanobjectnn_eval.yaml"
    restore = "restore:\n    generator: '%s'\n" % (tr.exp_dir / "generator_best_0.t7")
    cfg_path.write_text(CONFIG.format(root=str(root), model="classifier", restore=restore))      # (no data.kind: filled in)
    got = train_classification.main(["evalrun", "-c", str(cfg_path), "--eval"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["cls_acc"] == got["cls_acc"]
    assert got["epoch"] == "eval" and got["batches"] == rec["batches"]
    for k in ("cls_acc", "seg_acc", "m_acc", "class_acc"):
        assert got[k] == rec[k], k
    for k in ("loss", "loss_cls", "loss_seg"):
        assert abs(got[k] - rec[k]) <= 1e-6 * abs(rec[k]), (k, got[k], rec[k])


def test_three_output_models_fit_the_loss(tmp_path):
    """The upstream classifier returns (class logits, mask logits, lattice statistics): the loss indexes the output."""
    from cloud_transformers_amd import harness as H
    write_pair(tmp_path)
    (tmp_path / "classifier3.py").write_text(MODEL)
    cfg_path = tmp_path / "scanobjectnn.yaml"
    cfg_path.write_text(CONFIG.format(root=str(tmp_path), model="classifier3", restore=""))
    cfg = H.load_config(cfg_path)
    cfg["model"]["outputs"] = 3
    tr = H.Trainer(cfg, "classification_scanobjectnn", n_classes=3, device=DEV, make_dirs=False)
    batch = next(iter(tr.loader))
    assert len(tr.model(batch[0])) == 3
    want = expected_loss(tr.model, batch, 0.25)
    got = float(tr._eager_step(batch))
    assert np.isfinite(got) and abs(got - want) <= 1e-5 * abs(want), (got, want)
