"""ct_image_items on the device (cloud_transformers_amd.data.image_point): equal, bit for bit, to the numpy restatement of the
entry point's contract (tests/image_items_ref.py, whose agreement with Pillow is settled in tests/test_image_items_cpu.py) over
the shapes at which the kernel takes another path; the float stage on every byte value; the point part on clouds of every
length class; the argument checks; the public functions, eager and from a HIP-graph replay; training, validation and `--eval`
of train_reconstruction on a tiny tree; one forward / backward of the reference-shaped model with the ResNet-50 encoder."""
import json
import os

import numpy as np
import pytest
import torch

from tests import image_items_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits(got, want, what):
    g = got.cpu().numpy()
    assert g.shape == want.shape and g.dtype == np.float32, (what, g.shape, want.shape)
    bad = np.argwhere(bits(g) != bits(want))
    assert bad.size == 0, "%s differs at %d places, first %s: got %r want %r" % (what, len(bad), bad[0].tolist(), g[tuple(bad[0])],
                                                                               want[tuple(bad[0])])


def make_set(H, W, OH, OW, lengths, seed, n=None, images=None):
    """(host dict, DeviceImageToPoint) of len(lengths) random images with clouds of the given lengths."""
    from cloud_transformers_amd.data.image_point import DeviceImageToPoint
    rng = np.random.default_rng(seed)
    M = len(lengths)
    if images is None:
        images = rng.integers(0, 256, size=(M, H, W, 3), dtype=np.uint8)
        images[0, 0, 0], images[-1, -1, -1] = 255, 0
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    points = rng.uniform(0.0, 1.0, size=(int(offsets[-1]), 3)).astype(np.float32)
    class_id = (np.arange(M) % 2).astype(np.int64)
    ds = DeviceImageToPoint.from_arrays(images, points, offsets, class_id, ["a", "b"], DEV, (OH, OW), n or max(lengths))
    return {"images": images, "points": points, "offsets": offsets, "class_id": class_id}, ds


def draws(B, p_cap, n, seed):
    rng = np.random.default_rng(seed)
    perm = np.stack([rng.permutation(p_cap) for _ in range(B)]).astype(np.int64)
    return perm, rng.random((B, n)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the image part
IMAGE_SHAPES = [(224, 224, 128, 128),      # the workload
                (7, 5, 3, 4),              # taps clipped at both borders, odd widths, an unaligned RGB row
                (5, 9, 8, 16),             # upscaling, three taps
                (128, 128, 128, 128),      # identity on both axes
                (9, 224, 5, 128),          # five output rows: a ragged last band
                (300, 300, 16, 16),        # 39 taps, the longest staging
                (224, 160, 128, 91),       # not square, odd output width
                (6, 1000, 3, 250),         # a long unaligned row, four columns per lane
                (3, 9, 1, 4)]              # one output row: fewer than a band


@pytest.mark.parametrize("H,W,OH,OW", IMAGE_SHAPES)
def test_image_equals_the_contract_bit_for_bit(H, W, OH, OW):
    """B 3 with a repeated item out of 3 stored images (the last image's last dword ends the stored set), against Pillow's
    arithmetic restated in numpy; the points and classes of the same launch as well."""
    from cloud_transformers_amd.data.image_point import image_items_from_draws
    host, ds = make_set(H, W, OH, OW, [40, 17, 33], seed=H * 7 + W)
    item = np.array([2, 0, 2], np.int64)
    perm, u = draws(3, ds.p_cap, 24, seed=OW)
    img, pcd, cls = image_items_from_draws(ds, dev(item), dev(perm), dev(u), 24)
    assert_bits(img, R.image_reference(host["images"], item, OH, OW), "image %dx%d -> %dx%d" % (H, W, OH, OW))
    assert_bits(pcd, R.pcd_reference(host["points"], host["offsets"], item, perm, u, 24), "points")
    assert cls.dtype == torch.int64 and cls.tolist() == host["class_id"][item].tolist()


@pytest.mark.parametrize("H,W,OH,OW", [(200, 8, 100, 4), (224, 224, 128, 128)])
def test_image_bands_of_a_large_batch(H, W, OH, OW):
    """B 256, where the launch has workgroups enough with one band per image: the whole image as one band of 100 rows
    (200 x 8 -> 100 x 4: all 200 source rows staged), or as many rows as the staged plane holds (224 x 224 -> 128 x 128)."""
    from cloud_transformers_amd.data.image_point import image_items_from_draws
    host, ds = make_set(H, W, OH, OW, [9, 5], seed=H + OW)
    item = (np.arange(256) % 2).astype(np.int64)
    perm, u = draws(256, ds.p_cap, 4, seed=7)
    img, pcd, _ = image_items_from_draws(ds, dev(item), dev(perm), dev(u), 4)
    assert_bits(img, R.image_reference(host["images"], item, OH, OW), "image %dx%d -> %dx%d, B 256" % (H, W, OH, OW))
    assert_bits(pcd, R.pcd_reference(host["points"], host["offsets"], item, perm, u, 4), "points")


def test_float_stage_on_every_byte_value():
    """A 16 x 16 image that holds every byte value in every channel, at identity size: all 768 floats bit for bit."""
    from cloud_transformers_amd.data.image_point import image_items_from_draws
    plane = np.arange(256, dtype=np.uint8).reshape(16, 16)
    image = np.stack([plane, plane.T, plane[::-1]], axis=2)[None]
    host, ds = make_set(16, 16, 16, 16, [8], seed=0, images=image)
    perm, u = draws(1, 8, 8, seed=1)
    img, _, _ = image_items_from_draws(ds, dev(np.zeros(1, np.int64)), dev(perm), dev(u), 8)
    want = R.float_stage(image[0])[None]
    assert sorted(set(image[0, :, :, 1].reshape(-1).tolist())) == list(range(256)) and want.size == 768
    assert_bits(img, want, "float stage")


# ---------------------------------------------------------------------------------------------------------------------
# the point part
def test_points_equal_the_contract_bit_for_bit():
    """One batch of clouds with P == n, P > n, P < n (the top-up) and P == 1; n = 70 and p_cap = 131 are no multiples of 64; the
    top-up draws hold 0 and the largest float below 1 (whose product with P rounds to P: the clamp)."""
    from cloud_transformers_amd.data.image_point import image_items_from_draws
    n, lengths = 70, [70, 131, 23, 1, 70]
    host, ds = make_set(8, 8, 4, 4, lengths, seed=4)
    assert ds.p_cap == 131
    item = np.array([0, 1, 2, 3, 1, 2], np.int64)
    perm, u = draws(len(item), ds.p_cap, n, seed=6)
    top = np.nextafter(np.float32(1), np.float32(0))
    u[2, 23], u[2, 24], u[3, 1], u[3, 2], u[5, 69] = 0.0, top, top, 0.0, top
    _, pcd, cls = image_items_from_draws(ds, dev(item), dev(perm), dev(u), n)
    want = R.pcd_reference(host["points"], host["offsets"], item, perm, u, n)
    assert_bits(pcd, want, "points")
    assert np.array_equal(want[2][:, 24], host["points"][201 + 22]) and np.array_equal(want[3][:, 5], host["points"][224])
    assert cls.tolist() == host["class_id"][item].tolist()


def test_points_over_several_workgroups():
    """Clouds long enough that a row's positions and top-up slots are split over several workgroups (p_cap 5000, n 4096)."""
    from cloud_transformers_amd.data.image_point import image_items_from_draws
    n, lengths = 4096, [5000, 3000, 4097, 4096]
    host, ds = make_set(8, 8, 4, 4, lengths, seed=8)
    item = np.array([3, 2, 1, 0], np.int64)
    perm, u = draws(4, ds.p_cap, n, seed=9)
    _, pcd, _ = image_items_from_draws(ds, dev(item), dev(perm), dev(u), n)
    assert_bits(pcd, R.pcd_reference(host["points"], host["offsets"], item, perm, u, n), "points")


# ---------------------------------------------------------------------------------------------------------------------
# the argument checks
def test_bad_arguments_launch_nothing():
    """A null table, B 0, more taps than CT_IMAGE_TAPS_MAX and an output row whose staged source rows exceed the LDS budget
    (39 taps x 512 columns x 3 bytes > 36 KiB): CT_EINVAL through the raw ABI, and the outputs keep their contents."""
    import ctypes
    from cloud_transformers_amd import _lib
    from cloud_transformers_amd.data.image_point import _MEAN, _STD
    lib = _lib.load()
    host, ds = make_set(12, 10, 6, 5, [9, 4], seed=2)
    B, n = 2, 8
    item = dev(np.array([1, 0], np.int64))
    perm, u = (dev(a) for a in draws(B, ds.p_cap, n, seed=3))
    img = torch.full((B, 3, ds.OH, ds.OW), 7.0, device=DEV)
    pcd = torch.full((B, 3, n), 7.0, device=DEV)
    cls = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    good = dict(images=ds.images.data_ptr(), M=2, H=12, W=10, OH=6, OW=5, kx=ds.kx.data_ptr(), bx=ds.bx.data_ptr(), ksx=ds.kx.shape[1],
                ky=ds.ky.data_ptr(), by=ds.by.data_ptr(), ksy=ds.ky.shape[1], mean=_MEAN, std=_STD, points=ds.points.data_ptr(),
                offsets=ds.offsets.data_ptr(), class_id=ds.class_id.data_ptr(), p_cap=ds.p_cap, item=item.data_ptr(),
                perm=perm.data_ptr(), u_dup=u.data_ptr(), B=B, n=n, out_img=img.data_ptr(), out_pcd=pcd.data_ptr(),
                out_class=cls.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.ct_image_items(*[a[k] for k in good], None)

    for k in ("images", "kx", "bx", "ky", "by", "points", "offsets", "class_id", "item", "perm", "u_dup", "out_img", "out_pcd", "out_class"):
        assert call(**{k: None}) == -1, k
    assert call(mean=ctypes.POINTER(ctypes.c_float)()) == -1
    assert call(B=0) == -1 and call(n=0) == -1 and call(p_cap=(1 << 16) + 1) == -1 and call(M=0) == -1
    assert call(ksx=_lib.IMAGE_TAPS_MAX + 1) == -1 and call(ksy=_lib.IMAGE_TAPS_MAX + 1) == -1 and call(ksy=0) == -1
    assert call(W=_lib.IMAGE_W_MAX + 1) == -1 and call(OH=_lib.IMAGE_SIZE_MAX + 1) == -1
    assert call(H=300, ksy=39, OW=512) == -1                               # one output row: 39 * 512 * 3 bytes do not fit
    assert call(images=ds.images.data_ptr() + 1) == -1                     # not 4-byte aligned
    torch.cuda.synchronize()
    assert bool((img == 7.0).all()) and bool((pcd == 7.0).all()) and bool((cls == -7).all())
    assert call() == 0                                                     # and the same arguments unbroken do launch
    torch.cuda.synchronize()
    assert not bool((img == 7.0).any()) and not bool((pcd == 7.0).any()) and cls.tolist() == [1, 0]
    from cloud_transformers_amd.data.image_point import image_items_from_draws
    with pytest.raises(ValueError):
        image_items_from_draws(ds, item, perm[:, :-1], u, n)
    with pytest.raises(ValueError):
        image_items_from_draws(ds, item, perm, u, n + 1)
    with pytest.raises(RuntimeError):
        image_items_from_draws(ds, item.cpu(), perm, u, n)


# ---------------------------------------------------------------------------------------------------------------------
# the public functions
@pytest.fixture(scope="module")
def workload():
    """Six 224 x 224 renderings -> 128 x 128, clouds of 1500 .. 2300 points, 2048 slots."""
    return make_set(224, 224, 128, 128, [2300, 1500, 2048, 2049, 1900, 2200], seed=21, n=2048)


def test_image_items_public_function(workload):
    from cloud_transformers_amd.data.image_point import image_items
    host, ds = workload
    item = dev(np.array([0, 5, 1, 1], np.int64))
    outs = [image_items(ds, item, None, torch.Generator(device=DEV).manual_seed(11)) for _ in range(2)]
    for a, b in zip(*outs):
        assert torch.equal(a, b)                                           # equally seeded generators: equal bits
    other = image_items(ds, item, None, torch.Generator(device=DEV).manual_seed(12))
    assert torch.equal(other[0], outs[0][0]) and not torch.equal(other[1], outs[0][1]) and torch.equal(other[2], outs[0][2])
    img, pcd, cls = outs[0]
    assert tuple(img.shape) == (4, 3, 128, 128) and tuple(pcd.shape) == (4, 3, 2048) and cls.tolist() == [0, 1, 1, 1]
    assert_bits(img, R.image_reference(host["images"], [0, 5, 1, 1], 128, 128), "image")
    for b, g in enumerate([0, 5, 1, 1]):
        cloud = host["points"][host["offsets"][g]:host["offsets"][g + 1]]
        rows = {r.tobytes(): k for k, r in enumerate(cloud)}
        picked = [rows[r.tobytes()] for r in np.ascontiguousarray(pcd[b].t().cpu().numpy())]
        m = min(len(cloud), 2048)
        assert len(set(picked[:m])) == m                                   # without replacement, then repeats


def test_graph_replay_equals_eager(workload):
    """One capture of the launch on static draws, replayed with fresh items and draws copied in place."""
    from cloud_transformers_amd.data.image_point import image_draws, image_items_from_draws
    host, ds = workload
    B, n = 4, 2048
    gen = torch.Generator(device=DEV).manual_seed(5)
    item = dev(np.array([0, 1, 2, 3], np.int64))
    perm, u = image_draws(B, ds.p_cap, n, DEV, gen)
    image_items_from_draws(ds, item, perm, u, n)                           # (library load, allocator warm-up)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):           # no stream=: torch's own capture stream, which never ran anything eagerly
        outs = image_items_from_draws(ds, item, perm, u, n)
    for items in ([5, 4, 4, 0], [2, 2, 3, 1]):
        fresh_perm, fresh_u = image_draws(B, ds.p_cap, n, DEV, gen)
        with torch.no_grad():
            item.copy_(dev(np.array(items, np.int64)))
            perm.copy_(fresh_perm)
            u.copy_(fresh_u)
        g.replay()
        torch.cuda.synchronize()
        want = image_items_from_draws(ds, dev(np.array(items, np.int64)), fresh_perm, fresh_u, n)
        for a, b in zip(outs, want):
            assert torch.equal(a, b)
        assert outs[2].tolist() == host["class_id"][items].tolist()


def test_items_and_an_epoch_do_not_synchronise(workload):
    """No device-to-host synchronisation in image_items nor in an ImageBatches epoch: under torch's sync debug mode set to
    "error" a synchronising call raises — checked first on `.item()`, so that the mode is known to be live."""
    from cloud_transformers_amd.data.image_point import ImageBatches, image_items
    host, ds = workload
    item = dev(np.array([0, 1, 2, 3], np.int64))
    gen = torch.Generator(device=DEV).manual_seed(0)
    image_items(ds, item, 1024, gen)
    batches = ImageBatches(ds, 4, train=True, seed=3, points=1024)
    list(batches)
    probe = ds.points.sum()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        img, pcd, cls = image_items(ds, item, 1024, gen)
        batches.set_epoch(1)
        epoch = [(i, p, batches.last_items, batches.last_classes) for i, p in batches]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(img.shape) == (4, 3, 128, 128) and tuple(pcd.shape) == (4, 3, 1024)
    assert [tuple(e[0].shape[:1]) + tuple(e[1].shape) for e in epoch] == [(4, 4, 3, 1024), (2, 2, 3, 1024)]


@pytest.mark.parametrize("world", [1, 2])
def test_an_epoch_visits_every_index_of_the_shard_once(world):
    from torch.utils.data.distributed import DistributedSampler
    from cloud_transformers_amd.data.image_point import DeviceImageToPoint, ImageBatches
    M = 22
    rng = np.random.default_rng(1)
    images = rng.integers(0, 256, size=(M, 6, 6, 3), dtype=np.uint8)
    ds = DeviceImageToPoint.from_arrays(images, rng.random((M * 5, 3)), np.arange(M + 1) * 5, np.arange(M), [str(i) for i in range(M)],
                                        DEV, (4, 4), 8)                    # the class names the pair
    for rank in range(world):
        batches = ImageBatches(ds, 4, train=True, seed=2, rank=rank, world=world)
        sampler = DistributedSampler(range(M), num_replicas=world, rank=rank, shuffle=True, seed=2)
        for epoch in range(2):
            batches.set_epoch(epoch)
            sampler.set_epoch(epoch)
            got, classes = [], []
            for img, pcd in batches:
                assert tuple(img.shape[1:]) == (3, 4, 4) and tuple(pcd.shape[1:]) == (3, 8)
                got += batches.last_items.tolist()
                classes += batches.last_classes.tolist()
            assert got == classes == list(sampler)                         # torch's order, every index of the shard
            assert len(got) == M // world and len(set(got)) == len(got)


# ---------------------------------------------------------------------------------------------------------------------
# harness and entry point
CONFIG = '''
experiment:
    root: '{root}/exp'
    writer_root: '{root}/runs'
data:
    path: '{root}/data'
    batch_size: 4
    batch_size_val: 4
    num_workers: 0
    im_size: 32
    gt_size: 1024
    eval_points: 1024
    eval_noise: 512
model:
    generator: '{root}/tiny.py'
train:
    num_epochs: 2
    show_each: 1000
    save_each: 3
    save_each_epoch: 1
    val_emd_iters: 30
    optimizer:
        type: 'Adam'
        lr: !!float 1e-4
        betas: [!!float 0.9, !!float 0.999]
        weight_decay: !!float 0.0
    scheduler:
        type: 'StepLR'
        gamma: !!float 0.5
        step_size: 100000
{restore}
'''

TINY_MODEL = '''
from torch import nn
from layers.multihead_ct_adain import MultiHeadUnionAdaIn, forward_style
from layers.utils import AdaIn1dUpd


class Model(nn.Module):
    """The reconstructor in miniature: a two-layer convolutional encoder, the style mapping, two AdaIN blocks."""

    def __init__(self, num_latent=32, dim=32):
        super().__init__()
        self.encoder = nn.Sequential(nn.Conv2d(3, 8, 3, stride=2, padding=1), nn.ReLU(inplace=True),
                                     nn.Conv2d(8, 16, 3, stride=2, padding=1), nn.ReLU(inplace=True), nn.AdaptiveAvgPool2d((1, 1)))
        self.mapping = nn.Sequential(nn.Linear(16, num_latent), nn.ReLU(inplace=True))
        self.start = nn.Sequential(nn.Conv1d(3, dim, kernel_size=1, bias=False), AdaIn1dUpd(dim, num_latent=num_latent), nn.ReLU(True))
        self.attentions_decoder = nn.ModuleList([MultiHeadUnionAdaIn(model_dim=dim, features_dims=[4, 4], heads=[4, 4],
                                                                     tensor_sizes=[16, 8], model_dim_out=dim, n_latent=num_latent,
                                                                     tensor_dims=[2, 3]) for _ in range(2)])
        self.final = nn.Sequential(nn.Conv1d(dim, dim, kernel_size=1, bias=False), AdaIn1dUpd(dim, num_latent=num_latent),
                                   nn.ReLU(inplace=True), nn.Conv1d(dim, 3, kernel_size=1), nn.Sigmoid())

    def forward(self, noise, input):
        z = self.mapping(self.encoder(input).reshape(input.shape[0], -1))
        x = forward_style(self.start, noise, z)
        lattices_sizes = []
        for block in self.attentions_decoder:
            x, lattice_size = block(x, z, noise)
            lattices_sizes += lattice_size
        return forward_style(self.final, x, z).unsqueeze(2), lattices_sizes
'''


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """train_reconstruction on a tree of eight objects (32 x 32 renderings, 64-point clouds topped up to 1024): two epochs."""
    pytest.importorskip("PIL.Image", reason="the temporary tree's renderings are written with Pillow")
    from cloud_transformers_amd import train_reconstruction
    from tests.image_tree import make_tree
    root = tmp_path_factory.mktemp("recon")
    (root / "data").mkdir()
    make_tree(root / "data", objects=4, views=1, size=(32, 32), cloud=64, seed=3)
    (root / "tiny.py").write_text(TINY_MODEL)
    cfg_path = root / "reconstruction.yaml"
    cfg_path.write_text(CONFIG.format(root=str(root), restore=""))
    torch.manual_seed(0)
    records = train_reconstruction.main(["run", "-c", str(cfg_path)])
    exp = [p for p in (root / "exp").iterdir() if p.name.startswith("run_")]
    assert len(exp) == 1
    return {"root": root, "records": records, "exp": exp[0]}


def test_training_writes_records_and_checkpoints(trained):
    records, exp = trained["records"], trained["exp"]
    assert [r["epoch"] for r in records] == [0, 1] and all(r["batches"] == 2 for r in records) and records[0]["best"]
    assert [r["iters"] for r in records] == [2, 4]
    lines = [json.loads(line) for line in (exp / "reconstruction_val.jsonl").read_text().splitlines()]
    assert lines == json.loads(json.dumps(records))
    for rec in lines:
        assert np.isfinite(rec["loss_emd"]) and np.isfinite(rec["loss_chamfer"]) and rec["loss_emd"] > 0 and rec["loss_chamfer"] > 0
    for name in ("generator_epoch_0.t7", "g_opt_epoch_0.t7", "generator_epoch_1.t7", "generator_best_0.t7", "g_opt_best_0.t7",
                 "generator_iter_3.t7", "tiny.py", "reconstruction.yaml"):
        assert (exp / name).exists(), name
    state = torch.load(str(exp / "generator_best_0.t7"), map_location="cpu")
    assert "encoder.0.weight" in state and all(bool(torch.isfinite(v).all()) for v in state.values() if v.is_floating_point())


def test_eval_entry_point_writes_the_f1_table(trained, capsys):
    from cloud_transformers_amd import train_reconstruction
    root, exp = trained["root"], trained["exp"]
    cfg_path = root / "reconstruction_eval.yaml"
    cfg_path.write_text(CONFIG.format(root=str(root), restore="restore:\n    generator: '%s'\n" % (exp / "generator_best_0.t7")))
    res = train_reconstruction.main(["evalrun", "-c", str(cfg_path), "--eval"])
    out = capsys.readouterr().out
    assert "Overall" in out and "02691156" in out
    exp_eval = [p for p in (root / "exp").iterdir() if p.name.startswith("evalrun_")]
    assert len(exp_eval) == 1
    table = json.loads((exp_eval[0] / "reconstruction_test.json").read_text())
    assert table == json.loads(json.dumps(res)) and table["names"] == ["f1", "precision", "recall"]
    assert sorted(table["categories"]) == ["02691156", "03001627"] and table["overall"]["count"] == 8
    for row in list(table["categories"].values()) + [table["overall"]]:
        assert len(row["avg"]) == 3 and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in row["avg"])
    assert all(row["count"] == 4 for row in table["categories"].values())
    assert not list(exp_eval[0].glob("*.pickle"))


REFERENCE_SHAPED_MODEL = '''
from torch import nn
from layers.multihead_ct_adain import MultiHeadUnionAdaIn, forward_style
from layers.utils import AdaIn1dUpd

import torchvision.models as models

BLOCKS = [([4, 4], [128, 32]), ([16, 16], [64, 16]), ([16, 32], [16, 8])]


class ResNet50Bottom(nn.Module):
    def __init__(self, original_model):
        super().__init__()
        self.features = nn.Sequential(*list(original_model.children())[:-2])

    def forward(self, x):
        return self.features(x)


class Model(nn.Module):
    """The single-view reconstructor's shape: ResNet-50 trunk, pooled, mapped to the style; twelve AdaIN blocks of width 512."""

    def __init__(self, num_latent=512, dim=512):
        super().__init__()
        self.res50_model = nn.Sequential(ResNet50Bottom(models.resnet50(pretrained=False)), nn.AdaptiveAvgPool2d((1, 1)))
        self.mapping = nn.Sequential(nn.Linear(2048, num_latent), nn.ReLU(inplace=True))
        self.start = nn.Sequential(nn.Conv1d(3, dim, kernel_size=1, bias=False), AdaIn1dUpd(dim, num_latent=num_latent), nn.ReLU(True))
        self.attentions_decoder = nn.ModuleList([MultiHeadUnionAdaIn(model_dim=dim, features_dims=f, heads=[16, 16], tensor_sizes=s,
                                                                     model_dim_out=dim, n_latent=num_latent, tensor_dims=[2, 3])
                                                 for _ in range(4) for f, s in BLOCKS])
        self.final = nn.Sequential(nn.Conv1d(dim, dim, kernel_size=1, bias=False), AdaIn1dUpd(dim, num_latent=num_latent),
                                   nn.ReLU(inplace=True), nn.Conv1d(dim, 3, kernel_size=1), nn.Sigmoid())

    def forward(self, noise, input):
        z = self.mapping(self.res50_model(input).reshape(-1, 2048))
        x = forward_style(self.start, noise, z)
        lattices_sizes = []
        for block in self.attentions_decoder:
            x, lattice_size = block(x, z, noise)
            lattices_sizes += lattice_size
        return forward_style(self.final, x, z).unsqueeze(2), lattices_sizes
'''


def test_reference_shaped_model_with_the_resnet_encoder(tmp_path):
    """The reconstructor's module tree built through harness.get_model (layers/resnet.py's resnet50 where torchvision is absent),
    B 1 and 256 points: one forward and one backward pass of the Chamfer term; the gradients of the encoder and of the mapping
    are finite and not zero."""
    from cloud_transformers_amd import harness as H
    from cloud_transformers_amd.chamfer import loss_chamfer_adj
    from cloud_transformers_amd.metrics import sphere_noise
    path = tmp_path / "reconstructor.py"
    path.write_text(REFERENCE_SHAPED_MODEL)
    torch.manual_seed(0)
    model = H.get_model(path, {}).to(DEV)
    keys = list(model.state_dict())
    assert "res50_model.0.features.0.weight" in keys and "res50_model.0.features.7.2.bn3.running_var" in keys
    assert len(model.attentions_decoder) == 12
    model.train()
    gen = torch.Generator(device=DEV).manual_seed(1)
    img = torch.randn(1, 3, 128, 128, device=DEV, generator=gen)
    noise = sphere_noise(1, 256, DEV, generator=gen)
    gt = torch.rand(1, 3, 1, 256, device=DEV, generator=gen)
    rec, lattices = model(noise, img)
    assert tuple(rec.shape) == (1, 3, 1, 256) and len(lattices) >= 12
    loss = loss_chamfer_adj(rec, gt)
    loss.backward()
    assert np.isfinite(float(loss.detach()))
    for name in ("res50_model.0.features.0.weight", "res50_model.0.features.4.0.conv1.weight", "res50_model.0.features.7.2.conv3.weight",
                 "mapping.0.weight", "mapping.0.bias"):
        grad = dict(model.named_parameters())[name].grad
        assert grad is not None and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0.0, name
