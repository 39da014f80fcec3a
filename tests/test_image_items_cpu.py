"""The What3D reconstruction protocol without a GPU: the numpy restatement of ct_image_items (tests/image_items_ref.py) against
Pillow itself and against the golden file of Pillow's outputs; the PLY reader; the host loader on a temporary tree; the decode
cache; the ResNet-50 encoder and the torchvision stand-in of harness.get_model; the config defaults; the ABI entry."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import image_items_ref as R
from tests.conftest import load_golden
from tests.image_tree import make_tree, write_ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
@pytest.mark.parametrize("H,W,OH,OW", R.SHAPES)
def test_restatement_equals_pillow(H, W, OH, OW):
    Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed: the golden file holds its outputs instead")
    rng = np.random.default_rng(H * 1000 + W)
    img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    img[0, 0], img[-1, -1] = 255, 0
    want = np.asarray(Image.fromarray(img, "RGB").resize((OW, OH), Image.BILINEAR))
    got = R.resize_bilinear(img, OH, OW)
    assert got.shape == want.shape and np.array_equal(got, want), int(np.abs(got.astype(int) - want).max())


def test_restatement_equals_the_golden_file():
    gold = load_golden("image_items")
    cases = [k for k in gold if k != "meta"]
    assert len(cases) >= 5
    for name in cases:
        img, want = gold[name]["img"], gold[name]["out"]
        got = R.resize_bilinear(img, want.shape[0], want.shape[1])
        assert np.array_equal(got, want), name


def test_package_tables_equal_the_restatement():
    from cloud_transformers_amd.data.image_point import resize_tables
    for n_in, n_out in [(224, 128), (137, 128), (7, 3), (5, 4), (5, 8), (9, 16), (64, 128), (128, 128), (160, 91), (9, 5), (300, 16), (1, 1)]:
        k, b = resize_tables(n_in, n_out)
        k2, b2 = R.axis_tables(n_in, n_out)
        assert k.dtype == np.int32 and b.dtype == np.int32 and k.shape == k2.shape
        assert np.array_equal(k, k2) and np.array_equal(b, b2), (n_in, n_out)
    assert resize_tables(300, 16)[0].shape[1] == 39 and resize_tables(128, 128)[0].shape[1] == 3


def test_float_stage_equals_torch():
    """ToTensor and Normalize in torch (what the host loader runs) against the restatement, on every byte value."""
    Image = pytest.importorskip("PIL.Image", reason="ToTensor takes a PIL image")
    from cloud_transformers_amd.data.image_point import to_tensor_normalize
    img = np.stack([np.arange(256, dtype=np.uint8).reshape(16, 16)] * 3, axis=2)
    got = to_tensor_normalize(Image.fromarray(img, "RGB")).numpy()
    want = R.float_stage(img)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_pcd_reference_is_resample_pcd():
    """The compaction of a permutation of p_cap to the entries below P is a permutation of P; the top-up indexes the cloud."""
    rng = np.random.default_rng(3)
    points = rng.normal(size=(30, 3)).astype(np.float32)
    offsets = np.array([0, 10, 30])
    perm = np.stack([rng.permutation(20) for _ in range(2)])
    u = rng.random((2, 16)).astype(np.float32)
    out = R.pcd_reference(points, offsets, [0, 1], perm, u, 16)
    rows0 = {tuple(r) for r in points[:10]}
    assert {tuple(r) for r in out[0].T[:10]} == rows0 and all(tuple(r) in rows0 for r in out[0].T[10:])
    assert np.array_equal(out[1].T, points[10:][perm[1][:16]])


# ---------------------------------------------------------------------------------------------------------------------
# read_ply
@pytest.mark.parametrize("encoding", ["ascii", "binary"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("colour,faces", [(False, False), (True, False), (False, True), (True, True)])
def test_read_ply(tmp_path, encoding, dtype, colour, faces):
    from cloud_transformers_amd.data.image_point import read_ply
    xyz = np.random.default_rng(1).normal(size=(37, 3)).astype(dtype)
    path = tmp_path / "c.ply"
    write_ply(path, xyz, encoding, dtype, colour=colour, faces=faces)
    got = read_ply(path)
    assert got.dtype == np.float32 and got.shape == (37, 3) and np.array_equal(got, xyz.astype(np.float32))


def test_read_ply_errors(tmp_path):
    from cloud_transformers_amd.data.image_point import read_ply
    xyz = np.random.default_rng(2).normal(size=(5, 3)).astype(np.float32)

    def fails(path, word):
        with pytest.raises(ValueError) as ex:
            read_ply(path)
        assert str(path) in str(ex.value) and word in str(ex.value), str(ex.value)

    write_ply(tmp_path / "big.ply", xyz, "binary", fmt="binary_big_endian")
    fails(tmp_path / "big.ply", "binary_big_endian")
    write_ply(tmp_path / "list.ply", xyz, "ascii", list_prop=True)
    fails(tmp_path / "list.ply", "property list uchar int neighbours")
    for enc in ("ascii", "binary"):                                          # a short file: the last bytes are missing
        write_ply(tmp_path / "short.ply", xyz, enc)
        raw = (tmp_path / "short.ply").read_bytes()
        (tmp_path / "short.ply").write_bytes(raw[:-14])
        fails(tmp_path / "short.ply", "vert")
    (tmp_path / "noy.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float z\nend_header\n1 2\n")
    fails(tmp_path / "noy.ply", "'y'")
    (tmp_path / "int.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty int y\nproperty float z\nend_header\n1 2 3\n")
    fails(tmp_path / "int.ply", "property int y")
    (tmp_path / "head.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\n")
    fails(tmp_path / "head.ply", "end_header")
    (tmp_path / "not.ply").write_bytes(b"# .PCD v0.7\nVERSION 0.7\n")
    fails(tmp_path / "not.ply", "PCD")
    (tmp_path / "face.ply").write_bytes(b"ply\nformat ascii 1.0\nelement face 0\nproperty list uchar int vertex_indices\nelement vertex 1\n"
                                        b"property float x\nproperty float y\nproperty float z\nend_header\n1 2 3\n")
    fails(tmp_path / "face.ply", "element face 0")


# ---------------------------------------------------------------------------------------------------------------------
# the host loader and the cache
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    pytest.importorskip("PIL.Image", reason="the temporary tree's renderings are written with Pillow")
    root = tmp_path_factory.mktemp("what3d")
    return root, make_tree(root, objects=2, views=2, size=(40, 56), cloud=[20, 50], seed=5)


def test_image_to_point_items(tree):
    from cloud_transformers_amd.data.image_point import ImageToPoint, resize_size
    from datasets.image_point import ImageToPoint as ReExport
    root, made = tree
    assert ReExport is ImageToPoint
    ds = ImageToPoint(root, split="train", im_size=16, points=32)
    assert len(ds) == 8 and ds.class_to_id == {"airplane": "02691156", "chair": "03001627"}
    got = [(p.parents[1].name, p.parents[0].name, p.stem) for _, p in ds.data_pairs]
    assert got == made["pairs"] == sorted(made["pairs"])                      # sorted categories, objects, renderings
    assert all(i.stem == p.stem and i.suffix == ".png" and p.suffix == ".ply" for i, p in ds.data_pairs)
    assert resize_size(40, 56, 16) == (16, 22) and resize_size(56, 40, 16) == (22, 16) and resize_size(224, 224, 128) == (128, 128)
    for index in (0, 1, 5):
        np.random.seed(index)
        image, pcd = ds[index]
        pair = made["pairs"][index]
        assert image.dtype == torch.float32 and tuple(image.shape) == (3, 16, 22)
        assert pcd.dtype == torch.float32 and tuple(pcd.shape) == (3, 32)
        want = R.float_stage(R.resize_bilinear(made["images"][pair], 16, 22))
        assert np.array_equal(image.numpy().view(np.uint32), want.view(np.uint32)), index
        # resample_pcd on np.random: a permutation, topped up with repeats when the cloud is shorter
        cloud = made["clouds"][pair]
        np.random.seed(index)
        idx = np.random.permutation(len(cloud))
        if len(cloud) < 32:
            idx = np.concatenate([idx, np.random.randint(len(cloud), size=32 - len(cloud))])
        assert np.array_equal(pcd.numpy(), cloud[idx[:32]].T)
    test = ImageToPoint(root, split="test", im_size=16, points=10)
    item = test[6]
    assert len(item) == 3 and item[2] == "03001627" and tuple(item[1].shape) == (3, 10)


def test_image_to_point_keeps_the_assertions(tree, tmp_path):
    from cloud_transformers_amd.data.image_point import ImageToPoint
    root, _ = tree
    with pytest.raises(AssertionError):
        ImageToPoint(tmp_path / "absent")
    with pytest.raises(AssertionError):
        ImageToPoint(root, split="nosuchsplit")


def test_device_set_and_its_cache(tmp_path):
    pytest.importorskip("PIL.Image", reason="the temporary tree's renderings are written with Pillow")
    from cloud_transformers_amd.data import image_point as IP
    (tmp_path / "data").mkdir()
    made = make_tree(tmp_path / "data", objects=2, views=1, size=(12, 10), cloud=[7, 11, 5], seed=1, splits=("train",))
    host = IP.ImageToPoint(tmp_path / "data", split="train", im_size=6, points=8)
    cache = tmp_path / "cache"
    ds = IP.DeviceImageToPoint(host, "cpu", cache_dir=cache)
    assert not ds.from_cache and (cache / "image_point_train.npz").exists()
    assert ds.images.dtype == torch.uint8 and tuple(ds.images.shape) == (4, 12, 10, 3) and (ds.OH, ds.OW) == (7, 6)
    assert ds.offsets_host.tolist() == [0, 7, 18, 23, 30] and ds.p_cap == 11 and ds.offsets.dtype == torch.int64
    assert ds.class_names == ["02691156", "03001627"] and ds.class_id.tolist() == [0, 0, 1, 1]
    assert tuple(ds.kx.shape) == (6, 5) and tuple(ds.bx.shape) == (6, 2) and tuple(ds.ky.shape) == (7, 5) and ds.ky.dtype == torch.int32
    for i, pair in enumerate(made["pairs"]):
        assert np.array_equal(ds.images[i].numpy(), made["images"][pair])
        assert np.array_equal(ds.points[ds.offsets_host[i]:ds.offsets_host[i + 1]].numpy(), made["clouds"][pair])
    again = IP.DeviceImageToPoint(host, "cpu", cache_dir=cache)
    assert again.from_cache and torch.equal(again.images, ds.images) and torch.equal(again.points, ds.points)
    # a touched file invalidates the cache
    target = str(host.data_pairs[2][1])
    st = os.stat(target)
    os.utime(target, ns=(st.st_atime_ns, st.st_mtime_ns + 5_000_000_000))
    third = IP.DeviceImageToPoint(host, "cpu", cache_dir=cache)
    assert not third.from_cache and torch.equal(third.points, ds.points)
    assert IP.DeviceImageToPoint(host, "cpu", cache_dir=cache).from_cache
    # renderings of two sizes do not fit the device set
    from PIL import Image
    Image.fromarray(np.zeros((9, 10, 3), np.uint8), "RGB").save(str(host.data_pairs[1][0]))
    with pytest.raises(ValueError, match="one H x W"):
        IP.DeviceImageToPoint(host, "cpu")


# ---------------------------------------------------------------------------------------------------------------------
# the encoder and the stand-in
@pytest.fixture(scope="module")
def resnet():
    from cloud_transformers_amd.layers.resnet import resnet50
    torch.manual_seed(0)
    return resnet50()


def test_resnet50_tree(resnet):
    assert sum(p.numel() for p in resnet.parameters()) == 25557032
    sd = resnet.state_dict()
    for key, shape in (("layer1.0.downsample.0.weight", (256, 64, 1, 1)), ("layer4.2.conv3.weight", (2048, 512, 1, 1)),
                       ("fc.weight", (1000, 2048)), ("conv1.weight", (64, 3, 7, 7)), ("layer2.0.conv2.weight", (128, 128, 3, 3)),
                       ("layer3.5.bn3.running_var", (1024,)), ("bn1.num_batches_tracked", ())):
        assert tuple(sd[key].shape) == shape, key
    assert [n for n, _ in resnet.named_children()] == ["conv1", "bn1", "relu", "maxpool", "layer1", "layer2", "layer3", "layer4", "avgpool", "fc"]
    assert [len(getattr(resnet, "layer%d" % i)) for i in (1, 2, 3, 4)] == [3, 4, 6, 3]
    assert resnet.layer2[0].conv2.stride == (2, 2) and resnet.layer2[0].conv1.stride == (1, 1)      # the stride sits on the 3x3
    assert float(resnet.layer1[0].bn3.weight.detach().min()) == 1.0 and float(resnet.bn1.bias.detach().abs().max()) == 0.0
    std = float(resnet.layer4[2].conv3.weight.detach().std())
    assert abs(std - (2.0 / 2048) ** 0.5) < 0.05 * (2.0 / 2048) ** 0.5                      # Kaiming normal, fan-out


def test_resnet50_trunk_shape(resnet):
    trunk = torch.nn.Sequential(*list(resnet.children())[:-2]).eval()
    with torch.no_grad():
        out = trunk(torch.randn(2, 3, 128, 128))
    assert tuple(out.shape) == (2, 2048, 4, 4) and bool(torch.isfinite(out).all())


MODEL_FILE = '''
from torch import nn
import torchvision.models as models


class ResNet50Bottom(nn.Module):
    def __init__(self, original_model):
        super().__init__()
        self.features = nn.Sequential(*list(original_model.children())[:-2])


class Model(nn.Module):
    def __init__(self, pretrained=False):
        super().__init__()
        self.res50_model = nn.Sequential(ResNet50Bottom(models.resnet50(pretrained=pretrained)), nn.AdaptiveAvgPool2d((1, 1)))
'''


def test_get_model_offers_a_torchvision_stand_in(tmp_path, monkeypatch):
    from cloud_transformers_amd import harness as H
    from cloud_transformers_amd.layers import resnet as RN
    path = tmp_path / "encoder.py"
    path.write_text(MODEL_FILE)
    have_tv = "torchvision" in sys.modules
    before = set(sys.modules)
    model = H.get_model(path, {})
    assert set(sys.modules) == before and ("torchvision" in sys.modules) == have_tv
    keys = list(model.state_dict())
    assert keys[0] == "res50_model.0.features.0.weight" and "res50_model.0.features.7.2.conv3.weight" in keys
    assert not any(".fc." in k for k in keys)
    try:
        import torchvision  # noqa: F401
        return
    except ImportError:
        pass
    # pretrained=True: the file CLOUDCT_RESNET50_WEIGHTS names, else one warning and the random initialisation
    monkeypatch.setattr(RN, "_warned", False)
    monkeypatch.delenv(RN.WEIGHTS_ENV, raising=False)
    with pytest.warns(UserWarning, match=RN.WEIGHTS_ENV):
        H.get_model(path, {"pretrained": True})
    donor = RN.resnet50()
    torch.save(donor.state_dict(), str(tmp_path / "r50.pth"))
    monkeypatch.setenv(RN.WEIGHTS_ENV, str(tmp_path / "r50.pth"))
    loaded = H.get_model(path, {"pretrained": True})
    assert torch.equal(loaded.state_dict()["res50_model.0.features.0.weight"], donor.conv1.weight)
    assert not any(name.split(".")[0] == "torchvision" for name in sys.modules)      # (torch.save imports modules of its own)


# ---------------------------------------------------------------------------------------------------------------------
# config and ABI
def test_reconstruction_config_defaults():
    from cloud_transformers_amd.train_reconstruction import reconstruction_config
    src = {"data": {"path": "/x", "batch_size": 4, "gt_size": 2048}, "train": {"emd_iters": 7}}
    cfg = reconstruction_config(src)
    assert src == {"data": {"path": "/x", "batch_size": 4, "gt_size": 2048}, "train": {"emd_iters": 7}}      # a copy
    d, t = cfg["data"], cfg["train"]
    assert d["kind"] == "what3d_device" and d["seed"] == 42 and d["eval_points"] == 10000 and d["eval_noise"] == 8192
    assert d["gt_size"] == 2048 and d["im_size"] == 128 and d["batch_size_val"] == 4
    assert t["emd_eps"] == 0.005 and t["emd_iters"] == 7 and t["val_emd_eps"] == 0.004 and t["val_emd_iters"] == 3000
    assert t["f1_threshold"] == 0.01


def test_data_kind_error_names_what3d():
    from cloud_transformers_amd import harness as H
    with pytest.raises(ValueError, match="what3d_device"):
        H.make_dataset({"data": {"kind": "nonsense"}}, "segmentation", 3)


def test_abi_entry():
    from cloud_transformers_amd import _lib
    text = open(os.path.join(ROOT, "include", "cloudct.h")).read()
    assert re.search(r"^int ct_image_items\(", text, flags=re.M) and "#define CT_ABI_VERSION 3" in text
    assert "#define CT_IMAGE_TAPS_MAX %d" % _lib.IMAGE_TAPS_MAX in text
    assert "ct_image_items" in _lib.SIGNATURES and len(_lib.SIGNATURES["ct_image_items"][1]) == 27
    assert "ct_imageitems.hip" in _lib.HIP_SOURCES and os.path.exists(os.path.join(_lib.CSRC, "ct_imageitems.hip"))
    assert _lib.ABI_VERSION == 3
    _lib.build()
    assert _lib.load().ct_abi_version() == 3 and hasattr(_lib.load(), "ct_image_items")
