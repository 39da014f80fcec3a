"""The ShapeNet completion pieces without a GPU: ct_completion_items refuses bad arguments before touching the device;
read_pcd round-trips ASCII and binary files; the file list, the rendering choice and the two point transforms of
cloud_transformers_amd.data.completion.

The expectations for the file list, RandomSamplePoints and RandomMirrorPoints come from the cited lines of the upstream
datasets/grnet_completion.py (:246-258, :297-314, :400-512), not from running it: that module imports open3d, cv2, h5py and
transforms3d, none of which is installed where these fixtures are made, so it cannot produce a fixture."""
import ctypes
import json
import random

import numpy as np
import pytest
import torch

from tests.completion_tree import write_pcd


@pytest.fixture(scope="module")
def lib():
    from cloud_transformers_amd import _lib
    _lib.build()
    return _lib.load()


def test_completion_items_rejects_bad_arguments(lib):
    from cloud_transformers_amd import _lib
    b = ctypes.create_string_buffer(256)
    p = ctypes.cast(b, ctypes.c_void_p)

    def call(*, ins=(p,) * 4, scale=2.0, B=2, n_in=16, gt=64, outs=(p,) * 3):
        return lib.ct_completion_items(*ins, scale, B, n_in, gt, *outs, None)

    for k in range(4):                                                     # every null input
        ins = [p] * 4
        ins[k] = None
        assert call(ins=tuple(ins)) == -1, k
    for k in range(3):                                                     # every null output
        outs = [p] * 3
        outs[k] = None
        assert call(outs=tuple(outs)) == -1, k
    assert call(B=0) == -1 and call(B=-1) == -1 and call(B=65536) == -1
    assert call(n_in=0) == -1 and call(n_in=-4) == -1
    assert call(n_in=_lib.COMPLETION_N_MAX + 1, gt=1 << 20) == -1
    assert call(gt=15) == -1 and call(gt=0) == -1                          # gt < n_in
    assert call(gt=_lib.COMPLETION_GT_MAX + 1) == -1 and call(gt=1 << 40) == -1
    for scale in (0.0, -0.0, float("inf"), -float("inf"), float("nan")):
        assert call(scale=scale) == -1, scale
    del b


@pytest.mark.parametrize("encoding", ["ascii", "binary"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("extra", [False, True])
def test_read_pcd_round_trips(tmp_path, encoding, dtype, extra):
    from cloud_transformers_amd.data.completion import read_pcd
    rng = np.random.default_rng(3)
    xyz = rng.normal(size=(37, 3)).astype(dtype)
    xyz[4] = 0.0
    path = tmp_path / "cloud.pcd"
    write_pcd(path, xyz, encoding, dtype, extra)
    got = read_pcd(path)
    assert got.dtype == np.float32 and got.shape == (37, 3)
    np.testing.assert_array_equal(got, xyz.astype(np.float32))


def test_read_pcd_refuses_binary_compressed(tmp_path):
    from cloud_transformers_amd.data.completion import read_pcd
    path = tmp_path / "packed.pcd"
    write_pcd(path, np.zeros((2, 3), np.float32), "binary_compressed")
    with pytest.raises(ValueError) as ex:
        read_pcd(path)
    assert "packed.pcd" in str(ex.value) and "binary_compressed" in str(ex.value)


def _loader(tmp_path, n_renders=3):
    from cloud_transformers_amd.data.completion import ShapeNetDataLoader
    cats = [{"taxonomy_id": "t1", "taxonomy_name": "one", "train": ["m1", "m2"], "val": ["m2"], "test": ["m1"]},
            {"taxonomy_id": "t2", "taxonomy_name": "two", "train": ["m3"], "val": [], "test": ["m3"]}]
    (tmp_path / "cats.json").write_text(json.dumps(cats))
    root = str(tmp_path)
    return ShapeNetDataLoader(str(tmp_path / "cats.json"), root + "/%s/partial/%s/%s/%02d.pcd", root + "/%s/complete/%s/%s.pcd",
                              n_renders=n_renders, n_input=8, n_output=16)


def test_file_list_and_rendering_choice(tmp_path):
    """grnet_completion.py:417-424, :489-512: one entry per model in category order, `n_renders` renderings listed for TRAIN and
    one otherwise; :385: TRAIN draws the rendering with random.randint, the other subsets read rendering 0."""
    from cloud_transformers_amd.data.completion import DatasetSubset
    import datasets.grnet_completion as shim
    assert shim.ShapeNetDataLoader is not None and shim.DatasetSubset is DatasetSubset and shim.collate_fn is not None
    root = str(tmp_path)
    ld = _loader(tmp_path)
    train = ld.get_dataset(DatasetSubset.TRAIN)
    assert [(s["taxonomy_id"], s["model_id"]) for s in train.file_list] == [("t1", "m1"), ("t1", "m2"), ("t2", "m3")]
    assert train.file_list[1]["partial_cloud_path"] == [root + "/train/partial/t1/m2/%02d.pcd" % i for i in range(3)]
    assert train.file_list[2]["gtcloud_path"] == root + "/train/complete/t2/m3.pcd"
    val, test = ld.get_dataset(DatasetSubset.VAL), ld.get_dataset(DatasetSubset.TEST)
    assert [(s["taxonomy_id"], s["model_id"]) for s in val.file_list] == [("t1", "m2")]
    assert val.file_list[0]["partial_cloud_path"] == [root + "/val/partial/t1/m2/00.pcd"]
    assert [s["gtcloud_path"] for s in test.file_list] == [root + "/test/complete/t1/m1.pcd", root + "/test/complete/t2/m3.pcd"]
    assert train.options["shuffle"] and not val.options["shuffle"] and not test.options["shuffle"]
    assert (train.options["n_renderings"], val.options["n_renderings"], test.options["n_renderings"]) == (3, 1, 1)

    # rendering r of every model holds the constant r + 1: the item tells which file was read
    for subset, models in (("train", [("t1", "m1"), ("t1", "m2"), ("t2", "m3")]), ("val", [("t1", "m2")]), ("test", [("t1", "m1"), ("t2", "m3")])):
        for t, m in models:
            write_pcd(tmp_path / subset / "complete" / t / (m + ".pcd"), np.full((20, 3), 9.0, np.float32), "binary")
            for r in range(3 if subset == "train" else 1):
                write_pcd(tmp_path / subset / "partial" / t / m / ("%02d.pcd" % r), np.full((5 + r, 3), r + 1.0, np.float32))
    random.seed(5)
    np.random.seed(5)
    seen = set()
    for _ in range(40):
        tax, mid, data = train[1]
        assert (tax, mid) == ("t1", "m2")
        part, gt = data["partial_cloud"], data["gtcloud"]
        assert part.dtype == torch.float32 and tuple(part.shape) == (8, 3) and tuple(gt.shape) == (16, 3)
        r = int(abs(float(part[0, 1])))                                    # (y is never mirrored)
        seen.add(r - 1)
        assert int((part.abs().sum(1) > 0).sum()) == min(5 + (r - 1), 8)   # rendering r-1 has 5 + (r-1) rows, the rest is padding
    assert seen == {0, 1, 2}
    for ds in (val, test):
        for _ in range(5):
            _, _, data = ds[0]
            assert float(data["partial_cloud"][0, 1]) == 1.0               # rendering 0
    assert tuple(test[0][2]["gtcloud"].shape) == (20, 3)                   # TEST leaves gtcloud unsampled
    assert tuple(val[0][2]["gtcloud"].shape) == (16, 3)
    from cloud_transformers_amd.data.completion import collate_fn
    tax, mids, data = collate_fn([val[0], val[0]])
    assert tax == ["t1", "t1"] and mids == ["m2", "m2"] and tuple(data["partial_cloud"].shape) == (2, 8, 3)


def test_random_sample_points_pads_with_zeros_and_never_repeats():
    """grnet_completion.py:246-258: ptcloud[permutation[:n]], then zero rows up to n."""
    from cloud_transformers_amd.data.completion import RandomSamplePoints
    np.random.seed(0)
    cloud = np.arange(1, 31, dtype=np.float32)[:, None] * np.ones((1, 3), np.float32)        # distinct non-zero rows
    short = RandomSamplePoints({"n_points": 48})(cloud)
    assert short.shape == (48, 3)
    assert sorted(short[:30, 0].tolist()) == cloud[:, 0].tolist() and not short[30:].any()
    assert short[:30, 0].tolist() != cloud[:, 0].tolist()                  # a permutation, not the identity
    cut = RandomSamplePoints({"n_points": 12})(cloud)
    assert cut.shape == (12, 3) and len(set(cut[:, 0].tolist())) == 12 and set(cut[:, 0].tolist()) <= set(cloud[:, 0].tolist())
    same = RandomSamplePoints({"n_points": 30})(cloud)
    assert sorted(same[:, 0].tolist()) == cloud[:, 0].tolist()


@pytest.mark.parametrize("draw,sx,sz", [(0.0, -1, -1), (0.1, -1, -1), (0.25, -1, -1), (np.nextafter(0.25, 1), -1, 1), (0.4, -1, 1),
                                        (0.5, -1, 1), (np.nextafter(0.5, 1), 1, -1), (0.6, 1, -1), (0.75, 1, -1),
                                        (np.nextafter(0.75, 1), 1, 1), (0.9, 1, 1), (1.0, 1, 1)])
def test_random_mirror_points_ranges(draw, sx, sz):
    """grnet_completion.py:297-314: <= 0.25 mirrors x and z, (0.25, 0.5] x, (0.5, 0.75] z, above nothing."""
    from cloud_transformers_amd.data.completion import RandomMirrorPoints
    rng = np.random.default_rng(1)
    cloud = rng.normal(size=(11, 3)).astype(np.float32)
    got = RandomMirrorPoints()(cloud.copy(), draw)
    np.testing.assert_array_equal(got, cloud * np.array([sx, 1, sz], np.float32))


def test_mirror_takes_one_draw_for_both_clouds(monkeypatch):
    """grnet_completion.py:118-135: Compose draws once per transform and hands the same value to every object."""
    from cloud_transformers_amd.data import completion as C
    ld = C.ShapeNetDataLoader.__new__(C.ShapeNetDataLoader)
    ld.n_input, ld.n_output = 6, 9
    chain = ld._get_transforms(C.DatasetSubset.TRAIN)
    assert [type(t).__name__ for t, _ in chain.transformers] == ["RandomSamplePoints", "RandomSamplePoints", "RandomMirrorPoints", "ToTensor"]
    assert [type(t).__name__ for t, _ in ld._get_transforms(C.DatasetSubset.VAL).transformers] == ["RandomSamplePoints", "RandomSamplePoints", "ToTensor"]
    assert [(type(t).__name__, o) for t, o in ld._get_transforms(C.DatasetSubset.TEST).transformers] == [
        ("RandomSamplePoints", ["partial_cloud"]), ("ToTensor", ["partial_cloud", "gtcloud"])]
    for draw, sx, sz in ((0.1, -1, -1), (0.3, -1, 1), (0.7, 1, -1), (0.8, 1, 1)):
        draws = []

        def uniform(lo, hi, _d=draw):
            draws.append(_d)
            return _d
        monkeypatch.setattr(np.random, "uniform", uniform)
        data = chain({"partial_cloud": np.ones((6, 3), np.float32), "gtcloud": np.full((9, 3), 2.0, np.float32)})
        assert len(draws) == 4                                             # one per transform
        for key, c in (("partial_cloud", 1.0), ("gtcloud", 2.0)):
            assert data[key].dtype == torch.float32
            assert torch.equal(data[key], torch.tensor([sx * c, c, sz * c]).expand_as(data[key])), (draw, key)


def test_entry_point_config_defaults(tmp_path):
    from cloud_transformers_amd.train_completion import _parse, completion_config
    raw = {"data": {"batch_size": 2, "gt_size": 8192}, "train": {"chamfer_weight": 0.0}}
    cfg = completion_config(raw)
    assert cfg["data"] == {"batch_size": 2, "gt_size": 8192, "kind": "shapenet_completion", "n_renders": 1, "input_size": 2048,
                           "seed": 0, "batch_size_val": 2}
    assert cfg["train"]["val_emd_eps"] == 0.004 and cfg["train"]["val_emd_iters"] == 3000 and "kind" not in raw["data"]
    args = _parse(["exp", "-c", "x.yaml", "--eval"])
    assert args.eval and args.gpus == 1
    import utils.pcd_utils as shim
    assert shim.partial_postproces is not None and shim.sphere_noise is not None and shim.resample_pcd is not None
