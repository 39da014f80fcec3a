"""The S3DIS KPConv training pieces without a GPU: ct_kp_items refuses bad arguments before touching the device, the epoch
plan's sharding equals DistributedSampler(shuffle=False) + DataLoader(drop_last=True), the entry point's defaults on the
reference config's keys, and the rotation factors against angle_axis (datasets/s3dis_closer_utils.py:8-36)."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from cloud_transformers_amd import _lib
    _lib.build()
    return _lib.load()


def test_kp_items_rejects_bad_arguments(lib):
    from cloud_transformers_amd import _lib
    b = ctypes.create_string_buffer(256)
    p = ctypes.cast(b, ctypes.c_void_p)
    m, s = _lib.float_array([0.5, 0.5, 0.5]), _lib.float_array([0.2, 0.2, 0.2])

    def call(*, ins=(p,) * 10, M=8, mean=m, std=s, aug=(None, None, None), B=2, N=16, F=4, outs=(p,) * 5):
        return lib.ct_kp_items(*ins, M, mean, std, *aug, B, N, F, *outs, None)

    assert lib.ct_kp_items.argtypes is not None
    for k in range(10):                                                    # every null input
        ins = [p] * 10
        ins[k] = None
        assert call(ins=tuple(ins)) == -1, k
    for k in range(5):                                                     # every null output
        outs = [p] * 5
        outs[k] = None
        assert call(outs=tuple(outs)) == -1, k
    assert call(mean=None) == -1 and call(std=None) == -1
    assert call(B=0) == -1 and call(B=-3) == -1
    assert call(N=0) == -1 and call(N=_lib.NBR_K_MAX + 1) == -1
    assert call(M=0) == -1
    for F in (0, 2, 8, -1):
        assert call(F=F) == -1, F
    for aug in ((p, None, None), (None, p, None), (None, None, p), (p, p, None), (None, p, p)):
        assert call(aug=aug) == -1, aug                                    # R, s and j: all three or none
    del b


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n,bs", [(24, 6), (25, 4), (2000, 6), (7, 3)])
def test_plan_sharding_matches_distributed_sampler(world, n, bs):
    from cloud_transformers_amd.train_kpconv import shard_batches

    class Items(torch.utils.data.Dataset):
        def __len__(self):
            return n

        def __getitem__(self, i):
            return i

    for rank in range(world):
        smp = torch.utils.data.distributed.DistributedSampler(Items(), num_replicas=world, rank=rank, shuffle=False)
        want = [b.tolist() for b in torch.utils.data.DataLoader(Items(), batch_size=bs, sampler=smp, drop_last=True)]
        assert shard_batches(n, rank, world, bs) == want, (rank, world)
        keep = [b.tolist() for b in torch.utils.data.DataLoader(Items(), batch_size=bs, sampler=smp, drop_last=False)]
        assert shard_batches(n, rank, world, bs, drop_last=False) == keep, (rank, world)


REFERENCE_YAML = """
experiment:
    root: '{root}/exp'
    writer_root: '{root}/runs'
data:
    path: '{root}/Stanford3dDataset_v1.2'
    batch_size: 6
    batch_size_val: 6
    num_workers: 4
    num_points: 8192
    test_area: 'Area_5'
    data_percent: !!float 1.0
    aug: True
model:
    generator: './model_zoo/s3dis/segmenter_pad.py'
train:
    label_smooth: False
    num_epochs: 600
    show_each: 2000
    save_each: 25000
    save_each_epoch: 1
    val_step: 1
    optimizer:
        type: 'Adam'
        lr: !!float 1e-3
        betas: [!!float 0.9, !!float 0.999]
        weight_decay: !!float 0.0
    scheduler:
       type: 'StepLR'
       gamma: !!float 0.7
       step_size: 25000
"""


def test_entry_point_config_defaults(tmp_path):
    """configs/s3dis_kpconv.yaml as the reference ships it (no `kind`): FakeCFG's values (train_segmentation_kpconv.py:84-114)
    fill what it lacks, the keys it has are kept."""
    from cloud_transformers_amd import harness
    from cloud_transformers_amd.train_kpconv import _parse, kpconv_config
    path = tmp_path / "s3dis_kpconv.yaml"
    path.write_text(REFERENCE_YAML.format(root=tmp_path))
    raw = harness.load_config(path)
    cfg = kpconv_config(raw)
    d, t = cfg["data"], cfg["train"]
    assert d["kind"] == "s3dis_kpconv" and d["num_steps"] == 2000 and d["input_features_dim"] == 4 and d["num_classes"] == 13
    assert d["sampleDl"] == 0.04 and d["in_radius"] == 2.0 and d["color_drop"] == 0.2 and d["val_color_drop"] == 0.2
    assert d["test_area"] == "Area_5" and d["batch_size"] == 6 and d["num_points"] == 8192
    assert t["clip_grad_norm"] == 10 and t["val_step"] == 1 and t["save_each_epoch"] == 1
    assert t["val_votes"] == 2 and t["final_votes"] == 20 and t["num_epochs"] == 600
    assert "kind" not in raw["data"]                                       # the caller's config is not modified
    args = _parse(["exp", "-c", str(path)])
    assert args.gpus == 1 and not args.eval
    args = _parse(["exp", "-c", str(path), "--gpus", "2", "--eval"])
    assert args.gpus == 2 and args.eval


def _angle_axis_reference(angle, axis):
    """angle_axis of s3dis_closer_utils.py:8-36, restated in numpy float64, rounded to float32."""
    u = axis / np.linalg.norm(axis)
    cosval, sinval = np.cos(angle), np.sin(angle)
    cross = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return (cosval * np.eye(3) + sinval * cross + (1.0 - cosval) * np.outer(u, u)).astype(np.float32)


def test_rotation_factors_match_angle_axis():
    from cloud_transformers_amd.data.s3dis_kpconv import rotation_factors
    rng = np.random.default_rng(0)
    angles = rng.uniform(-3.1415926, 3.1415926, (64, 3))
    angles[0] = 0.0
    angles[1] = [3.1415926, -3.1415926, 1e-9]
    Rx, Ry, Rz = (f.numpy() for f in rotation_factors(torch.from_numpy(angles)))
    for b in range(angles.shape[0]):
        for R, a, ax in ((Rx, 0, [1.0, 0, 0]), (Ry, 1, [0, 1.0, 0]), (Rz, 2, [0, 0, 1.0])):
            want = _angle_axis_reference(angles[b, a], np.array(ax))
            np.testing.assert_array_equal(R[b], want)
    assert Rx.dtype == np.float32 and Rx.shape == (64, 3, 3)
    np.testing.assert_array_equal(Rx[0], np.eye(3, dtype=np.float32))
