"""ct_kp_items on the device (cloud_transformers_amd.data.s3dis_kpconv): `sample()` equals, bit for bit and draw for draw,
the torch sequence it replaced (restated here); augmented items equal a numpy float32 restatement from the (R, s, j) the
call used; the augmentation's draws cover the reference's ranges (train_segmentation_kpconv.py:84-130); count = 0."""
import numpy as np
import pytest
import torch

from tests.test_s3dis_kpconv_gpu import _areas

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def areas():
    return _areas(n=20000)


def _sampler(areas, N=2048, F=4, seed=0, drop=0.2):
    from cloud_transformers_amd.data.s3dis_kpconv import SphereSampler
    return SphereSampler(areas, N, in_radius=2.0, input_features_dim=F, color_drop=drop,
                         generator=torch.Generator(device="cuda").manual_seed(seed))


def _torch_sample(smp, B):
    """SphereSampler.sample as the torch sequence of the parent revision: per-item ball queries, then ~20 launches."""
    from cloud_transformers_amd.data.s3dis_kpconv import scene_seg_features
    smp.last_picks = []
    items = []
    for _ in range(B):
        ci, pick = smp._pick()
        idx, _, count = smp.indices[ci].query_radius(pick[None], smp.in_radius, smp.num_points)
        items.append((ci, pick, idx[0], count[0]))
    dev, N, gen = smp.device, smp.num_points, smp.gen
    cloud = torch.tensor([it[0] for it in items], dtype=torch.int64, device=dev)
    picks = torch.stack([it[1] for it in items])
    idx = torch.stack([it[2] for it in items])
    count = torch.stack([it[3] for it in items])
    nvalid = torch.clamp(count, max=N)
    slot = torch.arange(N, device=dev)[None, :]
    live = slot < nvalid[:, None]
    keys = torch.where(live, torch.rand(B, N, generator=gen, device=dev), torch.full((B, N), 2.0, device=dev))
    perm = torch.argsort(keys, dim=1)
    pad = torch.floor(torch.rand(B, N, generator=gen, device=dev) * nvalid[:, None]).long().clamp_(0, N - 1)
    src = torch.where(live, perm, perm.gather(1, pad))
    input_inds = idx.gather(1, src).clamp_(min=0)
    mask = live.to(torch.int32)
    g = input_inds + smp.offsets[cloud][:, None]
    original = smp._all_points[g]
    points = original - picks[:, None, :]
    height = original[:, :, 2:]
    colors = (smp._all_colors[g] - smp._mean) / smp._std
    drop = (torch.rand(B, generator=gen, device=dev) > smp.color_drop).float()
    colors = colors * drop[:, None, None]
    labels = smp._all_labels[g]
    features = scene_seg_features(smp.input_features_dim, points, colors, height)
    return points, mask, features, labels, cloud, input_inds


def _bits(t):
    t = t.cpu()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("F", [1, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("drop", [0.0, 0.2, 1.0])
def test_sample_bit_identical_to_the_torch_sequence(areas, F, drop):
    for seed in (0, 7):
        new, old = _sampler(areas, F=F, seed=seed, drop=drop), _sampler(areas, F=F, seed=seed, drop=drop)
        for call in range(2):
            got, want = new.sample(6), _torch_sample(old, 6)
            for k, (a, b) in enumerate(zip(got, want)):
                assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
                assert torch.equal(_bits(a), _bits(b)), (F, drop, seed, call, k)
        # the same draws were consumed: the generators are at the same state
        assert torch.equal(torch.rand(4, generator=new.gen, device="cuda"), torch.rand(4, generator=old.gen, device="cuda"))


def _np_points(areas, cloud, inds, pick):
    return areas[cloud].sub_points[inds].astype(np.float32) - pick.astype(np.float32)[None, :]


@pytest.mark.parametrize("F", [4, 6, 7])
def test_augmented_items_match_numpy_float32(areas, F):
    from cloud_transformers_amd.data.s3dis_kpconv import Augment
    aug, plain = _sampler(areas, F=F, seed=11), _sampler(areas, F=F, seed=11)
    cloud, picks = aug.plan(6)
    cloud2, picks2 = plain.plan(6)
    assert torch.equal(cloud, cloud2) and torch.equal(picks, picks2)
    points, mask, feats, labels, cl, inds = (t.cpu().numpy() for t in aug.items(cloud, picks, Augment()))
    R, s, j = (t.cpu().numpy() for t in aug.last_augment)
    p0, mask0, feats0, labels0, _, inds0 = (t.cpu().numpy() for t in plain.items(cloud, picks))
    assert R.shape == (6, 3, 3) and s.shape == (6, 3) and j.shape == (6, 2048, 3)
    np.testing.assert_array_equal(mask, mask0)                     # augmentation draws come after the slot draws
    np.testing.assert_array_equal(labels, labels0)
    np.testing.assert_array_equal(inds, inds0)
    pk = picks.cpu().numpy()
    for b in range(6):
        p = _np_points(areas, cl[b], inds[b], pk[b])
        np.testing.assert_array_equal(p, p0[b])
        want = np.empty_like(p)
        for i in range(3):
            q = (R[b, i, 0] * p[:, 0] + R[b, i, 1] * p[:, 1]) + R[b, i, 2] * p[:, 2]
            want[:, i] = q * s[b, i] + j[b, :, i]
        assert want.dtype == np.float32
        np.testing.assert_array_equal(points[b], want)
        z = areas[cl[b]].sub_points[inds[b], 2]
        if F == 4:
            np.testing.assert_array_equal(feats[b, 3], z)            # height: the un-augmented absolute z
        elif F == 6:
            np.testing.assert_array_equal(feats[b, 3:6], want.T)     # F = 6 / 7 take the augmented points
        else:
            np.testing.assert_array_equal(feats[b, 3], z)
            np.testing.assert_array_equal(feats[b, 4:7], want.T)
        np.testing.assert_array_equal(feats[b, :3], feats0[b, :3])   # colours untouched


def test_augment_draw_ranges():
    from cloud_transformers_amd.data.s3dis_kpconv import Augment
    gen = torch.Generator(device="cuda").manual_seed(5)
    R, s, j = (t.cpu().numpy() for t in Augment().draw(4096, 64, gen, "cuda"))
    ang = np.arctan2(R[:, 1, 0].astype(np.float64), R[:, 0, 0].astype(np.float64))
    assert ang.min() < -3.1 and ang.max() > 3.1
    assert np.all(np.abs(ang) <= 3.1415926 + 1e-6)
    np.testing.assert_array_equal(R[:, 2], np.tile(np.float32([0, 0, 1]), (4096, 1)))      # about z only
    assert (s[:, 0] < 0).any() and (s[:, 0] > 0).any()                                      # x mirrors ...
    assert (s[:, 1:] > 0).all()                                                             # ... only x
    a = np.abs(s)
    assert a.min() >= 0.7 - 1e-6 and a.max() <= 1.3 + 1e-6 and a.min() < 0.72 and a.max() > 1.28
    assert np.abs(j).max() <= 0.05 and 0.0008 < j.std() < 0.0012
    _, _, j = (t.cpu().numpy() for t in Augment(std=0.05).draw(512, 64, gen, "cuda"))
    assert np.abs(j).max() == np.float32(0.05)                                              # clipped at +-clip


def test_count_zero(areas):
    """A pick with an empty ball: mask all zero, indices 0, every slot the cloud's point 0 (what the torch code gives)."""
    from cloud_transformers_amd.data.s3dis_kpconv import COLOR_MEAN, COLOR_STD, kp_items
    smp = _sampler(areas, N=256, F=7, seed=3)
    B, N = 2, 256
    dev = "cuda"
    idx = torch.full((B, N), -1, dtype=torch.int64, device=dev)
    count = torch.zeros(B, dtype=torch.int64, device=dev)
    keys = torch.full((B, N), 2.0, device=dev)
    perm = torch.argsort(keys, dim=1)
    u = torch.rand(B, N, device=dev)
    cloud = torch.tensor([0, 1], device=dev)
    picks = torch.tensor([[100.0, 100.0, 100.0], [1.0, 2.0, 3.0]], device=dev)
    drop = torch.ones(B, device=dev)
    pts, mask, feats, labels, inds = kp_items(idx, count, perm, u, smp.offsets[cloud], picks, drop, smp._all_points,
                                              smp._all_colors, smp._all_labels, COLOR_MEAN, COLOR_STD, 7)
    assert int(mask.abs().sum()) == 0 and int(inds.abs().sum()) == 0
    for b in range(B):
        g = int(smp.offsets[cloud[b]])
        assert torch.equal(pts[b], (smp._all_points[g] - picks[b])[None].expand(N, 3))
        assert torch.equal(labels[b], smp._all_labels[g].expand(N))
        assert torch.equal(feats[b, 3], smp._all_points[g, 2].expand(N))
