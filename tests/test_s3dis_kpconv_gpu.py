"""The S3DIS KPConv protocol on the device (cloud_transformers_amd.data.s3dis_kpconv): sampler invariants, a numpy replay of
the potential field (datasets/s3dis_closer.py:239-276), the voting evaluator against a numpy restatement of the reference's
loop and metrics (datasets/s3dis_closer_train.py:134-167, datasets/s3dis_closer_utils.py:252-333), and one training step of a
padded segmenter (model_zoo/s3dis/segmenter_pad.py's structure) on a sampled batch."""
import numpy as np
import pytest
import torch

from tests.test_nbr_gpu import area_like, brute_nearest

pytestmark = pytest.mark.gpu

R = 2.0


def _areas(seeds=(0, 1), n=20000):
    from cloud_transformers_amd.data.s3dis_kpconv import Area
    from cloud_transformers_amd.data.subsampling import grid_subsampling
    out = []
    for s in seeds:
        rng = np.random.default_rng(100 + s)
        pts = area_like(n, 200 + s, size=(9.0 + s, 6.0, 3.0))
        cols = rng.integers(0, 256, (pts.shape[0], 3)).astype(np.float32)
        labs = rng.integers(0, 13, pts.shape[0]).astype(np.int32)
        sp, sc, sl = grid_subsampling(pts, features=cols, labels=labs[:, None], sampleDl=0.04)
        out.append(Area("Area_%d" % (s + 1), pts, cols, labs, sp, sc / np.float32(255), sl[:, 0].astype(np.int32)))
    return out


@pytest.fixture(scope="module")
def areas():
    return _areas()


def _sampler(areas, N=4096, F=4, seed=0, drop=0.2):
    from cloud_transformers_amd.data.s3dis_kpconv import SphereSampler
    return SphereSampler(areas, N, in_radius=R, input_features_dim=F, color_drop=drop,
                         generator=torch.Generator(device="cuda").manual_seed(seed))


def _ball(P, c, N):
    """(sorted first min(count, N) indices, count, their float32 d2) of the float32 brute force"""
    d = P - c[None, :]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    r2 = np.float32(R) * np.float32(R)
    sel = np.nonzero(d2 <= r2)[0]
    o = sel[np.lexsort((sel, d2[sel]))]
    return o[:N], sel.size, d2[o[:N]]


def test_sampler_invariants(areas):
    from cloud_transformers_amd.data.s3dis_kpconv import COLOR_MEAN, COLOR_STD
    N = 4096
    smp = _sampler(areas, N)
    for _ in range(2):
        points, mask, feats, labels, cloud, inds = (t.cpu().numpy() for t in smp.sample(6))
        picks = [(ci, p.cpu().numpy()) for ci, _, p in smp.last_picks]
        assert points.shape == (6, N, 3) and mask.shape == (6, N) and mask.dtype == np.int32 and feats.shape == (6, 4, N)
        assert labels.dtype == np.int64 and cloud.dtype == np.int64 and inds.dtype == np.int64
        for b in range(6):
            ci, pick = picks[b]
            assert cloud[b] == ci
            a = areas[ci]
            want, count, _ = _ball(a.sub_points, pick, N)
            n = min(count, N)
            assert mask[b].sum() == n and (mask[b, :n] == 1).all()
            assert sorted(inds[b, :n].tolist()) == sorted(want.tolist())             # the ball's first N, permuted
            assert set(inds[b, n:].tolist()) <= set(inds[b, :n].tolist())          # padding repeats valid slots
            np.testing.assert_array_equal(points[b], a.sub_points[inds[b]] - pick[None, :])
            assert (np.linalg.norm(points[b].astype(np.float64), axis=1) <= R * (1 + 1e-5)).all()
            np.testing.assert_array_equal(labels[b], a.sub_labels[inds[b]].astype(np.int64))
            np.testing.assert_array_equal(feats[b, 3], a.sub_points[inds[b], 2])      # height = absolute z
            col = (a.sub_colors[inds[b]].astype(np.float64) - np.asarray(COLOR_MEAN)) / np.asarray(COLOR_STD)
            got = feats[b, :3].T
            assert np.allclose(got, col, atol=1e-5) or (got == 0).all()              # colour drop: all or nothing


def test_feature_layouts(areas):
    outs = {F: _sampler(areas, 1024, F=F, seed=3, drop=0.0).sample(2) for F in (1, 3, 4, 5)}
    p4, _, f4, *_ = outs[4]
    for F, (p, m, f, lab, c, i) in outs.items():
        assert f.shape == (2, F, 1024)
        assert torch.equal(p, p4)                                                   # same seed: same spheres
    assert torch.equal(outs[1][2][:, 0], f4[:, 3])
    assert torch.equal(outs[3][2], f4[:, :3])
    assert torch.equal(outs[5][2][:, 0], torch.ones_like(f4[:, 0])) and torch.equal(outs[5][2][:, 1:], f4)


def test_potentials_replay(areas):
    """Replaying the exposed picks in numpy (pick rule, ball, Tukey weights) gives the same potentials."""
    N = 2048
    smp = _sampler(areas, N, seed=7)
    pots = [p.cpu().numpy().copy() for p in smp.potentials]
    r2 = np.float32(R) * np.float32(R)
    for _ in range(3):
        smp.sample(4)
        for ci, pi, pick in smp.last_picks:
            mins = [p.min() for p in pots]
            assert ci == int(np.argmin(mins))
            assert int(pi) == int(np.argmin(pots[ci]))
            o, _, d2 = _ball(areas[ci].sub_points, pick.cpu().numpy(), N)
            pots[ci][o] += np.square(np.float32(1) - d2 / r2)
    for a, b in zip(pots, smp.potentials):
        np.testing.assert_allclose(b.cpu().numpy(), a, atol=1e-6, rtol=0)


def test_same_seed_same_batches(areas):
    a, b = _sampler(areas, 2048, seed=11), _sampler(areas, 2048, seed=11)
    for _ in range(2):
        for x, y in zip(a.sample(3), b.sample(3)):
            assert torch.equal(x, y)
    c = _sampler(areas, 2048, seed=12)
    assert not torch.equal(c.sample(3)[0], a.sample(3)[0])


def _iou_from_confusions(confusions):
    """s3dis_closer_utils.py:252-279"""
    TP = np.diagonal(confusions, axis1=-2, axis2=-1)
    TP_plus_FN = np.sum(confusions, axis=-1)
    TP_plus_FP = np.sum(confusions, axis=-2)
    IoU = TP / (TP_plus_FP + TP_plus_FN - TP + 1e-6)
    mask = TP_plus_FN < 1e-3
    counts = np.sum(1 - mask, axis=-1, keepdims=True)
    mIoU = np.sum(IoU, axis=-1, keepdims=True) / (counts + 1e-6)
    IoU += mask * mIoU
    return IoU


def _confusion(t, p, C):
    return np.bincount(t.astype(np.int64) * C + p, minlength=C * C).reshape(C, C)


def test_vote_evaluator_against_reference_loop(areas):
    from cloud_transformers_amd.data.s3dis_kpconv import VoteEvaluator
    C, N, smooth = 13, 2048, 0.95
    smp = _sampler(areas, N, seed=5)
    ev = VoteEvaluator(areas, num_classes=C, smooth=smooth)
    # the reference's state (s3dis_closer_train.py:72-88; runing_vote_logits starts at zero)
    vsum = [np.zeros((C, a.sub_labels.shape[0]), np.float32) for a in areas]
    vcnt = [np.zeros((1, a.sub_labels.shape[0]), np.float32) + 1e-6 for a in areas]
    run = [np.zeros((C, a.sub_labels.shape[0]), np.float32) for a in areas]
    props = np.zeros(C, np.float32)
    for k in range(C):
        props[k] = np.sum([np.sum(a.labels == k) for a in areas])
    g = torch.Generator(device="cuda").manual_seed(9)
    for _ in range(5):
        _, mask, _, _, cloud, inds = smp.sample(4)
        pred = torch.randn(4, C, N, generator=g, device="cuda")
        ev.add(pred, mask, cloud, inds)
        pn, mn, cn, iv = pred.cpu().numpy(), mask.cpu().numpy(), cloud.cpu().numpy(), inds.cpu().numpy()
        for ib in range(4):                                    # s3dis_closer_train.py:134-145
            m = mn[ib].astype(bool)
            logits = pn[ib][:, m]
            ii = iv[ib][m]
            c = int(cn[ib])
            vsum[c][:, ii] = vsum[c][:, ii] + logits
            vcnt[c][:, ii] += 1
            run[c][:, ii] = smooth * run[c][:, ii] + (1 - smooth) * logits
    vote = [s / n for s, n in zip(vsum, vcnt)]
    np.testing.assert_allclose(ev.vote_logits().cpu().numpy(), np.concatenate(vote, 1), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(ev.running[:, :-1].cpu().numpy(), np.concatenate(run, 1), rtol=1e-6, atol=1e-7)

    def sub_metrics(logits_list):                              # sub_s3dis_metrics
        Cf = np.sum(np.stack([_confusion(a.sub_labels, np.argmax(lg, axis=0), C) for lg, a in zip(logits_list, areas)]),
                    axis=0).astype(np.float32)
        Cf *= np.expand_dims(props / (np.sum(Cf, axis=1) + 1e-6), 1)
        iou = _iou_from_confusions(Cf)
        return iou, np.mean(iou)

    for got, want in ((ev.sub_ious(), sub_metrics(vote)), (ev.sub_ious(running=True), sub_metrics(run))):
        np.testing.assert_allclose(got[0], want[0], rtol=1e-5, atol=1e-6)
        assert abs(got[1] - want[1]) < 1e-6

    # s3dis_metrics: every raw point takes its nearest subsampled point's vote (brute-force reprojection here)
    Cf = 0
    for a, lg, p in zip(areas, vote, ev.projections()):
        proj, _ = brute_nearest(a.sub_points, a.points)
        np.testing.assert_array_equal(p.cpu().numpy(), proj)
        Cf = Cf + _confusion(a.labels, np.argmax(lg[:, proj], axis=0), C)
    want = _iou_from_confusions(Cf)
    got = ev.full_ious()
    np.testing.assert_allclose(got[0], want, rtol=1e-9, atol=1e-12)
    assert abs(got[1] - np.mean(want)) < 1e-9


class SegmenterPad(torch.nn.Module):
    """The structure of model_zoo/s3dis/segmenter_pad.py (stem on [xyz, features], MultiHeadUnion blocks cycling the zoo's
    three head configurations, each given (points, pts_pad), classifier head), narrower and shorter for a test."""

    def __init__(self, n_features=4, n_classes=13, dim=128):
        super().__init__()
        from torch import nn
        from cloud_transformers_amd.layers.multihead_ct import MultiHeadUnion
        zoo = [([4, 4], [128, 32]), ([16, 16], [64, 16]), ([16, 32], [16, 8])]
        self.first_process = nn.Sequential(nn.Conv1d(3 + n_features, dim, kernel_size=1, bias=True), nn.BatchNorm1d(dim),
                                           nn.ReLU(inplace=True))
        self.attentions_encoder = nn.ModuleList([MultiHeadUnion(model_dim=dim, features_dims=f, heads=[16, 16], tensor_sizes=s,
                                                                model_dim_out=dim, tensor_dims=[2, 3]) for f, s in zoo])
        self.final = nn.Sequential(nn.Conv1d(dim, dim, kernel_size=1, bias=False), nn.BatchNorm1d(dim), nn.ReLU(inplace=True),
                                   nn.Conv1d(dim, n_classes, kernel_size=1))

    def forward(self, points, pts_pad, features):
        input_pts = points.permute(0, 2, 1)
        x = self.first_process(torch.cat([input_pts, features], dim=1))
        for blk in self.attentions_encoder:
            x, _ = blk(x, (input_pts, pts_pad))
        return self.final(x)


def test_segmenter_step_on_sampled_batch(areas):
    torch.manual_seed(0)
    smp = _sampler(areas, 2048, seed=21)
    points, mask, features, labels, _, _ = smp.sample(2)
    model = SegmenterPad().cuda().train()
    pred = model(points, mask, features)
    assert pred.shape == (2, 13, 2048)
    m = mask.float()
    loss = (torch.nn.functional.cross_entropy(pred, labels, reduction="none") * m).sum() / m.sum()
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    grads = [p.grad for p in model.parameters() if p.requires_grad]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)


def test_colour_normalisation_and_drop(areas):
    """color_drop = 0: every item's colours are (colour - COLOR_MEAN) / COLOR_STD (s3dis_closer.py:118-119,347-352);
    color_drop = 1: all zero; in between, each item keeps all of its colours or none, and both happen."""
    from cloud_transformers_amd.data.s3dis_kpconv import COLOR_MEAN, COLOR_STD
    mean, std = np.asarray(COLOR_MEAN), np.asarray(COLOR_STD)

    def items(drop, calls, B=6):
        smp = _sampler(areas, 1024, seed=31, drop=drop)
        for _ in range(calls):
            _, _, feats, _, cloud, inds = (t.cpu().numpy() for t in smp.sample(B))
            for b in range(B):
                want = (areas[cloud[b]].sub_colors[inds[b]].astype(np.float64) - mean) / std
                yield feats[b, :3].T, want

    for got, want in items(0.0, 2):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
    for got, _ in items(1.0, 1):
        assert (got == 0).all()
    kept = dropped = 0
    for got, want in items(0.5, 4):
        if (got == 0).all():
            dropped += 1
        else:
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
            kept += 1
    assert kept > 0 and dropped > 0, (kept, dropped)
