"""The fused metric table ct_chamfer_metrics, `Metrics.get_batch` against the per-sample `Metrics.get`, and
`train_completion.evaluate` at a test batch size above one against a per-sample recomputation."""
import ctypes

import numpy as np
import pytest
import torch

from tests.chamfer_counts_cases import counts_tensor, forward_case

pytestmark = pytest.mark.gpu

TH = 0.3      # the lattice gives sqrt(d) = sqrt(k) / 4: the nearest values, 0.25 and 0.3536, are far from it


def _metrics(d1, d2, c1, c2, th):
    """ct_chamfer_metrics through the C ABI -> (stats f64[B,2,3], table f32[B,4])."""
    from cloud_transformers_amd import _lib
    from cloud_transformers_amd.ops import _stream
    B, n, m = d1.shape[0], d1.shape[1], d2.shape[1]
    stats = torch.full((B, 2, 3), -1.0, dtype=torch.float64, device=d1.device)
    table = torch.full((B, 4), -1.0, dtype=torch.float32, device=d1.device)
    _lib.check(_lib.load().ct_chamfer_metrics(d1.data_ptr(), d2.data_ptr(), c1.data_ptr(), c2.data_ptr(), ctypes.c_float(th),
                                              stats.data_ptr(), table.data_ptr(), B, n, m, _stream(d1.device)), "ct_chamfer_metrics")
    return stats, table


def test_chamfer_metrics_on_the_forward_case():
    from cloud_transformers_amd.chamfer import chamfer_with_counts
    from cloud_transformers_amd.metrics import cloud_metrics, fscore_batch
    a, b, cnt1, cnt2, want = forward_case()
    ac, bc, c1, c2 = a.cuda(), b.cuda(), counts_tensor(cnt1), counts_tensor(cnt2)
    d1, d2, _, _ = chamfer_with_counts(ac, bc, c1, c2)
    assert torch.equal(d1.cpu(), want[0]) and torch.equal(d2.cpu(), want[1])
    stats, table = _metrics(d1, d2, c1, c2, TH)
    stats2, table2 = _metrics(d1, d2, c1, c2, TH)
    assert torch.equal(stats.view(torch.int64), stats2.view(torch.int64)) and torch.equal(table.view(torch.int32), table2.view(torch.int32))
    assert torch.equal(cloud_metrics(ac, bc, TH, c1, c2).view(torch.int32), table.view(torch.int32))      # the public path: the same table
    stats, table = stats.cpu().numpy(), table.cpu()
    for k in range(a.shape[0]):
        n1, n2 = cnt1[k], cnt2[k]
        for side, (d, c) in enumerate(((d1[k, :n1], n1), (d2[k, :n2], n2))):
            hits, sum_d, sum_s = stats[k, side]
            assert hits == int((torch.sqrt(d) < TH).sum()), (k, side)
            d32 = d.cpu().numpy()
            ref_d, ref_s = float(np.sum(d32.astype(np.float64))), float(np.sum(np.sqrt(d32).astype(np.float64)))
            print("cloud %d side %d: hits %d, sum d %.17g (numpy %.17g), sum sqrt %.17g (numpy %.17g)" % (k, side, hits, sum_d, ref_d, sum_s, ref_s))
            assert abs(sum_d - ref_d) <= 1e-12 * abs(ref_d) and abs(sum_s - ref_s) <= 1e-12 * abs(ref_s), (k, side)
        if n1 == 0 or n2 == 0:
            assert table[k, :3].tolist() == [0.0, 0.0, 0.0] and bool(torch.isnan(table[k, 3])), k
            continue
        fpr = fscore_batch(ac[k:k + 1, :n1], bc[k:k + 1, :n2], TH)[0].cpu()
        assert torch.equal(table[k, :3], fpr), (k, table[k].tolist(), fpr.tolist())
        cd = float(np.sum(d1[k, :n1].cpu().numpy().astype(np.float64)) / n1 + np.sum(d2[k, :n2].cpu().numpy().astype(np.float64)) / n2)
        assert abs(float(table[k, 3]) - cd) <= 1e-6 * abs(cd), (k, float(table[k, 3]), cd)
    assert 0.0 < float(table[3, 0]) < 1.0       # 129 queries against 7 targets: a threshold that splits the distances


def test_chamfer_metrics_null_counts_and_null_stats():
    from cloud_transformers_amd.metrics import cloud_metrics, fscore_batch
    g = torch.Generator().manual_seed(8)
    a = (torch.randint(0, 6, (2, 333, 3), generator=g).float() / 4).cuda()
    b = (torch.randint(0, 6, (2, 70, 3), generator=g).float() / 4).cuda()
    table = cloud_metrics(a, b, TH)
    assert torch.equal(table[:, :3], fscore_batch(a, b, TH))


@pytest.mark.parametrize("zeros", [0, 37, 511])
def test_get_batch_equals_get_per_sample(zeros):
    """B3 n512 m512 with `zeros` all-zero rows appended to every cloud (what ignore_zeros drops): the F-score of the clouds as
    given equals `Metrics.get`'s per sample; Chamfer x 1000 within 1e-5 relative (`Metrics.get`'s float32 torch mean is the
    looser side: 512 + zeros terms of half an ulp each, summed pairwise)."""
    from cloud_transformers_amd.metrics import Metrics
    from tests.test_metrics_gpu import _clouds
    pr, gt = _clouds(3, 512, 512, seed=zeros + 1)
    pad = torch.zeros(3, zeros, 3)
    pred = torch.cat([pr.permute(0, 2, 1), pad], dim=1).contiguous().cuda()
    gtc = torch.cat([gt.permute(0, 2, 1), pad], dim=1).contiguous().cuda()
    got = Metrics.get_batch(pred, gtc)
    assert tuple(got.shape) == (3, 2) and got.dtype == torch.float32 and got.is_cuda
    dense = Metrics.get_batch(pred, gtc, with_dense=True)
    assert torch.equal(dense[:, :2], got)
    for k in range(3):
        f, cd = Metrics.get(pred[k:k + 1], gtc[k:k + 1])
        print("cloud %d: F-Score %.9g (get %.9g), Chamfer x 1000 %.9g (get %.9g)" % (k, float(got[k, 0]), f, float(got[k, 1]), cd))
        assert float(got[k, 0]) == f, k
        assert abs(float(got[k, 1]) - cd) <= 1e-5 * abs(cd), k


# ---------------------------------------------------------------------------------------------------------------------
# evaluate at data.batch_size_test = 3
class _Stub(torch.nn.Module):
    """A fixed function of its inputs: the labelled noise cloud slightly inflated (its rows labelled 1 are the partial cloud's,
    which lie on the ground truth, so F-Score@0.01 is neither 0 nor 1), the first seven points zeroed (padding for
    ignore_zeros to drop), shifted by the partial cloud's mean times 1e-3.  Records the batch sizes it saw."""

    def __init__(self):
        super().__init__()
        self.batches = []

    def forward(self, noise, part):
        self.batches.append(noise.shape[0])
        rec = noise[:, :3] * 1.004 + 1e-3 * part[:, :, 0].mean(dim=2, keepdim=True)
        rec = torch.cat([torch.zeros_like(rec[:, :, :7]), rec[:, :, 7:]], dim=2)
        return rec[:, :, None], None


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The tiny tree of tests/completion_tree.py with five models in two taxonomies (batches of 3 and 2)."""
    from tests import completion_tree
    root = tmp_path_factory.mktemp("completion_eval")
    saved = completion_tree.TAXONOMIES
    completion_tree.TAXONOMIES = {"02691156": ["a1", "a2"], "03001627": ["c1", "c2", "c3"]}      # a batch that mixes taxonomies
    try:
        keys = completion_tree.make_tree(root, 64, 256)
    finally:
        completion_tree.TAXONOMIES = saved
    return keys


@pytest.mark.parametrize("source", ["host_loader", "resident"])
def test_evaluate_in_batches_of_three(tree, source, monkeypatch):
    """The table of `evaluate` at data.batch_size_test = 3 against the per-sample `Metrics.get` / `ChamferDistance` on the very
    (dense, gt) tensors the loop scored: counts equal, F-Score within 1e-6 absolute, Chamfer and dense loss within 1e-5
    relative.  The whole loop, from the first batch to the meter's copy, runs under torch's sync debug mode "error"."""
    from cloud_transformers_amd import metrics as M
    from cloud_transformers_amd import train_completion as T
    from cloud_transformers_amd.data.completion import DatasetSubset, DeviceShapeNetCompletion, shapenet_loader
    dev = torch.device("cuda", 0)
    cfg = T.completion_config({"data": dict(tree, batch_size_test=3, num_workers=0)})
    ds = shapenet_loader(cfg["data"]).get_dataset(DatasetSubset.TEST)
    resident = DeviceShapeNetCompletion(ds, dev) if source == "resident" else None
    ids = [s["taxonomy_id"] for s in ds.file_list]
    assert len(ids) == 5 and len(set(ids)) == 2

    seen = []
    original_get_batch = M.Metrics.get_batch.__func__
    original_result = M.TableMeter.result

    def recording(cls, pred, gt, *args, **kwargs):
        seen.append((pred.clone(), gt.clone()))
        return original_get_batch(cls, pred, gt, *args, **kwargs)

    def result(self):
        torch.cuda.set_sync_debug_mode("default")          # the loop is over: the one copy may synchronise
        return original_result(self)

    monkeypatch.setattr(M.Metrics, "get_batch", classmethod(recording))
    monkeypatch.setattr(M.TableMeter, "result", result)
    model = _Stub().to(dev)
    T.evaluate(model, cfg, dev, verbose=False, resident=resident)                 # (library load, allocator warm-up)
    seen.clear()
    model.batches.clear()
    probe = torch.ones(1, device=dev).sum()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                   # the mode is live
        res = T.evaluate(model, cfg, dev, verbose=False, resident=resident)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert model.batches == [3, 2] and [p.shape[0] for p, _ in seen] == [3, 2]

    chamfer = M.ChamferDistance()
    per_sample = []
    for pred, gt in seen:
        for k in range(pred.shape[0]):
            f, cd = M.Metrics.get(pred[k:k + 1], gt[k:k + 1])
            per_sample.append((f, cd, chamfer(pred[k:k + 1], gt[k:k + 1]).item() * 1000))
    assert len(per_sample) == 5
    assert res["names"] == ["F-Score", "ChamferDistance"] and list(res["taxonomies"]) == ["02691156", "03001627"]

    def check(row, rows):
        assert row["count"] == len(rows)
        f, cd = np.mean([r[0] for r in rows]), np.mean([r[1] for r in rows])
        print("count %d: F-Score %.9g (per sample %.9g), Chamfer %.9g (per sample %.9g)" % (row["count"], row["avg"][0], f, row["avg"][1], cd))
        assert abs(row["avg"][0] - f) <= 1e-6 and abs(row["avg"][1] - cd) <= 1e-5 * abs(cd)

    for t in set(ids):
        check(res["taxonomies"][t], [r for r, i in zip(per_sample, ids) if i == t])
    check(res["overall"], per_sample)
    dense = np.mean([r[2] for r in per_sample])
    assert abs(res["dense_loss"] - dense) <= 1e-5 * abs(dense)
    assert 0.0 < res["overall"]["avg"][0] < 1.0 and np.isfinite(res["overall"]["avg"][1])
    import json
    assert json.loads(json.dumps(res)) == res              # plain numbers: completion_test.json keeps its layout
