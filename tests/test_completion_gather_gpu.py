"""ct_completion_gather on the device (cloud_transformers_amd.data.completion): equal to the numpy restatement of its contract
(tests/completion_gather_ref.py, which tests/test_completion_gather_cpu.py ties to the host Dataset / Compose / collate chain)
over the cloud lengths, mirror draws and shapes at which the kernel takes another path; `DeviceCompletionBatches` on a tiny
dataset tree against the restated gather followed by `completion_items_from_draws` on recovered draws; no device-to-host
synchronisation; a HIP-graph replay with fresh draws; two steps, a validation and the test-split table of `harness.Trainer` /
`train_completion` on `data.kind: shapenet_completion_device`."""
import json
import os

import numpy as np
import pytest
import torch

from tests.completion_gather_ref import bits, reference_gather, synthetic_split

pytestmark = pytest.mark.gpu

# the smallest shapes at which each path can break: lengths around a wave / a ballot word (64), n_in and p_cap; gt lengths
# below, at and above n_out up to g_cap
N_IN, P_CAP, N_OUT, G_CAP, R = 128, 200, 256, 300, 2
P_LENGTHS = [1, 63, 64, 65, 127, 128, 129, 200]
G_LENGTHS = [251, 256, 293, 300]
U_MIRROR = [0.0, 0.25, float(np.nextafter(np.float32(0.25), np.float32(1))), 0.5, float(np.nextafter(np.float32(0.5), np.float32(1))),
            0.75, float(np.nextafter(np.float32(0.75), np.float32(1))), 0.99]
ITEM = [0, 0, 1, 1, 2, 2, 3, 3]                                            # repeated items ...
RENDERING = [0, 1, 0, 1, 0, 1, 0, 1]                                       # ... of mixed renderings: every stored cloud once


def _dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def split():
    """Host arrays of 4 models x 2 renderings with the lengths above; the second row of every cloud is exactly (0, 0, 0)."""
    return synthetic_split(P_LENGTHS, G_LENGTHS, R, seed=1)


def resident(arrays, n_in, n_out, R=R, sampled_gt=True):
    from cloud_transformers_amd.data.completion import DeviceShapeNetCompletion
    return DeviceShapeNetCompletion.from_arrays(*arrays, R, n_in, n_out, _dev(), sampled_gt=sampled_gt)


def draws(B, p_cap, g_cap, seed):
    rng = np.random.default_rng(seed)
    perm_in = np.stack([rng.permutation(p_cap) for _ in range(B)]).astype(np.int64)
    perm_gt = np.stack([rng.permutation(g_cap) for _ in range(B)]).astype(np.int64)
    return perm_in, perm_gt


def run(ds, item, rendering, perm_in, perm_gt, u_mirror, gt_scale):
    from cloud_transformers_amd.data.completion import completion_gather_from_draws
    up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).to(_dev())      # noqa: E731
    part, gt = completion_gather_from_draws(ds, up(item, np.int64), up(rendering, np.int64), up(perm_in, np.int64), up(perm_gt, np.int64),
                                            up(u_mirror, np.float32), gt_scale=gt_scale)
    return part.cpu().numpy(), gt.cpu().numpy()


def check(arrays, ds, item, rendering, perm_in, perm_gt, u_mirror, gt_scale, what):
    want = reference_gather(*arrays, ds.R, ds.p_cap, ds.g_cap, np.asarray(item), np.asarray(rendering), perm_in, perm_gt,
                            None if u_mirror is None else np.asarray(u_mirror, np.float32), gt_scale, ds.n_in, ds.n_out)
    got = run(ds, item, rendering, perm_in, perm_gt, u_mirror, gt_scale)
    for name, g, w in zip(("partial", "gt"), got, want):
        assert g.shape == w.shape and g.dtype == np.float32, (what, name)
        assert np.array_equal(g, w), "%s: %s differs at %d places, first %s" % (what, name, int((g != w).sum()), np.argwhere(g != w)[0].tolist())
        assert (bits(g) == bits(w)).all(), (what, name, "the sign of a zero")      # (a flip on both sides: the zeros agree too)
    return want


@pytest.mark.parametrize("mirror", ["draws", "none"])
@pytest.mark.parametrize("gt_perm", ["perm", "in_order"])
def test_equals_the_contract_over_lengths_and_mirror_draws(split, mirror, gt_perm):
    """B 8: every P of P_LENGTHS and every G of G_LENGTHS (twice), every u of U_MIRROR; u_mirror NULL; perm_gt NULL; source rows
    that are exactly zero.  Then the rows in another order with B 3 and scale 1."""
    ds = resident(split, N_IN, N_OUT)
    assert (ds.p_cap, ds.g_cap, ds.M, ds.R) == (P_CAP, G_CAP, 4, R)
    perm_in, perm_gt = draws(8, P_CAP, G_CAP, 11)
    perm_gt = perm_gt if gt_perm == "perm" else None
    u = U_MIRROR if mirror == "draws" else None
    want_p, want_g = check(split, ds, ITEM, RENDERING, perm_in, perm_gt, u, 2.0, "B8 %s %s" % (mirror, gt_perm))
    for b, P in enumerate(P_LENGTHS):
        rows = want_p[b, :min(P, N_IN)]
        assert not want_p[b, min(P, N_IN):].any() and len({r.tobytes() for r in rows}) == len(rows)      # zero padding, no repeats
        assert P < 3 or (rows == 0).all(axis=1).sum() <= 1                 # the stored zero row is kept as a row, at most once
    assert any((want_p[b, :min(P, N_IN)] == 0).all(axis=1).any() for b, P in enumerate(P_LENGTHS))
    assert not want_g[0, 251:].any() and want_g[0, :251].any(axis=1).sum() == 250        # G 251 < n_out: 5 zero rows follow
    sub = [5, 0, 6]
    check(split, ds, [ITEM[i] for i in sub], [RENDERING[i] for i in sub], perm_in[sub], None if perm_gt is None else perm_gt[sub],
          None if u is None else [u[i] for i in sub], 1.0, "B3 %s %s" % (mirror, gt_perm))


@pytest.mark.parametrize("n_in,n_out", [(1, 256), (127, 255), (126, 301), (128, 1), (200, 300), (256, 512)])
def test_equals_the_contract_over_output_sizes(split, n_in, n_out):
    """n_in 1; sizes that are no multiple of four (rows that do not start on 16 bytes: the scalar stores); n_out 1; sizes
    equal to and above the caps (every cloud padded)."""
    ds = resident(split, n_in, n_out)
    perm_in, perm_gt = draws(8, P_CAP, G_CAP, n_in * 7 + n_out)
    check(split, ds, ITEM, RENDERING, perm_in, perm_gt, U_MIRROR, 2.0, "n_in %d n_out %d" % (n_in, n_out))
    check(split, ds, ITEM[:2], RENDERING[:2], perm_in[:2], None, None, 2.0, "n_in %d n_out %d in order" % (n_in, n_out))


def test_equals_the_contract_with_the_longest_scan():
    """n_in 2048 with p_cap 65536: all 1024 ballot words of the scan, 32 workgroups per side; a short cloud beside the long."""
    arrays = synthetic_split([65536, 2047, 2049, 40000], [65536, 3000], 2, seed=2)
    ds = resident(arrays, 2048, 4096)
    assert ds.p_cap == 65536 and ds.g_cap == 65536
    perm_in, perm_gt = draws(4, 65536, 65536, 3)
    check(arrays, ds, [0, 0, 1, 1], [0, 1, 0, 1], perm_in, perm_gt, [0.1, 0.3, 0.7, 0.9], 2.0, "p_cap 65536")


def test_index_guards_and_argument_checks(split):
    """Items and renderings out of range are clamped; wrong shapes and dtypes raise before the launch."""
    from cloud_transformers_amd.data.completion import completion_gather_from_draws
    ds = resident(split, N_IN, N_OUT)
    perm_in, perm_gt = draws(4, P_CAP, G_CAP, 5)
    check(split, ds, [-3, 9, 1, 2], [0, 1, 7, -1], perm_in, perm_gt, None, 2.0, "clamped")
    t = lambda a: torch.from_numpy(a).to(_dev())      # noqa: E731
    item, rend = t(np.zeros(4, np.int64)), t(np.zeros(4, np.int64))
    with pytest.raises(ValueError, match="perm_in"):
        completion_gather_from_draws(ds, item, rend, t(perm_in[:, :-1].copy()), t(perm_gt), None)
    with pytest.raises(ValueError, match="perm_gt"):
        completion_gather_from_draws(ds, item, rend, t(perm_in), t(perm_gt[:3]), None)
    with pytest.raises(ValueError, match="u_mirror"):
        completion_gather_from_draws(ds, item, rend, t(perm_in), t(perm_gt), t(np.zeros(4, np.float64)))
    with pytest.raises(ValueError, match="rendering"):
        completion_gather_from_draws(ds, item, rend.int(), t(perm_in), t(perm_gt), None)
    with pytest.raises(TypeError):
        completion_gather_from_draws(ds, item.int(), rend, t(perm_in), t(perm_gt), None)
    with pytest.raises(RuntimeError, match="ct_completion_gather"):
        completion_gather_from_draws(ds, item, rend, t(perm_in), t(perm_gt), None, gt_scale=0.0)


def test_gather_from_a_graph_replay_with_fresh_draws(split):
    """One capture of completion_gather_from_draws on static draw buffers; replayed after the buffers take new draws."""
    from cloud_transformers_amd.data.completion import completion_gather_from_draws
    ds = resident(split, N_IN, N_OUT)
    dev = _dev()
    B = 8
    static = [torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int64, device=dev),
              torch.zeros(B, P_CAP, dtype=torch.int64, device=dev), torch.zeros(B, G_CAP, dtype=torch.int64, device=dev),
              torch.zeros(B, dtype=torch.float32, device=dev)]

    def fill(seed, item, rendering, u):
        perm_in, perm_gt = draws(B, P_CAP, G_CAP, seed)
        host = [np.asarray(item, np.int64), np.asarray(rendering, np.int64), perm_in, perm_gt, np.asarray(u, np.float32)]
        for s, h in zip(static, host):
            s.copy_(torch.from_numpy(h))
        return host

    host = fill(21, ITEM, RENDERING, U_MIRROR)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        completion_gather_from_draws(ds, *static)                          # (library load, allocator warm-up)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = completion_gather_from_draws(ds, *static)
    for k, args in enumerate(((21, ITEM, RENDERING, U_MIRROR), (22, ITEM[::-1], RENDERING, U_MIRROR[::-1]))):
        host = fill(*args)
        graph.replay()
        torch.cuda.synchronize()
        want = reference_gather(*split, R, P_CAP, G_CAP, *host, 2.0, N_IN, N_OUT)
        for g, w in zip(out, want):
            assert (bits(g.cpu().numpy()) == bits(w)).all(), "replay %d" % k


# ---------------------------------------------------------------------------------------------------------------------
# the batches of a dataset tree
T_IN, T_OUT = 128, 256


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from cloud_transformers_amd.data.completion import shapenet_loader
    from tests.completion_tree import make_tree
    root = tmp_path_factory.mktemp("gather_tree")
    keys = make_tree(root, T_IN, T_OUT)
    return {"root": root, "keys": keys, "loader": shapenet_loader(keys)}


def _batches(tree, subset, train, rank=0, world=1, seed=4):
    from cloud_transformers_amd.data import completion as C
    ds = C.DeviceShapeNetCompletion(tree["loader"].get_dataset(getattr(C.DatasetSubset, subset)), _dev())
    return C.DeviceCompletionBatches(ds, 2, train=train, seed=seed, rank=rank, world=world)


@pytest.mark.parametrize("subset,train", [("TRAIN", True), ("VAL", False), ("TEST", False)])
def test_device_batches_equal_the_restated_gather_and_items(tree, subset, train):
    """Every triple of an epoch equals completion_items_from_draws(restated gather, the same draws) bit for bit; the draws are
    recovered by re-seeding an equal generator and drawing in the documented order."""
    from cloud_transformers_amd.data import completion as C
    batches = _batches(tree, subset, train)
    ds = batches.ds
    assert (ds.n_in, ds.n_out, ds.sampled_gt, ds.R) == (T_IN, T_OUT, subset != "TEST", 2 if subset == "TRAIN" else 1)
    arrays = (ds.partial_points.cpu().numpy(), ds.partial_offsets_host, ds.gt_points.cpu().numpy(), ds.gt_offsets_host)
    batches.set_epoch(1)
    order = batches.epoch_order()
    assert sorted(order) == [0, 1, 2] and len(batches) == 2
    gen = torch.Generator(device=_dev()).manual_seed(4 * 1000003 + 0)
    seen = 0
    for k, (noise, part, gt) in enumerate(batches):
        idx = order[2 * k:2 * k + 2]
        B = len(idx)
        rendering, perm_in, perm_gt, u_mirror = C.completion_gather_draws(ds, B, train, gen)
        assert (perm_gt is None) == (subset == "TEST") and (u_mirror is None) == (not train)
        perm, u_dup, sphere = C.completion_draws(B, T_IN, T_OUT, _dev(), gen)
        host = lambda t: None if t is None else t.cpu().numpy()      # noqa: E731
        want_p, want_g = reference_gather(*arrays, ds.R, ds.p_cap, ds.g_cap, np.asarray(idx), host(rendering), host(perm_in), host(perm_gt),
                                          host(u_mirror), 2.0, T_IN, T_OUT)
        want_part, want_noise, _ = C.completion_items_from_draws(torch.from_numpy(want_p).to(_dev()), perm, u_dup, sphere, 2.0)
        assert tuple(noise.shape) == (B, 4, T_OUT) and tuple(part.shape) == (B, T_IN, 3) and tuple(gt.shape) == (B, T_OUT, 3)
        assert (bits(gt.cpu().numpy()) == bits(want_g)).all(), k
        assert torch.equal(part.view(torch.int32), want_part.view(torch.int32)) and torch.equal(noise.view(torch.int32), want_noise.view(torch.int32)), k
        assert batches.last_ids == ([ds.taxonomy_ids[i] for i in idx], [ds.model_ids[i] for i in idx])
        seen += B
    assert seen == 3


def test_device_batches_seeds_and_ranks(tree):
    epoch = lambda b: [tuple(t.clone() for t in triple) for triple in b]      # noqa: E731
    one, two = epoch(_batches(tree, "TRAIN", True)), epoch(_batches(tree, "TRAIN", True))
    assert len(one) == len(two) == 2
    for a, b in zip(one, two):
        assert all(torch.equal(x, y) for x, y in zip(a, b))                # the same seed: the same bits
    r0, r1 = epoch(_batches(tree, "TRAIN", True, rank=0, world=2)), epoch(_batches(tree, "TRAIN", True, rank=1, world=2))
    assert len(r0) == len(r1) == 1 and tuple(r0[0][2].shape) == tuple(r1[0][2].shape) == (2, T_OUT, 3)
    assert not torch.equal(r0[0][2], r1[0][2]) and not torch.equal(r0[0][1], r1[0][1]) and not torch.equal(r0[0][0], r1[0][0])


def test_gather_and_batches_do_not_synchronise(tree):
    """No device-to-host synchronisation in completion_gather (draws, argsorts, launch) nor in an epoch of
    DeviceCompletionBatches: under torch's sync debug mode set to "error" a synchronising call raises — checked first on
    `.item()`, so that the mode is known to be live."""
    from cloud_transformers_amd.data.completion import completion_gather
    batches = _batches(tree, "TRAIN", True)
    ds = batches.ds
    gen = torch.Generator(device=_dev()).manual_seed(0)
    item = torch.tensor([2, 0], dtype=torch.int64, device=_dev())
    completion_gather(ds, item, True, gen)                                 # (library load, allocator warm-up)
    list(batches)
    probe = item.sum()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        part, gt = completion_gather(ds, item, True, gen)
        triples = list(batches)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(part.shape) == (2, T_IN, 3) and tuple(gt.shape) == (2, T_OUT, 3) and len(triples) == 2
    assert bool(torch.isfinite(gt).all()) and bool(torch.isfinite(triples[1][0]).all())


# ---------------------------------------------------------------------------------------------------------------------
# harness and entry point
CONFIG = '''
experiment:
    root: '{root}/exp'
    writer_root: '{root}/runs'
data:
    kind: shapenet_completion_device
    cache_dir: '{root}/cache'
    category_path: '{category_path}'
    partial_path: '{partial_path}'
    gt_path: '{gt_path}'
    n_renders: 2
    input_size: 256
    gt_size: 1024
    batch_size: 2
    batch_size_val: 2
model:
    generator: '{root}/inpainter.py'
train:
    num_epochs: 2
    chamfer_weight: !!float 1.0
    val_emd_iters: 20
    optimizer:
        type: 'Adam'
        lr: !!float 1e-4
        betas: [!!float 0.9, !!float 0.999]
        weight_decay: !!float 0.0
{restore}
'''


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """Two eager steps (one per epoch: 3 models, batch 2, drop_last) with the validation between them; the directory and records."""
    from cloud_transformers_amd import harness as H
    from tests.completion_tree import make_tree
    root = tmp_path_factory.mktemp("completion_device")
    (root / "data").mkdir()
    keys = make_tree(root / "data", 256, 1024)
    (root / "inpainter.py").write_text("from tests.test_zoo_gpu import Inpainter as Model\n")
    cfg_path = root / "inpainting.yaml"
    cfg_path.write_text(CONFIG.format(root=str(root), restore="", **{k: keys[k] for k in ("category_path", "partial_path", "gt_path")}))
    torch.manual_seed(0)
    tr = H.Trainer(H.load_config(cfg_path), "completion", n_classes=256, device=_dev())
    hist = tr.fit(max_iters=2)
    return {"root": root, "keys": keys, "trainer": tr, "hist": hist, "cached": sorted(os.listdir(str(root / "cache")))}


def test_trainer_steps_and_validates_on_the_device_kind(trained):
    from cloud_transformers_amd.data.completion import DeviceCompletionBatches
    tr, hist = trained["trainer"], trained["hist"]
    assert isinstance(tr.loader, DeviceCompletionBatches) and isinstance(tr.val_loader, DeviceCompletionBatches) and len(tr.loader) == 1
    assert tr.loader.train and not tr.val_loader.train and len(tr.val_loader) == 2
    assert len(hist) == 2 and all(np.isfinite(h) and 0.0 < h < 10.0 for h in hist)
    records = tr.val_records
    assert len(records) == 1 and np.isfinite(records[0]["loss"]) and records[0]["batches"] == 2 and records[0]["best"]
    lines = (tr.exp_dir / "completion_val.jsonl").read_text().splitlines()
    assert len(lines) == 1 and json.loads(lines[0])["loss"] == records[0]["loss"]
    assert (tr.exp_dir / "generator_best_0.t7").exists()
    assert len(trained["cached"]) == 2                                     # the TRAIN and VAL subsets, decoded once each


def test_eval_writes_the_per_taxonomy_table_from_the_resident_test_subset(trained, capsys, monkeypatch):
    from cloud_transformers_amd import train_completion
    from cloud_transformers_amd.data import completion as C
    from tests.completion_tree import TAXONOMIES
    root, keys, tr = trained["root"], trained["keys"], trained["trainer"]
    cfg_path = root / "inpainting_eval.yaml"
    restore = "restore:\n    generator: '%s'\n" % (tr.exp_dir / "generator_best_0.t7")
    cfg_path.write_text(CONFIG.format(root=str(root), restore=restore, **{k: keys[k] for k in ("category_path", "partial_path", "gt_path")}))
    before = set(os.listdir(str(root / "exp")))
    calls = []
    gather = C.completion_gather
    monkeypatch.setattr(C, "completion_gather", lambda ds, *a, **k: (calls.append((ds.sampled_gt, ds.R, k.get("gt_scale"))), gather(ds, *a, **k))[1])
    res = train_completion.main(["evalrun", "-c", str(cfg_path), "--eval"])
    assert calls == [(False, 1, 1.0)] * 3                                  # the TEST subset, resident, gt as stored
    assert "TEST RESULTS" in capsys.readouterr().out
    new = sorted(set(os.listdir(str(root / "exp"))) - before)
    assert len(new) == 1
    assert json.loads((root / "exp" / new[0] / "completion_test.json").read_text()) == json.loads(json.dumps(res))
    assert res["names"] == ["F-Score", "ChamferDistance"]
    assert {t: row["count"] for t, row in res["taxonomies"].items()} == {t: len(m) for t, m in TAXONOMIES.items()}
    assert res["overall"]["count"] == 3 and all(np.isfinite(v) for v in res["overall"]["avg"])
