"""ct_completion_items on the device (cloud_transformers_amd.data.completion): equal, bit for bit, to the upstream
`partial_postproces` on its own recovered draws (tests/golden/completion_items_reference.npz, written by
tests/golden/gen_completion_golden.py) and to a numpy restatement of the entry point's contract (include/cloudct.h) over the
shapes at which the kernel takes another path; the public functions; no device-to-host synchronisation; one training step,
one validation and the test-split table of `harness.Trainer` / `train_completion` on a tiny dataset tree."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def reference_items(partial, perm, u_dup, sphere, scale):
    """The contract of ct_completion_items, restated in numpy (float32 throughout)."""
    B, n_in, _ = partial.shape
    gt = sphere.shape[2]
    q = (np.float32(scale) * partial).astype(np.float32)
    part = np.zeros((B, n_in, 3), np.float32)
    noise = np.zeros((B, 4, gt), np.float32)
    count = np.zeros(B, np.int32)
    for b in range(B):
        valid = ~((q[b] == 0).all(axis=1))
        v = int(valid.sum())
        c = q[b][valid]
        count[b] = v
        walk = np.clip(perm[b], 0, n_in - 1)
        part[b, :v] = q[b][walk[valid[walk]]]
        if v > 0:
            k = np.clip(np.floor(u_dup[b, v:] * np.float32(v)).astype(np.int64), 0, v - 1)
            part[b, v:] = c[k]
        noise[b, :3, :gt - v] = sphere[b, :, :gt - v]
        noise[b, :3, gt - v:] = c.T
        noise[b, 3, gt - v:] = 1.0
    return part, noise, count


def run_kernel(partial, perm, u_dup, sphere, scale):
    from cloud_transformers_amd.data.completion import completion_items_from_draws
    dev = torch.device("cuda", 0)
    part, noise, count = completion_items_from_draws(*[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (partial, perm, u_dup, sphere)],
                                                     scale=scale)
    return part.cpu().numpy(), noise.cpu().numpy(), count.cpu().numpy()


def assert_same(got, want, what):
    for name, g, w in zip(("part", "noise"), got[:2], want[:2]):
        assert g.shape == w.shape, (what, name)
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, "%s: %s differs at %d places, first %s: got %r want %r" % (
            what, name, len(bad), bad[0].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    assert got[2].dtype == np.int32 and got[2].tolist() == want[2].tolist(), (what, got[2].tolist(), want[2].tolist())


# ---------------------------------------------------------------------------------------------------------------------
# the upstream function's own outputs
def test_equals_the_upstream_partial_postproces_bit_for_bit():
    """The draws are recovered from the upstream outputs: row matching gives the permutation of the valid rows and the
    duplicate indices k, u = (k + 0.5) / v reproduces k under the kernel's floorf, the first gt - v rows of the labelled noise
    are the sphere points.  `perm` is built with the padding rows at its end and again with them scattered through it."""
    ref = np.load(os.path.join(ROOT, "tests", "golden", "completion_items_reference.npz"))
    partial, want_part, want_noise = ref["partial"], ref["part"], ref["noise"]
    B, n_in, _ = partial.shape
    gt = want_noise.shape[1]
    q = np.float32(2.0) * partial
    perm_end, perm_mix = np.zeros((B, n_in), np.int64), np.zeros((B, n_in), np.int64)
    u_dup = np.zeros((B, n_in), np.float32)
    sphere = np.full((B, 3, gt), 7.0, np.float32)                          # columns the kernel must not use stay recognisable
    counts = []
    for b in range(B):
        valid = np.flatnonzero(~((q[b] == 0).all(axis=1)))
        pad = np.flatnonzero((q[b] == 0).all(axis=1))
        v = len(valid)
        counts.append(v)
        row_of = {q[b, i].tobytes(): i for i in valid}
        assert len(row_of) == v
        order = [row_of[want_part[b, j].tobytes()] for j in range(v)]
        assert sorted(order) == valid.tolist()                             # upstream's first v rows: a permutation of the valid ones
        rank = {int(i): r for r, i in enumerate(valid)}
        k = np.array([rank[row_of[want_part[b, j].tobytes()]] for j in range(v, n_in)], np.int64)
        u_dup[b, v:] = ((k + 0.5) / v).astype(np.float32)
        assert (np.floor(u_dup[b, v:] * np.float32(v)).astype(np.int64) == k).all()
        perm_end[b] = np.concatenate([order, pad]).astype(np.int64)
        mixed, o, p = [], list(order), list(pad[::-1])
        while o or p:                                                      # padding rows first and in between
            if p:
                mixed.append(p.pop())
            if o:
                mixed.append(o.pop(0))
        perm_mix[b] = mixed
        assert sorted(perm_mix[b].tolist()) == list(range(n_in))
        sphere[b, :, :gt - v] = want_noise[b, :gt - v, :3].T
    assert counts == [40, 39, 64, 1]
    want = (want_part, np.ascontiguousarray(want_noise.transpose(0, 2, 1)), np.array(counts, np.int32))
    for name, perm in (("padding last", perm_end), ("padding scattered", perm_mix)):
        assert_same(run_kernel(partial, perm, u_dup, sphere, 2.0), want, name)


# ---------------------------------------------------------------------------------------------------------------------
# the contract over the shapes
N_INS = [1, 63, 64, 65, 1000, 2048, 16384]
SHAPES = sorted({(n, g) for n in N_INS for g in (n, n + 1, 16384) if g >= n})


def cloud(pattern, n_in, rng):
    """One cloud f32[n_in, 3] of distinct non-zero rows with the pattern's rows zeroed."""
    p = rng.uniform(0.05, 1.0, (n_in, 3)).astype(np.float32) * rng.choice(np.array([-1, 1], np.float32), (n_in, 3))
    keep = np.zeros(n_in, bool)
    if pattern == "none":
        pass
    elif pattern == "one":
        keep[rng.integers(n_in)] = True
    elif pattern == "all_but_one":
        keep[:] = True
        keep[rng.integers(n_in)] = False
    elif pattern == "all":
        keep[:] = True
    elif pattern == "tail":
        keep[max(0, n_in - 5):] = True
    elif pattern == "boundaries":                                          # rows next to the 64-row words and 256-word edges
        i = np.arange(n_in)
        keep[(i % 64 == 0) | (i % 64 == 63)] = True
    else:                                                                  # "mixed": half the rows, with the comparison's corner cases
        keep[:] = rng.random(n_in) < 0.5
        idx = np.flatnonzero(keep)
        if len(idx) > 4:
            p[idx[0], 0] = 0.0                                             # one zero coordinate: valid
            p[idx[1], 1:] = 0.0                                            # two zero coordinates: valid
            p[idx[2]] = [0.0, -0.0, np.float32(1e-30)]                     # tiny but not zero: valid
            p[idx[3]] = [np.nan, 0.0, 0.0]                                 # NaN: valid
    p[~keep] = 0.0
    z = np.flatnonzero(~keep)
    if pattern == "mixed" and len(z) > 1:
        p[z[0]] = [-0.0, 0.0, -0.0]                                        # -0 is zero
    return p


def batch(n_in, gt, patterns, seed):
    rng = np.random.default_rng(seed)
    B = len(patterns)
    partial = np.stack([cloud(pt, n_in, rng) for pt in patterns])
    perm = np.stack([rng.permutation(n_in) for _ in range(B)]).astype(np.int64)
    u_dup = rng.random((B, n_in), dtype=np.float32)
    u_dup[:, ::7] = 0.0
    u_dup[:, 3::11] = np.float32(1.0) - np.float32(2.0 ** -24)             # the largest draw below 1
    sphere = rng.normal(size=(B, 3, gt)).astype(np.float32)
    return partial, perm, u_dup, sphere


ALL_PATTERNS = ["none", "one", "all_but_one", "all", "tail", "boundaries", "mixed"]


@pytest.mark.parametrize("n_in,gt", SHAPES)
def test_equals_the_contract_bit_for_bit(n_in, gt):
    """B 7: v = 0, 1, n_in - 1 and n_in, valid rows only at the end, only at scan-block boundaries, and a mixed cloud; with
    gt == n_in the full cloud has gt == v (no noise columns); B 1 and B 2 as well; scale 1 and 2.  NaN rows compare by bits."""
    for B, patterns in ((7, ALL_PATTERNS), (1, ["mixed"]), (2, ["all", "mixed"])):
        args = batch(n_in, gt, patterns, seed=n_in * 31 + gt + B)
        for scale in (1.0, 2.0):
            want = reference_items(*args, scale)
            if B == 7:
                assert want[2][0] == 0 and want[2][1] == 1 and want[2][2] == n_in - 1 and want[2][3] == n_in
            assert_same(run_kernel(*args, scale), want, "B%d n_in %d gt %d scale %g" % (B, n_in, gt, scale))


# ---------------------------------------------------------------------------------------------------------------------
# the public functions
def _partial(B, n_in, seed, device):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(B, n_in, 3, generator=g) - 0.5
    for b in range(B):
        p[b, n_in - (b * n_in) // (B + 1):] = 0.0                          # cloud b has a zero tail of b * n_in / (B + 1) rows
    return p.to(device)


def test_completion_items_public_function():
    from cloud_transformers_amd.data.completion import completion_items
    dev = torch.device("cuda", 0)
    B, n_in, gt = 3, 200, 1024
    partial = _partial(B, n_in, 0, dev)
    outs = [completion_items(partial, gt, generator=torch.Generator(device=dev).manual_seed(11)) for _ in range(2)]
    for a, b in zip(*outs):
        assert torch.equal(a, b)                                           # the same seed: the same bits
    other = completion_items(partial, gt, generator=torch.Generator(device=dev).manual_seed(12))
    assert not torch.equal(other[0], outs[0][0]) and not torch.equal(other[1], outs[0][1])
    part, noise, count = (t.cpu().numpy() for t in outs[0])
    assert part.shape == (B, n_in, 3) and noise.shape == (B, 4, gt) and count.dtype == np.int32
    q = 2.0 * partial.cpu().numpy()
    for b in range(B):
        valid = q[b][~(q[b] == 0).all(1)]
        v = len(valid)
        assert count[b] == v == n_in - (b * n_in) // (B + 1)
        rows = sorted(r.tobytes() for r in valid)
        assert sorted(r.tobytes() for r in part[b, :v]) == rows            # a rearrangement of the valid rows
        assert {r.tobytes() for r in part[b, v:]} <= set(rows)             # the rest are members of it
        assert (noise[b, 3, :gt - v] == 0).all() and (noise[b, 3, gt - v:] == 1).all()
        assert np.abs(np.linalg.norm(noise[b, :3, :gt - v].astype(np.float64), axis=0) - 1).max() < 1e-6
        assert (bits(noise[b, :3, gt - v:].T) == bits(valid)).all()        # then the real points in their order


def test_partial_postproces_has_the_upstream_layout():
    """utils/pcd_utils.py:24-51 as train_inpainter.py:180-183 uses it: shapes, dtypes, device, and the caller's two permutes."""
    from utils.pcd_utils import partial_postproces
    dev = torch.device("cuda", 0)
    B, n_in, gt = 2, 96, 320
    data = _partial(B, n_in, 1, torch.device("cpu"))
    for given in (2 * data, (2 * data).to(dev)):                           # the caller has scaled it; host or device
        part, noise = partial_postproces(given, gt)
        assert part.is_cuda and noise.is_cuda and part.dtype == torch.float32 and noise.dtype == torch.float32
        assert tuple(part.shape) == (B, n_in, 3) and tuple(noise.shape) == (B, gt, 4)
        enc = part.permute(0, 2, 1)[:, :, None].cuda()
        lab = noise.permute(0, 2, 1).cuda()
        assert tuple(enc.shape) == (B, 3, 1, n_in) and tuple(lab.shape) == (B, 4, gt)
        assert lab.is_contiguous() and torch.equal(lab, lab.contiguous()) and torch.equal(enc, enc.contiguous())
        v = n_in - (1 * n_in) // (B + 1)
        assert torch.equal(lab[1, :3, gt - v:].t(), (2 * data[1, :v]).to(dev)) and bool((lab[1, 3, gt - v:] == 1).all())


def test_completion_items_does_not_synchronise():
    """No device-to-host synchronisation anywhere in completion_items (draws, argsort, launch): under torch's sync debug mode
    set to "error" a synchronising call raises — checked first on `.item()`, so that the mode is known to be live."""
    from cloud_transformers_amd.data.completion import completion_items
    dev = torch.device("cuda", 0)
    partial = _partial(2, 2048, 2, dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    completion_items(partial, 16384, generator=gen)                        # (library load, allocator warm-up)
    probe = partial.sum()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        part, noise, count = completion_items(partial, 16384, generator=gen)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert count.tolist() == [2048, 2048 - 2048 // 3] and tuple(noise.shape) == (2, 4, 16384)


# ---------------------------------------------------------------------------------------------------------------------
# harness and entry point
CONFIG = '''
experiment:
    root: '{root}/exp'
    writer_root: '{root}/runs'
data:
    kind: shapenet_completion
    category_path: '{category_path}'
    partial_path: '{partial_path}'
    gt_path: '{gt_path}'
    n_renders: 2
    input_size: 256
    gt_size: 1024
    batch_size: 2
    batch_size_val: 2
    num_workers: 0
model:
    generator: '{root}/inpainter.py'
train:
    num_epochs: 1
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
    """One eager step and one validation of the Trainer on the tiny tree; the directory and the records."""
    from cloud_transformers_amd import harness as H
    from tests.completion_tree import make_tree
    root = tmp_path_factory.mktemp("completion")
    (root / "data").mkdir()
    keys = make_tree(root / "data", 256, 1024)
    (root / "inpainter.py").write_text("from tests.test_zoo_gpu import Inpainter as Model\n")
    cfg_path = root / "inpainting.yaml"
    cfg_path.write_text(CONFIG.format(root=str(root), restore="", **{k: keys[k] for k in ("category_path", "partial_path", "gt_path")}))
    torch.manual_seed(0)
    np.random.seed(0)
    tr = H.Trainer(H.load_config(cfg_path), "completion", n_classes=256, device=torch.device("cuda", 0))
    hist = tr.fit(max_iters=1)
    records = tr.validate(epoch=0)
    return {"root": root, "keys": keys, "trainer": tr, "hist": hist, "records": records}


def test_trainer_steps_and_validates_on_shapenet_completion(trained):
    tr, hist, records = trained["trainer"], trained["hist"], trained["records"]
    from cloud_transformers_amd.data.completion import CompletionBatches
    assert isinstance(tr.loader, CompletionBatches) and len(tr.loader) == 1              # 3 models, batch 2, drop_last
    assert len(hist) == 1 and np.isfinite(hist[0]) and 0.0 < hist[0] < 10.0
    assert len(records) == 1 and np.isfinite(records[0]["loss"]) and records[0]["batches"] == 2 and records[0]["best"]
    # every batch's loss is the float32 sum of its two float32 terms (chamfer_weight 1): half an ulp, 2^-24 relative, per batch
    assert abs(records[0]["loss"] - (records[0]["loss_emd"] + records[0]["loss_chamfer"])) <= 2.0 ** -23 * records[0]["loss"]
    lines = (tr.exp_dir / "completion_val.jsonl").read_text().splitlines()
    assert len(lines) == 1 and json.loads(lines[0])["loss"] == records[0]["loss"]
    assert (tr.exp_dir / "generator_best_0.t7").exists() and (tr.exp_dir / "g_opt_best_0.t7").exists()
    noise, part, gt = next(iter(tr.loader))
    assert tuple(noise.shape) == (2, 4, 1024) and tuple(part.shape) == (2, 256, 3) and tuple(gt.shape) == (2, 1024, 3)
    assert noise.is_cuda and part.is_cuda and gt.is_cuda


def test_eval_writes_the_per_taxonomy_table(trained, capsys):
    from cloud_transformers_amd import train_completion
    from tests.completion_tree import TAXONOMIES
    root, keys, tr = trained["root"], trained["keys"], trained["trainer"]
    cfg_path = root / "inpainting_eval.yaml"
    restore = "restore:\n    generator: '%s'\n" % (tr.exp_dir / "generator_best_0.t7")
    cfg_path.write_text(CONFIG.format(root=str(root), restore=restore, **{k: keys[k] for k in ("category_path", "partial_path", "gt_path")}))
    before = set(os.listdir(str(root / "exp")))
    res = train_completion.main(["evalrun", "-c", str(cfg_path), "--eval"])
    assert "TEST RESULTS" in capsys.readouterr().out
    new = sorted(set(os.listdir(str(root / "exp"))) - before)
    assert len(new) == 1
    assert json.loads((root / "exp" / new[0] / "completion_test.json").read_text()) == json.loads(json.dumps(res))
    assert res["names"] == ["F-Score", "ChamferDistance"]
    assert {t: row["count"] for t, row in res["taxonomies"].items()} == {t: len(m) for t, m in TAXONOMIES.items()}
    total = sum(row["count"] for row in res["taxonomies"].values())
    assert res["overall"]["count"] == total == 3
    for k in range(2):
        mean = sum(row["count"] * row["avg"][k] for row in res["taxonomies"].values()) / total
        assert np.isfinite(mean) and abs(res["overall"]["avg"][k] - mean) <= 1e-9 * max(1.0, abs(mean))
