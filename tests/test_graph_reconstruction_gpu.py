"""The reconstruction task's training step as one HIP graph (`Trainer.fit(hip_graph=True)`): the sphere noise is drawn eagerly,
once per step and in step order, from the generator the eager step draws from, and copied into a static input of the graph.

The workload is the tiny tree of tests/image_tree.py (eight 32 x 32 renderings, 64-point clouds topped up to 256) and the
two-block reconstructor of tests/test_image_items_gpu.py; `train.deterministic: true`, `val_emd_iters` 8.

Eager against graphed, steps 2-3 (`test_graphed_history_against_eager`): the bound is what two EAGER runs of the same seed
differ by; where they are equal the graphed history must equal them too.  `train.deterministic` covers this library's
kernels; the tiny encoder's nn.Conv2d layers are MIOpen's, whose default weight-gradient of the first convolution is not
run-to-run equal (measured on an MI355X: 5.8e-11 between two eager runs and 1.2e-10 between eager and graph on gradients of
7.0e-4, every other gradient of step 1 bit-equal in both pairs; Adam's first steps are +-lr whatever a gradient's size, so two
EAGER histories then differ by up to 4.1e-5 at step 3, and one sample of that is no stable bound).  The three runs therefore
take torch's deterministic convolutions (`torch.backends.cudnn.deterministic`), under which every gradient of the eager and of
the captured step is bit-equal; measured so: the largest eager-against-eager difference is 0.0 and the graphed history is held
to equality."""
import copy

import pytest
import torch

from tests.test_image_items_gpu import CONFIG, TINY_MODEL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _stream_pool():
    """Every capture here creates a side stream; the pool's round robin is left where the suite before this module had it."""
    from tests.stream_pool import neutral_stream_pool
    with neutral_stream_pool():
        yield


DEV = torch.device("cuda", 0)
GT_SIZE = 256


@pytest.fixture(scope="module")
def workload(tmp_path_factory):
    pytest.importorskip("PIL.Image", reason="the temporary tree's renderings are written with Pillow")
    from cloud_transformers_amd import harness as H
    from cloud_transformers_amd.data.image_point import DeviceImageToPoint
    from tests.image_tree import make_tree
    root = tmp_path_factory.mktemp("recon_graph")
    (root / "data").mkdir()
    make_tree(root / "data", objects=4, views=1, size=(32, 32), cloud=64, seed=3)
    (root / "tiny.py").write_text(TINY_MODEL)
    cfg_path = root / "reconstruction.yaml"
    cfg_path.write_text(CONFIG.format(root=str(root), restore=""))
    cfg = H.load_config(cfg_path)
    cfg["data"].update(gt_size=GT_SIZE, batch_size=2, batch_size_val=4)
    cfg["train"].update(deterministic=True, val_emd_iters=8, num_epochs=1)
    from cloud_transformers_amd.train_reconstruction import reconstruction_config
    full = reconstruction_config(cfg)
    ds = DeviceImageToPoint(H.make_dataset(full, "reconstruction", None, train=True), DEV)
    return {"cfg": cfg, "ds": ds, "seed": int(full["data"]["seed"])}


def _trainer(workload, **data):
    from cloud_transformers_amd import harness as H
    cfg = copy.deepcopy(workload["cfg"])
    cfg["data"].update(data)
    torch.manual_seed(0)
    return H.Trainer(cfg, "reconstruction", None, device=DEV, make_dirs=False, dataset=workload["ds"])


def _noise_generator(workload):
    """Seeded as the reconstruction protocol seeds `noise_gen` on rank 0."""
    return torch.Generator(device=DEV).manual_seed(workload["seed"] * 1000003 + 15485863)


def _three_steps(workload, hip_graph):
    tr = _trainer(workload)
    chamfers = []
    tr.writer.add_scalar = lambda tag, value, global_step=None: chamfers.append(float(value)) if tag == "train/loss_chamfer" else None
    history = tr.fit(max_iters=3, hip_graph=hip_graph)
    return {"history": history, "chamfers": chamfers, "state": tr.protocol.noise_gen.get_state().clone(), "graphs": dict(tr._graphs)}


@pytest.fixture(scope="module")
def runs(workload):
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True                  # (the encoder's convolutions: see the module's docstring)
    try:
        return {"eager": _three_steps(workload, False), "eager2": _three_steps(workload, False), "graph": _three_steps(workload, True)}
    finally:
        torch.backends.cudnn.deterministic = prev


def test_fit_with_hip_graph_runs_three_steps(runs):
    """Before this feature `fit(hip_graph=True)` raised ValueError for the reconstruction task."""
    g = runs["graph"]
    assert len(g["history"]) == 3 and all(v == v and 0.0 < v < float("inf") for v in g["history"])
    assert len(g["graphs"]) == 1 and all(rec is not False for rec in g["graphs"].values())        # captured, not the eager fall-back


def test_graphed_history_against_eager(runs):
    e1, e2, g = runs["eager"]["history"], runs["eager2"]["history"], runs["graph"]["history"]
    print("eager", e1, "eager again", e2, "graphed", g)
    assert g[0] == e1[0] == e2[0]                              # same kernels, same weights, same noise: bit for bit
    spread = max(abs(a - b) for a, b in zip(e1[1:], e2[1:]))
    print("largest eager-against-eager difference, steps 2-3: %.3e" % spread)
    if spread == 0.0:
        assert g[1:] == e1[1:]
    else:
        assert max(abs(a - b) for a, b in zip(g[1:], e1[1:])) <= 2 * spread


def test_the_warm_up_consumes_no_draw(runs, workload):
    ref = _noise_generator(workload)
    from cloud_transformers_amd.metrics import sphere_noise
    for _ in range(3):
        sphere_noise(2, GT_SIZE, DEV, generator=ref)
    assert torch.equal(runs["eager"]["state"], ref.get_state())
    assert torch.equal(runs["graph"]["state"], runs["eager"]["state"])


def test_the_logged_chamfer_is_three_tensors_not_one(runs):
    c = runs["graph"]["chamfers"]
    assert len(c) == 3 and len(set(c)) == 3, c
    assert c[0] == runs["eager"]["chamfers"][0]                # step 1: the eager step's value


def test_the_noise_buffer_holds_the_draw_of_its_step(workload):
    from cloud_transformers_amd.metrics import sphere_noise
    tr = _trainer(workload)
    ref = _noise_generator(workload)
    tr._graphs = {}
    tr.model.train()
    tr.loader.set_epoch(0)
    seen = []
    for k, batch in enumerate(tr.loader):
        if k == 3:
            break
        tr._graph_step(batch)
        (rec,) = tr._graphs.values()
        assert rec is not False
        static = rec[1]
        assert len(static) == 3
        want = sphere_noise(batch[0].shape[0], GT_SIZE, DEV, generator=ref)
        assert torch.equal(static[2], want), k
        assert torch.equal(static[0], batch[0]) and torch.equal(static[1], batch[1])
        seen.append(static[2].clone())
    assert len(seen) == 3 and not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert torch.equal(tr.protocol.noise_gen.get_state(), ref.get_state())


def test_a_ragged_last_batch_gets_its_own_graph(workload):
    tr = _trainer(workload, batch_size=3, drop_last=False)
    history = tr.fit(hip_graph=True)                           # one epoch: batches of 3, 3 and 2, then the validation
    assert len(history) == 3 and all(v == v for v in history)
    assert len(tr._graphs) == 2 and all(rec is not False for rec in tr._graphs.values())
    assert len(tr.val_records) == 1 and tr.val_records[0]["batches"] == 2
