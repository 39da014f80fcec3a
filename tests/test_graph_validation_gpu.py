"""Validation passes by HIP-graph replay (`train.hip_graph_val`, `Trainer.validate(hip_graph=True)`): the per-batch work of every
task — eval-mode forward plus the validation loss terms — replayed as one graph per batch shape, parameter addresses and modes;
the meters stay eager on the static outputs.

The workloads are the tiny sets of the existing harness tests (tests/test_block_items_gpu.py, test_scan_items_gpu.py,
test_kpconv_train_gpu.py, test_completion_gather_gpu.py, test_image_items_gpu.py), `val_emd_iters` 8.  Every comparison is
between trainers built from the same seed (or one trainer with its validation loader's generator put back), so both sides see
the same batches; an eval forward has no order-dependent sum, so records are compared for equality.  Measured on an MI355X:
two eager validations are equal for all five tasks."""
import copy
import json

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _stream_pool():
    """Every capture here creates a side stream; the pool's round robin is left where the suite before this module had it."""
    from tests.stream_pool import neutral_stream_pool
    with neutral_stream_pool():
        yield


DEV = torch.device("cuda", 0)
TASKS = ("segmentation_blocks", "classification_scanobjectnn", "segmentation_kpconv", "completion", "reconstruction")


@pytest.fixture(scope="module")
def workloads(tmp_path_factory):
    """Per task: (config dictionary, Trainer arguments); the files are written once."""
    from cloud_transformers_amd import harness as H
    out = {}

    from tests import test_block_items_gpu as TB
    root = tmp_path_factory.mktemp("val_blocks")
    TB.write_blocks(root)
    (root / "segmenter.py").write_text(TB.MODEL)
    (root / "s3dis.yaml").write_text(TB.CONFIG.format(root=str(root), restore=""))
    out["segmentation_blocks"] = (H.load_config(root / "s3dis.yaml"), dict(n_classes=13))

    from tests import test_scan_items_gpu as TS
    root = tmp_path_factory.mktemp("val_scan")
    TS.write_pair(root)
    (root / "classifier.py").write_text(TS.MODEL)
    (root / "scan.yaml").write_text(TS.CONFIG.format(root=str(root), model="classifier", restore=""))
    out["classification_scanobjectnn"] = (H.load_config(root / "scan.yaml"), dict(n_classes=3))

    from tests import test_kpconv_train_gpu as TK
    from cloud_transformers_amd.train_kpconv import load_kpconv_areas
    root = tmp_path_factory.mktemp("val_kpconv")
    for a in range(1, 7):
        TK._write_room(root / "Stanford3dDataset_v1.2" / ("Area_%d" % a), 40 + a, (6.0 + a % 3, 5.0, 3.0))
    (root / "segmenter_pad_small.py").write_text(TK.MODEL)
    cfg = H.load_config(TK._config(root, False))
    cfg["data"].update(kind="s3dis_kpconv", num_steps=6, num_points=1024)
    cfg["train"].update(val_votes=2)
    areas = load_kpconv_areas(cfg)
    out["segmentation_kpconv"] = (cfg, dict(n_classes=13, dataset=areas))

    from tests import test_completion_gather_gpu as TC
    from tests.completion_tree import make_tree as completion_tree
    root = tmp_path_factory.mktemp("val_completion")
    (root / "data").mkdir()
    keys = completion_tree(root / "data", 256, 1024)
    (root / "inpainter.py").write_text("from tests.test_zoo_gpu import Inpainter as Model\n")
    (root / "inpainting.yaml").write_text(TC.CONFIG.format(root=str(root), restore="",
                                                           **{k: keys[k] for k in ("category_path", "partial_path", "gt_path")}))
    cfg = H.load_config(root / "inpainting.yaml")
    cfg["train"]["val_emd_iters"] = 8
    out["completion"] = (cfg, dict(n_classes=256))

    pytest.importorskip("PIL.Image", reason="the temporary tree's renderings are written with Pillow")
    from tests import test_image_items_gpu as TI
    from tests.image_tree import make_tree as image_tree
    root = tmp_path_factory.mktemp("val_recon")
    (root / "data").mkdir()
    image_tree(root / "data", objects=4, views=1, size=(32, 32), cloud=64, seed=3)
    (root / "tiny.py").write_text(TI.TINY_MODEL)
    (root / "reconstruction.yaml").write_text(TI.CONFIG.format(root=str(root), restore=""))
    cfg = H.load_config(root / "reconstruction.yaml")
    cfg["data"].update(gt_size=256, batch_size_val=3)          # 8 items: a ragged last validation batch
    cfg["train"]["val_emd_iters"] = 8
    out["reconstruction"] = (cfg, dict(n_classes=None))
    return out


def _trainer(workloads, task, **train_keys):
    from cloud_transformers_amd import harness as H
    cfg, kw = workloads[task]
    cfg = copy.deepcopy(cfg)
    cfg["train"].update(train_keys)
    torch.manual_seed(0)
    return H.Trainer(cfg, task, device=DEV, make_dirs=False, **kw)


def _validate(tr, hip_graph=None, epoch=0):
    kw = {} if hip_graph is None else {"hip_graph": hip_graph}
    if tr.task == "segmentation_kpconv":
        return tr.validate(2, epoch, **kw)
    return tr.validate(epoch=epoch, **kw)


def _same(a, b):
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)          # (NaN of an absent class included)


def _captured(tr):
    return 0 if tr._val_graph is None else tr._val_graph.graphs_captured


@pytest.mark.parametrize("task", TASKS)
def test_graphed_validation_returns_the_eager_record(workloads, task):
    eager, again, graphed = (_trainer(workloads, task) for _ in range(3))
    want, want2 = _validate(eager, False), _validate(again, False)
    got = _validate(graphed, True)
    print(task, "eager", want, "graphed", got)
    assert _same(want, want2), "two eager validations of %s differ" % task
    assert _same(got, want)
    assert _captured(graphed) >= 1 and not graphed._val_graph.eager            # replayed, not the eager fall-back
    assert eager._val_graph is None
    if task == "reconstruction":
        assert _captured(graphed) == 2 and got[0]["batches"] == 3              # batches of 3, 3 and 2: the ragged one has its graph
        assert torch.equal(graphed.protocol.noise_gen.get_state(), eager.protocol.noise_gen.get_state())        # the warm-ups drew nothing


def test_the_config_key_selects_it_and_the_default_launches_no_graph(workloads):
    tr = _trainer(workloads, "segmentation_blocks")
    assert "hip_graph_val" not in tr.cfg["train"] and tr._val_graph is None
    want = _validate(tr)
    assert tr._val_graph is None                               # no key: GraphedForward is never built
    keyed = _trainer(workloads, "segmentation_blocks", hip_graph_val=True)
    got = _validate(keyed)
    assert keyed._val_graph is not None and _captured(keyed) >= 1 and _same(got, want)
    off = _trainer(workloads, "segmentation_blocks", hip_graph_val=True)
    assert _same(_validate(off, hip_graph=False), want) and off._val_graph is None          # the argument overrides the key


def _rewind(tr, state):
    tr.val_loader.generator.set_state(state)


@pytest.fixture()
def blocks(workloads):
    """A blocks trainer after one graphed validation, and the state its validation loader's generator started that pass from."""
    tr = _trainer(workloads, "segmentation_blocks")
    tr.val_loader = tr.protocol.loader(tr, _val_data(tr), train=False)
    state = tr.val_loader.generator.get_state().clone()
    first = _validate(tr, True)
    return tr, state, first


def _val_data(tr):
    from cloud_transformers_amd import harness as H
    return H.make_dataset(tr.cfg, tr.task, tr.n_classes, train=False)


def _eager_at_current_weights(tr, state):
    _rewind(tr, state)
    return _validate(tr, False)


def _strip(records):
    return [{k: v for k, v in r.items() if k not in ("iters", "best", "macc_best")} for r in records]


def test_a_training_step_between_two_graphed_validations(blocks):
    tr, state, first = blocks
    n = _captured(tr)
    tr.model.train()
    tr._eager_step(next(iter(tr.loader)))
    _rewind(tr, state)
    second = _validate(tr, True)
    assert _captured(tr) == n                                  # the graph reads the weights where they live
    assert _same(_strip(second), _strip(_eager_at_current_weights(tr, state)))
    assert not _same(_strip(second), _strip(first))


def test_load_state_dict_between_two_graphed_validations(blocks):
    tr, state, first = blocks
    n = _captured(tr)
    g = torch.Generator().manual_seed(5)
    tr.model.load_state_dict({k: (v * (1 + 0.2 * torch.randn(v.shape, generator=g).to(v.device)) if v.is_floating_point() else v)
                              for k, v in tr.model.state_dict().items()})
    _rewind(tr, state)
    second = _validate(tr, True)
    assert _captured(tr) == n
    assert _same(_strip(second), _strip(_eager_at_current_weights(tr, state)))
    assert not _same(_strip(second), _strip(first))


def test_a_replaced_parameter_tensor_captures_anew(blocks):
    tr, state, first = blocks
    n = _captured(tr)
    p = next(tr.model.parameters())
    p.data = (p.data * 1.5).clone()                            # another tensor behind the Parameter: a stale address must not be replayed
    _rewind(tr, state)
    second = _validate(tr, True)
    assert _captured(tr) > n
    assert _same(_strip(second), _strip(_eager_at_current_weights(tr, state)))
    assert not _same(_strip(second), _strip(first))


def test_a_precision_change_captures_anew(blocks):
    import cloud_transformers_amd as ct
    tr, state, first = blocks
    n = _captured(tr)
    prev = ct.precision.get_mode()
    try:
        ct.set_matmul_precision("high")
        _rewind(tr, state)
        second = _validate(tr, True)
        assert _captured(tr) > n
        assert _same(_strip(second), _strip(_eager_at_current_weights(tr, state)))
    finally:
        ct.set_matmul_precision(prev)


@pytest.mark.parametrize("task", ["completion", "reconstruction"])
def test_emd_validation_steps_replay_without_a_host_synchronisation(workloads, task):
    tr = _trainer(workloads, task)
    _validate(tr, True)                                        # captures
    step = tr._val_runner(True)
    tr.model.eval()
    if task == "reconstruction":
        img, pcd = next(iter(tr.val_loader))
        args = (img, pcd, tr.protocol._draw_noise(pcd))
    else:
        args = tuple(next(iter(tr.val_loader)))
    n = _captured(tr)
    probe = args[0].sum()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()
        l_emd, l_cd = step(*args)
        kept = torch.stack([l_emd, l_cd]).clone()
        step(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _captured(tr) == n and bool(torch.isfinite(kept).all()) and float(kept[0]) > 0
    with torch.no_grad():
        want = tr._val_step(*args)
    assert torch.equal(kept, torch.stack(list(want)))


def _spy_on_eval_forward(monkeypatch):
    from cloud_transformers_amd import graphs
    made, real = [], graphs.eval_forward
    monkeypatch.setattr(graphs, "eval_forward", lambda *a, **k: (made.append(real(*a, **k)), made[-1])[1])
    return made


def test_reconstruction_eval_loop_honours_the_key(workloads, monkeypatch):
    """train_reconstruction.evaluate: two noise draws and two forwards per batch, the first reconstruction kept past the second
    replay; the F1 table equals the eager loop's."""
    from cloud_transformers_amd import graphs, harness as H
    from cloud_transformers_amd.data.image_point import DeviceImageToPoint, ImageBatches
    from cloud_transformers_amd.train_reconstruction import evaluate
    tr = _trainer(workloads, "reconstruction")
    test = DeviceImageToPoint(H.make_dataset(tr.cfg, "reconstruction", None, train="test"), DEV)
    made = _spy_on_eval_forward(monkeypatch)

    def run(flag):
        cfg = copy.deepcopy(tr.cfg)
        cfg["train"]["hip_graph_val"] = flag
        batches = ImageBatches(test, 3, train=False, seed=int(cfg["data"]["seed"]))          # 8 items: 3, 3 and 2
        return evaluate(tr.model, batches, cfg, generator=torch.Generator(device=DEV).manual_seed(7), verbose=False)

    want, got = run(False), run(True)
    assert made[0] is tr.model and isinstance(made[1], graphs.GraphedForward)
    assert made[1].graphs_captured == 2 and not made[1].eager and made[1].clone_outputs
    assert _same(got, want) and got["overall"]["count"] == 8


def test_completion_eval_loop_honours_the_key(workloads, monkeypatch):
    """train_completion.evaluate over the resident TEST subset, in batches of one and in batches of two."""
    from cloud_transformers_amd import graphs, harness as H
    from cloud_transformers_amd.data.completion import DatasetSubset, shapenet_loader
    from cloud_transformers_amd.train_completion import completion_config, evaluate
    cfg, kw = workloads["completion"]
    cfg = completion_config(cfg)
    torch.manual_seed(0)
    tr = H.Trainer(cfg, "completion", device=DEV, make_dirs=False, dataset=shapenet_loader(cfg["data"]).get_dataset(DatasetSubset.TEST), **kw)
    made = _spy_on_eval_forward(monkeypatch)
    for batch_size in (1, 2):
        del made[:]

        def run(flag):
            c = copy.deepcopy(cfg)
            c["train"]["hip_graph_val"] = flag
            return evaluate(tr.model, c, DEV, resident=tr.loader.ds, verbose=False, batch_size=batch_size)

        want, got = run(False), run(True)
        assert made[0] is tr.model and isinstance(made[1], graphs.GraphedForward)
        assert made[1].graphs_captured >= 1 and not made[1].eager
        assert _same(got, want) and got["overall"]["count"] == 3
