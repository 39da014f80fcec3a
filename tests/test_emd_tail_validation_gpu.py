"""`train.val_emd_tail`: a tiny synthetic completion validation (the tree of tests/test_graph_validation_gpu.py) with the key on
and off, eager and under `train.hip_graph_val` — the four runs give the same loss, EMD and Chamfer numbers exactly, and the
keyed records also say how the auctions ended."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
ITERS = 40


@pytest.fixture(scope="module", autouse=True)
def _stream_pool():
    from tests.stream_pool import neutral_stream_pool
    with neutral_stream_pool():
        yield


@pytest.fixture(scope="module")
def config(tmp_path_factory):
    from cloud_transformers_amd import harness as H
    from tests import test_completion_gather_gpu as TC
    from tests.completion_tree import make_tree as completion_tree
    root = tmp_path_factory.mktemp("val_tail_completion")
    (root / "data").mkdir()
    keys = completion_tree(root / "data", 256, 1024)
    (root / "inpainter.py").write_text("from tests.test_zoo_gpu import Inpainter as Model\n")
    (root / "inpainting.yaml").write_text(TC.CONFIG.format(root=str(root), restore="",
                                                           **{k: keys[k] for k in ("category_path", "partial_path", "gt_path")}))
    cfg = H.load_config(root / "inpainting.yaml")
    cfg["train"]["val_emd_iters"] = ITERS
    return cfg


def _validate(config, **train_keys):
    from cloud_transformers_amd import harness as H
    cfg = copy.deepcopy(config)
    cfg["train"].update(train_keys)
    torch.manual_seed(0)
    tr = H.Trainer(cfg, "completion", device=DEV, make_dirs=False, n_classes=256)
    return tr, tr.validate(epoch=0)


def test_the_four_validations_agree(config):
    from cloud_transformers_amd import _lib
    assert "val_emd_tail" not in config["train"]
    lib = _lib.load()
    runs = {}
    lib.ct_debug_set_emd_tail(2048, 3)                # the tail takes the clouds within these few iterations
    try:
        for tail in (False, True):
            for graph in (False, True):
                tr, rec = _validate(config, val_emd_tail=tail, hip_graph_val=graph)
                if graph:
                    assert tr._val_graph is not None and tr._val_graph.graphs_captured >= 1 and not tr._val_graph.eager
                runs[(tail, graph)] = rec[0]
    finally:
        lib.ct_debug_set_emd_tail(-1, 0)
    base = runs[(False, False)]
    print(runs)
    for key, rec in runs.items():
        for k in ("loss", "loss_emd", "loss_chamfer", "batches"):
            assert rec[k] == base[k], (key, k, rec[k], base[k])
        assert ("emd_unfinished" in rec) == key[0] and ("emd_first_empty_mean" in rec) == key[0]
    for graph in (False, True):
        rec = runs[(True, graph)]
        assert 0 < rec["emd_first_empty_mean"] <= ITERS and rec["emd_unfinished"] >= 0
        assert rec["emd_unfinished"] == runs[(True, False)]["emd_unfinished"]
        assert rec["emd_first_empty_mean"] == runs[(True, False)]["emd_first_empty_mean"]
