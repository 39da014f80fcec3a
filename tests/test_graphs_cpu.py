"""The parts of the graph-replay feature that need no GPU: the export, the `train.hip_graph_val` key and its default, and
the reconstruction task no longer refusing `train.hip_graph`."""
import inspect

import pytest


def test_the_package_exports_graphed_forward():
    import cloud_transformers_amd as ct
    from cloud_transformers_amd import graphs
    assert ct.GraphedForward is graphs.GraphedForward and "GraphedForward" in ct.__all__
    doc = graphs.GraphedForward.__doc__
    assert "OVERWRITTEN BY THE NEXT CALL" in doc and "clone_outputs=True" in doc


def test_training_mode_and_cpu_tensors_are_refused_before_any_device_work():
    import torch
    from cloud_transformers_amd import GraphedForward
    model = torch.nn.Sequential(torch.nn.Conv1d(3, 4, 1), torch.nn.BatchNorm1d(4))
    gf = GraphedForward(model)
    with pytest.raises(RuntimeError, match=r"Trainer\.fit\(hip_graph=True\)"):
        gf.key()
    model.eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        gf(torch.zeros(1, 3, 8))
    with pytest.raises(TypeError):
        gf(3)
    assert gf.graphs_captured == 0


def test_the_key_holds_addresses_and_modes():
    import torch
    import cloud_transformers_amd as ct
    model = torch.nn.Sequential(torch.nn.Conv1d(3, 4, 1), torch.nn.BatchNorm1d(4)).eval()
    gf = ct.GraphedForward(model)
    k0 = gf.key()
    assert gf.key() == k0
    with torch.no_grad():
        model[0].weight.mul_(2.0)                              # new values in place: the same key
    model.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    assert gf.key() == k0
    old = model[0].weight.data
    model[0].weight.data = old.clone()                         # another tensor: another key
    assert gf.key() != k0
    model[0].weight.data = old
    assert gf.key() == k0
    ct.freeze_norms(model)
    assert gf.key() != k0
    ct.unfreeze_norms(model)
    model.eval()
    assert gf.key() == k0
    prev = ct.precision.get_mode()
    try:
        ct.set_matmul_precision("high")
        assert gf.key() != k0
    finally:
        ct.set_matmul_precision(prev)
    prev = ct.precision.get_conv_mode()
    try:
        ct.set_conv_precision("high")
        assert gf.key() != k0
    finally:
        ct.set_conv_precision(prev)
    with ct.deterministic(not ct.is_deterministic()):
        assert gf.key() != k0
    assert gf.key() == k0


def test_hip_graph_val_defaults_to_false_and_grows_no_config():
    """The five config helpers: none adds the key (the pinned dictionaries of the existing tests stay as they are); it is read
    with a default where it is used."""
    from cloud_transformers_amd.train_classification import classification_config
    from cloud_transformers_amd.train_completion import completion_config
    from cloud_transformers_amd.train_kpconv import kpconv_config
    from cloud_transformers_amd.train_reconstruction import reconstruction_config
    from cloud_transformers_amd.train_segmentation import segmentation_config
    from cloud_transformers_amd.graphs import eval_forward
    for helper in (classification_config, completion_config, kpconv_config, reconstruction_config, segmentation_config):
        cfg = helper({"data": {"batch_size": 2}, "train": {}})
        assert "hip_graph_val" not in cfg["train"], helper.__name__
        assert cfg["train"].get("hip_graph_val", False) is False
        kept = helper({"data": {"batch_size": 2}, "train": {"hip_graph_val": True}})
        assert kept["train"]["hip_graph_val"] is True, helper.__name__
        marker = object()
        assert eval_forward(marker, cfg) is marker             # key unset: the model itself, nothing is built


def test_the_harness_reads_the_key_with_a_default():
    from cloud_transformers_amd import harness
    src = inspect.getsource(harness.Trainer._val_runner)
    assert '.get("hip_graph_val", False)' in src
    assert "hip_graph" in inspect.signature(harness.Trainer.validate).parameters


def test_the_reconstruction_refusal_is_gone():
    from cloud_transformers_amd import harness
    src = inspect.getsource(harness)
    assert "is not available for it" not in src and "draws its sphere noise inside the step" not in src


def test_a_cpu_trainer_validates_eagerly_whatever_the_key(tmp_path):
    """`_val_runner` hands back the eager step on a CPU device and builds no GraphedForward."""
    import torch
    from cloud_transformers_amd import harness as H

    class _T:
        cfg = {"train": {"hip_graph_val": True}}
        device = torch.device("cpu")
        _val_graph = None
        _val_step = staticmethod(lambda *t: t)

    t = _T()
    assert H.Trainer._val_runner(t) is t._val_step and t._val_graph is None
    assert H.Trainer._val_runner(t, hip_graph=False) is t._val_step
