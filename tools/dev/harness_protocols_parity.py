"""What harness.Trainer computes and writes for each of its seven tasks on tiny workloads, as one JSON per task: the record to
compare a change of the harness against its parent with.

    python tools/dev/harness_protocols_parity.py OUT_DIR [--tasks a,b,...]

The workloads are the five of tests/test_graph_validation_gpu.py's `workloads` fixture (its helpers build them) and the two
synthetic tasks on tests/test_harness_gpu.py's segmenter and a small classifier.  Per task, with `train.deterministic: true`: one
trainer runs three eager steps and an eager validation, a second one three steps with `hip_graph=True` and a graphed validation.
Kept per run: the loss history, the validation records as json.dumps gives them, the sorted file names of the experiment
directory, the bytes of its *.jsonl files, a digest of every generator state of the loaders and of the noise generator, and the
numbers of captured graphs.  Works on both sides of the move of the tasks' state to `Trainer.protocol`."""
import argparse
import copy
import hashlib
import json
import os
import sys
import tempfile
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch      # noqa: E402

DEV = torch.device("cuda", 0)
SYNTHETIC = {"segmentation": dict(n_classes=13, dataset_length=8, channels=6), "classification": dict(n_classes=5, dataset_length=8, channels=6)}
CLASSIFIER = '''
import torch
from torch import nn
from tests.test_zoo_gpu import Segmenter


class Model(nn.Module):
    def __init__(self, n_classes=5):
        super().__init__()
        self.body, self.head = Segmenter(n_classes=n_classes + 1), n_classes

    def forward(self, cloud):
        out = self.body(cloud)
        out = out[0] if isinstance(out, (tuple, list)) else out          # (B, n_classes + 1, 1, N)
        return out[:, :self.head, 0].mean(-1), out[:, self.head:, 0]
'''


class _Dirs:
    def __init__(self, base):
        self.base = Path(base)

    def mktemp(self, name):
        p = self.base / name
        p.mkdir()
        return p


def workloads(base):
    from cloud_transformers_amd import harness as H
    from tests import test_graph_validation_gpu as TV, test_harness_gpu as TH
    fixture = TV.workloads
    build = getattr(fixture, "__wrapped__", None) or fixture.__pytest_wrapped__.obj
    out = build(_Dirs(base))
    for task, kw in SYNTHETIC.items():
        root = Path(base) / ("syn_" + task)
        root.mkdir()
        (root / "segmenter.py").write_text(TH.MODEL if task == "segmentation" else CLASSIFIER)
        (root / "cfg.yaml").write_text(TH.CONFIG.format(root=str(root)))
        cfg = H.load_config(root / "cfg.yaml")
        cfg["model"]["n_classes"] = kw["n_classes"]
        out[task] = (cfg, kw)
    return out


def _digest(gen):
    return hashlib.sha1(gen.get_state().cpu().numpy().tobytes()).hexdigest()


def generator_states(tr):
    """{path: sha1 of the state} of every torch.Generator one or two attributes below the loaders, the KPConv data and the
    task's own state (`protocol`, or the trainer itself before it existed)."""
    found = {}
    roots = {"loader": tr.loader, "val_loader": tr.val_loader, "kp": tr.kp, "task": getattr(tr, "protocol", tr)}
    for name, obj in roots.items():
        for a, v in sorted(vars(obj).items()) if obj is not None and hasattr(obj, "__dict__") else []:
            if isinstance(v, torch.Generator):
                found["%s.%s" % (name, a.lstrip("_"))] = _digest(v)
            elif name != "task" and hasattr(v, "__dict__") and not isinstance(v, (torch.nn.Module, torch.Tensor)):
                for b, w in sorted(vars(v).items()):
                    if isinstance(w, torch.Generator):
                        found["%s.%s.%s" % (name, a, b)] = _digest(w)
    return found


def one_run(cfg, kw, task, base, graph):
    from cloud_transformers_amd import harness as H
    cfg = copy.deepcopy(cfg)
    cfg["train"]["deterministic"] = True
    cfg["experiment"] = {"root": str(Path(base) / "exp"), "writer_root": str(Path(base) / "runs")}
    torch.manual_seed(0)
    tr = H.Trainer(cfg, task, device=DEV, exp_name="parity", **kw)
    res = {"task": tr.task, "history": tr.fit(max_iters=3, hip_graph=graph)}
    res["step_graphs"] = [len(tr._graphs), sum(1 for r in tr._graphs.values() if r is not False)]
    if task not in SYNTHETIC:
        records = tr.validate(2, 0, hip_graph=graph) if tr.task == "segmentation_kpconv" else tr.validate(epoch=0, hip_graph=graph)
        res["val"] = json.dumps(records)
        res["val_records"] = json.dumps(tr.val_records)
        res["val_graphs"] = 0 if tr._val_graph is None else [tr._val_graph.graphs_captured, bool(tr._val_graph.eager)]
    torch.cuda.synchronize()
    files = sorted(os.listdir(tr.exp_dir))
    res["files"] = files
    res["jsonl"] = {f: (Path(tr.exp_dir) / f).read_bytes().decode() for f in files if f.endswith(".jsonl")}
    res["generators"] = generator_states(tr)
    res["iters"] = tr.iters
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--tasks", default=None)
    a = ap.parse_args()
    os.makedirs(a.out_dir, exist_ok=True)
    # the reconstruction's ResNet encoder runs the vendor's convolutions, whose backward is not run-to-run equal by default
    # (tests/test_graph_reconstruction_gpu.py): without this two runs of one tree already differ from the second step on
    torch.backends.cudnn.deterministic = True
    with tempfile.TemporaryDirectory() as base:
        todo = workloads(base)
        for task in (a.tasks.split(",") if a.tasks else todo):
            cfg, kw = todo[task]
            res = {}
            for graph in (False, True):
                run_dir = Path(base) / ("run_%s_%d" % (task, graph))
                run_dir.mkdir()
                res["graphed" if graph else "eager"] = one_run(cfg, kw, task, run_dir, graph)
            with open(os.path.join(a.out_dir, task + ".json"), "w") as f:
                json.dump(res, f, indent=1)
            print(task, "eager", res["eager"]["history"], "graphed", res["graphed"]["history"], flush=True)


if __name__ == "__main__":
    main()
