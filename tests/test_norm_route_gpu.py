"""ops.norm_route — the one place that decides whether a group of norms runs on the training kernels, the eval kernels, the
frozen (stored statistics, with gradients) path or through its modules — and the library entry points each composition calls
in each mode, as recorded from the twelve entry points at the commit before the router."""
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

KINDS = ["single", "split", "join", "union"]
B, C, N = 2, 8, 64


def _norm(channels, mode, cls=nn.BatchNorm1d):
    from cloud_transformers_amd import freeze_norms
    bn = cls(channels).cuda()
    if mode == "train":
        return bn.train()
    return freeze_norms(bn) if mode == "frozen" else bn.eval()


def _case(kind, modes, grad, device="cuda", cls=nn.BatchNorm1d, bias=False):
    """(arguments of ops.norm_route, arguments of the kind's entry points).  modes: one mode for all norms, or one per norm."""
    widths = {"single": [8], "split": [2, 6], "join": [2, 6], "union": [2, 4, 2, 4]}[kind]
    if isinstance(modes, str):
        modes = [modes] * len(widths)
    bns = [_norm(w, m, cls if i == 0 else nn.BatchNorm1d) for i, (w, m) in enumerate(zip(widths, modes))]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, C, N, generator=g).to(device).requires_grad_(grad)
    if kind == "single":
        return dict(norms=[(bns[0], x, None)]), (x, bns[0])
    if kind == "split":
        return dict(norms=[(bns[0], x, 2), (bns[1], x, 6)]), (x, bns[0], bns[1])
    if kind == "join":
        xs = [torch.randn(B, w, N, generator=g).to(device).requires_grad_(grad) for w in widths]
        return dict(norms=[(bn, xi, None) for bn, xi in zip(bns, xs)]), (xs, bns)
    convs = [nn.Conv1d(8, 6, 1, bias=bias and i == 1).cuda() for i in range(2)]
    return (dict(norms=[(bn, x, bn.num_features) for bn in bns], watch=[c.weight for c in convs], convs=convs),
            (x, convs, bns[0::2], bns[1::2]))


@pytest.mark.parametrize("kind", KINDS)
def test_route_table(kind):
    from cloud_transformers_amd import ops
    route = ops.norm_route
    assert route(**_case(kind, "train", True)[0]) == "train"
    assert route(**_case(kind, "train", False)[0]) == "train"
    with torch.no_grad():
        assert route(**_case(kind, "eval", False)[0]) == "eval"
        assert route(**_case(kind, "frozen", False)[0]) == "eval"            # marked or not: nothing is recorded
    assert route(**_case(kind, "frozen", True)[0]) == "frozen"
    assert route(**_case(kind, "eval", True)[0]) is None                     # unmarked, gradients: the modules
    if kind != "single":
        n = 4 if kind == "union" else 2
        assert route(**_case(kind, ["train"] + ["eval"] * (n - 1), True)[0]) is None
        with torch.no_grad():
            assert route(**_case(kind, ["eval"] * (n - 1) + ["train"], False)[0]) is None
        assert route(**_case(kind, ["frozen"] * (n - 1) + ["eval"], True)[0]) is None          # one norm unmarked
        # an unconverted BatchNorm1d beside a SyncBatchNorm (ops.norms_share_group; no process group needed)
        assert route(**_case(kind, "train", True, cls=nn.SyncBatchNorm)[0]) is None
    else:
        assert route(**_case(kind, "train", True, cls=nn.SyncBatchNorm)[0]) == "train"
    for switch, mode, grad in (("BN_EVAL", "eval", False), ("BN_FROZEN", "frozen", True)):
        saved = getattr(ops, switch)
        setattr(ops, switch, False)
        try:
            with torch.set_grad_enabled(grad):
                assert route(**_case(kind, mode, grad)[0]) is None
        finally:
            setattr(ops, switch, saved)
    for mode, grad in (("train", True), ("eval", False), ("frozen", True)):
        with torch.set_grad_enabled(grad):
            args = _case(kind, mode, grad, device="cpu")[0]
            args["norms"] = [(bn.cpu(), x, c) for bn, x, c in args["norms"]]
            assert route(**args) is None                                     # a CPU tensor
            if kind == "union":
                assert route(**_case(kind, mode, grad, bias=True)[0]) is None    # one projection with a bias
    if kind == "single":                                                     # the residual joins the watch list
        args, _ = _case(kind, "frozen", False)
        args["norms"][0][0].requires_grad_(False)
        res = torch.zeros(B, C, N, device="cuda")
        assert route(residual=res, **args) == "eval" and route(residual=res.clone().requires_grad_(True), **args) == "frozen"
        assert route(residual=res.cpu(), **args) is None
    if kind == "union":                                                      # ... and so do the projections' weights
        args, _ = _case(kind, "frozen", False)
        for bn, _, _ in args["norms"]:
            bn.requires_grad_(False)
        assert route(**args) == "frozen"
        for w in args["watch"]:
            w.requires_grad_(False)
        assert route(**args) == "eval"


# as recorded: (composition, mode, BN_GROUP_LAUNCH) -> the second arguments of the _lib.check calls, in order: one launch per
# direction for the whole group, or one per norm with the switch off (pinned for split and join), forward first.  At these shapes
# the union's products go to the library GEMM, which is not a call of this library.
LITERAL = {
    ("single", "train", True): ["ct_bn_group_fwd", "ct_bn_group_bwd"],
    ("single", "eval", True): ["ct_bn_eval_group_fwd"],
    ("single", "frozen", True): ["ct_bn_eval_group_fwd", "ct_bn_eval_group_bwd"],
    ("split", "train", True): ["ct_bn_group_fwd", "ct_bn_group_bwd"],
    ("split", "eval", True): ["ct_bn_eval_group_fwd"],
    ("split", "frozen", True): ["ct_bn_eval_group_fwd", "ct_bn_eval_group_bwd"],
    ("split", "train", False): ["ct_bn_group_fwd", "ct_bn_group_fwd", "ct_bn_group_bwd", "ct_bn_group_bwd"],
    ("split", "eval", False): ["ct_bn_eval_group_fwd", "ct_bn_eval_group_fwd"],
    ("split", "frozen", False): ["ct_bn_eval_group_fwd", "ct_bn_eval_group_fwd", "ct_bn_eval_group_bwd", "ct_bn_eval_group_bwd"],
    ("join", "train", True): ["ct_bn_group_fwd", "ct_bn_group_bwd"],
    ("join", "eval", True): ["ct_bn_eval_group_fwd"],
    ("join", "frozen", True): ["ct_bn_eval_group_fwd", "ct_bn_eval_group_bwd"],
    ("join", "train", False): ["ct_bn_group_fwd", "ct_bn_group_fwd", "ct_bn_group_bwd", "ct_bn_group_bwd"],
    ("join", "eval", False): ["ct_bn_eval_group_fwd", "ct_bn_eval_group_fwd"],
    ("join", "frozen", False): ["ct_bn_eval_group_fwd", "ct_bn_eval_group_fwd", "ct_bn_eval_group_bwd", "ct_bn_eval_group_bwd"],
    ("union", "train", True): ["ct_bn_group_fwd", "ct_bn_group_bwd"],
    ("union", "eval", True): ["ct_bn_eval_group_fwd"],
    ("union", "frozen", True): ["ct_bn_eval_group_fwd", "ct_bn_eval_group_bwd"],
}


@pytest.mark.parametrize("kind,mode,grouped", sorted(LITERAL))
def test_launch_sequences(kind, mode, grouped, monkeypatch):
    from cloud_transformers_amd import _lib, ops
    entry = {"single": {"train": ops.bn_relu, "eval": ops.bn_eval, "frozen": ops.bn_frozen},
             "split": {"train": ops.split_bn, "eval": ops.split_bn_eval, "frozen": ops.split_bn_frozen},
             "join": {"train": ops.join_bn_relu, "eval": ops.join_bn_relu_eval, "frozen": ops.join_bn_relu_frozen},
             "union": {"train": ops.union_keys_values, "eval": ops.union_keys_values_eval,
                       "frozen": ops.union_keys_values_frozen}}[kind][mode]
    seen, real = [], _lib.check
    monkeypatch.setattr(_lib, "check", lambda rc, name: (seen.append(name), real(rc, name))[1])
    monkeypatch.setattr(ops, "BN_GROUP_LAUNCH", grouped)
    grad = mode != "eval"
    with torch.set_grad_enabled(grad):
        route_args, args = _case(kind, mode, grad)
        assert ops.norm_route(**route_args) == mode
        out = entry(*args)
        outs = [out] if torch.is_tensor(out) else ([t for pair in out for t in pair] if kind == "union" else list(out))
        if grad:
            torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
    torch.cuda.synchronize()
    assert seen == LITERAL[kind, mode, grouped]
