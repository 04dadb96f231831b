"""Label smoothing of the training loss on the CPU paths (no GPU needed): the oracle backend's fused
head (ops.cpu_ref.fc_ce_train), the VGG engine built on it, the generic head's CPU fallback
(ops/functional.HeadCE), the ResNet model, and the argument / environment / command-line plumbing.
The reference everywhere is torch's ``F.cross_entropy(..., label_smoothing=eps)`` (mean reduction,
class-index targets)."""
import argparse

import pytest
import torch
import torch.nn.functional as F

from distributed_pytorch_amd.engine import VGGEngine
from distributed_pytorch_amd.models import VGG11
from distributed_pytorch_amd.models.resnet import ResNet
from distributed_pytorch_amd.ops import cpu_ref
from distributed_pytorch_amd.ops import functional as Fn

SHAPES = [(1, 512, 10), (5, 512, 10), (7, 64, 3), (5, 100, 16), (3, 1024, 16)]


def _x4(x):
    x4 = torch.zeros(x.shape[0], x.shape[2], x.shape[3], 4)
    x4[..., :3] = x.float().permute(0, 2, 3, 1)
    return x4


def _targets(B, J, g):
    """Class-index targets that include class 0 and class J-1 (B >= 2), the two ends of the row."""
    t = torch.randint(0, J, (B,), generator=g)
    t[0] = 0
    t[-1] = J - 1
    return t


@pytest.mark.parametrize("eps", [0.1, 0.5])
@pytest.mark.parametrize("B,Cin,J", SHAPES)
def test_cpu_ref_fc_ce_train_matches_torch(B, Cin, J, eps):
    """The oracle in float64 against torch float64 autograd: the closed forms are exact, so the
    bound is rounding only (1e-12 relative to the largest reference element)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(J, Cin, generator=g, dtype=torch.float64) * 0.1
    b = torch.randn(J, generator=g, dtype=torch.float64)
    t = _targets(B, J, g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    logits = xr @ wr.t() + br
    loss = F.cross_entropy(logits, t, label_smoothing=eps)
    gx, gw, gb = torch.autograd.grad(loss, (xr, wr, br))
    rows = F.cross_entropy(logits.detach(), t, label_smoothing=eps, reduction="none")
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    lr_, dl, dx, dw, db, lo, acc = z(B), z(B, J), z(B, Cin), z(J, Cin), z(J), z(1), z(1)
    cpu_ref.fc_ce_train(x, w, b, t, lr_, dl, dx, dw, db, lo, acc, label_smoothing=eps)
    for got, ref in ((lr_, rows), (lo, loss.detach().reshape(1)), (acc, loss.detach().reshape(1)), (dx, gx), (dw, gw),
                     (db, gb)):
        assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())
    assert dl.sum(1).abs().max().item() <= 1e-6 / B
    with pytest.raises(ValueError):
        cpu_ref.fc_ce_train(x, w, b, t, lr_, dl, dx, dw, db, lo, acc, label_smoothing=1.0)


def test_cpu_ref_zero_smoothing_is_the_plain_head():
    g = torch.Generator().manual_seed(4)
    B, Cin, J = 5, 64, 10
    x, w, b = torch.randn(B, Cin, generator=g), torch.randn(J, Cin, generator=g) * 0.1, torch.randn(J, generator=g)
    t = _targets(B, J, g)
    outs = []
    for kw in ({}, {"label_smoothing": 0.0}):
        o = [torch.zeros(B), torch.zeros(B, J), torch.zeros(B, Cin), torch.zeros(J, Cin), torch.zeros(J),
             torch.zeros(1), torch.zeros(1)]
        cpu_ref.fc_ce_train(x.clone(), w, b, t, *o, **kw)
        outs.append(o)
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)


def test_engine_grads_match_autograd_smoothed():
    """test_engine_cpu.test_engine_grads_match_autograd with the smoothed criterion on both sides
    (same seeds, batch and bounds: 1e-4)."""
    torch.manual_seed(1)
    m = VGG11().double()
    e = VGGEngine("VGG11", "cpu", max_batch=6, label_smoothing=0.1)
    e.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in m.state_dict().items()})
    x = torch.randn(6, 3, 32, 32, dtype=torch.float64)
    t = torch.randint(0, 10, (6,))
    loss = F.cross_entropy(m(x), t, label_smoothing=0.1)
    plain = F.cross_entropy(m(x), t).item()
    loss.backward()
    l2 = e.forward_backward(_x4(x), t)
    assert abs(l2.item() - loss.item()) < 1e-4
    assert abs(loss.item() - plain) > 1e-2  # the smoothed loss is a different number: the check above can tell
    for n, p in m.named_parameters():
        g = e._to_torch_layout(n, e.grads[n]).double()
        assert (g - p.grad).abs().max().item() < 1e-4 * max(1.0, p.grad.abs().max().item()), n


def test_engine_training_matches_torch_sgd_smoothed():
    """test_engine_cpu.test_engine_training_matches_torch_sgd with the smoothed criterion on both
    sides (3 steps, bounds 2e-4); loss_accum sums the smoothed losses."""
    torch.manual_seed(1)
    m = VGG11().double()
    e = VGGEngine("VGG11", "cpu", max_batch=8, lr=0.01, label_smoothing=0.1)
    e.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in m.state_dict().items()})
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    g = torch.Generator().manual_seed(0)
    total = 0.0
    for _ in range(3):
        x = torch.randn(8, 3, 32, 32, generator=g, dtype=torch.float64)
        t = torch.randint(0, 10, (8,), generator=g)
        opt.zero_grad()
        loss = F.cross_entropy(m(x), t, label_smoothing=0.1)
        loss.backward()
        opt.step()
        total += loss.item()
        e.forward_backward(_x4(x), t)
        e.sgd_step()
        e.finish_step()
    assert abs(float(e.loss_accum.reshape(-1)[0]) - total) < 2e-4 * max(1.0, total)
    sd = e.state_dict()
    for k, v in m.state_dict().items():
        if v.is_floating_point():
            assert (sd[k].double() - v).abs().max().item() < 2e-4 * max(1.0, v.abs().max().item()), k
        else:
            assert int(sd[k]) == int(v) == 3


def test_engine_eval_is_plain_cross_entropy():
    """Evaluation does not see label smoothing: same state, eps = 0.1 and eps = 0 -> the same
    accumulated test loss and correct count, bit for bit."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 32, 32, 4, generator=g)
    x[..., 3] = 0
    t = torch.randint(0, 10, (4,), generator=g)
    accs = []
    for eps in (0.1, 0.0):
        e = VGGEngine("VGG11", "cpu", max_batch=4, label_smoothing=eps)
        e.init_parameters(seed=2)
        e.begin_eval()
        e.eval_batch(x, t)
        accs.append(e.eval_acc.clone())
    assert torch.equal(accs[0], accs[1]) and accs[0][0] > 0


def test_head_ce_cpu_fallback_matches_torch():
    """HeadCE's CPU fallback (float64): loss and the gradients the node forms itself (dx, dW, db,
    upstream gradient 3.0) against autograd through mean-pool + linear + smoothed cross_entropy."""
    g = torch.Generator().manual_seed(8)
    N, H, C, J = 3, 2, 64, 10
    x = torch.randn(N, H, H, C, generator=g, dtype=torch.float64)
    w = torch.randn(J, C, generator=g, dtype=torch.float64) * 0.05
    b = torch.randn(J, generator=g, dtype=torch.float64) * 0.1
    t = _targets(N, J, g)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    lr = F.cross_entropy(xr.mean(dim=(1, 2)) @ wr.t() + br, t, label_smoothing=0.1)
    (3.0 * lr).backward()
    xd, wd, bd = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    lo = Fn.head_ce(xd, wd, bd, t, label_smoothing=0.1)
    (3.0 * lo).backward()
    assert torch.allclose(lo, lr.detach(), rtol=1e-12, atol=1e-14)
    for got, ref in ((xd.grad, xr.grad), (wd.grad, wr.grad), (bd.grad, br.grad)):
        assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    # eps = 0 and no argument: the plain head, bit for bit
    assert torch.equal(Fn.head_ce(x, w, b, t), Fn.head_ce(x, w, b, t, label_smoothing=0.0))
    assert torch.equal(Fn.head_ce(x, w, b, t), F.cross_entropy(x.mean(dim=(1, 2)) @ w.t() + b, t))


def test_resnet_smoothed_loss_matches_logits_head():
    """model(x, target) with label_smoothing=0.1 == the same model through head_logits + stock
    smoothed cross_entropy (float64 on the CPU path): loss and every parameter gradient."""
    torch.manual_seed(0)
    m = ResNet([1, 1, 1, 1], 10, label_smoothing=0.1).double()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(3, 40, 40, 3, generator=g, dtype=torch.float64)
    t = torch.randint(0, 10, (3,), generator=g)
    lo = m(x, t)
    (2.5 * lo).backward()
    got = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    lr = F.cross_entropy(m(x), t, label_smoothing=0.1)
    (2.5 * lr).backward()
    assert torch.allclose(lo, lr, rtol=1e-10, atol=1e-12)
    assert abs(lr.item() - F.cross_entropy(m(x), t).item()) > 1e-3  # smoothing changes the number
    for n, p in m.named_parameters():
        err = (got[n] - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-12)
        assert err < 1e-8, (n, float(err))
    # logits do not depend on it
    plain = ResNet([1, 1, 1, 1], 10).double()
    plain.load_state_dict(m.state_dict())
    assert plain.label_smoothing == 0.0
    plain.eval(), m.eval()
    assert torch.equal(plain(x), m(x))


@pytest.mark.parametrize("eps", [-0.1, 1.0])
def test_out_of_range_raises(eps, monkeypatch):
    x, w, b = torch.randn(2, 1, 1, 8), torch.randn(3, 8), torch.randn(3)
    t = torch.tensor([0, 2])
    with pytest.raises(ValueError):
        VGGEngine("VGG11", "cpu", max_batch=2, label_smoothing=eps)
    with pytest.raises(ValueError):
        Fn.head_ce(x, w, b, t, label_smoothing=eps)
    with pytest.raises(ValueError):
        ResNet([1, 1, 1, 1], 10, label_smoothing=eps)
    monkeypatch.setenv("DPA_LABEL_SMOOTHING", str(eps))
    with pytest.raises(ValueError):
        VGGEngine("VGG11", "cpu", max_batch=2)


def test_environment_and_argument(monkeypatch):
    monkeypatch.delenv("DPA_LABEL_SMOOTHING", raising=False)
    assert VGGEngine("VGG11", "cpu", max_batch=2).label_smoothing == 0.0
    monkeypatch.setenv("DPA_LABEL_SMOOTHING", "0.2")
    assert VGGEngine("VGG11", "cpu", max_batch=2).label_smoothing == 0.2
    assert VGGEngine("VGG11", "cpu", max_batch=2, label_smoothing=0.1).label_smoothing == 0.1  # the argument wins
    assert VGGEngine("VGG11", "cpu", max_batch=2, label_smoothing=0.0).label_smoothing == 0.0


def test_cli_flag_reaches_the_engine(monkeypatch):
    from distributed_pytorch_amd import train

    monkeypatch.setenv("DPA_LABEL_SMOOTHING", "0.3")
    ap = argparse.ArgumentParser()
    train.add_common_args(ap)
    args = ap.parse_args(["--batch-size", "4", "--label-smoothing", "0.1"])
    assert args.label_smoothing == 0.1
    assert train.build_engine(args, "cpu").label_smoothing == 0.1
    args = ap.parse_args(["--batch-size", "4"])  # flag left out: the environment, as for the LARS flags
    assert args.label_smoothing is None
    assert train.build_engine(args, "cpu").label_smoothing == 0.3
    with pytest.raises(ValueError):
        train.build_engine(ap.parse_args(["--batch-size", "4", "--label-smoothing", "1.0"]), "cpu")


def test_cli_run_reports_label_smoothing(tmp_path):
    """main.py --label-smoothing 0.1: trains, and the --json-metrics line carries the factor (as
    test_lars_cpu.test_cli_flags_reach_the_engine does for the LARS flags)."""
    import json
    import os
    import runpy
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jm = str(tmp_path / "m.json")
    argv = sys.argv
    sys.argv = ["main.py", "--device", "cpu", "--synthetic", "--batch-size", "4", "--max-iters", "2", "--train-size",
                "64", "--test-size", "8", "--label-smoothing", "0.1", "--json-metrics", jm]
    try:
        runpy.run_path(os.path.join(root, "main.py"), run_name="__main__")
    finally:
        sys.argv = argv
    rec = json.loads(open(jm).read().splitlines()[-1])
    assert rec["label_smoothing"] == 0.1
