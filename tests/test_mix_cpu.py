"""Mixup / CutMix on the CPU paths (no GPU needed): the host mix parameters (ops.cpu_ref.mix_params),
the oracle batch mixing (cpu_ref.augment_mix), the oracle head with pair targets
(cpu_ref.fc_ce_train(target2=, lam=)), the VGG engine built on it (set_mix), the generic head's CPU
path, the DeviceLoader options and the command line.  The loss reference everywhere is torch's
``F.cross_entropy`` with the probability targets lam * onehot(t1) + (1 - lam) * onehot(t2)."""
import json
import os
import runpy
import sys

import pytest
import torch
import torch.nn.functional as F

from distributed_pytorch_amd.data import DeviceLoader, ShardSampler
from distributed_pytorch_amd.data.cifar import MEAN as CIFAR_MEAN
from distributed_pytorch_amd.data.cifar import STD as CIFAR_STD
from distributed_pytorch_amd.data.cifar import synthetic_cifar
from distributed_pytorch_amd.engine import VGGEngine
from distributed_pytorch_amd.models import VGG11
from distributed_pytorch_amd.ops import cpu_ref
from distributed_pytorch_amd.ops import functional as Fn

SHAPES = [(1, 512, 10), (5, 512, 10), (7, 64, 3), (5, 100, 16), (3, 1024, 16)]
MEAN, STD = [0.49, 0.48, 0.45], [0.25, 0.24, 0.26]


def _x4(x):
    x4 = torch.zeros(x.shape[0], x.shape[2], x.shape[3], 4)
    x4[..., :3] = x.float().permute(0, 2, 3, 1)
    return x4


def _pair_targets(B, J, g):
    """t1, t2 and a per-row lambda that includes 0, 1 and a row with t1 == t2 (as far as B allows:
    row 0 has lam 0.3 and t1 == t2, row 1 lam 0, row 2 lam 1)."""
    t1 = torch.randint(0, J, (B,), generator=g)
    t2 = torch.randint(0, J, (B,), generator=g)
    lam = torch.rand(B, generator=g)
    t1[0], t2[0], lam[0] = 0, 0, 0.3
    t1[-1] = J - 1
    if B > 1:
        lam[1] = 0.0
    if B > 2:
        lam[2] = 1.0
    return t1, t2, lam.float()


def _soft(t1, t2, lam, J, dtype=torch.float64):
    la = lam.to(dtype).view(-1, 1)
    return la * F.one_hot(t1, J).to(dtype) + (1.0 - la) * F.one_hot(t2, J).to(dtype)


# ------------------------------------------------------------------ mix_params
def test_mix_params_deterministic_and_distinct():
    for mode in (cpu_ref.MIXUP, cpu_ref.CUTMIX):
        a = cpu_ref.mix_params(7, 123, mode, 1.0, 32, 32)
        assert a == cpu_ref.mix_params(7, 123, mode, 1.0, 32, 32)
        assert a != cpu_ref.mix_params(7, 124, mode, 1.0, 32, 32)
        assert a != cpu_ref.mix_params(8, 123, mode, 1.0, 32, 32)
    # the documented hash input: no sample slot of the batch (slot indices are < 2^31) produces it
    assert cpu_ref.MIX_SLOT >= 2 ** 31


@pytest.mark.parametrize("alpha", [0.2, 1.0])
def test_mix_params_ranges(alpha):
    Hs, Ws = 8, 12
    lams = []
    for salt in range(1000):
        lam, y0, y1, x0, x1 = cpu_ref.mix_params(3, salt, cpu_ref.MIXUP, alpha, Hs, Ws)
        assert 0.0 <= lam <= 1.0 and (y0, y1, x0, x1) == (0, 0, 0, 0)
        lams.append(lam)
        lam, y0, y1, x0, x1 = cpu_ref.mix_params(3, salt, cpu_ref.CUTMIX, alpha, Hs, Ws)
        assert 0.0 <= lam <= 1.0
        assert 0 <= y0 <= y1 <= Hs and 0 <= x0 <= x1 <= Ws  # inside the image
        assert lam == 1.0 - (y1 - y0) * (x1 - x0) / (Hs * Ws)  # the exact area share
    assert len(set(lams)) > 900  # a stream, not a constant


@pytest.mark.parametrize("alpha", [0.0, -0.5])
def test_mix_params_alpha_must_be_positive(alpha):
    for mode in (cpu_ref.MIXUP, cpu_ref.CUTMIX):
        with pytest.raises(ValueError):
            cpu_ref.mix_params(1, 2, mode, alpha, 32, 32)


# ------------------------------------------------------------------ cpu_ref.augment_mix
def _imgs(n, Hs, Ws, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, Hs, Ws, 3), generator=g, dtype=torch.uint8),
            torch.randint(0, 10, (n,), generator=g))


def _plain(images, labels, idx, seed, salt, pad=2):
    B, Hs, Ws = idx.numel(), images.shape[1], images.shape[2]
    a, t = torch.zeros(B, Hs, Ws, 4), torch.zeros(B, dtype=torch.int64)
    cpu_ref.augment(images, idx, labels, a, t, pad, True, seed, salt, MEAN, STD)
    return a, t


def _mixed(images, labels, idx, seed, salt, mode, lam, box=(0, 0, 0, 0), pad=2):
    B, Hs, Ws = idx.numel(), images.shape[1], images.shape[2]
    out, t, t2, lo = torch.zeros(B, Hs, Ws, 4), torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64), \
        torch.zeros(B)
    cpu_ref.augment_mix(images, idx, labels, out, t, t2, lo, pad, seed, salt, MEAN, STD, mode, lam, *box)
    return out, t, t2, lo


@pytest.mark.parametrize("B", [1, 2, 5])
def test_augment_mix_against_flip_construction(B):
    images, labels = _imgs(20, 8, 12)
    idx = torch.randperm(20, generator=torch.Generator().manual_seed(B))[:B]
    a, t = _plain(images, labels, idx, 5, 9)
    out, t1, t2, lo = _mixed(images, labels, idx, 5, 9, cpu_ref.MIXUP, 0.3)
    l32 = torch.tensor(0.3, dtype=torch.float32)
    assert torch.equal(out, l32 * a + (1 - l32) * a.flip(0))
    assert torch.equal(out[..., 3], torch.zeros(B, 8, 12))
    assert torch.equal(t1, t) and torch.equal(t2, t.flip(0)) and torch.equal(lo, torch.full((B,), 0.3))
    box = (1, 6, 3, 12)  # touches the right edge; rows != columns
    out, t1, t2, lo = _mixed(images, labels, idx, 5, 9, cpu_ref.CUTMIX, 0.5, box)
    ref = a.clone()
    for b in range(B):  # per slot, per pixel: an independent construction
        for y in range(box[0], box[1]):
            for x in range(box[2], box[3]):
                ref[b, y, x] = a[B - 1 - b, y, x]
    assert torch.equal(out, ref)
    assert torch.equal(t1, t) and torch.equal(t2, t.flip(0)) and torch.equal(lo, torch.full((B,), 0.5))
    if B == 1:  # a batch of one pairs with itself: the plain image (Mixup up to the blend's rounding)
        mixed = _mixed(images, labels, idx, 5, 9, cpu_ref.MIXUP, 0.3)[0]
        assert (mixed - a).abs().max() <= 1e-6 * a.abs().max()
        assert torch.equal(out, a)


def test_augment_mix_empty_and_full_box():
    images, labels = _imgs(20, 8, 12, seed=1)
    idx = torch.tensor([3, 17, 4, 4, 9])
    a, _ = _plain(images, labels, idx, 2, 40)
    assert torch.equal(_mixed(images, labels, idx, 2, 40, cpu_ref.CUTMIX, 1.0, (4, 4, 7, 7))[0], a)  # empty: bitwise
    assert torch.equal(_mixed(images, labels, idx, 2, 40, cpu_ref.CUTMIX, 0.0, (0, 8, 0, 12))[0], a.flip(0))
    assert torch.equal(_mixed(images, labels, idx, 2, 40, cpu_ref.MIXUP, 1.0)[0], a)
    assert torch.equal(_mixed(images, labels, idx, 2, 40, cpu_ref.MIXUP, 0.0)[0], a.flip(0))
    for bad in ((0, 9, 0, 12), (-1, 4, 0, 4), (5, 4, 0, 4)):
        with pytest.raises(ValueError):
            _mixed(images, labels, idx, 2, 40, cpu_ref.CUTMIX, 0.5, bad)
    with pytest.raises(ValueError):
        _mixed(images, labels, idx, 2, 40, cpu_ref.MIXUP, 1.5)


# ------------------------------------------------------------------ cpu_ref.fc_ce_train
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,Cin,J", SHAPES)
def test_cpu_ref_fc_ce_train_mix_matches_torch(B, Cin, J, eps):
    """The oracle in float64 against torch float64 autograd of the soft-target cross-entropy: the
    bounds of test_label_smoothing_cpu (1e-12 relative to the largest reference element; dlogits
    row sums at most 1e-6 / B)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(J, Cin, generator=g, dtype=torch.float64) * 0.1
    b = torch.randn(J, generator=g, dtype=torch.float64)
    t1, t2, lam = _pair_targets(B, J, g)
    q = _soft(t1, t2, lam, J)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    logits = xr @ wr.t() + br
    loss = F.cross_entropy(logits, q, label_smoothing=eps)
    gx, gw, gb = torch.autograd.grad(loss, (xr, wr, br))
    rows = F.cross_entropy(logits.detach(), q, label_smoothing=eps, reduction="none")
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    lr_, dl, dx, dw, db, lo, acc = z(B), z(B, J), z(B, Cin), z(J, Cin), z(J), z(1), z(1)
    cpu_ref.fc_ce_train(x, w, b, t1, lr_, dl, dx, dw, db, lo, acc, label_smoothing=eps, target2=t2, lam=lam)
    for got, ref in ((lr_, rows), (lo, loss.detach().reshape(1)), (acc, loss.detach().reshape(1)), (dx, gx), (dw, gw),
                     (db, gb)):
        assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())
    assert dl.sum(1).abs().max().item() <= 1e-6 / B
    for kw in ({"target2": t2}, {"lam": lam}):
        with pytest.raises(ValueError):
            cpu_ref.fc_ce_train(x, w, b, t1, lr_, dl, dx, dw, db, lo, acc, **kw)


def test_cpu_ref_lam_one_is_the_plain_head():
    """lam = 1 on every row is the class-index loss of target, whatever target2 says."""
    g = torch.Generator().manual_seed(4)
    B, Cin, J = 5, 64, 10
    x, w, b = (torch.randn(B, Cin, generator=g, dtype=torch.float64),
               torch.randn(J, Cin, generator=g, dtype=torch.float64) * 0.1, torch.randn(J, generator=g, dtype=torch.float64))
    t1, t2, _ = _pair_targets(B, J, g)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    outs = []
    for kw in ({}, {"target2": t2, "lam": torch.ones(B)}):
        o = [z(B), z(B, J), z(B, Cin), z(J, Cin), z(J), z(1), z(1)]
        cpu_ref.fc_ce_train(x.clone(), w, b, t1, *o, label_smoothing=0.1, **kw)
        outs.append(o)
    for a_, b_ in zip(*outs):
        assert (a_ - b_).abs().max().item() <= 1e-14


# ------------------------------------------------------------------ engine
def test_engine_grads_match_autograd_mixed():
    """test_label_smoothing_cpu.test_engine_grads_match_autograd_smoothed with pair targets set
    through set_mix (eps = 0.1 as well): the torch module in float64 with the soft-target
    criterion, bounds 1e-4.  set_mix(None, None) afterwards: bitwise the unmixed step."""
    torch.manual_seed(1)
    m = VGG11().double()
    e = VGGEngine("VGG11", "cpu", max_batch=6, label_smoothing=0.1)
    e.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in m.state_dict().items()})
    x = torch.randn(6, 3, 32, 32, dtype=torch.float64)
    g = torch.Generator().manual_seed(2)
    t1, t2, lam = _pair_targets(6, 10, g)
    t2b, lamb = torch.zeros(8, dtype=torch.int64), torch.zeros(8)  # persistent buffers longer than the batch
    t2b[:6], lamb[:6] = t2, lam
    loss = F.cross_entropy(m(x), _soft(t1, t2, lam, 10), label_smoothing=0.1)
    fcb = dict(m.named_parameters())["fc1.bias"]
    (plain,) = torch.autograd.grad(F.cross_entropy(m(x), t1, label_smoothing=0.1), fcb)
    loss.backward()
    e.set_mix(t2b, lamb)
    l2 = e.forward_backward(_x4(x), t1)
    assert abs(l2.item() - loss.item()) < 1e-4
    # the unmixed criterion's head gradient is many bounds away: the check below can tell the two apart
    assert (fcb.grad - plain).abs().max().item() > 100 * 1e-4 * max(1.0, fcb.grad.abs().max().item())
    for n, p in m.named_parameters():
        gr = e._to_torch_layout(n, e.grads[n]).double()
        assert (gr - p.grad).abs().max().item() < 1e-4 * max(1.0, p.grad.abs().max().item()), n
    e2 = VGGEngine("VGG11", "cpu", max_batch=6, label_smoothing=0.1)
    e2.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in m.state_dict().items()})
    ref = e2.forward_backward(_x4(x), t1).clone()
    e.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in m.state_dict().items()})
    e.set_mix(None, None)
    got = e.forward_backward(_x4(x), t1)
    assert torch.equal(got, ref) and torch.equal(e.grads.flat, e2.grads.flat)
    with pytest.raises(ValueError):
        e.set_mix(t2b, None)
    with pytest.raises(ValueError):
        e.set_mix(t2b.int(), lamb)
    e.set_mix(t2b[:4], lamb[:4])
    with pytest.raises(ValueError):
        e.forward_backward(_x4(x), t1)  # buffers shorter than the batch


def test_head_ce_cpu_path_matches_torch():
    """HeadCE's CPU path with pair targets (float64, upstream gradient 3.0) against autograd through
    mean-pool + linear + soft-target cross_entropy, eps 0 and 0.1."""
    g = torch.Generator().manual_seed(8)
    N, H, C, J = 4, 2, 64, 10
    x = torch.randn(N, H, H, C, generator=g, dtype=torch.float64)
    w = torch.randn(J, C, generator=g, dtype=torch.float64) * 0.05
    b = torch.randn(J, generator=g, dtype=torch.float64) * 0.1
    t1, t2, lam = _pair_targets(N, J, g)
    for eps in (0.0, 0.1):
        xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        lr = F.cross_entropy(xr.mean(dim=(1, 2)) @ wr.t() + br, _soft(t1, t2, lam, J), label_smoothing=eps)
        (3.0 * lr).backward()
        xd, wd, bd = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        lo = Fn.head_ce(xd, wd, bd, t1, label_smoothing=eps, target2=t2, lam=lam)
        (3.0 * lo).backward()
        assert torch.allclose(lo, lr.detach(), rtol=1e-12, atol=1e-14)
        for got, ref in ((xd.grad, xr.grad), (wd.grad, wr.grad), (bd.grad, br.grad)):
            assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    with pytest.raises(ValueError):
        Fn.head_ce(x, w, b, t1, target2=t2)
    # ResNet.forward passes them through
    from distributed_pytorch_amd.models.resnet import ResNet

    torch.manual_seed(0)
    m = ResNet([1, 1, 1, 1], 10).double()
    xi = torch.randn(4, 40, 40, 3, generator=g, dtype=torch.float64)
    ref = F.cross_entropy(m(xi), _soft(t1, t2, lam, 10))
    assert torch.allclose(m(xi, t1, t2, lam), ref, rtol=1e-10, atol=1e-12)
    assert torch.allclose(m(xi, t1), F.cross_entropy(m(xi), t1), rtol=1e-10, atol=1e-12)


# ------------------------------------------------------------------ DeviceLoader
def _loader(ds, **kw):
    sampler = ShardSampler(len(ds), shuffle=True, seed=3)
    return DeviceLoader(ds, 8, "cpu", sampler=sampler, train=True, seed=11, **kw)


@pytest.mark.parametrize("opt", ["mixup", "cutmix"])
def test_loader_resume_is_bitwise_and_last_batch_pairs_within_itself(opt):
    ds = synthetic_cifar(29, seed=2)  # 3 full batches of 8 and one of 5
    ld = _loader(ds, **{opt: 1.0})
    ld.set_epoch(2)
    assert ld.mix is not None and ld.mix[0].dtype == torch.int64 and ld.mix[1].dtype == torch.float32
    assert ld.mix[0].shape == (8,) and ld.mix[1].shape == (8,)
    full = [(x.clone(), t.clone(), ld.mix[0][:x.shape[0]].clone(), ld.mix[1][:x.shape[0]].clone()) for x, t in ld]
    assert [f[0].shape[0] for f in full] == [8, 8, 8, 5]
    ld2 = _loader(ds, **{opt: 1.0})
    ld2.set_epoch(2)
    part = [(x.clone(), t.clone(), ld2.mix[0][:x.shape[0]].clone(), ld2.mix[1][:x.shape[0]].clone())
            for x, t in ld2.iterate(start_batch=2)]
    assert len(part) == 2
    for a, b in zip(full[2:], part):
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    lams = [float(f[3][0]) for f in full]
    assert len(set(lams)) == 4 and all(0.0 <= l <= 1.0 for l in lams)  # one lambda per batch
    for x, t, t2, lam in full:
        assert torch.equal(t2, t.flip(0))  # partner m-1-b of the batch's own m samples (5 in the last one)
        assert torch.equal(lam, torch.full_like(lam, float(lam[0])))
    # the last batch against the oracle construction on its own 5 samples
    idx = ld._epoch_indices()[24:]
    salt = 2 * 1_000_003 + 3
    mode = cpu_ref.MIXUP if opt == "mixup" else cpu_ref.CUTMIX
    lam, *box = cpu_ref.mix_params(11, salt, mode, 1.0, 32, 32)
    a, t = torch.zeros(5, 32, 32, 4), torch.zeros(5, dtype=torch.int64)
    cpu_ref.augment(ds.images, idx, ds.labels, a, t, 4, True, 11, salt, CIFAR_MEAN, CIFAR_STD)
    if opt == "mixup":
        l32 = torch.tensor(lam, dtype=torch.float32)
        ref = l32 * a + (1 - l32) * a.flip(0)
    else:
        ref = a.clone()
        ref[:, box[0]:box[1], box[2]:box[3]] = a.flip(0)[:, box[0]:box[1], box[2]:box[3]]
    assert torch.equal(full[3][0], ref) and torch.equal(full[3][1], t)
    assert float(full[3][3][0]) == pytest.approx(lam, rel=1e-7)


def test_loader_options_off_is_todays_loader():
    ds = synthetic_cifar(20, seed=2)
    a, b = _loader(ds), _loader(ds, mixup=0.0, cutmix=0.0)
    assert a.mix is None and b.mix is None
    calls = []
    orig = cpu_ref.augment

    class K:  # the backend sees exactly the plain augment call
        @staticmethod
        def augment(*args):
            calls.append(len(args))
            return orig(*args)

    c = DeviceLoader(ds, 8, "cpu", sampler=ShardSampler(len(ds), shuffle=True, seed=3), train=True, seed=11, backend=K)
    for (x1, t1), (x2, t2), (x3, t3) in zip(a, b, c):
        assert torch.equal(x1, x2) and torch.equal(t1, t2) and torch.equal(x1, x3) and torch.equal(t1, t3)
    assert calls == [11, 11, 11]


def test_loader_value_errors():
    ds = synthetic_cifar(16, seed=2)
    with pytest.raises(ValueError):
        DeviceLoader(ds, 8, "cpu", mixup=0.2, cutmix=1.0)
    with pytest.raises(ValueError):
        DeviceLoader(ds, 8, "cpu", mixup=-0.1)
    with pytest.raises(ValueError):
        DeviceLoader(ds, 8, "cpu", cutmix=-1.0)
    with pytest.raises(ValueError):
        DeviceLoader(ds, 8, "cpu", train=False, mixup=0.2)
    with pytest.raises(ValueError):
        DeviceLoader(ds, 8, "cpu", train=False, cutmix=0.2)


# ------------------------------------------------------------------ command line
def _run_main(args):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    argv = sys.argv
    sys.argv = ["main.py", "--device", "cpu", "--synthetic", "--batch-size", "4", "--max-iters", "2", "--train-size",
                "64", "--test-size", "8"] + args
    try:
        runpy.run_path(os.path.join(root, "main.py"), run_name="__main__")
    finally:
        sys.argv = argv


def test_cli_run_reports_mixup(tmp_path):
    jm = str(tmp_path / "m.json")
    _run_main(["--mixup", "0.2", "--json-metrics", jm])
    rec = json.loads(open(jm).read().splitlines()[-1])
    assert rec["mixup"] == 0.2 and "cutmix" not in rec


def test_cli_mixup_and_cutmix_are_exclusive(tmp_path, capsys):
    with pytest.raises(SystemExit) as ei:
        _run_main(["--mixup", "0.2", "--cutmix", "1.0"])
    assert ei.value.code == 2
    assert "not allowed with" in capsys.readouterr().err
