"""The classifier head for wide class counts (fc_ce.hip fc_ce_wide_rows + gemm_f32 weight gradient +
fc_ce_wide_db_loss) on the GPU, through fc_ce_train / fc_ce_eval and the VGG engine at 100 classes.
The reference is torch fp64 autograd of ``F.cross_entropy(x @ w.T + b, target or probabilities,
label_smoothing=eps)``; the measure is test_ops_gpu.close (max abs diff over the reference's max abs) at
its 1e-5."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, Cin, J): one partial row tile and one class past a 16-class tile; partial last row tile, Cin no
# multiple of 16, J % 16 = 4; the engine's shape; both maxima (every wave's full class share)
SHAPES = [(5, 64, 17), (37, 516, 100), (256, 512, 100), (19, 1024, 1024)]
MODES = {"plain": 0.0, "smooth": 0.1, "mix": 0.1}


def _C():
    from distributed_pytorch_amd import _ext

    return _ext.require()


def close(a, b, tol, what):
    """test_ops_gpu.close (figures printed before the assert)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    d = (a - b).abs().max().item()
    s = b.abs().max().clamp_min(1e-6).item()
    print(f"{what}: max abs diff {d:.3e} scale {s:.3e} rel {d / s:.3e} (bound {tol:g})")
    assert d <= tol * s, f"{what}: max abs diff {d} vs scale {s}"


@functools.lru_cache(maxsize=None)
def _inputs(B, Cin, J):
    """x, w, b, targets (class 0 and class J-1 among them), second targets (row 1: t2 == t), lam, and
    the fp64 logits.  Every row's fp64 top-2 logit gap exceeds 1e-3 * max |logit| (asserted: the seed
    was picked for it), so no near-tie decides an argmax."""
    g = torch.Generator().manual_seed(10)
    x = torch.randn(B, Cin, generator=g)
    w = torch.randn(J, Cin, generator=g) * 0.1
    b = torch.randn(J, generator=g)
    t = torch.randint(0, J, (B,), generator=g)
    t[0], t[-1] = 0, J - 1
    t2 = torch.randint(0, J, (B,), generator=g)
    t2[1] = t[1]
    lam = torch.rand(B, generator=g)
    z = x.double() @ w.double().t() + b.double()
    top = z.topk(2, dim=1).values
    assert (top[:, 0] - top[:, 1]).min().item() > 1e-3 * z.abs().max().item()
    return x, w, b, t, t2, lam, z


@functools.lru_cache(maxsize=None)
def _reference(B, Cin, J, mode):
    """fp64: loss, dlogits, dx, dW, db"""
    x, w, b, t, t2, lam, _ = _inputs(B, Cin, J)
    xr, wr, br = (v.double().requires_grad_(True) for v in (x, w, b))
    z = xr @ wr.t() + br
    if mode == "mix":
        lam64 = lam.double()[:, None]
        q = lam64 * F.one_hot(t, J).double() + (1 - lam64) * F.one_hot(t2, J).double()
        loss = F.cross_entropy(z, q, label_smoothing=MODES[mode])
    else:
        loss = F.cross_entropy(z, t, label_smoothing=MODES[mode])
    return (loss.detach(),) + torch.autograd.grad(loss, (z, xr, wr, br))


def _outs(B, Cin, J):
    z = lambda *s: torch.zeros(*s, device="cuda")
    # loss_row, dlogits, dx, dw, db, loss_out, loss_accum
    return [z(B), z(B, J), z(B, Cin), z(J, Cin), z(J), z(1), z(1)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B,Cin,J", SHAPES)
def test_train_matches_fp64(B, Cin, J, mode):
    x, w, b, t, t2, lam = (v.cuda() for v in _inputs(B, Cin, J)[:6])
    loss, gz, gx, gw, gb = _reference(B, Cin, J, mode)
    lr_, dl, dx, dw, db, lo, acc = _outs(B, Cin, J)
    kw = dict(label_smoothing=MODES[mode], **(dict(target2=t2, lam=lam) if mode == "mix" else {}))
    _C().fc_ce_train(x, w, b, t, lr_, dl, dx, dw, db, lo, acc, **kw)
    torch.cuda.synchronize()
    for got, ref, what in ((lo, loss, "loss"), (acc, loss, "loss_accum"), (dl, gz, "dlogits"), (dx, gx, "dx"),
                           (dw, gw, "dW"), (db, gb, "db")):
        close(got, ref, 1e-5, what)


@pytest.mark.parametrize("B,Cin,J", SHAPES)
def test_eval_matches_fp64(B, Cin, J):
    x, w, b, t, _, _, z = _inputs(B, Cin, J)
    lr_ = torch.zeros(B, device="cuda")
    corr = torch.zeros(B, dtype=torch.int32, device="cuda")
    logits, ev = torch.zeros(B, J, device="cuda"), torch.zeros(2, device="cuda")
    _C().fc_ce_eval(x.cuda(), w.cuda(), b.cuda(), t.cuda(), lr_, corr, logits, ev)
    torch.cuda.synchronize()
    close(logits, z, 1e-5, "logits")
    close(ev[0:1], F.cross_entropy(z, t).reshape(1), 1e-5, "mean loss")
    assert int(ev[1].item()) == int((z.argmax(1) == t).sum()) == int(corr.sum().item())


@pytest.mark.parametrize("B,Cin,J", [(21, 512, 100), (21, 512, 12)])
def test_bn_in_bitwise(B, Cin, J):
    """BnIn prologue (the pattern of test_label_smoothing_gpu.test_fc_ce_bn_in_smoothed_bitwise): the
    stored features are max over the 4 pixels of relu(z * scale + shift), and every output equals, bit
    for bit, the same call fed those features without bn_z (J = 100: the wide kernels; J = 12: bn_z
    does not change which kernels run, the one-row-per-wave ones)."""
    g = torch.Generator().manual_seed(6)
    w, b = (torch.randn(J, Cin, generator=g) * 0.1).cuda(), torch.randn(J, generator=g).cuda()
    t = torch.randint(0, J, (B,), generator=g).cuda()
    z = torch.randn(B, 2, 2, Cin, generator=g)
    scale, shift = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.3
    # fmaf rounds once: the fp64 product is exact and the fp64 sum keeps 29 bits more than fp32
    feat = torch.relu(z.double() * scale.double() + shift.double()).float().reshape(B, 4, Cin).amax(1).cuda()
    a, p = _outs(B, Cin, J), _outs(B, Cin, J)
    xa = torch.zeros(B, Cin, device="cuda")
    _C().fc_ce_train(xa, w, b, t, *a, bn_z=z.cuda(), bn_scale=scale.cuda(), bn_shift=shift.cuda())
    _C().fc_ce_train(feat.contiguous(), w, b, t, *p)
    torch.cuda.synchronize()
    assert torch.equal(xa, feat)
    names = ("loss_row", "dlogits", "dx", "dW", "db", "loss", "loss_accum")
    for u, v, what in zip(a, p, names):
        print(f"{what}: max abs diff {(u - v).abs().max().item():.3e} of max abs {v.abs().max().item():.3e}")
    for u, v, what in zip(a, p, names):
        assert torch.equal(u, v), what
    assert a[0].abs().sum().item() > 0


def test_parts_and_repeat_bitwise():
    """parts=1 then parts=2 == parts=3, and two runs of parts=3 are bitwise equal."""
    B, Cin, J = 37, 516, 100
    x, w, b, t = (v.cuda() for v in _inputs(B, Cin, J)[:4])
    one, two, again = _outs(B, Cin, J), _outs(B, Cin, J), _outs(B, Cin, J)
    _C().fc_ce_train(x, w, b, t, *one, parts=3, label_smoothing=0.1)
    _C().fc_ce_train(x, w, b, t, *two, parts=1, label_smoothing=0.1)
    _C().fc_ce_train(x, w, b, t, *two, parts=2)
    _C().fc_ce_train(x, w, b, t, *again, parts=3, label_smoothing=0.1)
    torch.cuda.synchronize()
    for u, v, r in zip(one, two, again):
        assert torch.equal(u, v) and torch.equal(u, r)
    assert one[3].abs().sum().item() > 0 and one[5].item() > 0


@pytest.mark.parametrize("impl", ["fp32", "h2"])
def test_engine_step_100_classes_matches_torch(impl):
    """test_ops_gpu.test_engine_step_matches_torch (its comparison and tolerances) at 100 classes, batch 16."""
    from distributed_pytorch_amd.engine import VGGEngine
    from distributed_pytorch_amd.models.vgg import VGG

    torch.manual_seed(1)
    m, N = VGG("VGG11", 100).double(), 16
    x, t = torch.randn(N, 3, 32, 32, dtype=torch.float64), torch.randint(0, 100, (N,))
    e = VGGEngine("VGG11", "cuda", num_classes=100, max_batch=N, impl=impl)
    e.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in m.state_dict().items()})
    loss = F.cross_entropy(m(x), t)
    loss.backward()
    x4 = torch.zeros(N, 32, 32, 4)
    x4[..., :3] = x.float().permute(0, 2, 3, 1)
    l2 = e.forward_backward(x4.cuda(), t.cuda())
    torch.cuda.synchronize()
    assert abs(l2.item() - loss.item()) < 1e-4 * max(1.0, abs(loss.item()))
    for n, p in m.named_parameters():
        gd = e._to_torch_layout(n, e.grads[n]).cpu()
        if p.grad.abs().max() < 1e-6:  # conv bias grads are analytically 0 (BN follows)
            assert gd.abs().max().item() < 1e-4
        else:
            close(gd, p.grad, 1e-3, n)
    sd = e.state_dict()
    for k, v in m.state_dict().items():
        if "running" in k:
            close(sd[k], v, 1e-4, k)


def test_graphed_step_100_classes_matches_eager():
    """2 eager warm-up steps + 3 replays of the captured step == 5 eager steps, bit for bit (h2, fused head)."""
    from distributed_pytorch_amd.engine import VGGEngine
    from distributed_pytorch_amd.graph_step import GraphedStep
    from distributed_pytorch_amd.parallel import NullComm, make_sync

    g, N = torch.Generator().manual_seed(21), 16
    xs = torch.randn(5, N, 32, 32, 4, generator=g)
    xs[..., 3] = 0
    ts = torch.randint(0, 100, (5, N), generator=g)
    outs = []
    for graph in (False, True):
        e = VGGEngine("VGG11", "cuda", num_classes=100, max_batch=N, impl="h2", lr=0.02)
        e.init_parameters(seed=4)
        sync = make_sync("ddp", e, NullComm())
        gs = GraphedStep(e, sync, warmup=2) if graph else None
        xb, tb = torch.empty(N, 32, 32, 4, device="cuda"), torch.empty(N, dtype=torch.int64, device="cuda")
        losses = []
        for x, t in zip(xs, ts):
            xb.copy_(x)
            tb.copy_(t)
            if gs is not None:
                gs.run(xb, tb)
            else:
                sync.begin_step()
                e.forward_backward(xb, tb, grad_ready=sync.grad_ready, pre_forward=sync.pre_forward,
                                   params_free=sync.params_free)
                sync.update(sync.finish())
                e.finish_step()
            losses.append(e.loss.clone())
        torch.cuda.synchronize()
        assert gs is None or (gs.replays == 3 and gs.graph is not None)
        outs.append((e.params.flat.clone(), e.mom.flat.clone(), torch.stack(losses)))
    assert e.fused_head and all(torch.equal(a_, b_) for a_, b_ in zip(*outs))
