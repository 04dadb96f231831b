"""Mixup / CutMix on the GPU: the batch-mixing kernel (augment.hip augment_mix_kernel) against the
CPU oracle, the pair-target instances of the two loss heads (fc_ce.hip and head.hip MIX) against
torch fp64 autograd of ``F.cross_entropy`` with the probability targets
lam * onehot(t1) + (1 - lam) * onehot(t2), and the VGG engine with ``set_mix`` (eager, fused /
separate bn_apply head, captured graph).  Measures and bounds are those of the tests of the same
name in test_label_smoothing_gpu / test_ops_gpu."""
import pytest
import torch
import torch.nn.functional as F

from distributed_pytorch_amd.ops import cpu_ref

pytestmark = pytest.mark.gpu

MEAN, STD = [0.49, 0.48, 0.45], [0.25, 0.24, 0.26]


def _C():
    from distributed_pytorch_amd import _ext

    return _ext.require()


def close(a, b, tol, what=""):
    """test_ops_gpu.close: max abs diff over max abs of the reference (printed before the assert)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    d = (a - b).abs().max().item()
    s = b.abs().max().clamp_min(1e-6).item()
    print(f"{what}: max abs diff {d:.3e} scale {s:.3e} rel {d / s:.3e} (bound {tol:g})")
    assert d <= tol * s, f"{what}: max abs diff {d} vs scale {s}"


def rel(a, b):
    """test_layers_gpu.rel"""
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


# ------------------------------------------------------------------ augment_mix
_SETS = {}


def _image_set(Hs, Ws):
    """A 50-image uint8 set (host and device copies), built once per shape."""
    if (Hs, Ws) not in _SETS:
        g = torch.Generator().manual_seed(5 + Hs)
        imgs = torch.randint(0, 256, (50, Hs, Ws, 3), dtype=torch.uint8, generator=g)
        labels = torch.randint(0, 10, (50,), generator=g)
        _SETS[(Hs, Ws)] = (imgs, labels, imgs.cuda(), labels.cuda())
    return _SETS[(Hs, Ws)]


def _mix_both(Hs, Ws, B, mode, lam, box, pad, seed=99, salt=12345):
    imgs, labels, imgs_d, labels_d = _image_set(Hs, Ws)
    idx = torch.randint(0, 50, (B,), generator=torch.Generator().manual_seed(B))
    ref = [torch.empty(B, Hs, Ws, 4), torch.empty(B, dtype=torch.int64), torch.empty(B, dtype=torch.int64),
           torch.empty(B)]
    cpu_ref.augment_mix(imgs, idx, labels, *ref, pad, seed, salt, MEAN, STD, mode, lam, *box)
    out = [torch.full((B, Hs, Ws, 4), 7.0, device="cuda"), torch.full((B,), -1, dtype=torch.int64, device="cuda"),
           torch.full((B,), -1, dtype=torch.int64, device="cuda"), torch.full((B,), -1.0, device="cuda")]
    _C().augment_mix(imgs_d, idx.cuda(), labels_d, *out, pad, seed, salt, MEAN, STD, mode, lam, *box)
    plain = torch.empty(B, Hs, Ws, 4, device="cuda")
    _C().augment(imgs_d, idx.cuda(), labels_d, plain, None, pad, True, seed, salt, MEAN, STD)
    torch.cuda.synchronize()
    return ref, out, plain


@pytest.mark.parametrize("B", [1, 2, 5, 17])
@pytest.mark.parametrize("Hs,Ws,pad", [(32, 32, 4), (8, 12, 2)])
def test_augment_mixup_matches_reference(Hs, Ws, pad, B):
    for lam in (0.0, 0.3, 1.0):
        ref, out, plain = _mix_both(Hs, Ws, B, cpu_ref.MIXUP, lam, (0, 0, 0, 0), pad)
        close(out[0], ref[0], 1e-6, f"mixup {Hs}x{Ws} B={B} lam={lam}")
        assert torch.equal(out[0][..., 3], torch.zeros(B, Hs, Ws, device="cuda"))
        assert torch.equal(out[1].cpu(), ref[1]) and torch.equal(out[2].cpu(), ref[2])
        assert torch.equal(out[3].cpu(), ref[3])
        if lam == 1.0:
            assert torch.equal(out[0], plain)
        if lam == 0.0:
            assert torch.equal(out[0], plain.flip(0))


@pytest.mark.parametrize("B", [1, 2, 5, 17])
@pytest.mark.parametrize("Hs,Ws,pad", [(32, 32, 4), (8, 12, 2)])
def test_augment_cutmix_is_bitwise_the_reference(Hs, Ws, pad, B):
    boxes = {"empty": (Hs // 2, Hs // 2, 3, 3), "full": (0, Hs, 0, Ws), "interior": (2, Hs - 3, 1, Ws - 5),
             "two edges": (Hs - 3, Hs, 0, 4)}
    for name, box in boxes.items():
        lam = 1.0 - (box[1] - box[0]) * (box[3] - box[2]) / (Hs * Ws)
        ref, out, plain = _mix_both(Hs, Ws, B, cpu_ref.CUTMIX, lam, box, pad)
        assert torch.equal(out[0].cpu(), ref[0]), name
        assert torch.equal(out[1].cpu(), ref[1]) and torch.equal(out[2].cpu(), ref[2]), name
        assert torch.equal(out[3].cpu(), ref[3]), name
        if name == "empty":
            assert torch.equal(out[0], plain)
        if name == "full":
            assert torch.equal(out[0], plain.flip(0))


def test_augment_mix_rejects_bad_arguments():
    imgs, labels, imgs_d, labels_d = _image_set(8, 12)
    idx = torch.arange(3).cuda()
    o = lambda: (torch.empty(3, 8, 12, 4, device="cuda"), torch.empty(3, dtype=torch.int64, device="cuda"),
                 torch.empty(3, dtype=torch.int64, device="cuda"), torch.empty(3, device="cuda"))
    for mode, lam, box in ((2, 0.5, (0, 0, 0, 0)), (0, 1.5, (0, 0, 0, 0)), (1, 0.5, (0, 9, 0, 12)),
                           (1, 0.5, (0, 8, -1, 12)), (1, 0.5, (5, 4, 0, 12))):
        with pytest.raises(RuntimeError):
            _C().augment_mix(imgs_d, idx, labels_d, *o(), 2, 1, 2, MEAN, STD, mode, lam, *box)


# ------------------------------------------------------------------ fc_ce_train MIX
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


def _soft(t1, t2, lam, J):
    la = lam.double().view(-1, 1)
    return la * F.one_hot(t1, J).double() + (1.0 - la) * F.one_hot(t2, J).double()


def _head_inputs(B, Cin, J, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, generator=g)
    w = torch.randn(J, Cin, generator=g) * 0.1
    b = torch.randn(J, generator=g)
    return (x, w, b) + _pair_targets(B, J, g)


def _outs(B, Cin, J):
    z = lambda *s: torch.zeros(*s, device="cuda")
    # loss_row, dlogits, dx, dw, db, loss_out, loss_accum
    return [z(B), z(B, J), z(B, Cin), z(J, Cin), z(J), z(1), z(1)]


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,Cin,J", [(1, 512, 10), (5, 512, 10), (7, 64, 3), (5, 100, 16), (3, 1024, 16)])
def test_fc_ce_train_mix_matches_torch(B, Cin, J, eps):
    x, w, b, t1, t2, lam = _head_inputs(B, Cin, J)
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    loss = F.cross_entropy(xr @ wr.t() + br, _soft(t1, t2, lam, J), label_smoothing=eps)
    gx, gw, gb = torch.autograd.grad(loss, (xr, wr, br))
    d = lambda z: z.cuda()
    lr_, dl, dx, dw, db, lo, acc = _outs(B, Cin, J)
    _C().fc_ce_train(d(x), d(w), d(b), d(t1), lr_, dl, dx, dw, db, lo, acc, label_smoothing=eps, target2=d(t2),
                     lam=d(lam))
    torch.cuda.synchronize()
    close(lo, loss.detach(), 1e-5, "loss")
    close(acc, loss.detach(), 1e-5, "loss_accum")
    close(dx, gx, 1e-5, "dx")
    close(dw, gw, 1e-5, "dW")
    close(db, gb, 1e-5, "db")
    rs = dl.double().sum(1).abs().max().item()
    print(f"dlogits row sums: max |sum| {rs:.3e} (bound {1e-6 / B:.3e})")
    assert rs <= 1e-6 / B


def test_fc_ce_bn_in_mix_bitwise():
    """BnIn prologue with pair targets: the fused call == torch BN + ReLU + 2x2 max-pool features
    (fma, as the kernel and bn_apply compute them) followed by the plain MIX call, bit for bit in
    loss_row, dlogits, dx and the stored features."""
    B, Cin, J, eps = 5, 512, 10, 0.1
    _, w, b, t1, t2, lam = _head_inputs(B, Cin, J, seed=5)
    g = torch.Generator().manual_seed(6)
    z = torch.randn(B, 2, 2, Cin, generator=g)
    scale = torch.rand(Cin, generator=g) + 0.5
    shift = torch.randn(Cin, generator=g) * 0.3
    # the kernel's fmaf(z, scale, shift) rounds once: in float64 the product is exact and the sum keeps
    # 29 more bits than float32, so rounding it to float32 gives the fma's result
    feat = torch.relu(z.double() * scale.double() + shift.double()).float().reshape(B, 4, Cin).amax(1).cuda()
    z, scale, shift, w, b, t1, t2, lam = (v.cuda() for v in (z, scale, shift, w, b, t1, t2, lam))
    a = _outs(B, Cin, J)
    xa = torch.zeros(B, Cin, device="cuda")
    _C().fc_ce_train(xa, w, b, t1, *a, bn_z=z, bn_scale=scale, bn_shift=shift, label_smoothing=eps, target2=t2,
                     lam=lam)
    p = _outs(B, Cin, J)
    _C().fc_ce_train(feat.contiguous(), w, b, t1, *p, label_smoothing=eps, target2=t2, lam=lam)
    torch.cuda.synchronize()
    assert torch.equal(xa, feat)
    for u, v in zip(a, p):  # loss_row, dlogits, dx (and dW, db, loss)
        assert torch.equal(u, v)
    assert a[0].abs().sum().item() > 0


def test_fc_ce_parts_mix_bitwise():
    """Pair targets: the row kernel (parts=1, the only part that takes them) then the weight-gradient
    kernel (parts=2) == both in one call (parts=3)."""
    B, Cin, J = 5, 512, 10
    x, w, b, t1, t2, lam = (v.cuda() for v in _head_inputs(B, Cin, J, seed=7))
    one, two = _outs(B, Cin, J), _outs(B, Cin, J)
    _C().fc_ce_train(x, w, b, t1, *one, parts=3, label_smoothing=0.1, target2=t2, lam=lam)
    _C().fc_ce_train(x, w, b, t1, *two, parts=1, label_smoothing=0.1, target2=t2, lam=lam)
    _C().fc_ce_train(x, w, b, t1, *two, parts=2)
    torch.cuda.synchronize()
    for u, v in zip(one, two):
        assert torch.equal(u, v)
    assert one[3].abs().sum().item() > 0 and one[5].item() > 0


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,Cin,J", [(5, 512, 10), (5, 100, 16)])
def test_no_mix_arguments_is_todays_fused_head(B, Cin, J, eps):
    x, w, b, t1, t2, lam = (v.cuda() for v in _head_inputs(B, Cin, J, seed=9))
    plain, none = _outs(B, Cin, J), _outs(B, Cin, J)
    _C().fc_ce_train(x, w, b, t1, *plain, label_smoothing=eps)
    _C().fc_ce_train(x, w, b, t1, *none, label_smoothing=eps, target2=None, lam=None)
    mixed = _outs(B, Cin, J)
    _C().fc_ce_train(x, w, b, t1, *mixed, label_smoothing=eps, target2=t2, lam=lam)
    torch.cuda.synchronize()
    for u, v in zip(plain, none):
        assert torch.equal(u, v)
    assert not torch.equal(mixed[1], plain[1])  # and pair targets are not
    for kw in ({"target2": t2}, {"lam": lam}):
        with pytest.raises(RuntimeError, match="together"):
            _C().fc_ce_train(x, w, b, t1, *none, label_smoothing=eps, **kw)
    for kw in ({"target2": t2.int(), "lam": lam}, {"target2": t2, "lam": lam.double()}, {"target2": t2[:-1], "lam": lam},
               {"target2": t2, "lam": lam.cpu()}):
        with pytest.raises(RuntimeError):
            _C().fc_ce_train(x, w, b, t1, *none, label_smoothing=eps, **kw)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_no_mix_arguments_is_todays_softmax_ce(eps):
    g = torch.Generator().manual_seed(10)
    N, J = 4, 257
    logits = torch.randn(N, J, generator=g).cuda()
    t1, t2, lam = (v.cuda() for v in _pair_targets(N, J, g))
    outs = []
    for kw in ({}, {"target2": None, "lam": None}):
        lr_, dl, lo = torch.zeros(N, device="cuda"), torch.zeros(N, J, device="cuda"), torch.zeros(1, device="cuda")
        _C().softmax_ce(logits, t1, lr_, dl, None, lo, None, label_smoothing=eps, **kw)
        outs.append((lr_, dl, lo))
    torch.cuda.synchronize()
    for u, v in zip(*outs):
        assert torch.equal(u, v)
    for kw in ({"target2": t2}, {"lam": lam}):
        with pytest.raises(RuntimeError, match="together"):
            _C().softmax_ce(logits, t1, outs[0][0], outs[0][1], None, outs[0][2], None, label_smoothing=eps, **kw)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("N,H,C,J", [(3, 2, 64, 10), (2, 1, 64, 257), (2, 1, 64, 1000)])
def test_head_ce_mix_matches_torch(N, H, C, J, eps):
    """Generic head with pair targets, bf16 input, upstream gradient 3.0: the measure and bounds of
    test_label_smoothing_gpu.test_head_ce_smoothed_matches_torch."""
    from distributed_pytorch_amd.ops import functional as Fn

    g = torch.Generator().manual_seed(8)
    x = torch.randn(N, H, H, C, generator=g).to(torch.bfloat16)
    w = torch.randn(J, C, generator=g) * 0.05
    b = torch.randn(J, generator=g) * 0.1
    t1, t2, lam = _pair_targets(N, J, g)
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    lr = F.cross_entropy(xr.mean(dim=(1, 2)) @ wr.t() + br, _soft(t1, t2, lam, J), label_smoothing=eps)
    (3.0 * lr).backward()
    xd, wd, bd = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    lo = Fn.head_ce(xd, wd, bd, t1.cuda(), label_smoothing=eps, target2=t2.cuda(), lam=lam.cuda())
    (3.0 * lo).backward()
    torch.cuda.synchronize()
    figs = (abs(lo.item() - lr.item()), rel(xd.grad, xr.grad), rel(wd.grad, wr.grad), rel(bd.grad, br.grad))
    print("loss diff %.3e (loss %.4f)  rel dx %.3e  dW %.3e  db %.3e" % (figs[0], lr.item(), *figs[1:]))
    assert figs[0] < 1e-5 * max(1, abs(lr.item()))
    assert xd.grad.dtype == torch.bfloat16
    assert figs[1] < 1e-2 and figs[2] < 1e-5 and figs[3] < 1e-5


# ------------------------------------------------------------------ engine
def _batch8(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(8, 32, 32, 4)
    x[..., :3] = torch.randn(8, 32, 32, 3, generator=g)
    t1, t2, lam = _pair_targets(8, 10, g)
    return x, t1, t2, lam


def _two_steps(e, x, t):
    losses = []
    for _ in range(2):
        e.forward_backward(x, t)
        e.sgd_step()
        e.finish_step()
        losses.append(e.loss.clone().reshape(1))
    return torch.cat(losses)


def _engine_pair(mix, x, t1, t2, lam):
    """Two steps (engine defaults: lr 0.1, momentum 0.9, wd 1e-4) of the fp32 GPU engine and of the CPU
    engine from the same init_parameters(seed) on the same batch, with or without the pair targets:
    (gpu engine, gpu losses, cpu losses, l2 distance of the two parameter arenas over the norm of the
    CPU engine's, fp64 torch loss of the first step)."""
    from distributed_pytorch_amd.engine import VGGEngine
    from distributed_pytorch_amd.models import VGG11

    cpu = VGGEngine("VGG11", "cpu", max_batch=8)
    cpu.init_parameters(seed=5)
    m = VGG11().double()
    m.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in cpu.state_dict().items()})
    logits = m(x[..., :3].permute(0, 3, 1, 2).double())
    l64 = (F.cross_entropy(logits, _soft(t1, t2, lam, 10)) if mix else F.cross_entropy(logits, t1)).item()
    if mix:
        cpu.set_mix(t2, lam)
    lc = _two_steps(cpu, x, t1)
    e = VGGEngine("VGG11", "cuda", max_batch=8, impl="fp32")
    e.init_parameters(seed=5)
    if mix:
        e.set_mix(t2.cuda(), lam.cuda())
    lg = _two_steps(e, x.cuda(), t1.cuda())
    torch.cuda.synchronize()
    e.check_signals()
    pc = cpu.params.flat.double()
    return e, lg, lc, ((e.params.flat.cpu().double() - pc).norm() / pc.norm()).item(), l64


def test_engine_mixed_step_matches_cpu_engine(monkeypatch):
    """Two steps of the fp32 GPU engine against the CPU engine (ops.cpu_ref), both with pair targets
    set, under the bounds of test_label_smoothing_gpu.test_engine_smoothed_step_matches_cpu_engine:
    losses within 1e-4 * max(1, |loss|) (also the first loss against fp64 torch with the soft-target
    criterion), and the two parameter arenas at most 4x as far apart (l2, relative) as the same two
    engines on the same batch without a mix, whose GPU step runs only kernels that existed before.
    Then DPA_FUSED_HEAD=0 (separate bn_apply + plain MIX head) must equal the fused-head run bit for
    bit, and set_mix(None, None) must give bitwise the unmixed step."""
    from distributed_pytorch_amd.engine import VGGEngine

    x, t1, t2, lam = _batch8(11)
    monkeypatch.setenv("DPA_FUSED_HEAD", "1")
    e, lg, lc, d_mix, l64 = _engine_pair(True, x, t1, t2, lam)
    e_plain, lg0, lc0, d_plain, l64p = _engine_pair(False, x, t1, t2, lam)
    assert e.fused_head
    print("mix losses gpu", lg.tolist(), "cpu", lc.tolist(), "fp64", l64, "| plain gpu", lg0.tolist(), "cpu",
          lc0.tolist(), "fp64", l64p)
    print(f"parameter distance gpu-cpu after two steps: mix {d_mix:.3e}  plain {d_plain:.3e}")
    for a_, b_ in zip(lg.cpu().tolist(), lc.tolist()):
        assert abs(a_ - b_) < 1e-4 * max(1.0, abs(b_)), (a_, b_)
    assert abs(lg[0].item() - l64) < 1e-4 * max(1.0, abs(l64))
    assert abs(lg0[0].item() - l64p) < 1e-4 * max(1.0, abs(l64p))
    # the mixed and the plain run are far apart: the checks can tell them apart
    assert (e.params.flat - e_plain.params.flat).norm().item() > 10 * d_mix * e.params.flat.norm().item()
    assert d_mix <= 4.0 * d_plain + 1e-6, (d_mix, d_plain)
    monkeypatch.setenv("DPA_FUSED_HEAD", "0")
    e0 = VGGEngine("VGG11", "cuda", max_batch=8, impl="fp32")
    assert not e0.fused_head
    e0.init_parameters(seed=5)
    e0.set_mix(t2.cuda(), lam.cuda())
    l0 = _two_steps(e0, x.cuda(), t1.cuda())
    torch.cuda.synchronize()
    assert torch.equal(e0.params.flat, e.params.flat) and torch.equal(l0, lg)
    # cleared: bitwise the engine that never had a mix
    monkeypatch.setenv("DPA_FUSED_HEAD", "1")
    e1 = VGGEngine("VGG11", "cuda", max_batch=8, impl="fp32")
    e1.init_parameters(seed=5)
    e1.set_mix(t2.cuda(), lam.cuda())
    e1.set_mix(None, None)
    l1 = _two_steps(e1, x.cuda(), t1.cuda())
    torch.cuda.synchronize()
    assert torch.equal(e1.params.flat, e_plain.params.flat) and torch.equal(l1, lg0)


def test_graphed_step_over_mixing_loader_matches_eager():
    """GraphedStep over a Mixup loader at batch 8 (2 eager warm-up steps + 3 replays) == 5 eager steps
    on the same batches, bit for bit in parameters, momentum and losses.  The replayed batches have
    different lambdas, none of them 1: the graph reads lambda from the loader's device buffer."""
    from distributed_pytorch_amd.data import DeviceLoader
    from distributed_pytorch_amd.data.cifar import synthetic_cifar
    from distributed_pytorch_amd.engine import VGGEngine
    from distributed_pytorch_amd.graph_step import GraphedStep
    from distributed_pytorch_amd.parallel import NullComm, make_sync

    ds = synthetic_cifar(40, seed=3)
    outs = []
    for graph in (False, True):
        e = VGGEngine("VGG11", "cuda", max_batch=8, impl="x3", lr=0.02)
        e.init_parameters(seed=4)
        loader = DeviceLoader(ds, 8, "cuda", train=True, seed=17, mixup=1.0)
        e.set_mix(*loader.mix)
        sync = make_sync("ddp", e, NullComm())
        gs = GraphedStep(e, sync, warmup=2) if graph else None
        losses, lams = [], []
        for x, t in loader:
            lams.append(loader.mix[1][:8].clone())
            if gs is not None:
                gs.run(x, t)
            else:
                sync.begin_step()
                e.forward_backward(x, t, grad_ready=sync.grad_ready, pre_forward=sync.pre_forward,
                                   params_free=sync.params_free)
                sync.update(sync.finish())
                e.finish_step()
            losses.append(e.loss.clone())
        torch.cuda.synchronize()
        e.check_signals()
        if gs is not None:
            assert gs.replays == 3 and gs.graph is not None
        lam_b = [float(l[0]) for l in lams]
        assert all(torch.equal(l, torch.full_like(l, v)) for l, v in zip(lams, lam_b))
        assert len(set(lam_b[2:])) == 3 and all(0.0 < v < 1.0 for v in lam_b[2:]), lam_b
        outs.append((e.params.flat.clone(), e.mom.flat.clone(), torch.stack(losses)))
    for a_, b_ in zip(outs[0], outs[1]):
        assert torch.equal(a_, b_)
