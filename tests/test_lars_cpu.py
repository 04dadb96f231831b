"""LARS and global-norm gradient clipping on the flat arenas, CPU side: the plain-torch oracle of
the three kernels (ops/cpu_ref) against a hand-written per-tensor LARS in fp64, the CPU engine
against the reference module, the sync modes over two gloo ranks, the generic FlatSGD path, and
the unchanged default."""
import os

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

import dist_helpers as H
import lars_helpers as L
from distributed_pytorch_amd.engine import VGGEngine
from distributed_pytorch_amd.models import VGG11
from distributed_pytorch_amd.ops import cpu_ref

WORLD = 2


def close(a, b, tol):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    d = (a - b).abs().max().item()
    s = b.abs().max().clamp_min(1e-6).item()
    assert d <= tol * s, f"max abs diff {d} vs scale {s}"


def _x4(x):
    x4 = torch.zeros(x.shape[0], x.shape[2], x.shape[3], 4)
    x4[..., :3] = x.float().permute(0, 2, 3, 1)
    return x4


def test_block_map_layout():
    T = L.toy_tables(cpu_ref)
    assert cpu_ref.OPT_CHUNK == 8192
    assert T["segs"].tolist() == [[0, 1, 1], [1, 1, 1], [2, 2, 1], [4, 1, 0], [5, 4, 1]]
    bm = T["bmap"].tolist()
    assert [b[2] for b in bm] == [64, 8192, 8192, 64, 64, 8192, 8192, 8192, 128]
    assert bm[0][1] == 0 and all(a[1] + a[2] == b[1] for a, b in zip(bm, bm[1:]))  # the chunks tile the arena
    assert bm[-1][1] + bm[-1][2] == sum(L.TOY_EXTENTS)


@pytest.mark.parametrize("zeros", [False, True])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("first", [True, False])
def test_cpu_ref_matches_per_tensor_lars(first, clip, zeros):
    """cpu_ref's three functions == a loop over tensors in fp64 (clip_grad_norm_ semantics).
    zeros: segment "a" has g = 0 and segment "b" has p = 0, both must get ratio 1."""
    gscale = 0.5
    p, g, m = L.toy_arenas(3, zero_g="a" if zeros else None, zero_p="b" if zeros else None)
    norm = gscale * g.flat.double().norm().item()
    max_norm = 0.5 * norm if clip else 2.0 * norm
    ps = [p[n].clone() for n, _ in L.TOY]
    bs = [m[n].clone() for n, _ in L.TOY]
    total, c, ratios = L.lars_reference(ps, [g[n] for n, _ in L.TOY], bs, L.OPT["lr"], L.OPT["momentum"], L.OPT["wd"],
                                        gscale, first, L.OPT["trust"], L.OPT["eps"], max_norm)
    T = L.toy_tables(cpu_ref)
    L.run_step(cpu_ref, p.flat, g.flat, m.flat, T, gscale, max_norm, first)
    S = len(L.TOY)
    assert abs(T["stats"][2 * S].item() - total) <= 1e-12 * total
    assert abs(T["stats"][2 * S + 1].item() - c) <= 1e-12
    assert (c < 0.51) if clip else (c == 1.0)
    for i, (n, _) in enumerate(L.TOY):
        assert abs(T["table"][i].item() - ratios[i]) <= 1.2e-7 * ratios[i], n  # (the table is fp32)
        close(p[n], ps[i], 1e-6)
        close(m[n], bs[i], 1e-6)
    assert ratios[3] == 1.0 and T["table"][3].item() == 1.0  # the rank-1 tensor
    if zeros:
        assert T["table"][0].item() == 1.0 and T["table"][1].item() == 1.0
    else:
        assert all(r != 1.0 for i, r in enumerate(ratios) if i != 3)
    # the padding took no update
    for (n, _), ext in zip(L.TOY, L.TOY_EXTENTS):
        o, k = p.offsets[n], p.numels[n]
        assert p.flat[o + k:o + ext].abs().sum().item() == 0 and m.flat[o + k:o + ext].abs().sum().item() == 0


def test_cpu_ref_segmented_equals_flat_without_lars():
    """Ratio 1 and no clipping: the segmented update is sgd_flat, bit for bit."""
    p, g, m = L.toy_arenas(4)
    p2, m2 = p.flat.clone(), m.flat.clone()
    cpu_ref.sgd_flat(p2, g.flat, m2, L.OPT["lr"], L.OPT["momentum"], L.OPT["wd"], 0.5, False)
    T = L.toy_tables(cpu_ref, lars=False)
    L.run_step(cpu_ref, p.flat, g.flat, m.flat, T, 0.5, 1e30, False)
    assert torch.equal(p.flat, p2) and torch.equal(m.flat, m2)


LR, TRUST, CLIP = 1.0, 0.3, 1.0  # parameters move by > 100x the comparison bound in 3 steps


@pytest.fixture(scope="module")
def engine_vs_module():
    torch.manual_seed(1)
    m = VGG11().double()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    f32 = {k: v.float() if v.is_floating_point() else v for k, v in sd0.items()}
    e = VGGEngine("VGG11", "cpu", max_batch=4, lr=LR, optimizer="lars", trust_coef=TRUST, clip_grad_norm=CLIP)
    e.load_state_dict(f32)
    plain = VGGEngine("VGG11", "cpu", max_batch=4, lr=LR, optimizer="sgd", clip_grad_norm=0.0)
    plain.load_state_dict(f32)
    params = list(m.parameters())
    bufs = [torch.zeros_like(q) for q in params]
    g = torch.Generator().manual_seed(0)
    losses, clips = [], []
    for i in range(3):
        x = torch.randn(4, 3, 32, 32, generator=g, dtype=torch.float64)
        t = torch.randint(0, 10, (4,), generator=g)
        m.zero_grad()
        loss = F.cross_entropy(m(x), t)
        loss.backward()
        with torch.no_grad():
            total, c, _ = L.lars_reference([q.data for q in params], [q.grad for q in params], bufs, LR, 0.9, 1e-4,
                                           1.0, i == 0, TRUST, 1e-9, CLIP)
        for eng in (e, plain):
            l2 = eng.forward_backward(_x4(x), t)
            eng.sgd_step()
            eng.finish_step()
            if eng is e:
                losses.append((loss.item(), l2.item()))
                clips.append((total, c, e.opt_stats()))
    return dict(module=m, sd0=sd0, engine=e, plain=plain, losses=losses, clips=clips)


def test_cpu_engine_lars_matches_torch_oracle(engine_vs_module):
    """3 steps at batch 4 with LARS + clipping == the reference VGG11 module (fp64) under a
    per-parameter LARS written out in lars_helpers, to test_ddp_matches_torch_ddp's bounds."""
    r = engine_vs_module
    sd = r["engine"].state_dict()
    for k, v in r["module"].state_dict().items():
        if not v.is_floating_point():
            continue
        bound = 5e-4 * max(1.0, v.abs().max().item())
        d = (sd[k].double() - v).abs().max().item()
        assert d < bound, (k, d)
        if v.ndim >= 2:  # the adapted tensors moved by > 100x the bound: the comparison has teeth
            assert (v - r["sd0"][k]).abs().max().item() > 100 * bound, k
    assert all(abs(a - b) < 1e-3 for a, b in r["losses"]), r["losses"]
    for total, c, st in r["clips"]:
        assert c < 1.0 and abs(st["clip_coef"] - c) < 1e-4 * c and abs(st["grad_norm"] - total) < 1e-4 * total


def test_cpu_engine_lars_differs_from_plain_sgd(engine_vs_module):
    r = engine_vs_module
    a, b = r["engine"].params.flat, r["plain"].params.flat
    assert torch.isfinite(a).all()
    assert (a - b).abs().max().item() > 1e-2


def _spawn(fn, *args):
    port = H.free_port()
    mp.start_processes(fn, args=(WORLD, port) + args, nprocs=WORLD, join=True, start_method="spawn")


@pytest.fixture(scope="module")
def lars_modes(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("lars_modes"))
    out = {}
    for mode in ("gather", "allreduce", "ddp", "zero1"):
        _spawn(L.run_engine_mode_lars, mode, 3, d)
        out[mode] = [torch.load(os.path.join(d, f"lars_{mode}_{r}.pt"), weights_only=True) for r in range(WORLD)]
    return out


@pytest.mark.parametrize("mode", ["gather", "allreduce", "ddp"])
def test_two_ranks_lars_replicas_identical(lars_modes, mode):
    r0, r1 = lars_modes[mode]
    assert torch.equal(r0["params"], r1["params"]), f"{mode}: parameters diverged across ranks"
    assert r0["stats"]["clip_coef"] < 1.0 and r0["stats"]["tensors"]["layers.0.weight"]["trust_ratio"] != 1.0


def test_two_ranks_lars_modes_agree(lars_modes):
    a = lars_modes["gather"][0]["params"]
    for m in ("allreduce", "ddp"):
        b = lars_modes[m][0]["params"]
        assert (a - b).abs().max().item() < 1e-5 * max(1.0, a.abs().max().item()), m
    for r in range(WORLD):
        la = lars_modes["gather"][r]["losses"]
        for m in ("allreduce", "ddp"):
            assert all(abs(x - y) < 1e-4 for x, y in zip(la, lars_modes[m][r]["losses"]))


def test_two_ranks_zero1_refuses_lars(lars_modes):
    for r in range(WORLD):
        err = lars_modes["zero1"][r]["error"]
        assert err is not None and "zero1" in err and "shard" in err, err


def test_null_comm_zero1_runs_lars():
    """One rank without a communicator updates the whole arena, so zero1 works with LARS."""
    from distributed_pytorch_amd.parallel import NullComm, make_sync

    outs = []
    for mode in ("zero1", "ddp"):
        e = VGGEngine("VGG11", "cpu", max_batch=2, lr=0.05, optimizer="lars", clip_grad_norm=1.0)
        e.init_parameters(seed=2)
        sync = make_sync(mode, e, NullComm())
        x, t = H._batches(0, 1, n=2)[0]
        sync.begin_step()
        e.forward_backward(_x4(x), t, grad_ready=sync.grad_ready, pre_forward=sync.pre_forward,
                           params_free=sync.params_free)
        sync.update(sync.finish())
        e.finish_step()
        outs.append(e.params.flat.clone())
    assert torch.equal(outs[0], outs[1])


def test_fused_step_is_turned_off(monkeypatch, capsys):
    from distributed_pytorch_amd.parallel import NullComm, make_sync

    monkeypatch.setenv("DPA_FUSED_STEP", "1")
    e = VGGEngine("VGG11", "cpu", max_batch=2, clip_grad_norm=1.0)
    assert e.whole_arena_step and e.optimizer == "sgd"
    sync = make_sync("ddp", e, NullComm())
    assert sync.fuse_step is False and sync.fusable_step is False
    assert "DPA_FUSED_STEP=1 ignored" in capsys.readouterr().out
    plain = make_sync("ddp", VGGEngine("VGG11", "cpu", max_batch=2, optimizer="sgd", clip_grad_norm=0.0), NullComm())
    assert plain.fuse_step is True


def test_flat_sgd_lars_matches_oracle():
    """parallel/ddp.FlatSGD with LARS + clipping on the small ResNet of run_generic_ddp (fp64, one
    process) == the per-tensor oracle on a copy of the network.  Both run the same fp64 autograd,
    so they differ only by the rounding of the update: 1e-9 of each tensor's largest value."""
    from distributed_pytorch_amd.models.resnet import ResNet
    from distributed_pytorch_amd.parallel.ddp import DistributedDataParallel, FlatSGD

    torch.manual_seed(5)
    ours = ResNet([1, 1, 1, 1], 10).double()
    ref = ResNet([1, 1, 1, 1], 10).double()
    ref.load_state_dict(ours.state_dict())
    sd0 = {k: v.clone() for k, v in ours.state_dict().items()}
    g = torch.Generator().manual_seed(40)
    data = [(torch.randn(3, 32, 32, 3, generator=g, dtype=torch.float64), torch.randint(0, 10, (3,), generator=g))
            for _ in range(3)]
    kw = dict(lr=0.5, momentum=0.9, wd=1e-4, trust=0.1, clip=1.0)
    m = DistributedDataParallel(ours, None, bucket_mb=0.5)
    opt = FlatSGD(m, lr=kw["lr"], momentum=kw["momentum"], weight_decay=kw["wd"], trust_coef=kw["trust"],
                  clip_grad_norm=kw["clip"])
    rp = [q for q in ref.parameters() if q.requires_grad]
    bufs = [torch.zeros_like(q) for q in rp]
    for i, (x, t) in enumerate(data):
        opt.zero_grad()
        F.cross_entropy(m(x), t).backward()
        opt.step(m.finish())
        ref.zero_grad()
        F.cross_entropy(ref(x), t).backward()
        with torch.no_grad():
            _, c, _ = L.lars_reference([q.data for q in rp], [q.grad for q in rp], bufs, kw["lr"], kw["momentum"],
                                       kw["wd"], 1.0, i == 0, kw["trust"], 1e-9, kw["clip"])
        assert c < 1.0
    moved = 0.0
    for (k, a), b in zip(ours.state_dict().items(), ref.state_dict().values()):
        if a.is_floating_point():
            s = b.abs().max().clamp_min(1e-12).item()
            assert (a - b).abs().max().item() <= 1e-9 * s, k
            moved = max(moved, (b - sd0[k]).abs().max().item() / s)
    assert moved > 1e-2


def test_partial_update_raises_with_lars():
    e = VGGEngine("VGG11", "cpu", max_batch=2, optimizer="lars")
    with pytest.raises(ValueError, match="whole arena"):
        e.sgd_step(offset=64)
    with pytest.raises(ValueError, match="whole arena"):
        e.sgd_step(count=128)
    with pytest.raises(ValueError):
        VGGEngine("VGG11", "cpu", max_batch=2, optimizer="adam")


def test_environment_selects_lars(monkeypatch):
    monkeypatch.setenv("DPA_OPTIMIZER", "lars")
    monkeypatch.setenv("DPA_TRUST_COEF", "0.01")
    monkeypatch.setenv("DPA_CLIP_GRAD_NORM", "2.5")
    e = VGGEngine("VGG11", "cpu", max_batch=2)
    assert (e.optimizer, e.trust_coef, e.clip_grad_norm, e.whole_arena_step) == ("lars", 0.01, 2.5, True)
    e = VGGEngine("VGG11", "cpu", max_batch=2, optimizer="sgd", clip_grad_norm=0.0)  # arguments win
    assert not e.whole_arena_step


def test_cli_flags_reach_the_engine(tmp_path):
    """main.py --optimizer lars --clip-grad-norm 1: trains, and --json-metrics gains the norms."""
    import json
    import runpy
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    jm = str(tmp_path / "m.json")
    argv = sys.argv
    sys.argv = ["main.py", "--device", "cpu", "--synthetic", "--batch-size", "4", "--max-iters", "2", "--train-size",
                "64", "--test-size", "8", "--optimizer", "lars", "--trust-coef", "0.02", "--clip-grad-norm", "1",
                "--json-metrics", jm]
    try:
        runpy.run_path(os.path.join(root, "main.py"), run_name="__main__")
    finally:
        sys.argv = argv
    rec = json.loads(open(jm).read().splitlines()[-1])
    assert rec["grad_norm"] > 0 and 0 < rec["clip_coef"] <= 1.0


def test_default_is_unchanged(monkeypatch):
    """No argument, no environment variable: plain SGD through sgd_flat, equal to optimizer="sgd"."""
    for v in ("DPA_OPTIMIZER", "DPA_TRUST_COEF", "DPA_CLIP_GRAD_NORM"):
        monkeypatch.delenv(v, raising=False)
    outs = []
    for kw in ({}, {"optimizer": "sgd"}):
        e = VGGEngine("VGG11", "cpu", max_batch=4, lr=0.05, **kw)
        e.init_parameters(seed=3)
        assert not getattr(e, "whole_arena_step", False)
        for x, t in H._batches(0, 2):
            e.forward_backward(_x4(x), t)
            e.sgd_step()
            e.finish_step()
        outs.append((e.params.flat.clone(), e.mom.flat.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
