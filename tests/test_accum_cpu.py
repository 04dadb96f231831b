"""Gradient accumulation on the CPU backend (no GPU needed): the fold's reference, the accumulated
step against the engine oracle (bitwise) and against torch, short groups, two gloo ranks in all four
sync modes with every communicator call counted, and the command line."""
import argparse
import json
import os

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

import accum_helpers as AH
import dist_helpers as H
from distributed_pytorch_amd.accum import AccumulatedStep, updates_per_epoch, validate_args
from distributed_pytorch_amd.engine import VGGEngine
from distributed_pytorch_amd.models import VGG11
from distributed_pytorch_amd.ops import cpu_ref
from distributed_pytorch_amd.parallel import NullComm, make_sync
from distributed_pytorch_amd.schedule import lr_table
from distributed_pytorch_amd.utils.checkpoint import ResumeMismatch


# ---------------------------------------------------------------- cpu_ref.grad_fold
def test_cpu_ref_grad_fold_modes_on_a_slice():
    g = torch.Generator().manual_seed(0)
    acc0, g0 = torch.randn(96, generator=g), torch.randn(96, generator=g)
    off, cnt = 8, 36
    sl = slice(off, off + cnt)
    for mode in (0, 1, 2):
        acc, grad = acc0.clone(), g0.clone()
        cpu_ref.grad_fold(acc, grad, mode, off, cnt)
        want_acc, want_g = acc0.clone(), g0.clone()
        if mode == 0:
            want_acc[sl] = g0[sl]
        elif mode == 1:
            want_acc[sl] = torch.add(acc0[sl], g0[sl])
        else:
            want_g[sl] = torch.add(acc0[sl], g0[sl])
        assert torch.equal(acc, want_acc) and torch.equal(grad, want_g), mode
    acc, grad = acc0.clone(), g0.clone()
    cpu_ref.grad_fold(acc, grad, 1)  # defaults: the whole arena
    assert torch.equal(acc, torch.add(acc0, g0)) and torch.equal(grad, g0)
    acc = acc0.clone()
    cpu_ref.grad_fold(acc, grad, 1, 92)  # count -1: to the end
    assert torch.equal(acc[92:], torch.add(acc0[92:], g0[92:])) and torch.equal(acc[:92], acc0[:92])


@pytest.mark.parametrize("case", AH.refused_fold_arguments(), ids=lambda c: c[0])
def test_cpu_ref_grad_fold_refuses(case):
    _, acc, g, mode, off, cnt = case
    acc.fill_(1.0)
    g.fill_(2.0)
    with pytest.raises(ValueError):
        cpu_ref.grad_fold(acc, g, mode, off, cnt)
    assert bool((acc == 1).all()) and bool((g == 2).all())  # refused before anything was written


def test_cpu_ref_grad_fold_refuses_another_device():
    with pytest.raises(ValueError):
        cpu_ref.grad_fold(torch.zeros(8), torch.zeros(8, device="meta"), 0)


# ---------------------------------------------------------------- engine against the oracle
def _engine(**kw):
    e = VGGEngine("VGG11", "cpu", max_batch=4, lr=0.05, **kw)
    e.init_parameters(seed=3)
    return e


@pytest.mark.parametrize("opt", ["sgd", "lars"])
def test_accumulated_step_equals_oracle_bitwise(opt):
    """A = 3 (1/3 is not exact: a wrong scale cannot hide), two groups."""
    kw = AH.LARS if opt == "lars" else {}
    data = AH.batches(6, 4)
    groups = [data[:3], data[3:]]
    ref, e = _engine(**kw), _engine(**kw)
    sync = make_sync("ddp", e, NullComm())
    assert e.gacc is None
    for gi, group in enumerate(groups):
        AH.oracle_group(ref, group)
        AH.accumulated_groups(e, sync, [group], 3)
        assert e.steps_taken == ref.steps_taken == gi + 1
        AH.assert_same_state(AH.state(e), AH.state(ref), f"{opt} group {gi}")
        if opt == "lars":
            assert e.opt_stats() == ref.opt_stats()
    assert e.gacc is not None and ref.gacc is None
    assert int(e.nbt[0]) == 6  # BN statistics advanced on every micro-step


def test_accumulated_step_matches_torch():
    """Three backward() calls of loss / 3 into .grad, then one torch.optim.SGD step, on the reference
    module; the tolerance is test_engine_cpu's for its one-step comparison with autograd."""
    torch.manual_seed(1)
    m = VGG11().double()
    e = VGGEngine("VGG11", "cpu", max_batch=6, lr=0.01)
    e.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in m.state_dict().items()})
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    g = torch.Generator().manual_seed(0)
    group = []
    opt.zero_grad()
    for _ in range(3):
        x = torch.randn(6, 3, 32, 32, generator=g, dtype=torch.float64)
        t = torch.randint(0, 10, (6,), generator=g)
        (F.cross_entropy(m(x), t) / 3).backward()
        x4 = torch.zeros(6, 32, 32, 4)
        x4[..., :3] = x.float().permute(0, 2, 3, 1)
        group.append((x4, t))
    opt.step()
    AH.accumulated_groups(e, make_sync("allreduce", e, NullComm()), [group], 3)
    sd = e.state_dict()
    for k, v in m.state_dict().items():
        if v.is_floating_point():
            assert (sd[k].double() - v).abs().max().item() < 1e-4 * max(1.0, v.abs().max().item()), k
        else:
            assert int(sd[k]) == int(v) == 3


def test_short_group_of_one_is_an_ordinary_step():
    """5 batches with A = 2: groups of 2, 2 and 1; the last update (a = 1) is bitwise an ordinary step."""
    data = AH.batches(5, 4)
    ref, e = _engine(), _engine()
    sync = make_sync("ddp", e, NullComm())
    rsync = make_sync("ddp", ref, NullComm())
    AH.accumulated_groups(e, sync, [data[:2], data[2:4]], 2)
    AH.accumulated_groups(ref, rsync, [data[:2], data[2:4]], 2)
    step = AccumulatedStep(e, sync, 2)
    assert step.run(*data[4], last=True) is True and step.pos == 0
    rsync.begin_step()
    ref.forward_backward(*data[4], grad_ready=rsync.grad_ready, pre_forward=rsync.pre_forward,
                         params_free=rsync.params_free)
    rsync.update(rsync.finish())
    ref.finish_step()
    assert e.steps_taken == ref.steps_taken == 3
    AH.assert_same_state(AH.state(e), AH.state(ref), "short group")


def test_accum_steps_must_be_positive():
    e = _engine()
    with pytest.raises(ValueError):
        AccumulatedStep(e, make_sync("ddp", e, NullComm()), 0)


# ---------------------------------------------------------------- two gloo ranks, four modes
WORLD = 2
MODES = ("gather", "allreduce", "ddp", "zero1")


@pytest.fixture(scope="module")
def accum_mode_results(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("accum_modes"))
    out = {}
    for mode in MODES:
        mp.start_processes(AH.run_accum_mode, args=(WORLD, H.free_port(), mode, 2, 2, d), nprocs=WORLD, join=True,
                           start_method="spawn")
        out[mode] = [torch.load(os.path.join(d, f"accum_{mode}_{r}.pt"), weights_only=True) for r in range(WORLD)]
    return out


@pytest.mark.parametrize("mode", MODES)
def test_accum_replicas_identical(accum_mode_results, mode):
    r0, r1 = accum_mode_results[mode]
    assert r0["steps_taken"] == r1["steps_taken"] == 2
    assert torch.equal(r0["params"], r1["params"]), f"{mode}: parameters diverged across ranks"


def test_accum_modes_agree(accum_mode_results):
    a = accum_mode_results["gather"][0]["params"]
    for m in ("allreduce", "ddp", "zero1"):
        b = accum_mode_results[m][0]["params"]
        assert (a - b).abs().max().item() < 1e-5 * max(1.0, a.abs().max().item()), m
    for r in range(WORLD):
        la = accum_mode_results["gather"][r]["losses"]
        for m in ("allreduce", "ddp", "zero1"):
            lb = accum_mode_results[m][r]["losses"]
            assert all(abs(x - y) < 1e-4 for x, y in zip(la, lb))
    ref = accum_mode_results["ddp"][0]["mom"]
    for r in range(WORLD):  # zero1: prepare_checkpoint completes the sharded momentum
        m = accum_mode_results["zero1"][r]["mom"]
        assert (m - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item()), r


@pytest.mark.parametrize("mode", MODES)
def test_fold_only_micro_steps_touch_no_communicator(accum_mode_results, mode):
    """Zero communicator calls in the fold-only micro-steps; the closing micro-step of group i makes
    exactly the calls of the i-th ordinary step."""
    for r in range(WORLD):
        res = accum_mode_results[mode][r]
        assert res["micro"] == [[], []], (mode, r, res["micro"])
        assert len(res["closing"]) == 2 and all(len(c) > 0 for c in res["closing"])
        assert res["closing"] == res["ordinary"], (mode, r)


# ---------------------------------------------------------------- command line
def _ns(**kw):
    base = dict(accum_steps=1, checkpoint_every=0, stop_after_iters=None, graph=False)
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.mark.parametrize("kw", [dict(accum_steps=0), dict(accum_steps=-2), dict(accum_steps=2, checkpoint_every=3),
                                dict(accum_steps=4, stop_after_iters=6), dict(accum_steps=2, graph=True)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_validate_args_refuses(kw):
    with pytest.raises(ValueError):
        validate_args(_ns(**kw))


def test_validate_args_accepts():
    assert validate_args(_ns()) == 1
    assert validate_args(_ns(checkpoint_every=3, stop_after_iters=5, graph=True)) == 1  # A = 1: as before
    assert validate_args(_ns(accum_steps=2, checkpoint_every=4, stop_after_iters=6)) == 2
    assert validate_args(argparse.Namespace()) == 1


BASE = ["--device", "cpu", "--synthetic", "--batch-size", "8", "--test-size", "16", "--no-eval"]


@pytest.mark.parametrize("extra", [["--accum-steps", "0"], ["--accum-steps", "2", "--checkpoint-every", "3"],
                                   ["--accum-steps", "2", "--stop-after-iters", "3"],
                                   ["--accum-steps", "2", "--graph"]], ids=lambda e: " ".join(e))
def test_cli_refuses_before_touching_a_device(extra, monkeypatch):
    """The ValueError comes before the process context (and with it any device) is created."""
    from distributed_pytorch_amd import train

    def boom(*a, **kw):
        raise AssertionError("the device context was created before the arguments were checked")

    monkeypatch.setattr(train, "init_single", boom)
    with pytest.raises(ValueError):
        train.main_single(BASE + ["--train-size", "32"] + extra)


def test_schedule_counts_updates():
    assert updates_per_epoch(5, None, 2) == 3
    assert updates_per_epoch(5, 4, 2) == 2
    assert updates_per_epoch(5, 3, 2) == 2
    assert updates_per_epoch(6, None, 1) == 6


def _load(d):
    return torch.load(os.path.join(d, "rank0.pt"), weights_only=True)


def test_cli_schedule_length_and_metrics(tmp_path):
    """5 batches per epoch with A = 2: 3 updates per epoch, T = 6 over two epochs; the metrics lines
    carry accum_steps and effective_batch."""
    from distributed_pytorch_amd.train import main_single

    d, metrics = str(tmp_path / "ck"), str(tmp_path / "m.jsonl")
    main_single(BASE + ["--train-size", "40", "--epochs", "2", "--accum-steps", "2", "--lr-schedule", "cosine",
                        "--warmup-iters", "2", "--checkpoint-dir", d, "--json-metrics", metrics])
    ck = _load(d)
    want = lr_table(0.1, 6, warmup_iters=2, decay="cosine")
    assert ck["lr_schedule"] == want.spec and ck["steps_taken"] == 6 and ck["accum_steps"] == 2
    recs = [json.loads(l) for l in open(metrics).read().splitlines()]
    assert [(r["accum_steps"], r["effective_batch"]) for r in recs] == [(2, 16), (2, 16)]
    assert [r["lr"] for r in recs] == [float(want[2]), float(want[5])]


def test_cli_preempt_and_resume_is_bitwise_identical(tmp_path):
    """test_dist_cpu.test_preempt_and_resume_is_bitwise_identical with --accum-steps 2: stopped at a
    group boundary inside the second epoch and resumed == uninterrupted.  A resume under another A,
    or of a position inside a group of the running A, raises ResumeMismatch."""
    from distributed_pytorch_amd.train import main_single

    base = BASE + ["--train-size", "48", "--epochs", "2", "--accum-steps", "2"]  # 6 iterations per epoch
    a, b, c = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")
    main_single(base + ["--checkpoint-dir", a])
    main_single(base + ["--checkpoint-dir", b, "--stop-after-iters", "8"])
    mid = _load(b)
    assert (mid["epoch"], mid["batch_idx"], mid["steps_taken"], mid["accum_steps"]) == (1, 2, 4, 2)
    with pytest.raises(ResumeMismatch, match="accum-steps"):
        main_single(BASE + ["--train-size", "48", "--epochs", "2", "--checkpoint-dir", b, "--resume"])
    with pytest.raises(ResumeMismatch, match="accum-steps"):
        main_single(BASE + ["--train-size", "48", "--epochs", "2", "--accum-steps", "4", "--checkpoint-dir", b,
                            "--resume"])
    main_single(base + ["--checkpoint-dir", b, "--resume"])
    ca, cb = _load(a), _load(b)
    assert (ca["epoch"], ca["batch_idx"], ca["steps_taken"]) == (cb["epoch"], cb["batch_idx"], cb["steps_taken"]) \
        == (2, 0, 6)
    assert ca["model"].keys() == cb["model"].keys()
    for k in ca["model"]:
        assert torch.equal(ca["model"][k], cb["model"][k]), k
    for (ia, sa), (ib, sb) in zip(sorted(ca["optimizer"]["state"].items()), sorted(cb["optimizer"]["state"].items())):
        assert ia == ib and torch.equal(sa["momentum_buffer"], sb["momentum_buffer"]), ia
    # a checkpoint without the key (A = 1) standing at an odd batch, resumed under A = 2
    main_single(BASE + ["--train-size", "48", "--checkpoint-dir", c, "--stop-after-iters", "3"])
    assert "accum_steps" not in _load(c)
    with pytest.raises(ResumeMismatch):
        main_single(BASE + ["--train-size", "48", "--accum-steps", "2", "--checkpoint-dir", c, "--resume"])


def test_position_inside_a_group_is_refused(tmp_path):
    """A checkpoint of the running A whose batch position is no group boundary."""
    from distributed_pytorch_amd.utils import checkpoint

    e = _engine()
    checkpoint.save(str(tmp_path), 0, e, 0, 3, accum_steps=2)
    with pytest.raises(ResumeMismatch, match="inside a group"):
        checkpoint.load(str(tmp_path), 0, e, accum_steps=2)
    checkpoint.save(str(tmp_path), 0, e, 0, 4, accum_steps=2)
    assert checkpoint.load(str(tmp_path), 0, e, accum_steps=2)["batch_idx"] == 4


# ---------------------------------------------------------------- default path
def test_default_loop_is_the_eager_step(monkeypatch):
    """A = 1: the loop never allocates the accumulator and ends bitwise where _eager_step driven by
    hand ends."""
    from distributed_pytorch_amd import train
    from distributed_pytorch_amd.data import DeviceLoader, ShardSampler, get_datasets
    from distributed_pytorch_amd.parallel import init_single

    seen = []
    real = train.build_engine

    def spy(args, device):
        seen.append(real(args, device))
        return seen[-1]

    ap = argparse.ArgumentParser()
    train.add_common_args(ap)
    argv = BASE + ["--train-size", "32"]
    args = ap.parse_args(argv)
    assert args.accum_steps == 1
    with monkeypatch.context() as mpatch:
        mpatch.setattr(train, "build_engine", spy)
        train.main_single(argv)
    e = seen[0]
    assert e.gacc is None and e.steps_taken == 4

    torch.manual_seed(args.seed)
    train_set, _ = get_datasets(args.data_root, True, 32, 16)
    ctx = init_single("cpu")
    sampler = ShardSampler(len(train_set), num_replicas=1, rank=0, shuffle=True, seed=args.sampler_seed,
                           drop_last=False)
    loader = DeviceLoader(train_set, 8, ctx.device, sampler=sampler, train=True, seed=args.seed * 7919)
    ref = train.build_engine(args, ctx.device)
    ref.init_parameters(seed=args.seed)
    sync = make_sync("allreduce", ref, ctx.comm)
    loader.set_epoch(0)
    ref.loss_accum.zero_()
    for x, t in loader.iterate(0):
        train._eager_step(ref, sync, x, t)
    assert ref.gacc is None
    AH.assert_same_state(AH.state(e), AH.state(ref), "default loop")
