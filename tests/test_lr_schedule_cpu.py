"""Learning-rate schedules on the host: the float32 table of schedule.lr_table against torch's
schedulers, its composition and edge cases, the CPU engine following a table bit for bit like an
engine whose constant rate is set by hand before every step, and preempt / resume of a scheduled
run through the command line (with the checkpoint's schedule check)."""
import math
import os

import numpy as np
import pytest
import torch

from distributed_pytorch_amd.schedule import lr_at, lr_table

BASE, T = 0.4, 37


def _torch_rates(make, n=T):
    """The rate torch's scheduler gives every iteration 0 .. n-1 (stepped once per iteration)."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=BASE)
    sched = make(opt)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    return out


CASES = {
    "warmup": (dict(warmup_iters=5, warmup_factor=0.1),
               lambda o: torch.optim.lr_scheduler.LinearLR(o, start_factor=0.1, total_iters=5)),
    "poly": (dict(decay="poly", power=2.0),
             lambda o: torch.optim.lr_scheduler.PolynomialLR(o, total_iters=T, power=2.0)),
    "cosine": (dict(decay="cosine", end_lr=1e-3),
               lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=T, eta_min=1e-3)),
    "step": (dict(decay="step", milestones=(10, 20, 30), gamma=0.1),
             lambda o: torch.optim.lr_scheduler.MultiStepLR(o, milestones=[10, 20, 30], gamma=0.1)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_table_matches_torch_scheduler(name):
    """|table[t] - torch[t]| <= 2^-23 * base: one float32 ulp at base (the table's single rounding
    costs at most half of it, torch's fp64 recursion far less)."""
    kw, make = CASES[name]
    tab = lr_table(BASE, T, **kw)
    ref = _torch_rates(make)
    assert tab.dtype == np.float32 and tab.shape == (T,)
    err = max(abs(float(tab[t]) - ref[t]) for t in range(T))
    print(f"{name}: max |table - torch| = {err / BASE:.3e} x base (bound {2.0 ** -23:.3e})")
    assert err <= 2.0 ** -23 * BASE
    assert len({float(v) for v in tab}) > 1  # the schedule really moves


def test_warmup_composes_with_decay():
    """The decay after a warmup of W steps is the decay without warmup over T - W steps, bitwise;
    the warmup part is the warmup-only table's."""
    full = lr_table(BASE, T, warmup_iters=5, decay="cosine", end_lr=1e-3)
    tail = lr_table(BASE, T - 5, decay="cosine", end_lr=1e-3)
    assert np.array_equal(np.asarray(full[5:]), np.asarray(tail))
    assert np.array_equal(np.asarray(full[:5]), np.asarray(lr_table(BASE, T, warmup_iters=5)[:5]))
    assert float(full[0]) == float(np.float32(BASE * 0.1)) and float(full[5]) == float(np.float32(BASE))


def test_table_holds_last_value_and_carries_spec():
    tab = lr_table(BASE, 5, decay="poly", power=1.0, end_lr=0.01)
    assert [lr_at(tab, t) for t in (4, 5, 100)] == [float(tab[4])] * 3
    assert lr_at(tab, 0) == float(np.float32(BASE))
    s = tab.spec
    assert s == {"base_lr": BASE, "total_iters": 5, "warmup_iters": 0, "warmup_factor": 0.1, "decay": "poly",
                 "power": 1.0, "end_lr": 0.01, "milestones": [], "gamma": 0.1}
    for v in s.values():  # plain values only: what a checkpoint / a JSON line can hold
        assert type(v) in (int, float, str, list)
    # poly with power 1 ends one step above end_lr; the closed form at the last step
    assert abs(float(tab[4]) - (0.01 + (BASE - 0.01) * (1 - 4 / 5))) <= 2.0 ** -24 * BASE
    assert math.isclose(float(lr_table(BASE, 3)[2]), BASE, rel_tol=1e-7)


@pytest.mark.parametrize("kw", [
    dict(total_iters=0),
    dict(warmup_iters=-1),
    dict(warmup_iters=T, decay="cosine"),
    dict(warmup_iters=T + 3, decay="poly"),
    dict(warmup_factor=0.0),
    dict(warmup_factor=1.5),
    dict(decay="exponential"),
    dict(decay="step", gamma=0.0),
    dict(decay="step", gamma=-0.5),
    dict(decay="poly", end_lr=-1e-3),
    dict(decay="step", milestones=(20, 10)),
])
def test_invalid_arguments_raise(kw):
    args = dict(base_lr=BASE, total_iters=T)
    args.update(kw)
    with pytest.raises(ValueError):
        lr_table(**args)


def test_warmup_longer_than_run_is_allowed_for_constant():
    tab = lr_table(BASE, 4, warmup_iters=10)
    assert float(tab[3]) == float(np.float32(BASE * (0.1 + 0.9 * 3 / 10)))


def _batches(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        x = torch.zeros(8, 32, 32, 4)
        x[..., :3] = torch.randn(8, 32, 32, 3, generator=g)
        out.append((x, torch.randint(0, 10, (8,), generator=g)))
    return out


def test_cpu_engine_follows_table_bitwise():
    """Six steps under a warmup + poly table == six steps of today's constant-rate path with
    engine.lr set to float(table[t]) before each step: parameters, momentum and losses, bitwise."""
    from distributed_pytorch_amd.engine import VGGEngine

    tab = lr_table(0.1, 6, warmup_iters=2, warmup_factor=0.1, decay="poly", power=2.0)
    assert len({float(v) for v in tab}) == 6
    batches = _batches(6)
    outs = []
    for scheduled in (True, False):
        e = VGGEngine("VGG11", "cpu", max_batch=8)
        e.init_parameters(seed=3)
        if scheduled:
            e.set_lr_schedule(tab)
            assert e.lr_spec == tab.spec and e.current_lr() == float(tab[0])
        else:
            assert e.lr_spec is None and e.current_lr() == e.lr
        losses = []
        for t, (x, y) in enumerate(batches):
            if not scheduled:
                e.lr = float(tab[t])
            e.forward_backward(x, y)
            e.sgd_step()
            e.finish_step()
            losses.append(e.loss.clone())
            if scheduled:
                assert e.current_lr() == float(tab[t]) and e.lr_position() == t + 1
        outs.append((e.params.flat.clone(), e.mom.flat.clone(), torch.stack(losses)))
        if scheduled:
            assert e.optimizer_state_dict()["param_groups"][0]["lr"] == 0.1  # the base rate
            e.set_lr_schedule(None)
            assert e.lr_spec is None and e.current_lr() == e.lr
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _load(d):
    return torch.load(os.path.join(d, "rank0.pt"), weights_only=True)


def test_cli_preempt_and_resume_with_schedule_is_bitwise_identical(tmp_path):
    """test_dist_cpu.test_preempt_and_resume_is_bitwise_identical, one process on the CPU, under
    --warmup-iters 6 --lr-schedule cosine: preempted at iteration 4 (inside the warmup) and resumed
    == uninterrupted.  A resume under another schedule, or of a schedule-less checkpoint under a
    schedule (and the reverse), raises ResumeMismatch."""
    from distributed_pytorch_amd.train import main_single
    from distributed_pytorch_amd.utils.checkpoint import ResumeMismatch

    base = ["--device", "cpu", "--synthetic", "--batch-size", "8", "--train-size", "48", "--test-size", "16",
            "--epochs", "2", "--no-eval"]  # 6 iterations per epoch: T = 12
    sched = ["--warmup-iters", "6", "--lr-schedule", "cosine"]
    a, b, c = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")
    metrics = str(tmp_path / "m.jsonl")
    main_single(base + sched + ["--checkpoint-dir", a, "--json-metrics", metrics])
    main_single(base + sched + ["--checkpoint-dir", b, "--stop-after-iters", "4"])
    mid = _load(b)
    assert (mid["epoch"], mid["batch_idx"], mid["steps_taken"]) == (0, 4, 4)
    want = lr_table(0.1, 12, warmup_iters=6, decay="cosine")
    assert mid["lr_schedule"] == want.spec
    assert mid["optimizer"]["param_groups"][0]["lr"] == 0.1
    with pytest.raises(ResumeMismatch, match="schedule"):
        main_single(base + ["--warmup-iters", "6", "--lr-schedule", "poly", "--checkpoint-dir", b, "--resume"])
    with pytest.raises(ResumeMismatch, match="schedule"):
        main_single(base + ["--checkpoint-dir", b, "--resume"])
    main_single(base + sched + ["--checkpoint-dir", b, "--resume"])
    ca, cb = _load(a), _load(b)
    assert (ca["epoch"], ca["batch_idx"], ca["steps_taken"]) == (cb["epoch"], cb["batch_idx"], cb["steps_taken"]) \
        == (2, 0, 12)
    assert ca["model"].keys() == cb["model"].keys()
    for k in ca["model"]:
        assert torch.equal(ca["model"][k], cb["model"][k]), k
    for (ia, sa), (ib, sb) in zip(sorted(ca["optimizer"]["state"].items()), sorted(cb["optimizer"]["state"].items())):
        assert ia == ib and torch.equal(sa["momentum_buffer"], sb["momentum_buffer"]), ia
    # the metrics lines carry the rate of each epoch's last step and the spec
    import json

    recs = [json.loads(l) for l in open(metrics).read().splitlines()]
    assert [r["lr"] for r in recs] == [float(want[5]), float(want[11])]
    assert recs[0]["lr_schedule"] == want.spec
    # a schedule-less checkpoint resumed under a schedule
    main_single(base + ["--checkpoint-dir", c, "--stop-after-iters", "2"])
    assert "lr_schedule" not in _load(c)
    with pytest.raises(ResumeMismatch, match="schedule"):
        main_single(base + sched + ["--checkpoint-dir", c, "--resume"])
