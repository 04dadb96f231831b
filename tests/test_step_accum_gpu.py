"""Gradient accumulation on the GPU: the fold kernel bitwise against torch.add, the accumulated step
bitwise against the engine oracle (tests/accum_helpers.py) for every conv implementation, under a
schedule, on a 1-rank RCCL communicator, and with two processes sharing the GPU in all four sync
modes."""
import os

import pytest
import torch

import accum_helpers as AH

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "accum_gpu_worker.py")


def _C():
    from distributed_pytorch_amd import _ext

    return _ext.require()


# ---------------------------------------------------------------- the fold kernel
def _special(n, seed):
    """n fp32 values: randn with +-0, denormals, +-inf and extremes sprinkled in."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g)
    sp = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, float("inf"), float("-inf"), 3.4e38, -3.4e38,
                       1.17549435e-38, -1.17549435e-38])
    idx = torch.randperm(n, generator=g)[: min(n, 4 * sp.numel())]
    v[idx] = sp.repeat(4)[: idx.numel()]
    return v


def _bits(t):
    return t.view(torch.int32)


def _check_fold(C, n, offset=0, count=-1, seed=0):
    acc0, g0 = _special(n, seed).cuda(), _special(n, seed + 1).cuda()
    if n >= 8:  # the same special values meeting each other: -0 + -0, +0 + -0, denormal + denormal, inf + inf
        g0[: n // 2] = acc0[: n // 2].flip(0)
    hi = n if count < 0 else offset + count
    for mode in (0, 1, 2):
        acc, g = acc0.clone(), g0.clone()
        C.grad_fold(acc, g, mode, offset, count)
        want_acc, want_g = acc0.clone(), g0.clone()
        if mode == 0:
            want_acc[offset:hi] = g0[offset:hi]
        elif mode == 1:
            want_acc[offset:hi] = torch.add(acc0[offset:hi], g0[offset:hi])
        else:
            want_g[offset:hi] = torch.add(acc0[offset:hi], g0[offset:hi])
        torch.cuda.synchronize()
        # bit patterns (NaN from inf - inf compares equal to itself this way; -0 differs from +0)
        assert torch.equal(_bits(acc), _bits(want_acc)), (n, mode, "acc")
        assert torch.equal(_bits(g), _bits(want_g)), (n, mode, "g")


@pytest.mark.parametrize("n", [4, 260, 4096 * 256 * 4 + 4], ids=["n4", "n260", "past_grid_cap"])
def test_grad_fold_bitwise(n):
    """n = 260: not a multiple of the block; n = 4096 * 256 * 4 + 4: one float4 more than the capped
    grid covers in one pass, so the grid-stride loop runs twice for one thread."""
    _check_fold(_C(), n, seed=n % 97)


def test_grad_fold_slice_leaves_the_rest():
    """offset = 64, count = 4 * 257 inside a larger tensor: the elements outside stay bit for bit."""
    _check_fold(_C(), 4096, offset=64, count=4 * 257, seed=3)


def test_grad_fold_adds_special_values_like_torch():
    C = _C()
    a = torch.tensor([0.0, -0.0, -0.0, 1e-45, 1e-39, float("inf"), float("-inf"), 1.17549435e-38], device="cuda")
    b = torch.tensor([-0.0, -0.0, 0.0, 1e-45, -3e-39, float("inf"), 1.0, -1e-45], device="cuda")
    acc = a.clone()
    C.grad_fold(acc, b, 1)
    want = torch.add(a, b)
    assert torch.equal(_bits(acc), _bits(want))
    assert _bits(acc)[1].item() == -2 ** 31 and _bits(acc)[0].item() == 0  # -0 + -0 = -0 ; +0 + -0 = +0
    assert acc[3].item() != 0.0  # denormals are not flushed


def test_grad_fold_refuses_before_launch():
    C = _C()
    for name, acc, g, mode, off, cnt in AH.refused_fold_arguments("cuda"):
        acc.fill_(1.0)
        g.fill_(2.0)
        with pytest.raises(ValueError):
            C.grad_fold(acc, g, mode, off, cnt)
        torch.cuda.synchronize()
        assert bool((acc == 1).all()) and bool((g == 2).all()), name
    with pytest.raises(ValueError):  # different devices
        C.grad_fold(torch.zeros(8, device="cuda"), torch.zeros(8), 0)
    with pytest.raises(ValueError):
        C.grad_fold(torch.zeros(8), torch.zeros(8), 0)


# ---------------------------------------------------------------- engine against the oracle
def _engine(impl, **kw):
    from distributed_pytorch_amd.engine import VGGEngine

    e = VGGEngine("VGG11", "cuda", max_batch=8, impl=impl, lr=0.05, **kw)
    e.init_parameters(seed=3)
    return e


def _oracle_case(impl, opt, mix=False, **kw):
    """A = 3, two groups at batch 8: the accumulated path against the oracle, bitwise, after each."""
    from distributed_pytorch_amd.parallel import NullComm, make_sync

    okw = dict(AH.LARS) if opt == "lars" else {}
    okw.update(kw)
    data = AH.batches(6, 8, "cuda", seed=13)
    ref, e = _engine(impl, **okw), _engine(impl, **okw)
    if mix:
        g = torch.Generator().manual_seed(2)
        t2 = torch.randint(0, 10, (8,), generator=g).cuda()
        lam = torch.full((8,), 0.3, device="cuda")
        ref.set_mix(t2, lam)
        e.set_mix(t2, lam)
    sync = make_sync("ddp", e, NullComm())
    for gi, group in enumerate((data[:3], data[3:])):
        AH.oracle_group(ref, group)
        AH.accumulated_groups(e, sync, [group], 3)
        torch.cuda.synchronize()
        assert e.steps_taken == ref.steps_taken == gi + 1
        AH.assert_same_state(AH.state(e), AH.state(ref), f"{impl} {opt} group {gi}")
        if opt == "lars":
            assert e.opt_stats() == ref.opt_stats()
    e.check_signals()
    ref.check_signals()
    assert e.gacc is not None and ref.gacc is None
    return e


@pytest.mark.parametrize("opt", ["sgd", "lars"])
@pytest.mark.parametrize("impl", ["fp32", "h2", "x3", "bf16"])
def test_accumulated_step_equals_oracle_bitwise(impl, opt):
    e = _oracle_case(impl, opt)
    assert (e.wstream is not None) == (os.environ.get("DPA_WGRAD_STREAM", "1") == "1")


def test_accumulated_step_equals_oracle_on_one_stream(monkeypatch):
    """DPA_WGRAD_STREAM=0: one stream, no signals -- every fold is on the main stream."""
    monkeypatch.setenv("DPA_WGRAD_STREAM", "0")
    e = _oracle_case("h2", "sgd")
    assert e.wstream is None and not e.ksignal


def test_accumulated_step_equals_oracle_with_mixup_and_smoothing():
    _oracle_case("h2", "sgd", mix=True, label_smoothing=0.1)


def test_scheduled_accumulated_run_follows_the_table():
    """Warmup + cosine over 4 updates, A = 2: after every update the scheduled run equals, bitwise, the
    unscheduled accumulated run whose lr was set to float(table[t]) by hand before the group."""
    from distributed_pytorch_amd.accum import AccumulatedStep
    from distributed_pytorch_amd.parallel import NullComm, make_sync
    from distributed_pytorch_amd.schedule import lr_table

    tab = lr_table(0.05, 4, warmup_iters=2, decay="cosine", end_lr=1e-3)
    assert len({float(v) for v in tab}) == 4
    data = AH.batches(8, 8, "cuda", seed=29)
    sch, ref = _engine("h2"), _engine("h2")
    sch.set_lr_schedule(tab)
    ssync, rsync = make_sync("ddp", sch, NullComm()), make_sync("ddp", ref, NullComm())
    sstep, rstep = AccumulatedStep(sch, ssync, 2), AccumulatedStep(ref, rsync, 2)
    for t in range(4):
        ref.lr = float(tab[t])
        for x, y in data[2 * t:2 * t + 2]:
            sstep.run(x, y)
            rstep.run(x, y)
        torch.cuda.synchronize()
        assert sch.steps_taken == t + 1 and sch.current_lr() == float(tab[t]) and sch.lr_position() == t + 1
        AH.assert_same_state(AH.state(sch), AH.state(ref), f"update {t}")
    sch.check_signals()


# ---------------------------------------------------------------- communicators, child processes
def _launch(kind, outdir, nprocs, env=None):
    from distributed_pytorch_amd.parallel import spawn

    rc = spawn.launch(WORKER, [kind, outdir], nprocs, timeout_s=100, extra_env=env or {})
    assert rc == 0, f"{kind}: ranks exited with {rc}"


def _load(outdir, label, rank):
    return torch.load(os.path.join(outdir, f"{label}_{rank}.pt"), weights_only=True)


KEYS = ("params", "mom", "buffers", "wplanes")


def test_one_rank_rccl_ddp_equals_nullcomm(tmp_path):
    """A 1-rank RCCL communicator in DDP mode: the merge rides in front of every bucket's all-reduce
    (comm stream, and the main stream for the tail bucket); bitwise the NullComm path after two groups."""
    d = str(tmp_path)
    _launch("rccl1", d, 1, {"DPA_FORCE_COMM": "1", "DPA_COMM_TIMEOUT": "60"})
    a, b = _load(d, "null", 0), _load(d, "rccl1", 0)
    assert a["comm"] == "null" and b["comm"] != "null"
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert a["losses"] == b["losses"]


def test_two_processes_share_the_gpu_all_modes(tmp_path):
    """Two ranks on one GPU through gloo (host staging), A = 2, two groups: replicas bitwise identical
    in every mode and every mode bitwise every other (a sum of two and its scaling by powers of two
    are exact in any order)."""
    d = str(tmp_path)
    _launch("gloo", d, 2)
    modes = ("gather", "allreduce", "ddp", "zero1")
    out = {m: [_load(d, m, r) for r in range(2)] for m in modes}
    for m in modes:
        assert out[m][0]["world"] == 2
        assert torch.equal(out[m][0]["params"], out[m][1]["params"]), f"{m}: replicas differ"
        assert torch.equal(out[m][0]["wplanes"], out[m][1]["wplanes"]), f"{m}: replicas' weight planes differ"
    for m in modes[1:]:
        for k in ("params", "mom", "wplanes"):
            assert torch.equal(out[m][0][k], out["gather"][0][k]), (m, k)
