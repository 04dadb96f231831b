"""Learning-rate schedules on the GPU (kernels/lr_sched.hip and the device-rate instances of the
update kernels in sgd.hip / lars.hip).  Every new path is pinned bitwise against a path the project
already has: lr_advance against the host's table, sgd_flat / sgd_segmented given the rate as a
device word against the same calls given the same float32 rate as a float, and the scheduled engine
(eager, captured, resumed into a capture, per-bucket update placement) against an engine whose
constant rate is set to float(table[t]) by hand before every step."""
import pytest
import torch

from distributed_pytorch_amd.schedule import lr_table

pytestmark = pytest.mark.gpu


def _C():
    from distributed_pytorch_amd import _ext

    return _ext.require()


def _dev(a):
    return torch.from_numpy(a.copy()).cuda()


# ------------------------------------------------------------------ lr_advance
def test_lr_advance_host_positions():
    """Table of 5, host positions 0..7: lr_dev is bitwise table[min(pos, 4)], step_dev == pos + 1
    (whatever the counter held before)."""
    tab = lr_table(0.3, 5, warmup_iters=2, decay="cosine", end_lr=0.01)
    assert len({float(v) for v in tab}) == 5
    td = _dev(tab)
    step = torch.full((1,), 99, dtype=torch.int64, device="cuda")
    lr = torch.zeros(1, device="cuda")
    for pos in range(8):
        _C().lr_advance(td, step, lr, pos, False)
        assert lr.item() == float(tab[min(pos, 4)]), pos
        assert step.item() == pos + 1
    assert torch.equal(td.cpu(), torch.from_numpy(tab.copy()))  # the table is read only


def test_lr_advance_device_counter():
    """Device-driven from step_dev = 3: table[3], table[4], table[4]; the counter ends at 6 and the
    host position argument is ignored."""
    tab = lr_table(0.3, 5, decay="poly", power=2.0, end_lr=0.01)
    td = _dev(tab)
    step = torch.full((1,), 3, dtype=torch.int64, device="cuda")
    lr = torch.zeros(1, device="cuda")
    got = []
    for _ in range(3):
        _C().lr_advance(td, step, lr, 0, True)
        got.append(lr.item())
    assert got == [float(tab[3]), float(tab[4]), float(tab[4])]
    assert step.item() == 6


def test_bindings_check_arguments():
    C_ = _C()
    td = _dev(lr_table(0.1, 4))
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    lr = torch.zeros(1, device="cuda")
    with pytest.raises(RuntimeError):
        C_.lr_advance(td.cpu(), step, lr, 0, False)  # CPU table
    with pytest.raises(RuntimeError):
        C_.lr_advance(td[:0], step, lr, 0, False)  # T >= 1
    with pytest.raises(RuntimeError):
        C_.lr_advance(td.double(), step, lr, 0, False)  # dtype
    with pytest.raises(RuntimeError):
        C_.lr_advance(td, step.int(), lr, 0, False)  # counter dtype
    with pytest.raises(RuntimeError):
        C_.lr_advance(td, step, torch.zeros(2, device="cuda"), 0, False)  # one word
    with pytest.raises(RuntimeError):
        C_.lr_advance(td[::2], step, lr, 0, False)  # not contiguous
    with pytest.raises(RuntimeError):
        C_.lr_advance(td, step, lr, -1, False)
    p = torch.zeros(64, device="cuda")
    with pytest.raises(RuntimeError):
        C_.sgd_flat(p, p.clone(), p.clone(), lr.cpu(), 0.9, 1e-4, 1.0, False)  # CPU rate
    with pytest.raises(RuntimeError):
        C_.sgd_flat(p, p.clone(), p.clone(), lr.double(), 0.9, 1e-4, 1.0, False)
    for rate in (lr, 0.1):
        with pytest.raises(RuntimeError):
            C_.sgd_flat(p, p.clone(), p.clone(), rate, 0.9, 1e-4, 1.0, False, 32, 64)  # slice past the end
        with pytest.raises(RuntimeError):
            C_.sgd_flat(p, p.clone(), p.clone(), rate, 0.9, 1e-4, 1.0, False, 2, 4)  # unaligned slice
    torch.cuda.synchronize()


def test_sgd_flat_rejects_negative_offset():
    """offset = -4, count = 8 satisfies the alignment and upper-bound checks; it is refused before
    any launch, with a float rate and with a device rate.  p, g, buf are the views base[64:128], so
    that a build without the check would write inside a live allocation."""
    C_ = _C()
    lr = torch.full((1,), 0.1, device="cuda")
    bases = [torch.ones(128, device="cuda") for _ in range(3)]
    p, g, buf = (b[64:128] for b in bases)
    for rate in (0.1, lr):
        with pytest.raises(RuntimeError, match="offset"):
            C_.sgd_flat(p, g, buf, rate, 0.9, 1e-4, 1.0, False, -4, 8)
    assert all(bool((b == 1).all()) for b in bases)


# ------------------------------------------------------------------ update kernels
RATE = float(lr_table(0.37, 9, warmup_iters=3, decay="cosine")[5])  # an inexact float32 rate


def _planes(np_, n):
    if np_ == 0:
        return None
    return torch.zeros(np_, n, device="cuda", dtype=torch.float16 if np_ == 2 else torch.bfloat16)


def _arena(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=g) * s).cuda() for s in (0.1, 0.01, 0.05)]  # p, g, buf


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("np_", [0, 1, 3, 2])
@pytest.mark.parametrize("n,offset,count", [(64, 0, -1), (4160, 0, -1), (4160, 64, 128)])
def test_sgd_flat_dlr_same_bits_as_sgd_flat(n, offset, count, np_, first):
    """The same float32 rate once from device memory and once as the argument: p, buf and the
    planes are bitwise equal; outside an [offset, offset + count) slice nothing is written."""
    C_ = _C()
    p, g, buf = _arena(n, 31)
    pa, ba, pb, bb = p.clone(), buf.clone(), p.clone(), buf.clone()
    pla, plb = _planes(np_, n), _planes(np_, n)
    lr = torch.tensor([RATE], device="cuda")
    assert lr.item() == RATE
    C_.sgd_flat(pa, g, ba, RATE, 0.9, 1e-4, 0.5, first, offset, count, pla)
    C_.sgd_flat(pb, g, bb, lr, 0.9, 1e-4, 0.5, first, offset, count, plb)
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(ba, bb)
    hi = n if count < 0 else offset + count
    assert not torch.equal(pb[offset:hi], p[offset:hi])
    assert torch.equal(pb[:offset], p[:offset]) and torch.equal(pb[hi:], p[hi:])
    assert torch.equal(bb[:offset], buf[:offset]) and torch.equal(bb[hi:], buf[hi:])
    if np_:
        assert torch.equal(pla, plb)
        assert plb[:, offset:hi].float().abs().sum().item() > 0
        assert plb[:, :offset].float().abs().sum().item() == 0 and plb[:, hi:].float().abs().sum().item() == 0
        C_.h2_overflow(True)
    assert lr.item() == RATE  # read only


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("np_", [0, 1, 3, 2])
def test_sgd_segmented_dlr_same_bits_as_sgd_segmented(np_, first):
    """Two segments of 64 + 8256 elements (the second spans two chunks) with a non-trivial ratio
    table: the device-rate instance gives the bits of the float-rate one."""
    from distributed_pytorch_amd.utils.arena import block_map

    C_ = _C()
    n = 64 + 8256
    bmap, segs = block_map([(0, 64, 1), (64, 8256, 2)], int(C_.OPT_CHUNK), True, "cuda")
    assert bmap.shape[0] == 3 and segs[1, 1].item() == 2
    table = torch.tensor([0.7, 1.3, 0.45], device="cuda")  # r_0, r_1, gmul
    p, g, buf = _arena(n, 32)
    pa, ba, pb, bb = p.clone(), buf.clone(), p.clone(), buf.clone()
    pla, plb = _planes(np_, n), _planes(np_, n)
    lr = torch.tensor([RATE], device="cuda")
    C_.sgd_segmented(pa, g, ba, bmap, table, RATE, 0.9, 1e-4, first, pla)
    C_.sgd_segmented(pb, g, bb, bmap, table, lr, 0.9, 1e-4, first, plb)
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(ba, bb)
    assert not torch.equal(pb[:64], p[:64]) and not torch.equal(pb[8192 + 64:], p[8192 + 64:])
    if np_:
        assert torch.equal(pla, plb) and plb.float().abs().sum().item() > 0
        C_.h2_overflow(True)


# ------------------------------------------------------------------ engine
def _batches(n, batch, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        x = torch.zeros(batch, 32, 32, 4)
        x[..., :3] = torch.randn(batch, 32, 32, 3, generator=g)
        out.append((x.cuda(), torch.randint(0, 10, (batch,), generator=g).cuda()))
    return out


def _result(e, losses):
    torch.cuda.synchronize()
    e.check_signals()
    return e.params.flat.clone(), e.mom.flat.clone(), torch.stack(losses)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _run_eager(tab, batches, scheduled, **kw):
    from distributed_pytorch_amd.engine import VGGEngine

    e = VGGEngine("VGG11", "cuda", max_batch=8, impl="fp32", **kw)
    e.init_parameters(seed=5)
    if scheduled:
        e.set_lr_schedule(tab)
    losses = []
    for t, (x, y) in enumerate(batches):
        if not scheduled:
            e.lr = float(tab[t])
        e.forward_backward(x, y)
        e.sgd_step()
        e.finish_step()
        losses.append(e.loss.clone())
        if scheduled and t in (0, len(batches) - 1):
            assert e.current_lr() == float(tab[t]) and e.lr_position() == t + 1
    return _result(e, losses)


@pytest.mark.parametrize("opt", [{}, {"optimizer": "lars", "clip_grad_norm": 1.0}], ids=["sgd", "lars_clip"])
def test_engine_eager_follows_table(opt):
    """Warmup + cosine over 5 steps at batch 8: bitwise the engine given engine.lr = float(table[t])
    before each step (today's constant-rate kernels), and bitwise repeatable."""
    tab = lr_table(0.05, 5, warmup_iters=2, decay="cosine", end_lr=1e-3)
    assert len({float(v) for v in tab}) == 5
    batches = _batches(5, 8, 41)
    a = _run_eager(tab, batches, True, **opt)
    b = _run_eager(tab, batches, True, **opt)
    ref = _run_eager(tab, batches, False, **opt)
    assert _same(a, b), "scheduled runs differ from each other"
    assert _same(a, ref), "scheduled run differs from the hand-set constant-rate run"


def test_engine_without_schedule_has_no_schedule_state():
    """No schedule: the words lr_advance would write do not exist, before and after a step, and
    again after a schedule was set and cleared."""
    from distributed_pytorch_amd.engine import VGGEngine

    e = VGGEngine("VGG11", "cuda", max_batch=8, impl="fp32")
    (x, y), = _batches(1, 8, 42)
    for _ in range(2):
        assert not hasattr(e, "step_dev") and not hasattr(e, "lr_dev") and e.lr_spec is None
        assert e.current_lr() == e.lr
        with pytest.raises(ValueError):
            e.lr_position()
        e.forward_backward(x, y)
        e.sgd_step()
        e.finish_step()
        assert not hasattr(e, "step_dev") and not hasattr(e, "lr_dev")
        e.set_lr_schedule(lr_table(0.1, 3))
        assert e.step_dev.dtype == torch.int64 and e.lr_dev.dtype == torch.float32
        e.set_lr_schedule(None)
    torch.cuda.synchronize()


def _sync_step(e, sync, xb, tb):
    sync.begin_step()
    e.forward_backward(xb, tb, grad_ready=sync.grad_ready, pre_forward=sync.pre_forward, params_free=sync.params_free)
    sync.update(sync.finish())
    e.finish_step()


def _cpu_batches(n, batch, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(batch, 32, 32, 4, generator=g), torch.randint(0, 10, (batch,), generator=g))
            for _ in range(n)]


def _fill(xb, tb, x, t):
    xb.copy_(x)
    xb[..., 3] = 0
    tb.copy_(t)


def test_graphed_step_follows_table():
    """The shape of test_label_smoothing_gpu.test_graphed_step_smoothed_matches_eager (batch 64, x3)
    under a table whose six values all differ: 2 eager steps + 4 replays == 6 eager steps, bitwise;
    afterwards the device counter is 6 and the rate table[5].  A build that bakes the rate into the
    graph replays table[2] four times and fails here."""
    from distributed_pytorch_amd.engine import VGGEngine
    from distributed_pytorch_amd.graph_step import GraphedStep
    from distributed_pytorch_amd.parallel import NullComm, make_sync

    tab = lr_table(0.02, 6, warmup_iters=2, decay="poly", power=2.0, end_lr=1e-3)
    assert len({float(v) for v in tab}) == 6
    batches = _cpu_batches(6, 64, 21)
    outs = []
    for graph in (False, True):
        e = VGGEngine("VGG11", "cuda", max_batch=64, impl="x3", lr=0.02)
        e.init_parameters(seed=4)
        e.set_lr_schedule(tab)
        sync = make_sync("ddp", e, NullComm())
        gs = GraphedStep(e, sync, warmup=2) if graph else None
        xb = torch.empty(64, 32, 32, 4, device="cuda")
        tb = torch.empty(64, dtype=torch.int64, device="cuda")
        losses = []
        for x, t in batches:
            _fill(xb, tb, x, t)
            if gs is not None:
                gs.run(xb, tb)
            else:
                _sync_step(e, sync, xb, tb)
            losses.append(e.loss.clone())
        torch.cuda.synchronize()
        if gs is not None:
            assert gs.replays == 4 and gs.graph is not None
        assert e.lr_position() == 6 and e.current_lr() == float(tab[5])
        outs.append(_result(e, losses))
    assert _same(outs[0], outs[1])


def test_graphed_step_captures_on_first_step_after_resume():
    """A run resumed at step 3 (state loaded, steps_taken = 3) under GraphedStep(warmup=2) captures
    on its first run, with the device counter seeded from the host's count: three graphed steps ==
    the eager continuation, bitwise."""
    from distributed_pytorch_amd.engine import VGGEngine
    from distributed_pytorch_amd.graph_step import GraphedStep
    from distributed_pytorch_amd.parallel import NullComm, make_sync

    tab = lr_table(0.02, 6, warmup_iters=2, decay="cosine", end_lr=1e-3)
    assert len({float(v) for v in tab}) == 6
    batches = _cpu_batches(6, 64, 22)
    xb = torch.empty(64, 32, 32, 4, device="cuda")
    tb = torch.empty(64, dtype=torch.int64, device="cuda")
    e = VGGEngine("VGG11", "cuda", max_batch=64, impl="x3", lr=0.02)
    e.init_parameters(seed=4)
    e.set_lr_schedule(tab)
    sync = make_sync("ddp", e, NullComm())
    for x, t in batches[:3]:
        _fill(xb, tb, x, t)
        _sync_step(e, sync, xb, tb)
    torch.cuda.synchronize()
    sd, osd = e.state_dict(), e.optimizer_state_dict()
    losses = []
    for x, t in batches[3:]:
        _fill(xb, tb, x, t)
        _sync_step(e, sync, xb, tb)
        losses.append(e.loss.clone())
    ref = _result(e, losses)

    r = VGGEngine("VGG11", "cuda", max_batch=64, impl="x3", lr=0.02)
    r.set_lr_schedule(tab)
    r.load_state_dict(sd)
    r.load_optimizer_state_dict(osd)
    r.steps_taken = 3
    gs = GraphedStep(r, make_sync("ddp", r, NullComm()), warmup=2)
    losses = []
    for x, t in batches[3:]:
        _fill(xb, tb, x, t)
        gs.run(xb, tb)
        losses.append(r.loss.clone())
    assert gs.replays == 3  # no eager step: the first run captured
    got = _result(r, losses)
    assert r.lr_position() == 6 and r.current_lr() == float(tab[5])
    assert _same(ref, got)


def test_per_bucket_update_placement_reads_the_same_rate(monkeypatch):
    """DPA_FUSED_STEP=1 (per-bucket updates on the wgrad stream, behind main-stream work of the
    step) under a schedule: 4 steps bitwise equal to the default placement."""
    from distributed_pytorch_amd.engine import VGGEngine
    from distributed_pytorch_amd.parallel import NullComm, make_sync

    tab = lr_table(0.05, 4, warmup_iters=2, decay="poly", power=1.0, end_lr=1e-3)
    assert len({float(v) for v in tab}) == 4
    batches = _batches(4, 8, 43)
    outs = []
    for fused in ("0", "1"):
        monkeypatch.setenv("DPA_FUSED_STEP", fused)
        e = VGGEngine("VGG11", "cuda", max_batch=8, impl="fp32")
        e.init_parameters(seed=5)
        e.set_lr_schedule(tab)
        sync = make_sync("ddp", e, NullComm())
        assert sync.fuse_step == (fused == "1")
        losses = []
        for x, y in batches:
            _sync_step(e, sync, x, y)
            losses.append(e.loss.clone())
        outs.append(_result(e, losses))
    assert _same(outs[0], outs[1])


def test_flat_sgd_follows_table():
    """parallel/ddp.FlatSGD(schedule=table) on a small module: 4 steps bitwise equal to FlatSGD with
    opt.lr = float(table[t]) set before each step."""
    from distributed_pytorch_amd.parallel.ddp import DistributedDataParallel, FlatSGD

    tab = lr_table(0.2, 4, warmup_iters=1, decay="cosine", end_lr=0.01)
    g = torch.Generator().manual_seed(50)
    data = [(torch.randn(16, 40, generator=g).cuda(), torch.randn(16, 8, generator=g).cuda()) for _ in range(4)]
    outs = []
    for scheduled in (True, False):
        torch.manual_seed(7)
        m = torch.nn.Sequential(torch.nn.Linear(40, 24), torch.nn.Tanh(), torch.nn.Linear(24, 8)).cuda()
        ddp = DistributedDataParallel(m)
        opt = FlatSGD(ddp, lr=0.2, momentum=0.9, weight_decay=1e-4, schedule=tab if scheduled else None)
        for t, (x, y) in enumerate(data):
            if not scheduled:
                opt.lr = float(tab[t])
            opt.zero_grad()
            (ddp(x) - y).square().mean().backward()
            opt.step(ddp.finish())
            if scheduled:
                assert opt.current_lr() == float(tab[t]) and opt.step_dev.item() == t + 1
        torch.cuda.synchronize()
        outs.append((ddp.flat_params.clone(), opt.buf.clone()))
    assert _same(outs[0], outs[1])
