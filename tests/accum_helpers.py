"""Shared pieces of the gradient-accumulation tests: the engine oracle (micro-batch gradients summed
with torch.add in the fixed order, then one ordinary update), the state comparison, a communicator
wrapper that records every call, and the worker of the two-rank gloo test.  Spawned processes import
this module by name (tests/ is on their sys.path)."""
import os

import torch

import dist_helpers as H

LARS = dict(optimizer="lars", trust_coef=0.02, clip_grad_norm=1.0)  # as tests/lars_helpers.py


def refused_fold_arguments(dev="cpu"):
    """(name, acc, g, mode, offset, count) of every argument set grad_fold must refuse."""
    f = lambda n=64, **kw: torch.zeros(n, device=dev, **kw)
    return [
        ("acc not fp32", f(dtype=torch.float64), f(), 0, 0, -1),
        ("g not fp32", f(), f(dtype=torch.float16), 0, 0, -1),
        ("acc not contiguous", f(128)[::2], f(), 0, 0, -1),
        ("g not contiguous", f(), f(128)[::2], 0, 0, -1),
        ("different lengths", f(64), f(68), 0, 0, -1),
        ("unknown mode", f(), f(), 3, 0, -1),
        ("negative mode", f(), f(), -1, 0, -1),
        ("negative offset", f(), f(), 0, -4, 4),
        ("negative count", f(), f(), 0, 0, -4),
        ("offset not a multiple of 4", f(), f(), 0, 2, 4),
        ("count not a multiple of 4", f(), f(), 0, 4, 6),
        ("length not a multiple of 4", f(66), f(66), 0, 0, -1),
        ("slice past the end", f(), f(), 0, 60, 8),
        ("offset past the end", f(), f(), 0, 68, -1),
    ]


def batches(n, bs, device="cpu", seed=5):
    """n batches of bs NHWC samples (4th channel zero) with their targets."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        x = torch.zeros(bs, 32, 32, 4)
        x[..., :3] = torch.randn(bs, 32, 32, 3, generator=g)
        out.append((x.to(device), torch.randint(0, 10, (bs,), generator=g).to(device)))
    return out


def state(e):
    """Everything an accumulated step must leave bitwise equal to the oracle's."""
    s = {"params": e.params.flat, "mom": e.mom.flat, "buffers": e.buffers.flat, "nbt": e.nbt,
         "loss_accum": e.loss_accum}
    if e.wplanes is not None:
        s["wplanes"] = e.wplanes.view(torch.int16)  # bit patterns: the comparison is of bits, NaN-proof
    return {k: v.detach().clone().cpu() for k, v in s.items()}


def assert_same_state(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


def oracle_group(e, group, sync_scale=1.0):
    """The issue's oracle for one group on engine e: forward_backward alone on each micro-batch with
    the gradient cloned, BN buffers / nbt (and the loss sum) restored, the clones summed with
    torch.add in the order (((g_0 + g_1) + g_2) + ...); then the replay -- the first a-1 micro-batches
    (the BN buffers advance the same way), the last one, the summed gradient copied into the arena and
    ``sgd_step(sync_scale / a)``."""
    buf0, nbt0, la0 = e.buffers.flat.clone(), e.nbt.clone(), e.loss_accum.clone()
    gs = []
    for x, t in group:
        e.forward_backward(x, t)
        gs.append(e.grads.flat.clone())
    e.buffers.flat.copy_(buf0)
    e.nbt.copy_(nbt0)
    e.loss_accum.copy_(la0)
    total = gs[0].clone()
    for g in gs[1:]:
        total = torch.add(total, g)
    for x, t in group:
        e.forward_backward(x, t)
    e.grads.flat.copy_(total)
    e.sgd_step(sync_scale / len(group))
    e.finish_step()


def accumulated_groups(e, sync, groups, accum_steps):
    """Drive AccumulatedStep over the groups (a short one is closed with last=True)."""
    from distributed_pytorch_amd.accum import AccumulatedStep

    step = AccumulatedStep(e, sync, accum_steps)
    for group in groups:
        for k, (x, t) in enumerate(group):
            closed = step.run(x, t, last=k == len(group) - 1)
            assert closed == (k == len(group) - 1)
    return step


class CountingComm:
    """Delegates to a communicator and records the name of every method called on it."""

    def __init__(self, inner):
        self._inner = inner
        self.calls = []

    def __getattr__(self, k):
        v = getattr(self._inner, k)
        if not callable(v):
            return v

        def call(*a, **kw):
            self.calls.append(k)
            return v(*a, **kw)

        return call


def run_accum_mode(rank, world, port, mode, n_groups, accum_steps, outdir):
    """Two gloo ranks: n_groups ordinary steps on one engine (the call lists an ordinary step makes),
    then n_groups accumulated groups on another, with every communicator call recorded per
    micro-step."""
    import torch.distributed as dist

    from distributed_pytorch_amd.accum import AccumulatedStep
    from distributed_pytorch_amd.engine import VGGEngine
    from distributed_pytorch_amd.parallel import TorchComm, make_sync

    H._init(rank, world, port)
    inner = TorchComm(device=torch.device("cpu"))
    data = H._batches(rank, n_groups * accum_steps)

    ordinary = []
    c0 = CountingComm(inner)
    e0 = VGGEngine("VGG11", "cpu", max_batch=4, lr=0.01)
    e0.init_parameters(seed=1 + rank)
    s0 = make_sync(mode, e0, c0)
    for x, t in data[:n_groups]:
        c0.calls = []
        s0.begin_step()
        e0.forward_backward(H._x4(x), t, grad_ready=s0.grad_ready, pre_forward=s0.pre_forward,
                            params_free=s0.params_free)
        s0.update(s0.finish())
        e0.finish_step()
        ordinary.append(list(c0.calls))

    comm = CountingComm(inner)
    e = VGGEngine("VGG11", "cpu", max_batch=4, lr=0.01)
    e.init_parameters(seed=1 + rank)  # different per rank: the start-up broadcast unifies them
    sync = make_sync(mode, e, comm)
    step = AccumulatedStep(e, sync, accum_steps)
    micro, closing, losses = [], [], []
    for i, (x, t) in enumerate(data):
        comm.calls = []
        closed = step.run(H._x4(x), t)
        (closing if closed else micro).append(list(comm.calls))
        losses.append(float(e.loss.item()))
    if mode == "ddp":
        wait = sync.pre_forward()
        if wait is not None:
            wait()
    sync.prepare_checkpoint()
    torch.save({"params": e.params.flat.clone(), "mom": e.mom.flat.clone(), "buffers": e.buffers.flat.clone(),
                "losses": losses, "steps_taken": e.steps_taken, "ordinary": ordinary, "micro": micro,
                "closing": closing}, os.path.join(outdir, f"accum_{mode}_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()
