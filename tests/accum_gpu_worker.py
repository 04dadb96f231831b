"""One rank of the multi-process gradient-accumulation tests on the GPU (tests/test_step_accum_gpu.py),
started as a plain child process with the torchrun environment (parallel/spawn.py sets it).

    python tests/accum_gpu_worker.py rccl1 OUTDIR   one rank; DPA_FORCE_COMM=1 makes its communicator a
                                                    1-rank RCCL one: two groups in DDP mode on it, and
                                                    the same two groups on a NullComm
    python tests/accum_gpu_worker.py gloo OUTDIR    two ranks sharing one GPU, gradients through gloo:
                                                    two groups in each of the four sync modes

Writes OUTDIR/LABEL_RANK.pt with the parameter and momentum arenas, the BN buffers and the losses.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_pytorch_amd.accum import AccumulatedStep  # noqa: E402
from distributed_pytorch_amd.engine import VGGEngine  # noqa: E402
from distributed_pytorch_amd.parallel import NullComm, init_env, make_sync  # noqa: E402

N, A, GROUPS = 8, 2, 2


def batches(rank):
    g = torch.Generator().manual_seed(700 + rank)
    out = []
    for _ in range(A * GROUPS):
        x = torch.zeros(N, 32, 32, 4)
        x[..., :3] = torch.randn(N, 32, 32, 3, generator=g)
        out.append((x, torch.randint(0, 10, (N,), generator=g)))
    return out


def run(ctx, comm, mode, label, outdir, seed):
    dev = ctx.device
    e = VGGEngine("VGG11", dev, max_batch=N, impl="h2", lr=0.02)
    e.init_parameters(seed=seed)
    sync = make_sync(mode, e, comm)
    step = AccumulatedStep(e, sync, A)
    losses = []
    for x, t in batches(ctx.rank):
        step.run(x.to(dev), t.to(dev))
        losses.append(float(e.loss.item()))
    assert step.pos == 0 and e.steps_taken == GROUPS and e.gacc is not None
    sync.prepare_checkpoint()
    torch.cuda.synchronize(dev)
    e.check_signals()
    comm.check()
    torch.save({"params": e.params.flat.cpu(), "mom": e.mom.flat.cpu(), "buffers": e.buffers.flat.cpu(),
                "wplanes": e.wplanes.view(torch.int16).cpu(), "losses": losses, "comm": comm.name,
                "world": ctx.world}, os.path.join(outdir, f"{label}_{ctx.rank}.pt"))


def main():
    kind, outdir = sys.argv[1], sys.argv[2]
    if kind == "rccl1":
        ctx = init_env(device="cuda", comm="rccl")
        assert ctx.world == 1 and ctx.comm.name != "null", "expected a forced 1-rank communicator"
        run(ctx, NullComm(), "ddp", "null", outdir, seed=1)
        run(ctx, ctx.comm, "ddp", "rccl1", outdir, seed=1)
    else:
        ctx = init_env(device="cuda", comm="gloo")
        for mode in ("gather", "allreduce", "ddp", "zero1"):
            # different init per rank: the start-up broadcast must unify them
            run(ctx, ctx.comm, mode, mode, outdir, seed=1 + ctx.rank)
    ctx.barrier()
    ctx.shutdown()


if __name__ == "__main__":
    main()
