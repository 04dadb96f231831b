"""Shared pieces of the LARS / gradient-clipping tests: the hand-written per-tensor oracle (fp64,
torch.nn.utils.clip_grad_norm_ semantics), the five-segment toy arena, and the worker of the
two-rank gloo test.  Spawned processes import this module by name (tests/ is on their sys.path)."""
import os

import torch

import dist_helpers as H

OPT = dict(lr=0.1, momentum=0.9, wd=1e-4, trust=0.02, eps=1e-9)

# (name, shape): a segment smaller than a block, exactly one chunk, one chunk plus a 64-element
# tail, a rank-1 tensor (10 elements, padded to 64) between large ones, several chunks + odd tail
TOY = [("a", (8, 8)), ("b", (64, 128)), ("c", (129, 64)), ("v", (10,)), ("d", (386, 64))]
TOY_EXTENTS = [64, 8192, 8256, 64, 24704]


def lars_reference(ps, gs, bufs, lr, momentum, wd, gscale, first, trust=None, eps=1e-9, max_norm=0.0):
    """One step on lists of tensors, in place, in fp64 arithmetic: global-norm clipping of the
    scaled gradients (clip_grad_norm_: c = min(1, max_norm / (total + 1e-6))), then per tensor
    LARS with the learning rate outside the momentum (trust ratio on tensors of rank >= 2 whose
    parameter and gradient norms are both positive; ``trust=None``: plain SGD).
    Returns (total norm, clip coefficient, [trust ratios])."""
    g64 = [g.double() * gscale for g in gs]
    total = torch.stack([g.norm() for g in g64]).norm().item()
    c = min(1.0, max_norm / (total + 1e-6)) if max_norm > 0 else 1.0
    ratios = []
    for p, g, b in zip(ps, g64, bufs):
        p64, g = p.double(), g * c
        pn, gn = p64.norm().item(), g.norm().item()
        r = trust * pn / (gn + wd * pn + eps) if trust is not None and p.ndim >= 2 and pn > 0 and gn > 0 else 1.0
        d = (g + wd * p64) * r
        nb = d if first else momentum * b.double() + d
        b.copy_(nb)
        p.copy_(p64 - lr * nb)
        ratios.append(r)
    return total, c, ratios


def toy_arenas(seed=0, scales=(1.0, 1.0, 1.0, 1.0, 1.0), zero_g=None, zero_p=None):
    """(params, grads, momentum) arenas of the TOY layout on the CPU: randn times the segment's
    scale in the tensors, zero in the padding."""
    from distributed_pytorch_amd.utils.arena import Arena

    gen = torch.Generator().manual_seed(seed)
    p = Arena(TOY, "cpu")
    g, m = p.like(), p.like()
    for (name, _), s in zip(TOY, scales):
        for a in (p, g, m):
            a[name].copy_(torch.randn(a[name].shape, generator=gen) * s)
    if zero_g is not None:
        g[zero_g].zero_()
    if zero_p is not None:
        p[zero_p].zero_()
    return p, g, m


def toy_tables(K, lars=True, device="cpu"):
    """Block map, segment table and the three work tables of the TOY arena for backend K."""
    from distributed_pytorch_amd.utils.arena import Arena, block_map

    bmap, segs = block_map(Arena(TOY, "cpu").segments(), int(K.OPT_CHUNK), lars, device)
    S = segs.shape[0]
    return dict(bmap=bmap, segs=segs, partials=torch.zeros(bmap.shape[0], 2, dtype=torch.float64, device=device),
                table=torch.ones(S + 1, dtype=torch.float32, device=device),
                stats=torch.zeros(2 * S + 2, dtype=torch.float64, device=device))


def run_step(K, p, g, m, T, gscale, max_norm, first, planes=None, trust=OPT["trust"]):
    """The optimizer step (a) -> (b) -> (c) of backend K on flat arenas p, g, m (tables T)."""
    K.sqnorm_partials(p, g, T["bmap"], T["partials"], T["segs"].shape[0])
    K.lars_finalize(T["partials"], T["segs"], T["table"], T["stats"], gscale, max_norm, trust, OPT["wd"], OPT["eps"])
    K.sgd_segmented(p, g, m, T["bmap"], T["table"], OPT["lr"], OPT["momentum"], OPT["wd"], first, planes)


def run_engine_mode_lars(rank, world, port, mode, steps, outdir):
    """dist_helpers.run_engine_mode with LARS + clipping (gloo, CPU); zero1 must refuse."""
    import torch.distributed as dist

    from distributed_pytorch_amd.engine import VGGEngine
    from distributed_pytorch_amd.parallel import TorchComm, make_sync

    H._init(rank, world, port)
    comm = TorchComm(device=torch.device("cpu"))
    e = VGGEngine("VGG11", "cpu", max_batch=4, lr=0.05, optimizer="lars", trust_coef=0.02, clip_grad_norm=1.0)
    e.init_parameters(seed=1 + rank)
    out = {}
    if mode == "zero1":
        try:
            make_sync(mode, e, comm)
            out["error"] = None
        except ValueError as err:
            out["error"] = str(err)
    else:
        sync = make_sync(mode, e, comm)
        losses = []
        for x, t in H._batches(rank, steps):
            sync.begin_step()
            e.forward_backward(H._x4(x), t, grad_ready=sync.grad_ready, pre_forward=sync.pre_forward,
                               params_free=sync.params_free)
            sync.update(sync.finish())
            e.finish_step()
            losses.append(float(e.loss.item()))
        out = {"params": e.params.flat.clone(), "losses": losses, "stats": e.opt_stats()}
    torch.save(out, os.path.join(outdir, f"lars_{mode}_{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()
