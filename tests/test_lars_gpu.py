"""LARS and global-norm gradient clipping on the GPU (kernels/lars.hip): the three kernels against
fp64 torch and the CPU oracle (ops/cpu_ref) on the five-segment toy arena of lars_helpers, the
engine's step against the oracle applied to snapshots of its arenas, the captured-graph step, and
two ranks sharing the GPU in every sync mode."""
import json
import os
import subprocess
import sys

import pytest
import torch

import lars_helpers as L
from distributed_pytorch_amd.ops import cpu_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (1e-3, 1.0, 1e3, 1.0, 1e-3)  # per segment
S = len(L.TOY)


def _C():
    from distributed_pytorch_amd import _ext

    return _ext.require()


def close(a, b, tol):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    d = (a - b).abs().max().item()
    s = b.abs().max().clamp_min(1e-6).item()
    assert d <= tol * s, f"max abs diff {d} vs scale {s}"


def _split_planes(p, np_):
    """The exact operand planes of fp32 p: bf16 planes (NP 1 / 3) or the fp16 pair of p * H2_SW."""
    if np_ != 2:
        return cpu_ref.split_bf16(p, np_)
    xs = p * 256.0
    h0 = xs.half()
    return torch.stack([h0, (xs - h0.float()).half()])


def _planes(np_, n):
    if np_ == 0:
        return None
    return torch.zeros(np_, n, device="cuda", dtype=torch.float16 if np_ == 2 else torch.bfloat16)


def test_opt_chunk_exported():
    assert _C().OPT_CHUNK == cpu_ref.OPT_CHUNK == 8192


def test_sqnorm_partials_match_fp64():
    """Per-segment sums of squares within 1e-9 relative of fp64 torch (the squares are exact in
    fp64 and n * 2^-53 for n <= 24704 is far below that), and bitwise equal from launch to launch."""
    C_ = _C()
    p, g, _ = L.toy_arenas(7, SCALES)
    T = L.toy_tables(C_, device="cuda")
    pd, gd = p.flat.cuda(), g.flat.cuda()
    C_.sqnorm_partials(pd, gd, T["bmap"], T["partials"], S)
    first = T["partials"].clone()
    T["partials"].fill_(-1.0)
    C_.sqnorm_partials(pd, gd, T["bmap"], T["partials"], S)
    torch.cuda.synchronize()
    assert torch.equal(first, T["partials"])
    part = first.cpu()
    for (name, _), (f, c, _) in zip(L.TOY, T["segs"].tolist()):
        for col, a in ((0, p), (1, g)):
            ref = a[name].double().square().sum().item()
            got = part[f:f + c, col].sum().item()
            assert abs(got - ref) <= 1e-9 * ref, (name, col, got, ref)


@pytest.mark.parametrize("zeros", [False, True])
def test_finalize_matches_cpu_oracle(zeros):
    """Trust ratios within 1 ulp of fp32 (2.4e-7 relative) of the CPU oracle's, the clip
    coefficient and the norms within fp64 summation error (41280 elements: 41280 * 2^-53 < 1e-11);
    ratio exactly 1 for the g = 0, the p = 0 and the rank-1 segments."""
    C_ = _C()
    p, g, m = L.toy_arenas(8, SCALES, zero_g="a" if zeros else None, zero_p="b" if zeros else None)
    gscale = 0.5
    max_norm = 0.5 * gscale * g.flat.double().norm().item()
    Tc = L.toy_tables(cpu_ref)
    cpu_ref.sqnorm_partials(p.flat, g.flat, Tc["bmap"], Tc["partials"], S)
    cpu_ref.lars_finalize(Tc["partials"], Tc["segs"], Tc["table"], Tc["stats"], gscale, max_norm, L.OPT["trust"],
                          L.OPT["wd"], L.OPT["eps"])
    T = L.toy_tables(C_, device="cuda")
    C_.sqnorm_partials(p.flat.cuda(), g.flat.cuda(), T["bmap"], T["partials"], S)
    C_.lars_finalize(T["partials"], T["segs"], T["table"], T["stats"], gscale, max_norm, L.OPT["trust"], L.OPT["wd"],
                     L.OPT["eps"])
    torch.cuda.synchronize()
    tab, ref = T["table"].cpu(), Tc["table"]
    assert ((tab - ref).abs() <= 2.4e-7 * ref.abs()).all(), (tab, ref)
    st, rst = T["stats"].cpu(), Tc["stats"]
    assert ((st - rst).abs() <= 1e-11 * rst.abs()).all(), (st, rst)
    assert abs(st[2 * S + 1].item() - 0.5) < 1e-6  # max_norm is half the norm
    assert tab[3].item() == 1.0
    if zeros:
        assert tab[0].item() == 1.0 and tab[1].item() == 1.0
    else:
        assert all(tab[i].item() != 1.0 for i in (0, 1, 2, 4))


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("np_", [0, 1, 2, 3])
def test_sgd_segmented_matches_cpu_ref(np_, first):
    C_ = _C()
    p, g, m = L.toy_arenas(9)
    gscale = 0.5
    max_norm = 0.5 * gscale * g.flat.double().norm().item()
    pd, gd, md = p.flat.cuda(), g.flat.cuda(), m.flat.cuda()
    planes = _planes(np_, pd.numel())
    L.run_step(C_, pd, gd, md, L.toy_tables(C_, device="cuda"), gscale, max_norm, first, planes)
    L.run_step(cpu_ref, p.flat, g.flat, m.flat, L.toy_tables(cpu_ref), gscale, max_norm, first)
    torch.cuda.synchronize()
    close(pd, p.flat, 1e-6)
    close(md, m.flat, 1e-6)
    if np_:
        assert torch.equal(planes.cpu(), _split_planes(pd.cpu(), np_))
        assert not C_.h2_overflow(True)


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("np_", [0, 1, 2, 3])
def test_sgd_segmented_same_bits_as_sgd_flat(np_, first):
    """LARS off and max_norm = 1e30 (c = 1): every ratio is 1 and gmul = gs, and the segmented
    update gives the bits of sgd_flat (parameters, momentum and planes)."""
    C_ = _C()
    p, g, m = L.toy_arenas(10, SCALES)
    gd = g.flat.cuda()
    pa, ma, pb, mb = p.flat.cuda(), m.flat.cuda(), p.flat.cuda(), m.flat.cuda()
    pla, plb = _planes(np_, pa.numel()), _planes(np_, pa.numel())
    C_.sgd_flat(pa, gd, ma, L.OPT["lr"], L.OPT["momentum"], L.OPT["wd"], 0.5, first, 0, -1, pla)
    T = L.toy_tables(C_, lars=False, device="cuda")
    L.run_step(C_, pb, gd, mb, T, 0.5, 1e30, first, plb)
    torch.cuda.synchronize()
    assert T["table"].cpu().tolist() == [1.0] * S + [0.5]
    assert torch.equal(pa, pb) and torch.equal(ma, mb)
    assert not torch.equal(pa, p.flat.cuda())
    if np_:
        assert torch.equal(pla, plb)
        C_.h2_overflow(True)


def test_bindings_check_arguments():
    C_ = _C()
    p, g, m = L.toy_arenas(1)
    T = L.toy_tables(C_, device="cuda")
    pd, gd, md = p.flat.cuda(), g.flat.cuda(), m.flat.cuda()
    with pytest.raises(RuntimeError):
        C_.sqnorm_partials(p.flat, gd, T["bmap"], T["partials"], S)  # CPU tensor
    with pytest.raises(RuntimeError):
        C_.sqnorm_partials(pd, gd[:-64], T["bmap"], T["partials"], S)  # sizes
    with pytest.raises(RuntimeError):
        C_.sqnorm_partials(pd, gd, T["bmap"].int(), T["partials"], S)  # dtype
    with pytest.raises(RuntimeError):
        C_.sqnorm_partials(pd, gd, T["bmap"], T["partials"][:-1], S)  # partials size
    with pytest.raises(RuntimeError):
        C_.lars_finalize(T["partials"], T["segs"], T["table"][:-1], T["stats"], 1.0, 0.0, 0.02, 1e-4, 1e-9)
    with pytest.raises(RuntimeError):
        C_.sgd_segmented(pd, gd, md[:-64], T["bmap"], T["table"], 0.1, 0.9, 1e-4, False, None)
    with pytest.raises(RuntimeError):
        C_.sgd_segmented(pd, gd, md, T["bmap"].t(), T["table"], 0.1, 0.9, 1e-4, False, None)  # not contiguous
    # a block-map entry outside the arena is skipped by the kernels, the rest is updated
    bad = T["bmap"].clone()
    bad[1, 1] = pd.numel()  # chunk of segment "b" moved past the end
    T2 = dict(T, bmap=bad)
    before = pd.clone()
    L.run_step(C_, pd, gd, md, T2, 1.0, 0.0, False)
    torch.cuda.synchronize()
    assert torch.equal(pd[64:64 + 8192], before[64:64 + 8192])
    assert not torch.equal(pd[:64], before[:64]) and not torch.equal(pd[64 + 8192:], before[64 + 8192:])


@pytest.mark.parametrize("impl", ["h2", "fp32"])
def test_engine_lars_step_matches_cpu_ref(impl):
    """Two steps at batch 16: each update, applied by the oracle to snapshots of the arenas taken
    right before it, gives the engine's parameters and momentum (this isolates the optimizer from
    conv precision); opt_stats' gradient norm is the snapshot's fp64 norm."""
    from distributed_pytorch_amd.engine import VGGEngine
    from distributed_pytorch_amd.utils.arena import block_map

    e = VGGEngine("VGG11", "cuda", max_batch=16, impl=impl, lr=0.1, optimizer="lars", trust_coef=0.02,
                  clip_grad_norm=1.0)
    e.init_parameters(seed=6)
    bmap, segs = block_map(e.params.segments(), cpu_ref.OPT_CHUNK, True)
    T = dict(bmap=bmap, segs=segs, partials=torch.zeros(bmap.shape[0], 2, dtype=torch.float64),
             table=torch.ones(segs.shape[0] + 1), stats=torch.zeros(2 * segs.shape[0] + 2, dtype=torch.float64))
    gen = torch.Generator().manual_seed(16)
    for step in range(2):
        x = torch.zeros(16, 32, 32, 4)
        x[..., :3] = torch.randn(16, 32, 32, 3, generator=gen)
        t = torch.randint(0, 10, (16,), generator=gen)
        e.forward_backward(x.cuda(), t.cuda())
        torch.cuda.synchronize()
        p, g, m = e.params.flat.cpu(), e.grads.flat.cpu(), e.mom.flat.cpu()
        e.sgd_step()
        e.finish_step()
        st = e.opt_stats()
        cpu_ref.sqnorm_partials(p, g, T["bmap"], T["partials"], segs.shape[0])
        cpu_ref.lars_finalize(T["partials"], T["segs"], T["table"], T["stats"], 1.0, 1.0, 0.02, e.weight_decay, 1e-9)
        cpu_ref.sgd_segmented(p, g, m, T["bmap"], T["table"], e.lr, e.momentum, e.weight_decay, step == 0)
        close(e.params.flat, p, 1e-6)
        close(e.mom.flat, m, 1e-6)
        norm = g.double().norm().item()
        assert abs(st["grad_norm"] - norm) <= 1e-9 * norm, (st["grad_norm"], norm)
        assert st["clip_coef"] < 1.0 and st["tensors"]["layers.0.weight"]["trust_ratio"] != 1.0
        assert st["tensors"]["layers.0.bias"]["trust_ratio"] == 1.0
        if e.wplanes is not None:  # the operand planes follow the updated parameters
            assert torch.equal(e.wplanes.cpu(), _split_planes(e.params.flat.cpu(), e.np))
    e.check_signals()
    with pytest.raises(ValueError, match="whole arena"):
        e.sgd_step(offset=64)


@pytest.mark.parametrize("impl", ["x3", "bf16"])
def test_graphed_step_with_lars_matches_eager(impl):
    """The optimizer's three launches have no host round trip, so the captured step replays them:
    2 eager warm-up steps + 2 replays == 4 eager steps, bitwise."""
    from distributed_pytorch_amd.engine import VGGEngine
    from distributed_pytorch_amd.graph_step import GraphedStep
    from distributed_pytorch_amd.parallel import NullComm, make_sync

    g = torch.Generator().manual_seed(21)
    batches = [(torch.randn(32, 32, 32, 4, generator=g), torch.randint(0, 10, (32,), generator=g)) for _ in range(4)]
    outs = []
    for graph in (False, True):
        e = VGGEngine("VGG11", "cuda", max_batch=32, impl=impl, lr=0.02, optimizer="lars", trust_coef=0.02,
                      clip_grad_norm=1.0)
        e.init_parameters(seed=4)
        sync = make_sync("ddp", e, NullComm())
        gs = GraphedStep(e, sync, warmup=2) if graph else None
        xb = torch.empty(32, 32, 32, 4, device="cuda")
        tb = torch.empty(32, dtype=torch.int64, device="cuda")
        losses = []
        for x, t in batches:
            xb.copy_(x)
            xb[..., 3] = 0
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
        if gs is not None:
            assert gs.replays == 2 and gs.graph is not None
        assert e.opt_stats()["clip_coef"] < 1.0
        outs.append((e.params.flat.clone(), e.mom.flat.clone(), torch.stack(losses)))
    for a_, b_ in zip(outs[0], outs[1]):
        assert torch.equal(a_, b_)


LARS_ENV = {"DPA_OPTIMIZER": "lars", "DPA_CLIP_GRAD_NORM": "1"}


def _bench_two_ranks(mode, env_extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--comm", "gloo", "--mode", mode,
           "--steps", "2", "--warmup", "1", "--solo-steps", "0", "--diag-steps", "0", "--batch", "32",
           "--launch-timeout", "100"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "DPA_OPTIMIZER", "DPA_TRUST_COEF", "DPA_CLIP_GRAD_NORM"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, r.stdout[-2000:]
    return json.loads(lines[-1])


@pytest.fixture(scope="module")
def lars_runs():
    return {}


@pytest.mark.parametrize("mode", ["ddp", "allreduce", "gather"])
def test_two_ranks_share_one_gpu_with_lars(lars_runs, mode):
    d = _bench_two_ranks(mode, LARS_ENV)
    lars_runs[mode] = d
    assert d["n_gpus"] == 2 and d["config"]["sync_mode"] == mode, d
    assert d["replicas_identical"] is True and d["replica_param_max_diff"] == 0.0, d
    assert d["final_loss"] == d["final_loss"], d


def test_two_ranks_lars_modes_agree_bitwise(lars_runs):
    """W = 2: the scale 1/2 is a power of two, so |2x| / 2 = |x| exactly in fp64 and
    (2x) fl(c / 2) = x fl(c): the strict cross-mode oracle of test_multirank_gpu carries over.  The
    run without the variables must end elsewhere."""
    assert len(lars_runs) == 3, "needs every mode's run"
    sums = {m: d["param_checksum"] for m, d in lars_runs.items()}
    assert len(set(sums.values())) == 1, sums
    plain = _bench_two_ranks("ddp", {})
    assert plain["replicas_identical"] is True
    assert plain["param_checksum"] != sums["ddp"], (plain["param_checksum"], sums)
