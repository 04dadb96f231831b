"""Multi-rank rehearsal of the GPU training path on a one-GPU box.

RCCL refuses two ranks on one GPU, so these runs put 2 ranks on the same device and move the
gradients through gloo with host staging (``--comm gloo``, parallel/comm.py TorchComm).  Everything
else is the multi-GPU code path of bench.py: the N-rank launcher (parallel/spawn.py), the engine's
two-stream backward with kernel-start signals, the sync strategies (bucketed DDP / per-tensor
all-reduce / gather-scatter / ZeRO-1) on a side stream, the per-bucket fused SGD and the
cross-rank replica check.  Each mode must end with bit-identical parameters on both ranks, and —
the reference's correctness oracle (the three modes give bit-identical parameters at
the same seed) — every mode with the same parameters as every other: with two ranks a sum of two
gradients and its halving are exact in any order.

The oracle is strict: no kernel serialisation, bitwise equality, no re-runs.  Until round 6 it was
not (runs of several processes sharing one GPU were not run-to-run reproducible, so the checks ran
serialised, to 1e-4, with one re-run).  The cause was found by differential replay
(tools/replay_check.py, docs/PERF_NOTES.md round 6): the first-layer conv kernel's packed fp32 FMAs
(v_pk_fma_f32) produced a wrong value for one 16-lane pass now and then under multi-process load;
built without packed fp32 that kernel replays bit-exactly, and so do the runs."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["ddp", "allreduce", "gather", "zero1"]
SERIAL: dict = {}  # (the oracle runs unserialised since round 6, module docstring)


def _agree(sums):
    """The cross-mode oracle over {label: checksum}: bitwise one value (no tolerance, no re-run)."""
    assert len(set(sums.values())) == 1, sums


def _run(mode):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--comm", "gloo", "--mode", mode,
           "--steps", "3", "--warmup", "2", "--solo-steps", "0", "--diag-steps", "1", "--launch-timeout", "100"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **SERIAL)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, r.stdout[-2000:]
    return json.loads(lines[-1])


@pytest.fixture(scope="module")
def runs():
    return {}


@pytest.mark.parametrize("mode", MODES)
def test_two_ranks_share_one_gpu(runs, mode):
    d = _run(mode)
    runs[mode] = d
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2", d
    assert d["config"]["sync_mode"] == mode, d
    assert d["replicas_identical"] is True and d["replica_param_max_diff"] == 0.0, d
    assert d["value"] > 0 and d["final_loss"] == d["final_loss"], d


def test_modes_agree(runs):
    """The reference oracle (same seed, same parameters in every mode), two ranks
    sharing one GPU through gloo: bitwise (a sum of two gradients and its halving are exact)."""
    if len(runs) < len(MODES):
        pytest.skip("needs every mode's run")
    _agree({m: runs[m]["param_checksum"] for m in MODES})


def test_four_ranks_ddp_share_one_gpu():
    """W = 4 (bucket all-reduce of four contributions, 1/W folded into the update)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "4", "--comm", "gloo", "--mode",
           "ddp", "--steps", "2", "--warmup", "1", "--solo-steps", "0", "--diag-steps", "0", "--batch", "64",
           "--launch-timeout", "100"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 4 and d["replicas_identical"] is True, d


def test_resnet_generic_ddp_two_ranks():
    """The generic path (autograd + hook DDP over the flat arena, parallel/ddp.py) with a real
    communicator: ResNet-50 at a small batch and image size, replicas bitwise identical."""
    cmd = [sys.executable, os.path.join(ROOT, "bench_resnet.py"), "--gpus", "2", "--comm", "gloo", "--steps", "2",
           "--warmup", "1", "--batch", "8", "--image", "64", "--launch-timeout", "100"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["replicas_identical"] is True, d


def test_torchrun_launch_two_ranks():
    """The driver's launch form: torch.distributed.run --nproc-per-node 2 ... bench.py --gpus 2."""
    from distributed_pytorch_amd.parallel.spawn import free_port

    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2",
           "--comm", "gloo", "--steps", "3", "--warmup", "1", "--solo-steps", "2", "--diag-steps", "1"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "DPA_STORE_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["config"]["launcher"] == "torchrun" and d["replicas_identical"] is True, d
    assert d["solo_img_s"] and d["scaling_efficiency"] is not None, d


def test_main_ddp_training_two_ranks(tmp_path):
    """The reference's mode-C entry point (main_ddp.py under torchrun) trains on the GPU engine with
    2 ranks: reference log lines, full-test-set evaluation on every rank, per-rank checkpoints."""
    from distributed_pytorch_amd.parallel.spawn import free_port

    ck = tmp_path / "ck"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "main_ddp.py"), "--comm", "gloo",
           "--synthetic", "--train-size", "10240", "--test-size", "1024", "--checkpoint-dir", str(ck)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "DPA_STORE_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert out.count("Epoch: 1, Iteration: 1-20, Average Loss:") == 2, out[-3000:]  # 20 iterations per rank
    assert out.count("Test set: Average loss:") == 2 and "/1024 (" in out, out[-3000:]
    assert (ck / "rank0.pt").exists() and (ck / "rank1.pt").exists()


@pytest.mark.parametrize("world,stage,inbox", [(2, 0, 0), (3, 0, 0), (4, 0, 0), (8, 0, 0), (2, 65536, 40000)])
def test_ipc_collectives_ranks_share_one_gpu(world, stage, inbox):
    """every peer-memory collective (all-reduce sum/max/min, broadcast, gather,
    reduce-scatter, all-gather, barrier) between 2 / 3 / 4 / 8 processes on one GPU, through the
    registered (in place) and the bounced (inbox) input paths: bitwise the rank-order fp32 reduction
    or the exact copy, nothing outside the target touched, no wait timed out, no tensor through the
    host (tests/ipc_worker.py; native-store rendezvous, no torch.distributed group at all).
    stage / inbox: buffers smaller than the collectives (every one runs as several pieces)."""
    from distributed_pytorch_amd.parallel.spawn import free_port

    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "tests", "ipc_worker.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    if stage:
        env["DPA_IPC_TEST_STAGE"] = str(stage)
    if inbox:
        env["DPA_IPC_TEST_INBOX"] = str(inbox)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "DPA_STORE_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["world"] == world and d["bitwise_ok"] and not d["timeout"], d
    assert d["inner_tensor_ops"] == 0 and len(d["results"]) >= 12, d


def _bench(args, script="bench.py", timeout=110, env_extra=None):
    full = ["--full"] if script == "bench.py" else []  # (the replica check and the diagnostic steps)
    cmd = [sys.executable, os.path.join(ROOT, script)] + full + args + ["--launch-timeout", str(timeout - 10)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **(env_extra or {}))
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, r.stdout[-2000:]
    return json.loads(lines[-1])


# the collectives each mode must have run on the peer kernels (after start-up)
_MODE_OPS = {"ddp": {"all_reduce", "broadcast"}, "allreduce": {"all_reduce"}, "gather": {"gather", "broadcast"},
             "zero1": {"reduce_scatter", "all_gather", "broadcast"}}


@pytest.fixture(scope="module")
def ipc_runs():
    return {}


def _ipc_run(mode, world):
    return _bench(["--gpus", str(world), "--comm", "ipc", "--mode", mode, "--steps", "3", "--warmup", "2",
                   "--solo-steps", "0", "--diag-steps", "1"] + (["--batch", "64"] if world > 2 else []),
                  env_extra=SERIAL)


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("mode", MODES)
def test_modes_on_peer_kernels(ipc_runs, mode, world):
    """every sync mode with EVERY collective on the peer-memory kernels (--comm
    ipc: mode A's gather -> mean -> broadcast, DDP's bucket all-reduces and BN-buffer broadcasts,
    ZeRO-1's reduce-scatter / all-gather, the start-up broadcast): replicas bitwise identical, and no
    tensor byte through gloo or the host (the communicator wraps nothing)."""
    d = _ipc_run(mode, world)
    ipc_runs[(mode, world)] = d
    assert d["n_gpus"] == world and d["config"]["sync_mode"] == mode and d["config"]["comm"] == "ipc-standalone", d
    assert d["replicas_identical"] is True and d["replica_param_max_diff"] == 0.0, d
    assert d["ipc_inner_tensor_ops"] == 0, d
    assert _MODE_OPS[mode] <= set(d["ipc_ops_by_kind"]), d["ipc_ops_by_kind"]


def test_peer_kernel_modes_agree(ipc_runs, runs):
    """The reference oracle (same seed, same parameters in every mode) on the peer
    kernels, bitwise: every mode at W=2 lands on the parameters of the gloo (host-staged) runs (a
    sum of two is exact in any order), and at W=4 (rank-order sums in every mode) every mode on the
    parameters of every other."""
    need = [(m, w) for m in MODES for w in (2, 4)]
    if not all(k in ipc_runs for k in need) or not runs:
        pytest.skip("needs every mode's run")
    w2 = {("ipc", m): ipc_runs[(m, 2)]["param_checksum"] for m in MODES}
    w2.update({("gloo", m): d["param_checksum"] for m, d in runs.items()})
    _agree(w2)
    _agree({m: ipc_runs[(m, 4)]["param_checksum"] for m in MODES})


def test_ddp_eight_ranks_share_one_gpu():
    """W = 8 (the node size the driver's scaling run uses) of the DDP mode on the
    peer kernels, batch 32 per rank, eight processes on one GPU."""
    d = _bench(["--gpus", "8", "--comm", "ipc", "--mode", "ddp", "--steps", "2", "--warmup", "1", "--solo-steps", "0",
                "--diag-steps", "0", "--batch", "32"])
    assert d["n_gpus"] == 8 and d["replicas_identical"] is True and d["ipc_inner_tensor_ops"] == 0, d


def test_resnet_generic_ddp_on_peer_kernels():
    """The hook-based generic DDP (parallel/ddp.py, ResNet-50) with every collective on the peer
    kernels, 2 ranks on one GPU: replicas bitwise identical."""
    d = _bench(["--gpus", "2", "--comm", "ipc", "--steps", "2", "--warmup", "1", "--batch", "8", "--image", "64"],
               script="bench_resnet.py")
    assert d["n_gpus"] == 2 and d["replicas_identical"] is True, d


def test_ipc_ddp_matches_gloo(runs):
    """Bucketed DDP with the collectives on the peer-memory kernels wrapped around the gloo
    communicator (--ipc on, 2 ranks on one GPU): replicas identical and -- a sum of two is exact in
    any order -- bitwise the parameters of the gloo run of the same mode."""
    args = ["--gpus", "2", "--comm", "gloo", "--mode", "ddp", "--ipc", "on", "--steps", "3", "--warmup", "2",
            "--solo-steps", "0", "--diag-steps", "1"]
    d = _bench(args, env_extra=SERIAL)
    assert d["replicas_identical"] is True and d["ipc_allreduce_ops"] and d["ipc_allreduce_ops"] > 0, d
    if "ddp" in runs:
        assert d["param_checksum"] == runs["ddp"]["param_checksum"], (d["param_checksum"], runs["ddp"])


def test_ipc_live_agreement_checks():
    """with the peer kernels carrying the run, every diagnostic step re-reduces
    the live gradient arena and checks it through the store (checksums, nothing shared with the
    device path); the verdicts are in the JSON."""
    d = _bench(["--gpus", "2", "--comm", "ipc", "--mode", "ddp", "--steps", "2", "--warmup", "1", "--solo-steps", "0",
                "--diag-steps", "3"])
    chk = d["ipc_live_check"]
    assert chk["checks"] == 3 and chk["ok"] is True and chk["max_rel_err"] < 1e-6, chk


def test_ipc_forced_disagreement_drops_plan():
    """a peer all-reduce that disagrees (injected: the last rank's result is
    corrupted before the check) makes the comm tuner drop every IPC plan on every rank -- the run
    finishes on the wrapped communicator, replicas identical, no hang -- and a live check reports
    the failure instead of raising."""
    env = {"DPA_IPC_TEST_DISAGREE": "1"}
    d = _bench(["--gpus", "2", "--comm", "gloo", "--mode", "ddp", "--ipc", "auto", "--steps", "2", "--warmup", "1",
                "--solo-steps", "0", "--diag-steps", "0", "--comm-tune-steps", "1"], env_extra=env, timeout=200)
    tune = d["config"]["comm_tune"]
    assert tune is not None and tune["ipc_check"] is not None and tune["ipc_check"]["ok"] is False, tune
    assert tune["chosen"]["ipc_blocks"] is None and not any("ipc" in k for k in tune["ms_per_step"]), tune
    assert d["replicas_identical"] is True, d
    d2 = _bench(["--gpus", "2", "--comm", "ipc", "--mode", "ddp", "--steps", "2", "--warmup", "1", "--solo-steps", "0",
                 "--diag-steps", "1"], env_extra=env)
    assert d2["ipc_live_check"]["ok"] is False and d2["ipc_live_check"]["checks"] == 1, d2["ipc_live_check"]


def test_ipc_allreduce_stress_ranks_share_one_gpu():
    """The training pattern on the peer all-reduce, 300 times with new data each time (a kernel on
    the compute stream rewrites the registered arena, the collective runs right behind it, the next
    iteration overlaps): every sum exact (tests/ipc_stress_worker.py)."""
    from distributed_pytorch_amd.parallel.spawn import free_port

    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "ipc_stress_worker.py")]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", DPA_IPC_STRESS_ITERS="300")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "DPA_STORE_PORT"):
        env.pop(k, None)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = [json.loads(l) for l in r.stdout.replace("}{", "}\n{").splitlines() if l.startswith("{")]
    assert len(rows) == 4 and all(d["bad_iters"] == 0 and not d["timeout"] for d in rows), rows


def _w4_checksums(comm, runs=3):
    sums = []
    for _ in range(runs):
        d = _bench(["--gpus", "4", "--comm", comm, "--mode", "ddp", "--steps", "3", "--warmup", "2",
                    "--solo-steps", "0", "--diag-steps", "0", "--batch", "64", "--comm-tune", "off"])
        assert d["replicas_identical"] is True, d
        sums.append(d["param_checksum"])
    return sums


@pytest.mark.parametrize("comm", ["gloo", "ipc"])
def test_four_rank_training_run_to_run(comm):
    """Four processes on one GPU, three runs of the same seed: bitwise the same parameters (the
    round-5 open issue, fixed in round 6 -- module docstring)."""
    sums = _w4_checksums(comm)
    assert len(set(sums)) == 1, sums
