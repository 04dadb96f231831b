"""Learning-rate schedules as a host-built table.

``lr_table`` evaluates warmup + decay in Python floats (fp64) for every global update step
``t = 0 .. total_iters - 1`` and rounds each value ONCE to float32.  The device never evaluates a
schedule formula: ``lr_advance`` (kernels/lr_sched.hip) reads ``table[min(t, T - 1)]`` into a
device-resident rate that the update kernels read, so the rate is bitwise the host's on the CPU
oracle and on the GPU, and a captured step follows it from replay to replay.

With ``W = warmup_iters``, ``F = warmup_factor``, ``T = total_iters``::

    t <  W : lr = base * (F + (1 - F) * t / W)                     (torch LinearLR, 0 < F <= 1)
    t >= W : u = (t - W) / max(T - W, 1)
      constant : base
      poly     : end + (base - end) * (1 - u) ** power             (power 1: linear; LARS paper: 2)
      cosine   : end + (base - end) * 0.5 * (1 + cos(pi * u))
      step     : base * gamma ** #{m in milestones : t >= m}       (milestones: absolute iterations)

Steps at or past ``T`` hold ``table[T - 1]`` (``lr_at``; the kernel clamps the same way).
"""
from __future__ import annotations

import math
import zlib
from typing import Optional, Sequence

import numpy as np

DECAYS = ("constant", "poly", "cosine", "step")


class LRTable(np.ndarray):
    """float32 [T] with the ``spec`` dict of the arguments that built it (plain ints, floats,
    strings and lists: what a checkpoint stores and the metrics line prints)."""

    spec: Optional[dict] = None

    def __array_finalize__(self, obj):
        self.spec = None  # a slice or a copy is another table: the arguments no longer describe it


def lr_table(base_lr: float, total_iters: int, warmup_iters: int = 0, warmup_factor: float = 0.1,
             decay: str = "constant", power: float = 2.0, end_lr: float = 0.0, milestones: Sequence[int] = (),
             gamma: float = 0.1) -> LRTable:
    T, W, F = int(total_iters), int(warmup_iters), float(warmup_factor)
    base, end, power, gamma = float(base_lr), float(end_lr), float(power), float(gamma)
    ms = [int(m) for m in milestones]
    if T < 1:
        raise ValueError(f"lr_table: total_iters must be >= 1, got {total_iters}")
    if W < 0:
        raise ValueError(f"lr_table: warmup_iters must be >= 0, got {warmup_iters}")
    if decay not in DECAYS:
        raise ValueError(f"lr_table: decay must be one of {DECAYS}, got {decay!r}")
    if W >= T and decay != "constant":
        raise ValueError(f"lr_table: warmup_iters {W} leaves no iteration of {T} for the {decay} decay")
    if not 0.0 < F <= 1.0:
        raise ValueError(f"lr_table: warmup_factor must be in (0, 1], got {warmup_factor}")
    if not gamma > 0.0:
        raise ValueError(f"lr_table: gamma must be > 0, got {gamma}")
    if not end >= 0.0:
        raise ValueError(f"lr_table: end_lr must be >= 0, got {end_lr}")
    if any(b < a for a, b in zip(ms, ms[1:])):
        raise ValueError(f"lr_table: milestones must be sorted, got {list(milestones)}")
    vals = []
    span = max(T - W, 1)
    for t in range(T):
        if t < W:
            v = base * (F + (1.0 - F) * t / W)
        elif decay == "constant":
            v = base
        elif decay == "poly":
            v = end + (base - end) * (1.0 - (t - W) / span) ** power
        elif decay == "cosine":
            v = end + (base - end) * 0.5 * (1.0 + math.cos(math.pi * ((t - W) / span)))
        else:
            v = base * gamma ** sum(1 for m in ms if t >= m)
        vals.append(v)
    out = np.asarray(vals, dtype=np.float64).astype(np.float32).view(LRTable)
    out.spec = {"base_lr": base, "total_iters": T, "warmup_iters": W, "warmup_factor": F, "decay": decay,
                "power": power, "end_lr": end, "milestones": ms, "gamma": gamma}
    return out


def lr_at(table, t: int) -> float:
    """The rate of global step t: ``table[min(t, T - 1)]`` as a Python float."""
    return float(table[min(max(int(t), 0), len(table) - 1)])


def as_table(table) -> np.ndarray:
    """A schedule given as an ``lr_table``, a float32 array or a 1-D tensor -> float32 [T >= 1]."""
    if hasattr(table, "detach"):
        table = table.detach().cpu().numpy()
    a = np.asarray(table)
    if a.dtype != np.float32 or a.ndim != 1 or a.shape[0] < 1:
        raise ValueError("learning-rate table must be float32 [T] with T >= 1 (schedule.lr_table builds one)")
    return np.ascontiguousarray(a)


def table_spec(table, spec: Optional[dict] = None) -> dict:
    """The spec that travels with a table: the one given, else the table's own (``lr_table``), else
    its length and checksum (a hand-made table)."""
    if spec is None:
        spec = getattr(table, "spec", None)
    if spec is None:
        a = as_table(table)
        spec = {"decay": "table", "total_iters": int(a.shape[0]), "crc32": int(zlib.crc32(a.tobytes()))}
    return dict(spec)


def table_from_args(args, iters_per_epoch: int) -> Optional[LRTable]:
    """The command line's schedule (train.add_common_args), or None when neither ``--lr-schedule``
    nor ``--warmup-iters`` is given.  ``--lr-milestones`` are epochs; ``iters_per_epoch`` is this
    rank's iterations per epoch."""
    decay = getattr(args, "lr_schedule", None)
    warm = int(getattr(args, "warmup_iters", 0) or 0)
    if decay is None and warm <= 0:
        return None
    ms = getattr(args, "lr_milestones", None) or ""
    try:
        epochs = [float(s) for s in str(ms).split(",") if s.strip()]
    except ValueError:
        raise ValueError(f"--lr-milestones must be comma-separated epochs, got {ms!r}") from None
    return lr_table(args.lr, int(args.epochs) * int(iters_per_epoch), warm, getattr(args, "warmup_factor", 0.1),
                    decay or "constant", getattr(args, "lr_power", 2.0), getattr(args, "lr_end", 0.0),
                    [int(round(e * iters_per_epoch)) for e in epochs], getattr(args, "lr_gamma", 0.1))
