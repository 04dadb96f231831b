"""FlatUpdate — the parameter update over flat fp32 arenas, shared by ``VGGEngine`` and
``parallel.ddp.FlatSGD``: one place for the choice of launches and for the state they need.

  plain SGD                 sgd_flat over the arena or a slice of it (one launch)
  LARS / gradient clipping  sqnorm_partials → lars_finalize → sgd_segmented over the whole arena
                            (three launches, kernels/lars.hip), on workspaces built once
  learning-rate schedule    ``advance()`` first (lr_advance, kernels/lr_sched.hip): the step's rate
                            from the table into the word ``lr_dev``, which the same update functions
                            then take as their rate in place of a float

The backend ``K`` is the native extension or :mod:`~distributed_pytorch_amd.ops.cpu_ref` (same
names, same signatures); the schedule's tensors live on the arena's device under either.
"""
from __future__ import annotations

from typing import Iterable, Optional, Tuple

import torch

from .schedule import as_table, table_spec
from .utils.arena import block_map

SCHEDULE_TENSORS = ("table_dev", "step_dev", "lr_dev")


class FlatUpdate:
    """``segments`` (``(offset, padded length, ndim)`` per tensor, ``Arena.segments()``) makes the
    update the whole-arena one: ``adapt`` puts a LARS trust ratio (``trust_coef``, ``lars_eps``) on
    every tensor of rank >= 2, ``clip_grad_norm`` > 0 clips the global gradient norm.  ``like``: the
    parameter arena (device and dtype of the workspaces)."""

    def __init__(self, K, like: torch.Tensor, segments: Optional[Iterable[Tuple[int, int, int]]] = None,
                 adapt: bool = False, trust_coef: float = 0.0, clip_grad_norm: float = 0.0, lars_eps: float = 1e-9):
        self.K, self.like = K, like
        self.trust_coef, self.clip_grad_norm, self.lars_eps = trust_coef, clip_grad_norm, lars_eps
        self.spec: Optional[dict] = None  # of the schedule; SCHEDULE_TENSORS exist only while one is set
        self.whole_arena = segments is not None
        if self.whole_arena:
            dev = like.device
            self.bmap, self.segs = block_map(segments, int(K.OPT_CHUNK), adapt, dev)
            nseg = self.segs.shape[0]
            self.partials = torch.zeros(self.bmap.shape[0], 2, dtype=torch.float64, device=dev)
            # trust ratio per segment, then the gradient multiplier (an oracle run on an arena of
            # another precision keeps them in that precision)
            self.table = torch.ones(nseg + 1, dtype=like.dtype, device=dev)
            self.norms = torch.zeros(2 * nseg + 2, dtype=torch.float64, device=dev)

    # ------------------------------------------------------------------ schedule
    def set_schedule(self, table, spec: Optional[dict] = None) -> None:
        """A float32 rate table indexed by the global update step (``schedule.lr_table``; steps at
        or past its end hold the last value), uploaded once; ``None`` clears the schedule."""
        for a in SCHEDULE_TENSORS:
            self.__dict__.pop(a, None)
        self.spec = None
        if table is None:
            return
        tab = as_table(table)
        self.spec = table_spec(table, spec)
        dev = self.like.device
        self.table_dev = torch.from_numpy(tab.copy()).to(dev)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self.lr_dev = self.table_dev[:1].clone()

    def advance(self, host_step: int) -> None:
        """First launch of a scheduled step: lr_dev = table[min(step, T - 1)].  Eager: the step is
        the host's count (it stays the single truth, so whatever restores it -- a checkpoint, the
        comm tuner -- moves the schedule with it).  Under capture: the device counter, so that
        every replay advances by itself (GraphedStep seeds it)."""
        from_device = self.like.is_cuda and torch.cuda.is_current_stream_capturing()
        self.K.lr_advance(self.table_dev, self.step_dev, self.lr_dev, host_step, from_device)

    def current_lr(self) -> float:
        """The scheduled rate of the most recent step (synchronises); before the first: table[0]."""
        return float(self.lr_dev.item())

    def lr_position(self) -> int:
        """The schedule's step counter (synchronises): the number of scheduled steps begun, counted
        from the global step 0."""
        if self.spec is None:
            raise ValueError("lr_position: no learning-rate schedule is set")
        return int(self.step_dev.item())

    # ------------------------------------------------------------------ update
    def update(self, p, g, buf, lr: float, momentum: float, weight_decay: float, grad_scale: float, first: bool,
               offset: int = 0, count: int = -1, planes=None) -> None:
        """One update of p / buf (and the operand planes) from g.  ``lr`` is the constant rate; under
        a schedule the word that ``advance`` wrote replaces it."""
        K = self.K
        if self.spec is not None:
            lr = self.lr_dev
        if not self.whole_arena:
            K.sgd_flat(p, g, buf, lr, momentum, weight_decay, grad_scale, first, offset, count, planes)
            return
        if offset != 0 or (count >= 0 and count != p.numel()):
            raise ValueError("sgd_step: LARS / gradient clipping update the whole arena (the norms of a "
                             f"slice are not defined); got offset={offset}, count={count}")
        K.sqnorm_partials(p, g, self.bmap, self.partials, self.segs.shape[0])
        K.lars_finalize(self.partials, self.segs, self.table, self.norms, grad_scale, self.clip_grad_norm,
                        self.trust_coef, weight_decay, self.lars_eps)
        K.sgd_segmented(p, g, buf, self.bmap, self.table, lr, momentum, weight_decay, first, planes)

    def stats(self) -> dict:
        """The last whole-arena update's norms as Python values (synchronises): ``grad_norm`` (of
        the scaled gradient, before clipping), ``clip_coef``, and per segment ``p_norm``, ``g_norm``
        and ``trust_ratio``."""
        if not self.whole_arena:
            raise ValueError("opt_stats: the update is plain SGD (no LARS, no gradient clipping)")
        st, tb = self.norms.cpu().tolist(), self.table.cpu().tolist()
        S = self.segs.shape[0]
        return {"grad_norm": st[2 * S], "clip_coef": st[2 * S + 1], "p_norm": st[:S], "g_norm": st[S:2 * S],
                "trust_ratio": tb[:S]}


class ScheduleTensors:
    """For the owner of a FlatUpdate ``self.upd``: the schedule's tensors under the owner's own
    ``table_dev`` / ``step_dev`` / ``lr_dev`` while a schedule is set, and no such attribute when
    none is."""

    def __getattr__(self, name):
        if name in SCHEDULE_TENSORS and "upd" in self.__dict__:
            return getattr(self.__dict__["upd"], name)
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")
