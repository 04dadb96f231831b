"""Gradient accumulation: one optimizer update per group of ``A = accum_steps`` loader batches.

The loader batches of an epoch form groups in index order, ``[0..A-1]``, ``[A..2A-1]``, ...; a group
ends after ``A`` batches, at the end of the epoch or at ``--max-iters``, whichever comes first, so
its length is ``a <= A``.  With micro-batch gradients ``g_0 .. g_{a-1}`` (each the mean over its own
micro-batch)::

    micro-step k < a-1 :  forward + backward, then   acc = g_0          (k = 0, "store")
                                                     acc = acc + g_k    (k > 0, "add")
                          no collective of any kind, no update, no BN-buffer broadcast
    micro-step a-1     :  forward + backward, then   g = acc + g_{a-1}  ("merge", skipped when a = 1)
                          then the mode's ordinary sync of g and the ordinary update with
                          grad_scale = sync_scale / a

The folds are plain fp32 additions in that fixed order (kernels/grad_fold.hip, one launch per bucket
from the sync strategy's ``grad_ready``, under the rest of the backward).  BN running statistics
advance on every micro-step; ``steps_taken`` -- the momentum's first-step flag, the schedule's
position, the health step number -- counts updates.  A short group weighs each of its micro-batches
by ``1 / a``, and a partial last loader batch weighs as much as a full one.
"""
from __future__ import annotations

import torch

from .utils.profiling import trace_range


def updates_per_epoch(n_batches: int, max_iters, accum_steps: int) -> int:
    """Optimizer updates of one epoch: ``ceil(min(n_batches, max_iters) / accum_steps)`` -- what a
    learning-rate schedule's length and ``--warmup-iters`` count."""
    n = min(int(n_batches), int(max_iters)) if max_iters else int(n_batches)
    a = int(accum_steps)
    return (n + a - 1) // a


def validate_args(args) -> int:
    """The command line's ``--accum-steps`` checked against the options it constrains; returns it.
    Touches no device."""
    a = getattr(args, "accum_steps", 1)
    a = 1 if a is None else int(a)
    if a < 1:
        raise ValueError(f"--accum-steps must be >= 1, got {a}")
    if a == 1:
        return a
    every = getattr(args, "checkpoint_every", 0) or 0
    if every % a:
        raise ValueError(f"--checkpoint-every {every} is not a multiple of --accum-steps {a}: a checkpoint is "
                         "taken only where a group of micro-batches ends")
    stop = getattr(args, "stop_after_iters", None)
    if stop and stop % a:
        raise ValueError(f"--stop-after-iters {stop} is not a multiple of --accum-steps {a}: a run stops only "
                         "where a group of micro-batches ends")
    if getattr(args, "graph", False):
        raise ValueError("--graph with --accum-steps > 1: a captured accumulated step is not implemented")
    return a


class AccumulatedStep:
    """Drives ``engine`` and ``sync`` through groups of ``accum_steps`` micro-steps.  ``run`` counts
    the position inside the group; ``last=True`` closes a short group.  After the closing micro-step
    it calls ``sync.update(scale / a)`` and ``engine.finish_step()``."""

    def __init__(self, engine, sync, accum_steps: int):
        if int(accum_steps) < 1:
            raise ValueError(f"accum_steps must be >= 1, got {accum_steps}")
        self.engine, self.sync = engine, sync
        self.accum_steps = int(accum_steps)
        self.pos = 0  # micro-steps of the open group already folded
        if self.accum_steps > 1:
            sync.accumulate(self.accum_steps)

    def run(self, x: torch.Tensor, target: torch.Tensor, last: bool = False) -> bool:
        """One micro-step on a loader batch; returns True when it closed its group (an update ran)."""
        e, s = self.engine, self.sync
        closing = last or self.pos == self.accum_steps - 1
        with trace_range("step" if closing else "micro_step"):
            if not closing:
                s.begin_micro_step(first=self.pos == 0)
                with trace_range("fwd_bwd"):
                    e.forward_backward(x, target, grad_ready=s.grad_ready, pre_forward=s.pre_forward,
                                       params_free=s.params_free)
                s.finish_micro_step()
                e.finish_micro_step()
                self.pos += 1
                return False
            a = self.pos + 1
            if a == 1:
                s.begin_step()  # a group of one: an ordinary step, nothing folded
            else:
                s.begin_final_step()
            with trace_range("fwd_bwd"):
                e.forward_backward(x, target, grad_ready=s.grad_ready, pre_forward=s.pre_forward,
                                   params_free=s.params_free)
            with trace_range("sync"):
                gscale = s.finish()
            with trace_range("sgd"):
                s.update(gscale / a)
            e.finish_step()
            self.pos = 0
            return True
