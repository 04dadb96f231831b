"""Flat arenas: many named tensors packed into ONE contiguous buffer.

Parameters, gradients and momentum live in three arenas with identical layouts, so the fused
SGD kernel is one launch over the whole model, DDP buckets are plain contiguous slices (no
``copy_bucket_to_grad``), and gather/broadcast move one buffer (SURVEY §7.1 "Flat parameter/grad
arenas").  Each entry starts on a 64-element (256 B) boundary so every view is float4-aligned.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Iterable, List, Tuple

import torch

ALIGN = 64


class Arena:
    def __init__(self, entries: Iterable[Tuple[str, Tuple[int, ...]]], device, dtype=torch.float32, align=ALIGN):
        self.shapes: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
        self.offsets: Dict[str, int] = {}
        self.numels: Dict[str, int] = {}
        off = 0
        for name, shape in entries:
            n = 1
            for s in shape:
                n *= int(s)
            self.shapes[name] = tuple(int(s) for s in shape)
            self.offsets[name] = off
            self.numels[name] = n
            off += (n + align - 1) // align * align
        self.numel = off
        self.device = torch.device(device)
        self.dtype = dtype
        self.flat = torch.zeros(max(off, align), device=device, dtype=dtype)
        self.views: "OrderedDict[str, torch.Tensor]" = OrderedDict(
            (k, self.flat[self.offsets[k]:self.offsets[k] + self.numels[k]].view(self.shapes[k])) for k in self.shapes)

    def like(self) -> "Arena":
        """A zero-initialised arena with the same layout."""
        return Arena(self.shapes.items(), self.device, self.dtype)

    def names(self) -> List[str]:
        return list(self.shapes.keys())

    def span(self, names: Iterable[str]) -> Tuple[int, int]:
        """[start, end) element range covering the given (adjacent) entries, padded ends included."""
        names = list(names)
        lo = min(self.offsets[n] for n in names)
        hi = max(self.offsets[n] + (self.numels[n] + ALIGN - 1) // ALIGN * ALIGN for n in names)
        return lo, hi

    def segments(self) -> List[Tuple[int, int, int]]:
        """The segment table in arena order: (offset, padded extent, tensor rank) per entry.  The
        segments tile ``[0, numel)``; the padding is part of its entry's segment."""
        return [(self.offsets[k], (self.numels[k] + ALIGN - 1) // ALIGN * ALIGN, len(self.shapes[k]))
                for k in self.shapes]

    def __getitem__(self, name: str) -> torch.Tensor:
        return self.views[name]

    def __contains__(self, name: str) -> bool:
        return name in self.views


def block_map(segments: Iterable[Tuple[int, int, int]], chunk: int, adapt: bool, device=None):
    """The optimizer's block map of an arena (ops: sqnorm_partials / lars_finalize / sgd_segmented).

    ``segments``: (offset, padded extent, tensor rank) per entry, ascending and disjoint.  Each
    segment is cut into chunks of at most ``chunk`` elements (the last one may be shorter; every
    length is a multiple of 64).  Returns two int64 tensors on ``device``:

    * ``bmap [nblocks, 3]``: (segment, start, length) of every chunk;
    * ``segs [nseg, 3]``: (first chunk, chunks, adapted) of every segment, where a segment is
      adapted (gets a LARS trust ratio) when ``adapt`` is set and its tensor has rank >= 2.
    """
    if chunk <= 0 or chunk % ALIGN:
        raise ValueError(f"block_map: chunk must be a positive multiple of {ALIGN}")
    bmap, segs, end = [], [], 0
    for s, (off, ext, rank) in enumerate(segments):
        if off < end or off % ALIGN or ext <= 0 or ext % ALIGN:
            raise ValueError(f"block_map: segment {s} (offset {off}, extent {ext}) is not an aligned, ascending range")
        end = off + ext
        first = len(bmap)
        for start in range(off, end, chunk):
            bmap.append((s, start, min(chunk, end - start)))
        segs.append((first, len(bmap) - first, 1 if adapt and rank >= 2 else 0))
    if not segs:
        raise ValueError("block_map: no segments")
    return (torch.tensor(bmap, dtype=torch.int64, device=device).reshape(-1, 3),
            torch.tensor(segs, dtype=torch.int64, device=device).reshape(-1, 3))
