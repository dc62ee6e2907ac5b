"""--optimizer lars on the flat buffers (the definition: docs/ACCURACY.md).

* `lars_update_`: the definition for one tensor in torch, at the dtype of its
  arguments - the CPU / oracle engines' update (fp32) and, on float64 copies,
  the reference the GPU tests hold the kernels to.
* `lars_table`: the segment table of csrc/kernels/lars.h, checked here because
  the kernels trust it.
* `LarsState`: what one engine keeps on the device (table, per-chunk sums,
  `ratio`), allocated once so the two launches of a step capture into a graph.
"""

from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

from .. import config as C
from ..ops import native, ptr, stream_handle
from ..parallel.flat import ALIGN, FlatLayout


def adapted(spec) -> bool:
    """LARS adapts the tensors with two or more axes (conv and FC weights);
    biases and BatchNorm scale / shift step at r = 1 with no weight decay."""
    return len(spec.shape) >= 2


def lars_update_(w: torch.Tensor, g: torch.Tensor, m: torch.Tensor, adapt: bool,
                 opt: C.OptimizerSpec, lr, mu, gscale=1.0, r=None):
    """One tensor's step in place on w and m; returns its trust ratio.  `r`
    given: used as it is (the kernel's ratio as the operand of the update)."""
    g = g * gscale
    if r is None:
        nw, ng = w.norm(), g.norm()
        r = opt.eta * nw / (ng + opt.wd * nw) if adapt and nw > 0 and ng > 0 else 1.0
    u = r * (g + opt.wd * w) if adapt else g
    m.mul_(mu).add_(u)
    w.sub_(lr * (u + mu * m if opt.nesterov else m))
    return r


def lars_table(segments: Sequence[Tuple[int, int, bool]]) -> Tuple[List[List[int]], int]:
    """(offset, numel, adapted) per tensor -> the table rows {offset, numel,
    adapted, first chunk, nchunks} and the chunk total."""
    chunk = native().optim.LARS_CHUNK
    rows, first, end = [], 0, 0
    for off, n, ad in segments:
        if off % ALIGN or off < end or n < 1:
            raise ValueError(f"lars segment (offset {off}, numel {n}) must start on a {ALIGN}-float "
                             f"boundary at or after the previous one's end ({end}) and hold a float")
        nc = -(-n // chunk)
        rows.append([off, n, int(bool(ad)), first, nc])
        first, end = first + nc, off + n
    if not rows:
        raise ValueError("lars needs at least one tensor")
    return rows, first


class LarsState:
    def __init__(self, segments: Sequence[Tuple[int, int, bool]], opt: C.OptimizerSpec,
                 device: torch.device):
        rows, self.nchunks = lars_table(segments)
        self.opt, self.ntensors = opt, len(rows)
        self.extent = rows[-1][0] + rows[-1][1]  # floats of the flat buffers the table covers
        self.table = torch.tensor(rows, dtype=torch.int64).to(device)
        self.part = torch.zeros(self.nchunks, 2).to(device)
        self.ratio = torch.ones(self.ntensors).to(device)

    @classmethod
    def for_layout(cls, layout: FlatLayout, opt: C.OptimizerSpec, device: torch.device):
        return cls([(layout.offsets[s.name], s.numel, adapted(s)) for s in layout.specs], opt,
                   device)

    def step(self, w: torch.Tensor, g: torch.Tensor, mom: torch.Tensor, momentum: float,
             gscale: float, lr: torch.Tensor, step: torch.Tensor) -> None:
        """Both launches on the current stream: w, mom and `ratio` updated at the
        device LR `lr`, the device step counter `step` advanced by one."""
        for t in (w, g, mom):
            if (t.dtype != torch.float32 or t.device != self.table.device or not t.is_contiguous()
                    or t.numel() < self.extent):
                raise ValueError(f"lars step: needs contiguous fp32 buffers of at least "
                                 f"{self.extent} floats on {self.table.device}")
        o = self.opt
        native().optim.lars_step(ptr(w), ptr(g), ptr(mom), ptr(self.table), self.ntensors,
                                 self.nchunks, ptr(self.part), ptr(self.ratio), o.eta, o.wd,
                                 o.nesterov, momentum, gscale, ptr(lr), ptr(step), stream_handle())
