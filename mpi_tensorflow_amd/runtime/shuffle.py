"""Per-pass shuffled (--shuffle) and augmented (--augment) training batches:
the pass bookkeeping the engines share.

The step kernels, the executors and the captured graphs read the batch of
step s at `batch_offset(s)` of the engine's device-resident shard and know
nothing of shuffling.  With shuffle on, the engine keeps a pristine copy of
its shard beside that working copy, and the rows of pass p = `pass_of(s)`
(the wrap period of the offset) are the pristine rows in the order
`rng.shuffle_perm(rng.shuffle_key(seed, rank, p), n_local)`: loading a pass
rewrites the working copy in place - one `shuffle_rows` launch on the compute
stream (csrc/kernels/shuffle.hip; the permutation is computed in the kernel)
or, on the PyTorch paths, an index with the host permutation.  The pointers
never change, the order is a pure function of the step (a resumed run needs no
extra state), and each rank permutes inside its own shard with its own key.

With augment on, the same load also shifts and flips every image
(`rng.augment_params` / `rng.augment_np` are the definition): the draw of a row
is a pure function of (seed, rank, pass, pristine row index), so it means the
same with and without shuffle, pass 0 included.  On the native path the load
stays one launch (`augment_rows`, csrc/kernels/augment.hip: the gather and the
transform in one pass over the shard); with augment alone the order is the
file order.

A spec with rotate, scale or cutout takes the affine load instead: the same
draw chain continued (`rng.affine_params`), a per-row inverse affine map with
bilinear sampling (`rng.affine_np` is the definition), still one launch
(`affine_rows`), reading one 3 x 129 int32 table uploaded at construction.
Specs without those items keep the shift / flip load unchanged.

With mix on (--mix mixup:M / cutmix:M) the pass as loaded above is blended row
by row with partner rows of the same pass (`rng.mix_params` / `rng.mix_np` are
the definition; the draw of a row is a pure function of (seed, rank, pass,
working row index)).  The loader then writes a staging copy (`mid_x` /
`mid_y`; with neither shuffle nor augment the pristine copy itself serves) and
one `mix_rows` launch writes the working copy together with `work_y2` (the
partner's label) and `work_lam` (the row's own share), which the soft-target
loss reads beside `work_y`.
"""

from __future__ import annotations

from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from ..utils import rng
from ..utils.data import batch_offset, pass_of


def batch_rows(seed: int, rank: int, step: int, n_local: int, batch: int) -> np.ndarray:
    """Shard rows (pristine order) of the batch of step `step` with shuffle on."""
    perm = rng.shuffle_perm(rng.shuffle_key(seed, rank, pass_of(step, n_local, batch)), n_local)
    off = batch_offset(step, n_local, batch)
    return perm[off:off + batch]


class PassShuffler:
    """Keeps `work_x` / `work_y` (the tensors the step reads; only their first
    `n_local` rows are touched, rows past them are the any-batch-size pad) in
    the order of one pass.  `native`: the extension module for the HIP path,
    which rewrites the tensors passed in; None for the PyTorch path, which
    leaves them untouched and hands out a working copy of its own
    (`work_x` / `work_y`: the engine reads those instead).

    `augment`: None or (K, flip, fill, (H, W, C)), the per-pass shift / flip of
    the NHWC images, or (config.AugmentSpec, (H, W, C)) for a spec with rotate,
    scale or cutout (held as `affine`); `shuffle=False` keeps the file order
    (augment only)."""

    def __init__(self, seed: int, rank: int, n_local: int, batch: int, work_x: torch.Tensor,
                 work_y: torch.Tensor, native=None, augment=None, shuffle: bool = True,
                 mix=None):
        self.seed, self.rank, self.n, self.B = int(seed), int(rank), int(n_local), int(batch)
        self.shuffle = bool(shuffle)
        self.augment = None
        self.affine = None  # (spec, (H, W, C)) with rotate / scale / cutout in the spec
        self.tables = None  # ... and rng.affine_tables of it, uploaded once on the native path
        if augment is not None:
            spec = augment[0] if len(augment) == 2 else None
            K, flip, fill = (spec.K, spec.flip, spec.fill) if spec is not None else augment[:3]
            H, W, C = (int(v) for v in augment[-1])
            K = int(K)
            if K < 0 or K >= min(H, W):
                raise ValueError(f"augment shift {K} must be below min(H, W) = {min(H, W)}")
            if tuple(work_x.shape[1:]) != (H, W, C):
                raise ValueError(f"augment: rows of shape {tuple(work_x.shape[1:])}, images "
                                 f"{(H, W, C)}")
            if spec is not None and spec.affine:
                if spec.cutout >= min(H, W):
                    raise ValueError(f"augment cutout {spec.cutout} must be below min(H, W) = "
                                     f"{min(H, W)}")
                self.affine = (spec, (H, W, C))
                self.tables = rng.affine_tables(spec.rotate, spec.scale)
                if native is not None:
                    self.tables = torch.from_numpy(self.tables).to(work_x.device)
            elif K > 0 or flip:
                self.augment = (K, bool(flip), float(fill), (H, W, C))
        if native is not None:  # the executors hold the pointers of the working copy
            self.work_x, self.work_y = work_x, work_y
            self.src_x = work_x[:self.n].clone()
            self.src_y = work_y[:self.n].clone()
        else:  # a host tensor may alias the caller's array: it stays the pristine copy
            self.src_x, self.src_y = work_x[:self.n], work_y[:self.n]
            self.work_x, self.work_y = work_x.clone(), work_y.clone()
        self.row_elems = int(np.prod(work_x.shape[1:]))
        self._C = native
        if native is not None and (work_x.dtype != torch.float32 or work_y.dtype != torch.int32):
            raise TypeError("shuffle_rows moves fp32 rows and int32 labels")
        # mix = (kind, M): every loaded pass blended with partner rows; work_y2 /
        # work_lam have the rows of work_y (pad rows: label 0, share 1)
        self.mix = None
        self.mix_table = None
        self.work_y2 = self.work_lam = None
        self.mid_x, self.mid_y = self.src_x, self.src_y
        if mix is not None:
            kind, M = mix
            if work_x.dim() != 4:
                raise ValueError(f"mix: rows of shape {tuple(work_x.shape[1:])} are not images")
            H, W, C = (int(v) for v in work_x.shape[1:])
            self.mix = (str(kind), float(M), (H, W, C))
            self.mix_table = rng.mix_table(kind, M, H, W)
            self.work_y2 = torch.zeros_like(self.work_y)
            self.work_lam = torch.ones(self.work_y.shape[0], dtype=torch.float32,
                                       device=self.work_y.device)
            if native is not None:
                self.mix_table = torch.from_numpy(self.mix_table).to(work_x.device)
                if self.shuffle or self.augment is not None or self.affine is not None:
                    self.mid_x = torch.empty_like(self.src_x)
                    self.mid_y = torch.empty_like(self.src_y)
        self.loaded: Optional[int] = None  # the pass the working copy holds

    def key(self, p: int) -> int:
        return rng.shuffle_key(self.seed, self.rank, p)

    def perm(self, p: int) -> np.ndarray:
        """Pristine row of every working row in pass p."""
        return rng.shuffle_perm(self.key(p), self.n) if self.shuffle else np.arange(self.n)

    def augment_key(self, p: int) -> int:
        return rng.augment_key(self.seed, self.rank, p)

    def mix_key(self, p: int) -> int:
        return rng.mix_key(self.seed, self.rank, p)

    def mix_params(self, p: int):
        """The mix draws of pass p (rng.mix_params)."""
        _, _, (H, W, _) = self.mix
        table = self.mix_table.cpu().numpy() if torch.is_tensor(self.mix_table) else self.mix_table
        return rng.mix_params(self.mix_key(p), self.n, table, H, W)

    def load(self, p: int) -> None:
        """Working copy := pristine rows in the order, and with the draws, of
        pass p, on the current stream (idempotent)."""
        if p == self.loaded:
            return
        if self._C is not None:
            from ..ops import ptr, stream_handle
            # with mix the loader fills the staging copy and mix_rows the working one
            out_x, out_y = ((self.work_x, self.work_y) if self.mix is None
                            else (self.mid_x, self.mid_y))
            if self.mix is not None and self.mid_x is self.src_x:  # mix alone: no staging load
                pass
            elif self.affine is not None:
                spec, (H, W, C) = self.affine
                self._C.ops.affine_rows(ptr(self.src_x), ptr(self.src_y), ptr(out_x),
                                        ptr(out_y), self.n, H, W, C, self.shuffle,
                                        self.key(p) if self.shuffle else 0, self.augment_key(p),
                                        spec.K, spec.flip, spec.fill, ptr(self.tables),
                                        spec.cutout, stream_handle())
            elif self.augment is None:
                self._C.ops.shuffle_rows(ptr(self.src_x), ptr(self.src_y), ptr(out_x),
                                         ptr(out_y), self.n, self.row_elems, self.key(p),
                                         stream_handle())
            else:
                K, flip, fill, (H, W, C) = self.augment
                self._C.ops.augment_rows(ptr(self.src_x), ptr(self.src_y), ptr(out_x),
                                         ptr(out_y), self.n, H, W, C, self.shuffle,
                                         self.key(p) if self.shuffle else 0, self.augment_key(p),
                                         K, flip, fill, stream_handle())
            if self.mix is not None:
                kind, _, (H, W, C) = self.mix
                self._C.ops.mix_rows(ptr(self.mid_x), ptr(self.mid_y), ptr(self.work_x),
                                     ptr(self.work_y), ptr(self.work_y2), ptr(self.work_lam),
                                     self.n, H, W, C, kind == "cutmix", self.mix_key(p),
                                     ptr(self.mix_table), stream_handle())
        else:
            rows = self.perm(p)
            x, y = self.src_x, self.src_y
            if self.shuffle:
                idx = torch.from_numpy(rows).to(self.work_x.device)
                x, y = x[idx], y[idx]
            if self.affine is not None:
                spec, (H, W, _) = self.affine
                q = rng.affine_params(self.augment_key(p), rows, spec, H, W, self.tables)
                x = rng.affine_torch(x, q.m, q.dy, q.dx, q.flipped, spec.fill, q.cutout)
            elif self.augment is not None:
                K, flip, fill, _ = self.augment
                x = rng.augment_torch(x, *rng.augment_params(self.augment_key(p), rows, K, flip),
                                      fill)
            if self.mix is not None:
                x, y, y2, lam = rng.mix_torch(x, y, self.mix_params(p), self.mix[0])
                self.work_y2[:self.n] = y2
                self.work_lam[:self.n] = lam
            self.work_x[:self.n] = x
            self.work_y[:self.n] = y
        self.loaded = p

    def ensure(self, step: int) -> None:
        """The working copy holds the order the batch of `step` is read in."""
        self.load(pass_of(step, self.n, self.B))

    def segments(self, step: int, k: int) -> Iterator[Tuple[int, int]]:
        """Cuts the k steps from `step` at the pass boundaries: (pass, steps)."""
        while k > 0:
            p = pass_of(step, self.n, self.B)
            # first step of pass p + 1: the smallest s with s * B >= (p + 1) * (n - B)
            nxt = -(-(p + 1) * (self.n - self.B) // self.B)
            m = min(k, nxt - step)
            yield p, m
            step += m
            k -= m


def make_shuffler(cfg, rank: int, n_local: int, work_x: torch.Tensor, work_y: torch.Tensor,
                  native=None, image_shape=None) -> Optional[PassShuffler]:
    """The engine's shuffler, or None (nothing allocated) with shuffle,
    augment and mix off.  `rank` is the rank of the engine's dropout stream (0 under
    quirk Q14); `image_shape`: (H, W, C) of a row, which augment needs."""
    shuffle = bool(getattr(cfg, "shuffle", False))
    spec = getattr(cfg, "augment", None)
    mix = getattr(cfg, "mix", None)
    if not shuffle and spec is None and mix is None:
        return None
    if mix is not None:
        from ..config import parse_mix
        mix = parse_mix(mix)
    augment = None
    if spec is not None:
        from ..config import parse_augment_spec
        if image_shape is None:
            raise ValueError("augment needs the image shape of the shard's rows")
        s, shape = parse_augment_spec(spec, cfg.model), tuple(int(v) for v in image_shape)
        augment = (s, shape) if s.affine else (s.K, s.flip, s.fill, shape)
    return PassShuffler(cfg.seed, rank, n_local, cfg.batch_size, work_x, work_y, native,
                        augment=augment, shuffle=shuffle, mix=mix)
