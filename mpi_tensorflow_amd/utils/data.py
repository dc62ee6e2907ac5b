"""Data layer: acquisition, sizing/splitting, per-rank sharding, synthetic data.

Reference behaviour (`/root/reference/mpipy.py`):
  * `data_exist_here` (`:185-199`) creates ./data and downloads missing MNIST
    files; every rank calls it concurrently (quirk Q3) and the error handler
    names an undefined exception (Q4).
  * sizing (`:211-213`): tr_size = 55000//P*P, ts_size = 10000//P*P,
    val_size = 5000//P*P.
  * rank 0 reads 60000 train + ts_size test rows (`:215-218`); validation =
    first val_size train rows, train = rows [val_size, tr_size) (`:219-222`).
  * `comm.Scatter` x6 (`:236-241`) hands every rank a contiguous chunk.  The
    train receive buffer is tr_size//P rows but only (tr_size-val_size)/P rows
    are sent, so the tail stays zero (Q5).

Here every rank loads or generates ONLY its own shard (deterministic row
ranges), so no collective is needed; rank 0 alone touches the network/disk
for acquisition and the others wait at a barrier (fixes Q3/Q4).  With no
MNIST files on disk (the GPU pool has no network) a deterministic synthetic
MNIST-shaped dataset is used instead: same shapes, dtypes and value range,
class-conditional so that accuracy is meaningful.
"""

from __future__ import annotations

import dataclasses
import os
import urllib.request
from typing import Dict, Optional, Tuple

import numpy as np

from .. import config as C
from .idx import extract_data, extract_labels


# ---------------------------------------------------------------- sizing --
@dataclasses.dataclass(frozen=True)
class SplitSizes:
    world: int
    tr_size: int
    ts_size: int
    val_size: int

    @property
    def train_rows(self) -> int:  # rows actually scattered (mpipy.py:221-222)
        return self.tr_size - self.val_size

    @property
    def train_local(self) -> int:  # real rows per rank
        return self.train_rows // self.world

    @property
    def train_local_padded(self) -> int:  # receive-buffer rows (mpipy.py:230)
        return self.tr_size // self.world

    @property
    def test_local(self) -> int:
        return self.ts_size // self.world

    @property
    def val_local(self) -> int:
        return self.val_size // self.world


def split_sizes(world: int, train_rows: int = C.TRAIN_ROWS, test_rows: int = C.TEST_ROWS,
                val_rows: int = C.VAL_ROWS) -> SplitSizes:
    """mpipy.py:211-213 rounding of the global splits to multiples of P."""
    if world <= 0:
        raise ValueError("world size must be positive")
    return SplitSizes(world, train_rows // world * world, test_rows // world * world,
                      val_rows // world * world)


def local_train_rows(sizes: SplitSizes, pad: bool) -> int:
    """N_local: the row count that drives steps/epoch and the LR decay period
    (mpipy.py:62, :79 use train_data.shape[0]).  Q5 padding => tr_size//P."""
    return sizes.train_local_padded if pad else sizes.train_local


def steps_per_run(n_local: int, epochs: int = C.ITERATION, batch: int = C.BATCH_SIZE) -> int:
    """mpipy.py:79: iteration * N_local // batch_size."""
    return epochs * n_local // batch


def batch_offset(step: int, n_local: int, batch: int = C.BATCH_SIZE) -> int:
    """mpipy.py:80: (step * batch) % (N_local - batch)  (quirk Q16 kept)."""
    if n_local <= batch:
        raise ValueError(f"local shard ({n_local} rows) must exceed the batch ({batch})")
    return (step * batch) % (n_local - batch)


def pass_of(step: int, n_local: int, batch: int = C.BATCH_SIZE) -> int:
    """The pass step `step` belongs to: how often `batch_offset` has wrapped.
    Within one pass the offsets rise by `batch`, so no row repeats."""
    if n_local <= batch:
        raise ValueError(f"local shard ({n_local} rows) must exceed the batch ({batch})")
    return (step * batch) // (n_local - batch)


def num_syncs(steps: int, every: int = C.SYNC_EVERY) -> int:
    """How many periodic syncs a run performs (step>0 and step%every==0)."""
    return max(0, (steps - 1) // every)


def shard_ranges(sizes: SplitSizes, rank: int) -> Dict[str, Tuple[int, int]]:
    """Global row ranges [start, stop) this rank owns, per split, in the
    coordinates of the files (train/val index the 60000-row train file)."""
    if not 0 <= rank < sizes.world:
        raise ValueError(f"rank {rank} outside world {sizes.world}")
    tl, sl, vl = sizes.train_local, sizes.test_local, sizes.val_local
    return {
        "train": (sizes.val_size + rank * tl, sizes.val_size + (rank + 1) * tl),
        "test": (rank * sl, (rank + 1) * sl),
        "val": (rank * vl, (rank + 1) * vl),
    }


# ----------------------------------------------------------- acquisition --
def data_exist_here(data_file_name: str, data_dir: str = "data", download: bool = False,
                    url: str = C.DATA_URL) -> str:
    """mpipy.py:185-199 without the bugs: call on ONE rank, raise a real error."""
    os.makedirs(data_dir, exist_ok=True)
    path = os.path.join(data_dir, data_file_name)
    if not os.path.exists(path) and download:
        tmp = path + ".part"
        try:
            urllib.request.urlretrieve(url + data_file_name, tmp)
            os.replace(tmp, path)
        except Exception as e:  # pragma: no cover - no network in CI
            if os.path.exists(tmp):
                os.remove(tmp)
            raise RuntimeError(f"download of {data_file_name} failed: {e}") from e
    return path


def mnist_files_present(data_dir: str) -> bool:
    return all(os.path.exists(os.path.join(data_dir, f)) for f in C.MNIST_FILES.values())


# ------------------------------------------------------------- synthetic --
_SYN_CHUNK = 1000


def _prototypes(seed: int, classes: int, h: int, w: int, c: int) -> np.ndarray:
    """Class templates: thresholded smooth random fields (stroke-like masks)."""
    rng = np.random.default_rng([seed, 7919, classes, h, w, c])
    coarse = rng.standard_normal((classes, max(2, h // 4), max(2, w // 4), c))
    # nearest-neighbour upsample + 3x3 box blur -> blobs
    up = np.repeat(np.repeat(coarse, int(np.ceil(h / coarse.shape[1])), 1),
                   int(np.ceil(w / coarse.shape[2])), 2)[:, :h, :w, :]
    pad = np.pad(up, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    blur = sum(pad[:, dy:dy + h, dx:dx + w, :] for dy in range(3) for dx in range(3)) / 9.0
    thr = np.quantile(blur.reshape(classes, -1), 0.78, axis=1).reshape(classes, 1, 1, 1)
    return (blur > thr).astype(np.float32)


# Synthetic task design (v2).  The v1 task (one fixed template per class +
# small noise) was solved to ~100 % within tens of steps, so the final-accuracy
# half of the headline metric carried no information.  v2 composes every
# image from a POOL of stroke templates that the classes SHARE:
#   * class c is a fixed set of 3 pool templates (classes overlap pairwise);
#   * each of the class's templates is present with prob. 0.82 (at least one),
#     at an independent +-2 px shift and a random weight in [0.45, 1.0];
#   * one distractor template of another class appears with prob. 0.6;
#   * random contrast / brightness and Gaussian pixel noise.
# Templates that go missing make some images genuinely ambiguous, so the
# Bayes accuracy is below 100 % and the reached accuracy depends on how well
# the network is trained (docs/ACCURACY.md has the calibration).
_POOL = 16
_PER_CLASS = 3


def _class_codes(seed: int, classes: int) -> np.ndarray:
    rng = np.random.default_rng([seed, 104729, classes])
    seen, codes = set(), []
    while len(codes) < classes:
        c = tuple(sorted(rng.choice(_POOL, _PER_CLASS, replace=False).tolist()))
        if c not in seen:
            seen.add(c)
            codes.append(c)
    return np.asarray(codes, dtype=np.int64)


def _shift_add(out: np.ndarray, src: np.ndarray, w: np.ndarray, sy: np.ndarray,
               sx: np.ndarray) -> None:
    """out[i] += w[i] * roll(src[i], (sy[i], sx[i])), grouped by shift."""
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            sel = np.nonzero((sy == dy) & (sx == dx))[0]
            if sel.size:
                out[sel] += w[sel, None, None, None] * np.roll(src[sel], (dy, dx), axis=(1, 2))


def _synthetic_chunk(kind: str, chunk: int, seed: int, classes: int,
                     shape: Tuple[int, int, int]) -> Tuple[np.ndarray, np.ndarray]:
    h, w, c = shape
    pool = _prototypes(seed, _POOL, h, w, c)
    codes = _class_codes(seed, classes)
    kid = {"train": 1, "test": 2}[kind]
    rng = np.random.default_rng([seed, kid, chunk, h, w, c, 2])
    n = _SYN_CHUNK
    labels = rng.integers(0, classes, size=n).astype(np.int64)
    keep = rng.random((n, _PER_CLASS)) < 0.82
    keep[np.arange(n), rng.integers(0, _PER_CLASS, size=n)] = True
    out = np.zeros((n, h, w, c), np.float32)
    for j in range(_PER_CLASS):
        wt = np.where(keep[:, j], rng.uniform(0.45, 1.0, size=n), 0.0).astype(np.float32)
        _shift_add(out, pool[codes[labels, j]], wt, rng.integers(-2, 3, size=n),
                   rng.integers(-2, 3, size=n))
    other = (labels + rng.integers(1, classes, size=n)) % classes
    dj = codes[other, rng.integers(0, _PER_CLASS, size=n)]
    dw = np.where(rng.random(n) < 0.6, rng.uniform(0.3, 0.7, size=n), 0.0).astype(np.float32)
    _shift_add(out, pool[dj], dw, rng.integers(-2, 3, size=n), rng.integers(-2, 3, size=n))
    gain = rng.uniform(0.5, 1.0, size=(n, 1, 1, 1)).astype(np.float32)
    bias = rng.uniform(-0.05, 0.15, size=(n, 1, 1, 1)).astype(np.float32)
    noise = rng.standard_normal(out.shape).astype(np.float32)
    u8 = np.clip((gain * np.minimum(out, 1.2) + bias + 0.28 * noise) * 255.0, 0, 255)
    return u8.astype(np.uint8), labels


def synthetic_rows(kind: str, start: int, stop: int, seed: int = C.SEED,
                   classes: int = C.NUM_CLASSES,
                   shape: Tuple[int, int, int] = (C.IMAGE_SIZE, C.IMAGE_SIZE, 1)
                   ) -> Tuple[np.ndarray, np.ndarray]:
    """Rows [start, stop) of the deterministic synthetic split `kind`, as
    (float32 images in [-0.5, 0.5] NHWC, int64 labels).  Row r is the same
    no matter which rank or world size asks for it."""
    if stop <= start:
        h, w, c = shape
        return np.zeros((0, h, w, c), np.float32), np.zeros((0,), np.int64)
    xs, ys = [], []
    for ch in range(start // _SYN_CHUNK, (stop - 1) // _SYN_CHUNK + 1):
        u8, lab = _synthetic_chunk(kind, ch, seed, classes, shape)
        lo = max(start, ch * _SYN_CHUNK) - ch * _SYN_CHUNK
        hi = min(stop, (ch + 1) * _SYN_CHUNK) - ch * _SYN_CHUNK
        xs.append(u8[lo:hi])
        ys.append(lab[lo:hi])
    u8 = np.concatenate(xs)
    x = (u8.astype(np.float32) - C.PIXEL_DEPTH / 2.0) / C.PIXEL_DEPTH
    return x, np.concatenate(ys)


# -------------------------------------------------------------- shards --
@dataclasses.dataclass
class Shard:
    train_x: np.ndarray
    train_y: np.ndarray
    test_x: np.ndarray
    test_y: np.ndarray
    val_x: np.ndarray
    val_y: np.ndarray
    synthetic: bool
    sizes: SplitSizes

    @property
    def n_local(self) -> int:
        return self.train_x.shape[0]


def load_mnist_shard(rank: int, world: int, data_dir: str = "data",
                     synthetic: Optional[bool] = None, pad: bool = False,
                     seed: int = C.SEED) -> Shard:
    """This rank's train/test/val rows (what the reference's six Scatters
    deliver, mpipy.py:230-241)."""
    sizes = split_sizes(world)
    rng_ = shard_ranges(sizes, rank)
    use_syn = (not mnist_files_present(data_dir)) if synthetic is None else synthetic
    if use_syn:
        tx, ty = synthetic_rows("train", *rng_["train"], seed=seed)
        sx, sy = synthetic_rows("test", *rng_["test"], seed=seed)
        vx, vy = synthetic_rows("train", *rng_["val"], seed=seed)
    else:
        f = {k: os.path.join(data_dir, v) for k, v in C.MNIST_FILES.items()}
        a, b = rng_["train"]
        tx = extract_data(f["train_images"], b)[a:]
        ty = extract_labels(f["train_labels"], b)[a:]
        a, b = rng_["test"]
        sx = extract_data(f["test_images"], b)[a:]
        sy = extract_labels(f["test_labels"], b)[a:]
        a, b = rng_["val"]
        vx = extract_data(f["train_images"], b)[a:]
        vy = extract_labels(f["train_labels"], b)[a:]
    if pad:  # quirk Q5: receive buffer tr_size//P rows, tail left zero
        n_pad = sizes.train_local_padded
        px = np.zeros((n_pad,) + tx.shape[1:], np.float32)
        py = np.zeros((n_pad,), np.int64)
        px[: tx.shape[0]] = tx
        py[: ty.shape[0]] = ty
        tx, ty = px, py
    return Shard(np.ascontiguousarray(tx, np.float32), ty, np.ascontiguousarray(sx, np.float32), sy,
                 np.ascontiguousarray(vx, np.float32), vy, use_syn, sizes)


def synthetic_image_shard(rank: int, world: int, rows_per_rank: int, test_per_rank: int,
                          shape: Tuple[int, int, int], classes: int = 10,
                          seed: int = C.SEED) -> Shard:
    """Synthetic CIFAR-shaped (32x32x3) or ImageNet-shaped (224x224x3) shard
    for the LeNet-5 / ResNet-18 configs (BASELINE.json configs 4-5)."""
    a = rank * rows_per_rank
    tx, ty = synthetic_rows("train", a, a + rows_per_rank, seed, classes, shape)
    b = rank * test_per_rank
    sx, sy = synthetic_rows("test", b, b + test_per_rank, seed, classes, shape)
    sizes = SplitSizes(world, rows_per_rank * world, test_per_rank * world, 0)
    return Shard(tx, ty, sx, sy, sx[:0], sy[:0], True, sizes)


def synthetic_images_torch(n: int, shape: Tuple[int, int, int], classes: int = 10,
                           seed: int = C.SEED, start: int = 0, device="cpu", split: str = "train",
                           noise: float = 0.35):
    """Large-image synthetic task (ResNet-18 at 224x224x3), generated with
    torch: the v2 design of `_synthetic_chunk` scaled to the image size, so
    the final accuracy is informative (it is not separable at a glance):
      * a pool of 16 smooth colour templates (coarse random fields at 1/16 of
        the resolution, bilinear upsampled, tanh-squashed) SHARED by the
        classes: class c is a fixed set of 3 pool templates;
      * each of the class's templates present with prob. 0.8 (at least one),
        weight U(0.45, 1), independent circular shift of up to h/14 px;
      * a distractor template of another class with prob. 0.6;
      * random gain / bias and Gaussian pixel noise (`noise`).
    Values in [-0.5, 0.5], NHWC float32, int64 labels.  Deterministic in
    (seed, split, start): rows [start, start + n)."""
    import torch

    h, w, c = shape
    pool_n, per = _POOL, _PER_CLASS
    g = torch.Generator(device="cpu").manual_seed(seed * 1000003 + 17)
    ch, cw = max(2, h // 16), max(2, w // 16)
    coarse = torch.randn(pool_n, c, ch, cw, generator=g)
    tpl = torch.tanh(2.0 * torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear",
                                                           align_corners=False))
    codes = torch.from_numpy(_class_codes(seed, classes))
    salt = {"train": 0, "test": 1 << 40, "val": 2 << 40}[split]
    gl = torch.Generator(device="cpu").manual_seed(seed * 7919 + start + salt)
    labels = torch.randint(0, classes, (n,), generator=gl)
    keep = torch.rand(n, per, generator=gl) < 0.8
    keep[torch.arange(n), torch.randint(0, per, (n,), generator=gl)] = True
    wts = torch.where(keep, 0.45 + 0.55 * torch.rand(n, per, generator=gl), torch.zeros(()))
    other = (labels + torch.randint(1, classes, (n,), generator=gl)) % classes
    dist = codes[other, torch.randint(0, per, (n,), generator=gl)]
    dw = torch.where(torch.rand(n, generator=gl) < 0.6, 0.3 + 0.4 * torch.rand(n, generator=gl),
                     torch.zeros(()))
    smax = max(2, h // 14)
    shifts = torch.randint(-smax, smax + 1, (n, per + 1, 2), generator=gl)
    gain = 0.5 + 0.5 * torch.rand(n, 1, 1, 1, generator=gl)
    bias = -0.05 + 0.2 * torch.rand(n, 1, 1, 1, generator=gl)
    gn = torch.Generator(device=device).manual_seed(seed * 104729 + start + salt)
    tpl = tpl.to(device)
    ar_h = torch.arange(h, device=device)
    ar_w = torch.arange(w, device=device)
    x = torch.empty(n, h, w, c, device=device)
    for a in range(0, n, 64):  # chunks keep the gathers small
        b = min(n, a + 64)
        m = b - a
        img = torch.zeros(m, c, h, w, device=device)
        srcs = [(codes[labels[a:b], j], wts[a:b, j]) for j in range(per)] + [(dist[a:b], dw[a:b])]
        for j, (ids, wt) in enumerate(srcs):
            sy = shifts[a:b, j, 0].to(device)
            sx = shifts[a:b, j, 1].to(device)
            yi = (ar_h[None, :] - sy[:, None]) % h  # circular shift, per sample
            xi = (ar_w[None, :] - sx[:, None]) % w
            t = tpl[ids.to(device)]  # [m, c, h, w]
            t = t.gather(2, yi[:, None, :, None].expand(m, c, h, w))
            t = t.gather(3, xi[:, None, None, :].expand(m, c, h, w))
            img += wt.to(device)[:, None, None, None] * t
        img = gain[a:b].to(device) * img + bias[a:b].to(device)
        img = img + noise * torch.randn(img.shape, generator=gn, device=device)
        x[a:b] = (0.25 * img).clamp_(-0.5, 0.5).permute(0, 2, 3, 1)
    return x, labels
