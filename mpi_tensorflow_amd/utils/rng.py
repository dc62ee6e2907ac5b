"""Counter-based dropout RNG shared bit-for-bit by the HIP kernels and the
PyTorch oracle.

The reference draws its dropout mask with TF1's stateful Philox stream
(`tf.nn.dropout(hidden, 0.5, seed=1)`, `/root/reference/mpipy.py:166`); that
stream cannot be reproduced outside TF, and its op seed is identical on every
rank (quirk Q14).  Here each mask element is a pure function of
(seed, rank, step, element index), so it needs no RNG state on the device
(graph-capturable: the step comes from the device-side step counter) and
the oracle can regenerate exactly the mask a kernel used.

    key  = mix(mix(seed * 0x9E3779B9 + rank) ^ (step * 0x85EBCA6B + salt))
    u    = (mix(index ^ key) >> 8) * 2^-24          in [0, 1)
    keep = u < keep_prob,  scale = 1 / keep_prob

`mix` is a 32-bit integer avalanche hash (xor-shift / multiply).  The HIP
side lives in `csrc/kernels/common.h` (`dropout_key`, `dropout_keep`).
"""

from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
GOLDEN = 0x9E3779B9
STEP_MUL = 0x85EBCA6B
EVAL_SALT = 0x5BD1E995  # separates the eval-time (quirk Q8) stream
SHUFFLE_SALT = 0x2545F491  # ... and the per-pass row order (--shuffle)
AUGMENT_SALT = 0x68E31DA4  # ... and the per-pass shift / flip draws (--augment)


def _mix_np(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def dropout_key(seed: int, rank: int, step: int, salt: int = 0) -> int:
    a = _mix_np(np.array([(seed * GOLDEN + rank) & M32], np.uint64))[0]
    b = np.uint64(((step * STEP_MUL) + salt) & M32)
    return int(_mix_np(np.array([a ^ b], np.uint64))[0])


def shuffle_key(seed: int, rank: int, pass_: int) -> int:
    """Key of the row order of training pass `pass_` (--shuffle): the dropout
    key with the pass in the place of the step.  `rank` is the rank the
    dropout stream uses (0 on every rank under quirk Q14)."""
    return dropout_key(seed, rank, pass_, SHUFFLE_SALT)


def _feistel_np(x: np.ndarray, h: int, rk) -> np.ndarray:
    mask = np.uint64((1 << h) - 1)
    left, right = x >> np.uint64(h), x & mask
    for k in rk:
        left, right = right, left ^ (_mix_np(right ^ np.uint64(k)) & mask)
    return (left << np.uint64(h)) | right


def shuffle_perm(key: int, n: int) -> np.ndarray:
    """perm(0..n-1) as int64: a balanced 4-round Feistel network over
    [0, 2^bits), bits = the even bit length of n - 1 (at least 2), walked
    along its cycle until it lands below n.  F is a bijection of the domain
    and the walk stays on the cycle of i < n, so it ends and perm is a
    bijection of [0, n).  The device side is `csrc/kernels/shuffle.hip`."""
    if n <= 0:
        return np.zeros(0, np.int64)
    bits = max(2, int(n - 1).bit_length())
    bits += bits & 1
    h = bits // 2
    rk = [int(_mix_np(np.array([(key + r * GOLDEN) & M32], np.uint64))[0]) for r in range(4)]
    x = _feistel_np(np.arange(n, dtype=np.uint64), h, rk)
    while True:
        out = np.nonzero(x >= np.uint64(n))[0]
        if out.size == 0:
            return x.astype(np.int64)
        x[out] = _feistel_np(x[out], h, rk)


def augment_key(seed: int, rank: int, pass_: int) -> int:
    """Key of the augmentation draws of training pass `pass_` (--augment);
    `rank` as in `shuffle_key`."""
    return dropout_key(seed, rank, pass_, AUGMENT_SALT)


def augment_params(key: int, rows, K: int, flip: bool):
    """(dy, dx, flipped) of the pristine shard rows `rows` under `key`: a pure
    function of (key, row), so the order and the grouping of `rows` do not
    matter.  dy, dx int64 in [-K, K] (the modulo bias is below (2K+1) / 2^32),
    flipped bool (all False without `flip`).  The device side is
    `csrc/kernels/augment.hip`.

        h0 = mix(key ^ row), h1 = mix(h0 + GOLDEN), h2 = mix(h1 + GOLDEN)
        dy = h0 % (2K+1) - K, dx = h1 % (2K+1) - K, flipped = h2 >> 31
    """
    s = np.asarray(rows).astype(np.uint64)
    h0 = _mix_np(s ^ np.uint64(key))
    h1 = _mix_np(h0 + np.uint64(GOLDEN))
    h2 = _mix_np(h1 + np.uint64(GOLDEN))
    span = np.uint64(2 * K + 1)
    dy = (h0 % span).astype(np.int64) - K
    dx = (h1 % span).astype(np.int64) - K
    fl = (h2 >> np.uint64(31)).astype(bool) if flip else np.zeros(s.shape, bool)
    return dy, dx, fl


def _augment_index(xp, n, H, W, dy, dx, fl):
    """Source line / column of every output line / column, [n, H] and [n, W]
    (`xp`: numpy or torch, whose arange / where agree here)."""
    ys = xp.arange(H)[None, :] + dy[:, None]
    cols = xp.arange(W)[None, :]
    xs = xp.where(fl[:, None], W - 1 - cols, cols) + dx[:, None]
    return ys, xs


def augment_np(x_nhwc: np.ndarray, dy, dx, flip, fill: float) -> np.ndarray:
    """out[i, y, x, c] = x[i, y + dy[i], xs + dx[i], c] with xs = W - 1 - x where
    flip[i], else x; `fill` where that pixel lies outside the image."""
    x = np.asarray(x_nhwc)
    n, H, W, _ = x.shape
    ys, xs = _augment_index(np, n, H, W, np.asarray(dy), np.asarray(dx), np.asarray(flip, bool))
    inside = (((ys >= 0) & (ys < H))[:, :, None] & ((xs >= 0) & (xs < W))[:, None, :])[..., None]
    got = x[np.arange(n)[:, None, None], ys.clip(0, H - 1)[:, :, None], xs.clip(0, W - 1)[:, None, :]]
    return np.where(inside, got, x.dtype.type(fill))


def augment_torch(x_nhwc, dy, dx, flip, fill: float):
    """`augment_np` on a torch tensor, on its device (dy, dx, flip: numpy)."""
    import torch

    x = x_nhwc
    n, H, W, _ = x.shape
    dev = x.device
    ys, xs = _augment_index(torch, n, H, W, torch.from_numpy(np.asarray(dy, np.int64)),
                            torch.from_numpy(np.asarray(dx, np.int64)),
                            torch.from_numpy(np.asarray(flip, bool)))
    ys, xs = ys.to(dev), xs.to(dev)
    inside = (((ys >= 0) & (ys < H))[:, :, None] & ((xs >= 0) & (xs < W))[:, None, :])[..., None]
    got = x[torch.arange(n, device=dev)[:, None, None], ys.clamp(0, H - 1)[:, :, None],
            xs.clamp(0, W - 1)[:, None, :]]
    return torch.where(inside, got, torch.full((), fill, dtype=x.dtype, device=dev))


def keep_mask_np(key: int, n: int, keep_prob: float) -> np.ndarray:
    idx = np.arange(n, dtype=np.uint64)
    h = _mix_np(idx ^ np.uint64(key))
    u = (h >> np.uint64(8)).astype(np.float64) * (2.0 ** -24)
    return u < np.float32(keep_prob)


def keep_mask_torch(key: int, shape, keep_prob: float, device=None):
    """Same mask as a torch bool tensor (computed with numpy on the host)."""
    import torch

    n = 1
    for s in shape:
        n *= int(s)
    m = keep_mask_np(key, n, keep_prob).reshape(tuple(shape))
    return torch.from_numpy(m).to(device=device)
