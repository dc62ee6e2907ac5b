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

from typing import NamedTuple, Optional, Tuple

import numpy as np

M32 = 0xFFFFFFFF
GOLDEN = 0x9E3779B9
STEP_MUL = 0x85EBCA6B
EVAL_SALT = 0x5BD1E995  # separates the eval-time (quirk Q8) stream
SHUFFLE_SALT = 0x2545F491  # ... and the per-pass row order (--shuffle)
AUGMENT_SALT = 0x68E31DA4  # ... and the per-pass shift / flip draws (--augment)
MIX_SALT = 0x3C6EF372  # ... and the per-pass mixup / cutmix draws (--mix)


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


# ---- rotate / scale / cutout (--augment rotate:D, scale:P, cutout:S) --------
# Integer coordinates (Q16 matrix, Q17 pixels) and single fp32 operations per
# sample, so numpy, torch and csrc/kernels/augment.hip agree bit for bit; the
# definition is spelled out in docs/ACCURACY.md.
AFFINE_LEVELS = 129  # angle / scale levels, level 64 is the identity
Q16 = 1 << 16


def affine_tables(D: float, P: float) -> np.ndarray:
    """int32 [3, 129]: cosT, sinT, invT of the levels i = 0..128, a = (i - 64) / 64:
    rint(cos(radians(D a)) 2^16), rint(sin(radians(D a)) 2^16), rint(2^16 / (1 + P a / 100)),
    computed in float64.  The oracle and the kernel read this one table."""
    a = (np.arange(AFFINE_LEVELS, dtype=np.float64) - 64.0) / 64.0
    ang = np.radians(float(D) * a)
    return np.stack([np.rint(np.cos(ang) * Q16), np.rint(np.sin(ang) * Q16),
                     np.rint(Q16 / (1.0 + float(P) * a / 100.0))]).astype(np.int32)


class AffineParams(NamedTuple):
    """The draws of `affine_params`: per row dy, dx (int64), flipped (bool),
    m (int64 [n, 4]: m00, m01, m10, m11 in Q16), the levels ia, ib behind m, and
    cutout = (S, cy0, cx0) or None."""
    dy: np.ndarray
    dx: np.ndarray
    flipped: np.ndarray
    m: np.ndarray
    ia: np.ndarray
    ib: np.ndarray
    cutout: Optional[Tuple[int, np.ndarray, np.ndarray]]


def affine_params(key: int, rows, spec, H: int, W: int, tables=None) -> AffineParams:
    """The draws of the pristine shard rows `rows` under `key` for `spec`
    (K, flip, rotate, scale, cutout: config.AugmentSpec): the chain of
    `augment_params` continued, h_{k+1} = mix(h_k + GOLDEN) up to h6.

        dy, dx, flipped from h0, h1, h2 as in `augment_params`
        ia = h3 % 129, ib = h4 % 129        (levels of `affine_tables`)
        cy0 = h5 % (H - S + 1), cx0 = h6 % (W - S + 1)
        m00 = m11 = r(cosT[ia] invT[ib]), m01 = r(sinT[ia] invT[ib]),
        m10 = r(-sinT[ia] invT[ib]),  r(v) = (v + 32768) >> 16 in 64 bits
    """
    s = np.asarray(rows).astype(np.uint64)
    dy, dx, fl = augment_params(key, s, spec.K, spec.flip)
    h = _mix_np(s ^ np.uint64(key))
    hs = [h]
    for _ in range(6):
        h = _mix_np(h + np.uint64(GOLDEN))
        hs.append(h)
    T = affine_tables(spec.rotate, spec.scale) if tables is None else np.asarray(tables)
    T = T.astype(np.int64).reshape(3, AFFINE_LEVELS)
    ia = (hs[3] % np.uint64(AFFINE_LEVELS)).astype(np.int64)
    ib = (hs[4] % np.uint64(AFFINE_LEVELS)).astype(np.int64)
    co, si, inv = T[0][ia], T[1][ia], T[2][ib]
    m00 = (co * inv + 32768) >> 16
    m = np.stack([m00, (si * inv + 32768) >> 16, (-si * inv + 32768) >> 16, m00], axis=-1)
    cutout = None
    S = int(spec.cutout)
    if S > 0:
        cutout = (S, (hs[5] % np.uint64(H - S + 1)).astype(np.int64),
                  (hs[6] % np.uint64(W - S + 1)).astype(np.int64))
    return AffineParams(dy, dx, fl, m, ia, ib, cutout)


def affine_coords(xp, m, dy, dx, fl, H: int, W: int):
    """Source coordinate of every output pixel in Q17 pixels, (SX, SY), int64
    [n, H, W] (`xp`: numpy or torch; m [n, 4], dy, dx int64 and fl bool of it).

        u2 = 2x - (W-1), v2 = 2y - (H-1)
        SX = m00 u2 + m01 v2 + ((W-1) << 16);  flipped: SX = ((W-1) << 17) - SX;  SX += dx << 17
        SY = m10 u2 + m11 v2 + ((H-1) << 16);  SY += dy << 17
    """
    kw = {} if xp is np else {"device": m.device}
    u2 = (2 * xp.arange(W, **kw) - (W - 1))[None, None, :]
    v2 = (2 * xp.arange(H, **kw) - (H - 1))[None, :, None]
    c = [m[:, k][:, None, None] for k in range(4)]
    SX = c[0] * u2 + c[1] * v2 + ((W - 1) << 16)
    SY = c[2] * u2 + c[3] * v2 + ((H - 1) << 16)
    SX = xp.where(fl[:, None, None], ((W - 1) << 17) - SX, SX)
    return SX + (dx[:, None, None] << 17), SY + (dy[:, None, None] << 17)


def _affine_chunk(n: int, H: int, W: int) -> int:
    return max(1, min(n, (1 << 21) // (H * W)))  # rows a slice: the int64 planes stay small


def affine_np(x_nhwc: np.ndarray, m, dy, dx, flipped, fill: float, cutout=None) -> np.ndarray:
    """Per-row inverse affine map with bilinear sampling, then the cutout.
    With (ix, fx) = (SX >> 17, (SX & 0x1FFFF) 2^-17) of `affine_coords`, the
    same for (iy, fy), and taps outside the image = `fill`:

        t = (1 - fx) src[iy][ix] + fx src[iy][ix+1]
        b = (1 - fx) src[iy+1][ix] + fx src[iy+1][ix+1]
        out = (1 - fy) t + fy b        every -, *, + one fp32 operation

    `cutout` = (S, cy0, cx0): out = fill for cy0 <= y < cy0 + S, cx0 <= x < cx0 + S."""
    x = np.asarray(x_nhwc)
    n, H, W, _ = x.shape
    m, dy, dx = np.asarray(m, np.int64).reshape(n, 4), np.asarray(dy, np.int64), np.asarray(dx, np.int64)
    fl = np.asarray(flipped, bool)
    f32, fv = np.float32, x.dtype.type(fill)
    out = np.empty_like(x)
    step = _affine_chunk(n, H, W)
    for a in range(0, n, step):
        z = slice(a, min(n, a + step))
        SX, SY = affine_coords(np, m[z], dy[z], dx[z], fl[z], H, W)
        ix, iy = SX >> 17, SY >> 17
        fx = ((SX & 0x1FFFF).astype(f32) * f32(2.0 ** -17))[..., None]
        fy = ((SY & 0x1FFFF).astype(f32) * f32(2.0 ** -17))[..., None]
        rows = np.arange(z.start, z.stop)[:, None, None]

        def tap(ty, tx):
            inside = ((ty >= 0) & (ty < H) & (tx >= 0) & (tx < W))[..., None]
            return np.where(inside, x[rows, ty.clip(0, H - 1), tx.clip(0, W - 1)], fv)

        gx, gy = f32(1) - fx, f32(1) - fy
        t = gx * tap(iy, ix) + fx * tap(iy, ix + 1)
        b = gx * tap(iy + 1, ix) + fx * tap(iy + 1, ix + 1)
        o = gy * t + fy * b
        if cutout is not None:
            S, cy0, cx0 = cutout
            cy = np.asarray(cy0, np.int64)[z, None, None]
            cx = np.asarray(cx0, np.int64)[z, None, None]
            ys, xs = np.arange(H)[None, :, None], np.arange(W)[None, None, :]
            hole = (ys >= cy) & (ys < cy + S) & (xs >= cx) & (xs < cx + S)
            o = np.where(hole[..., None], fv, o)
        out[z] = o
    return out


def affine_torch(x_nhwc, m, dy, dx, flipped, fill: float, cutout=None):
    """`affine_np` on a torch tensor, on its device (the parameters: numpy)."""
    import torch

    x = x_nhwc
    n, H, W, _ = x.shape
    dev = x.device

    def dev64(v, shape=(-1,)):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.int64)).reshape(shape)).to(dev)

    m, dy, dx = dev64(m, (n, 4)), dev64(dy), dev64(dx)
    fl = torch.from_numpy(np.ascontiguousarray(np.asarray(flipped, bool))).to(dev)
    fv = torch.full((), fill, dtype=x.dtype, device=dev)
    out = torch.empty_like(x)
    step = _affine_chunk(n, H, W)
    for a in range(0, n, step):
        z = slice(a, min(n, a + step))
        SX, SY = affine_coords(torch, m[z], dy[z], dx[z], fl[z], H, W)
        ix, iy = SX >> 17, SY >> 17
        fx = ((SX & 0x1FFFF).to(torch.float32) * 2.0 ** -17)[..., None]
        fy = ((SY & 0x1FFFF).to(torch.float32) * 2.0 ** -17)[..., None]
        rows = torch.arange(z.start, z.stop, device=dev)[:, None, None]

        def tap(ty, tx):
            inside = ((ty >= 0) & (ty < H) & (tx >= 0) & (tx < W))[..., None]
            return torch.where(inside, x[rows, ty.clamp(0, H - 1), tx.clamp(0, W - 1)], fv)

        gx, gy = 1.0 - fx, 1.0 - fy
        t = gx * tap(iy, ix) + fx * tap(iy, ix + 1)
        b = gx * tap(iy + 1, ix) + fx * tap(iy + 1, ix + 1)
        o = gy * t + fy * b
        if cutout is not None:
            S, cy0, cx0 = cutout
            cy, cx = dev64(cy0)[z, None, None], dev64(cx0)[z, None, None]
            ys = torch.arange(H, device=dev)[None, :, None]
            xs = torch.arange(W, device=dev)[None, None, :]
            hole = (ys >= cy) & (ys < cy + S) & (xs >= cx) & (xs < cx + S)
            o = torch.where(hole[..., None], fv, o)
        out[z] = o
    return out


# ---- mixup / cutmix and soft targets (--mix, --label-smoothing) -------------
# Integer draws and a Q16 table, single fp32 operations per pixel, so numpy,
# torch and augment::mix_rows (csrc/kernels/augment.hip) agree bit for bit; docs/ACCURACY.md spells the
# definition out.
MIX_LEVELS = 129  # level 0 is "no mixing"


def mix_key(seed: int, rank: int, pass_: int) -> int:
    """Key of the mix draws of training pass `pass_` (--mix); `rank` as in
    `shuffle_key`."""
    return dropout_key(seed, rank, pass_, MIX_SALT)


def mix_table(kind: str, M: float, H: int, W: int) -> np.ndarray:
    """int32 [3, 129]: wq | bh | bw of the levels l = 0..128, Mq = rint(65536 M / 100).
    mixup: wq[l] = (Mq l + 64) >> 7 (the partner's share in Q16), no box.
    cutmix: a = (Mq l + 64) >> 7, bh = min(H, floor(H sqrt(a / 65536) + 0.5)), bw
    likewise with W, wq = rint(65536 bh bw / (H W)): the share the box really has.
    Computed in float64; the oracle and the kernel read this one table."""
    if kind not in ("mixup", "cutmix"):
        raise ValueError(f"unknown mix kind {kind!r}")
    Mq = int(np.rint(65536.0 * float(M) / 100.0))
    a = (Mq * np.arange(MIX_LEVELS, dtype=np.int64) + 64) >> 7
    if kind == "mixup":
        z = np.zeros(MIX_LEVELS, np.int64)
        return np.stack([a, z, z]).astype(np.int32)
    r = np.sqrt(a.astype(np.float64) / 65536.0)
    bh = np.minimum(H, np.floor(H * r + 0.5)).astype(np.int64)
    bw = np.minimum(W, np.floor(W * r + 0.5)).astype(np.int64)
    wq = np.rint(65536.0 * (bh * bw).astype(np.float64) / float(H * W)).astype(np.int64)
    return np.stack([wq, bh, bw]).astype(np.int32)


def mix_params(key: int, n: int, table, H: int, W: int):
    """(partner, lamq, cy, cx, bh, bw) of the working rows i = 0..n-1 of a pass
    under `key`, int64 each; lam = lamq 2^-16 is the row's own share.

        g0 = mix(key ^ i), g1 = mix(g0 + GOLDEN), g2 = mix(g1 + GOLDEN)
        level = g0 % 129, lamq = 65536 - wq[level], bh, bw = table[1:, level]
        partner = shuffle_perm(mix(key ^ GOLDEN), n)[i]
        cy = g1 % (H - bh + 1), cx = g2 % (W - bw + 1)
    """
    T = np.asarray(table).astype(np.int64).reshape(3, MIX_LEVELS)
    i = np.arange(n, dtype=np.uint64)
    g0 = _mix_np(i ^ np.uint64(key))
    g1 = _mix_np(g0 + np.uint64(GOLDEN))
    g2 = _mix_np(g1 + np.uint64(GOLDEN))
    level = (g0 % np.uint64(MIX_LEVELS)).astype(np.int64)
    bh, bw = T[1][level], T[2][level]
    pkey = int(_mix_np(np.array([(key ^ GOLDEN) & M32], np.uint64))[0])
    partner = shuffle_perm(pkey, n)
    cy = (g1 % (H - bh + 1).astype(np.uint64)).astype(np.int64)
    cx = (g2 % (W - bw + 1).astype(np.uint64)).astype(np.int64)
    return partner, 65536 - T[0][level], cy, cx, bh, bw


def _mix_box(xp, H, W, cy, cx, bh, bw, **kw):
    ys, xs = xp.arange(H, **kw)[None, :, None], xp.arange(W, **kw)[None, None, :]
    cy, cx, bh, bw = (v[:, None, None] for v in (cy, cx, bh, bw))
    return ((ys >= cy) & (ys < cy + bh) & (xs >= cx) & (xs < cx + bw))[..., None]


def mix_np(A: np.ndarray, A_y: np.ndarray, params, kind: str):
    """The mixed pass (x, y1, y2, lam) of the NHWC fp32 pass A with labels A_y.
    mixup: x[i] = lam A[i] + w A[j], w = 1 - lam, each product and the sum one
    rounded fp32 operation; cutmix: x[i] = A[j] inside the row's box, A[i]
    elsewhere.  y1 = A_y, y2 = A_y[j], lam float32 (exact: a multiple of 2^-16)."""
    A = np.asarray(A)
    j, lamq, cy, cx, bh, bw = (np.asarray(v, np.int64) for v in params)
    lam = lamq.astype(np.float32) * np.float32(2.0 ** -16)
    if kind == "mixup":
        w = (65536 - lamq).astype(np.float32) * np.float32(2.0 ** -16)
        sh = (-1,) + (1,) * (A.ndim - 1)
        x = lam.reshape(sh) * A + w.reshape(sh) * A[j]
    else:
        _, H, W, _ = A.shape
        x = np.where(_mix_box(np, H, W, cy, cx, bh, bw), A[j], A)
    y = np.asarray(A_y)
    return x.astype(A.dtype), y.copy(), y[j], lam


def mix_torch(A, A_y, params, kind: str):
    """`mix_np` on torch tensors, on their device (the parameters: numpy)."""
    import torch

    dev = A.device

    def dev64(v):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(v, np.int64))).to(dev)

    j, lamq, cy, cx, bh, bw = (dev64(v) for v in params)
    lam = lamq.to(torch.float32) * 2.0 ** -16
    if kind == "mixup":
        w = (65536 - lamq).to(torch.float32) * 2.0 ** -16
        sh = (-1,) + (1,) * (A.dim() - 1)
        x = lam.reshape(sh) * A + w.reshape(sh) * A[j]
    else:
        _, H, W, _ = A.shape
        x = torch.where(_mix_box(torch, H, W, cy, cx, bh, bw, device=dev), A[j], A)
    return x, A_y.clone(), A_y[j], lam


def soft_targets(y1, y2, lam, eps: float, classes: int) -> np.ndarray:
    """float64 [n, classes]: t = (1 - eps) (lam onehot(y1) + (1 - lam) onehot(y2))
    + eps / classes; y2 / lam None: lam = 1."""
    y1 = np.asarray(y1).astype(np.int64)
    n = y1.shape[0]
    lam = np.ones(n) if lam is None else np.asarray(lam, np.float64)
    y2 = y1 if y2 is None else np.asarray(y2).astype(np.int64)
    a = np.zeros((n, classes), np.float64)
    a[np.arange(n), y1] += lam
    a[np.arange(n), y2] += 1.0 - lam
    return (1.0 - float(eps)) * a + float(eps) / classes


def soft_xent_torch(logits, y1, y2=None, lam=None, eps: float = 0.0):
    """Mean soft-target cross-entropy of the torch paths, -(t log_softmax(z)).sum(1).mean(),
    with t formed in float64 as `soft_targets` forms it and rounded once to the
    dtype of the logits."""
    import torch

    C = logits.shape[1]
    a = torch.nn.functional.one_hot(y1.long(), C).double()
    if lam is not None:
        l = lam.double()[:, None]
        a = l * a + (1.0 - l) * torch.nn.functional.one_hot(y2.long(), C).double()
    t = ((1.0 - float(eps)) * a + float(eps) / C).to(logits.dtype)
    return -(t * torch.log_softmax(logits, 1)).sum(1).mean()


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
