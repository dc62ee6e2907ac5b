"""Float64 stage references for the bf16 MNIST step (csrc/kernels/mnist_bf16.hip
and the bf16 kernels of mnist.hip), plain torch / numpy, no GPU.

Every stage reference takes the stage's inputs exactly as the kernels left
them on the device (bf16 values, argmax bytes, bf16 weight shadows), so the
reference sees the same rounded operands and the same masks as the kernel.
What is left between the two is the fp32 accumulation order plus, for a bf16
output, one rounding; `tol()` bounds both (worst case, derived, not tuned).

Layouts: the table at the top of csrc/kernels/mnist_bf16.h.  The codecs here
are written as view / permute of that table; tests/test_mnist_bf16_ref_cpu.py
checks them against index-by-index loops of the same table.

Logical forms: activations NHWC, conv weights HWIO (as [25, ci, co] per tap),
fc1 weight [3136, 512] with feature i = (py * 7 + px) * 64 + co.  Pool argmax
code q = 2 * dy + dx (dy, dx the position in the 2 x 2 window).
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
EPS = 2.0 ** -23      # fp32 accumulation: one product + one add per term, one spare bit
BF16_REL = 2.0 ** -8  # RNE to 8 significant bits: at most half an ulp = 2^-8 relative

# true K of every stage (Bp: rows the step computes)
N_CONV1, N_CONV2, N_FC1, N_DX, N_BWD_DATA, N_FC2 = 25, 800, 3136, 512, 1600, 512


def n_dw1(bp):
    return bp


def n_dw2(images):
    return images * 14 * 16


def n_conv1_filter(bp):
    return bp * 784


# ------------------------------------------------------------------ RNE ----
def bf16_bits(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> the bf16 bit pattern (int16 tensor) by round-to-nearest-even,
    integer arithmetic on the bit pattern (NaN stays a quiet NaN)."""
    u = x.detach().contiguous().to(torch.float32).cpu().numpy().view(np.uint32).astype(np.uint64)
    r = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    r = np.where(nan, (u >> np.uint64(16)) | np.uint64(0x40), r)
    return torch.from_numpy((r & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16).copy())


def bits_to_f32(b: torch.Tensor) -> torch.Tensor:
    u = b.contiguous().cpu().numpy().view(np.uint16).astype(np.uint32) << np.uint32(16)
    return torch.from_numpy(u.view(np.float32).copy())


def bf16_rne(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> fp32 holding the RNE bf16 value."""
    return bits_to_f32(bf16_bits(x)).reshape(x.shape)


def bf16_trunc(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> fp32 with the low 16 bits cleared (the wrong rounding)."""
    u = x.detach().contiguous().to(torch.float32).cpu().numpy().view(np.uint32) & np.uint32(0xFFFF0000)
    return torch.from_numpy(u.view(np.float32).copy()).reshape(x.shape)


def as_bits(t: torch.Tensor) -> torch.Tensor:
    """A bf16 (or int16) buffer as int16 bit patterns on the CPU, flat."""
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


# --------------------------------------------------------------- codecs ----
# unpack_*: the flat device buffer -> the logical tensor (same dtype);
# pack_*: the inverse.  B = batch rows of the buffer.
def unpack_a1p(buf, B):  # [2][B][18][18][16], ci = 16 s + c -> [B, 18, 18, 32] (border 2)
    return buf.reshape(2, B, 18, 18, 16).permute(1, 2, 3, 0, 4).reshape(B, 18, 18, 32)


def pack_a1p(x):
    B = x.shape[0]
    return x.reshape(B, 18, 18, 2, 16).permute(3, 0, 1, 2, 4).reshape(-1)


def unpack_a1t(buf, B):  # [B][18][32][24] = [n][Y][ci][X] -> [B, 18, 24, 32] (X >= 18: padding)
    return buf.reshape(B, 18, 32, 24).permute(0, 1, 3, 2)


def pack_a1t(x):
    return x.permute(0, 1, 3, 2).reshape(-1)


def unpack_a2p(buf, B):  # [196][B][16], i = 16 k + c -> [B, 3136]
    return buf.reshape(196, B, 16).permute(1, 0, 2).reshape(B, 3136)


def pack_a2p(x):
    B = x.shape[0]
    return x.reshape(B, 196, 16).permute(1, 0, 2).reshape(-1)


def unpack_a2t(buf, B):  # [B/16][3136][16] -> [B, 3136]
    return buf.reshape(B // 16, 3136, 16).permute(0, 2, 1).reshape(B, 3136)


def pack_a2t(x):
    B = x.shape[0]
    return x.reshape(B // 16, 16, 3136).permute(0, 2, 1).reshape(-1)


def unpack_dh16(buf, B):  # [32][B][16], j = 16 k + c -> [B, 512]
    return buf.reshape(32, B, 16).permute(1, 0, 2).reshape(B, 512)


def pack_dh16(x):
    B = x.shape[0]
    return x.reshape(B, 32, 16).permute(1, 0, 2).reshape(-1)


def unpack_dht(buf, B):  # [B/16][512][16] -> [B, 512]
    return buf.reshape(B // 16, 512, 16).permute(0, 2, 1).reshape(B, 512)


def pack_dht(x):
    B = x.shape[0]
    return x.reshape(B // 16, 16, 512).permute(0, 2, 1).reshape(-1)


def unpack_dy2p(buf, B):  # [4][B][18][18][16], co = 16 k + c -> [B, 18, 18, 64] (border 2)
    return buf.reshape(4, B, 18, 18, 16).permute(1, 2, 3, 0, 4).reshape(B, 18, 18, 64)


def pack_dy2p(x):
    B = x.shape[0]
    return x.reshape(B, 18, 18, 4, 16).permute(3, 0, 1, 2, 4).reshape(-1)


def unpack_dy2t(buf, B):  # [B][14][64][16] = [n][y][co][x] -> [B, 14, 16, 64] (x 14 / 15 zero)
    return buf.reshape(B, 14, 64, 16).permute(0, 1, 3, 2)


def pack_dy2t(x):
    return x.permute(0, 1, 3, 2).reshape(-1)


def unpack_w2t(buf):  # [25][2][64][16]: B[k = ci][n = co] per tap -> [25, 32, 64]
    return buf.reshape(25, 2, 64, 16).permute(0, 1, 3, 2).reshape(25, 32, 64)


def pack_w2t(w):
    return w.reshape(25, 2, 16, 64).permute(0, 1, 3, 2).reshape(-1)


def unpack_w2b(buf):  # [25][4][32][16]: B[k = co][n = ci] per tap -> [25, 32, 64]
    return buf.reshape(25, 4, 32, 16).permute(0, 2, 1, 3).reshape(25, 32, 64)


def pack_w2b(w):
    return w.reshape(25, 32, 4, 16).permute(0, 2, 1, 3).reshape(-1)


def unpack_w1t(buf):  # [196][512][16]: B[k = i][n = j] -> [3136, 512]
    return buf.reshape(196, 512, 16).permute(0, 2, 1).reshape(3136, 512)


def pack_w1t(w):
    return w.reshape(196, 16, 512).permute(0, 2, 1).reshape(-1)


def unpack_w1b(buf):  # [32][3136][16]: B[k = j][n = i] -> [3136, 512]
    return buf.reshape(32, 3136, 16).permute(1, 0, 2).reshape(3136, 512)


def pack_w1b(w):
    return w.reshape(3136, 32, 16).permute(1, 0, 2).reshape(-1)


def interior(xp):  # [B, 18, 18, C] -> [B, 14, 14, C]
    return xp[:, 2:16, 2:16, :]


def border_mask():  # [18, 18] bool: True on the 2-pixel border
    m = torch.ones(18, 18, dtype=torch.bool)
    m[2:16, 2:16] = False
    return m


# ------------------------------------------------------------ tolerance ----
def tol(ref, S, n, bf16_out=False):
    """The bound on |got - ref| of an output accumulated in fp32 over n
    products whose absolute values sum to S: acc = n 2^-23 S (worst case;
    the one spare bit covers the MFMA's internal adder and the split-K /
    two-chain regrouping); a bf16 output adds one RNE of a value within acc
    of ref: 2^-8 (|ref| + acc)."""
    acc = n * EPS * S
    return acc + BF16_REL * (ref.abs() + acc) if bf16_out else acc


def check(got, ref, S, n, bf16_out=False, zero=None, scale=1.0):
    """-> (worst err / tol, number over the bound, number of structural-zero
    violations).  zero: bool mask of elements that must be exactly 0.  scale:
    multiplies acc (a 1-Lipschitz epilogue followed by a scale)."""
    got = got.to(F64)
    t = tol(ref, S * scale, n, bf16_out)
    err = (got - ref).abs()
    bad_fin = int((~torch.isfinite(got)).sum())
    over = torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))
    ratio = torch.where(t > 0, err / t.clamp_min(1e-300), over)
    nzero = 0
    if zero is not None:
        nzero = int((got[zero] != 0).sum())
    worst = float(ratio.max()) if ratio.numel() else 0.0
    return worst, int((err > t).sum()) + bad_fin, nzero


def check_argmax(z, acc, codes):
    """The argmax rule.  z [..., 4] fp64 pre-pool values (bias included) per
    quadrant, acc [..., 4] or [...] their accumulation bound, codes [...] the
    device's bytes.  A window is compared only where the fp64 maximum is > 0
    and leads the runner-up by more than 2 acc; elsewhere the code only has
    to be in 0..3.  -> (mismatches among the compared, codes out of range,
    share of the active windows (max > 0) left out)."""
    if acc.dim() == z.dim():
        acc = acc.max(-1).values
    top = z.topk(2, dim=-1)
    best, second, arg = top.values[..., 0], top.values[..., 1], top.indices[..., 0]
    active = best > 0
    sure = active & ((best - second) > 2 * acc)
    codes = codes.to(torch.int64)
    mism = int((sure & (codes != arg)).sum())
    oob = int(((codes < 0) | (codes > 3)).sum())
    left = float((active & ~sure).sum()) / max(1, int(active.sum()))
    return mism, oob, left


# ------------------------------------------------------ stage references ----
def _quads(z):  # [B, 2P, 2P, C] -> [B, P, P, C, 4], q = 2 dy + dx
    B, H, W, C = z.shape
    return z.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)


def _conv_same(x_nhwc, w_taps, kh=5):
    """5 x 5 SAME convolution, NHWC x [25, ci, co] -> NHWC."""
    ci, co = w_taps.shape[1], w_taps.shape[2]
    w = w_taps.reshape(kh, kh, ci, co).permute(3, 2, 0, 1)
    return F.conv2d(x_nhwc.permute(0, 3, 1, 2), w, padding=2).permute(0, 2, 3, 1)


def conv_pool(x, w_taps, bias, dt=F64):
    """conv 5x5 SAME + bias + ReLU + 2x2 max-pool.  x [B, H, W, ci], w_taps
    [25, ci, co].  -> ref [B, H/2, W/2, co], S (same shape: the winning
    quadrant's bound), zq [.., co, 4] pre-pool values with bias, Sq [.., co, 4]."""
    x, w, b = x.to(dt), w_taps.to(dt), bias.to(dt)
    zq = _quads(_conv_same(x, w) + b)
    Sq = _quads(_conv_same(x.abs(), w.abs()) + b.abs())
    best = zq.max(-1)
    ref = best.values.clamp_min(0)
    S = Sq.max(-1).values  # any quadrant may win within acc: the largest bound
    return ref, S, zq, Sq


def conv1_pool(x, w1, b1, dt=F64):
    """x [B, 28, 28, 1] fp32 rows, w1 [5, 5, 1, 32] fp32, b1 [32]."""
    return conv_pool(x.reshape(-1, 28, 28, 1), w1.reshape(25, 1, 32), b1, dt)


def conv2_pool(a1, w2_taps, b2, dt=F64):
    """a1 [B, 14, 14, 32] (unpacked device a1p interior), w2_taps [25, 32, 64]
    (unpacked w2t shadow), b2 [64] fp32.  ref as [B, 3136] in (py, px, co)."""
    ref, S, zq, Sq = conv_pool(a1, w2_taps, b2, dt)
    B = ref.shape[0]
    return ref.reshape(B, 3136), S.reshape(B, 3136), zq.reshape(B, 3136, 4), Sq.reshape(B, 3136, 4)


def fc1_fwd(a2, w1, b3, keep_mask, keep_prob, dt=F64):
    """hd = dropout(relu(a2 W1 + b3)).  a2 [B, 3136], w1 [3136, 512] (w1t
    shadow).  keep_mask None: no dropout.  -> hd, S (of the pre-activation)."""
    a2, w1, b3 = a2.to(dt), w1.to(dt), b3.to(dt)
    z = a2 @ w1 + b3
    S = a2.abs() @ w1.abs() + b3.abs()
    h = z.clamp_min(0)
    if keep_mask is not None:
        h = h * keep_mask.to(dt) / keep_prob
    return h, S


def head_loss(hd, w4, b4, labels, lb, dt=F64):
    """logits = hd W4 + b4; loss rows; dlog = (softmax - onehot) / lb, rows
    >= lb exactly zero.  -> dict(logits, S_logits, loss, dlog)."""
    hd, w4, b4 = hd.to(dt), w4.to(dt), b4.to(dt)
    B = hd.shape[0]
    logits = hd @ w4 + b4
    S = hd.abs() @ w4.abs() + b4.abs()
    lse = torch.logsumexp(logits, 1)
    lab = labels.to(torch.int64)
    loss = lse - logits.gather(1, lab[:, None])[:, 0]
    p = torch.softmax(logits, 1)
    p = p - F.one_hot(lab, 10).to(dt)
    dlog = p / lb
    valid = (torch.arange(B) < lb)
    loss = torch.where(valid, loss, torch.zeros_like(loss))
    dlog = dlog * valid[:, None].to(dt)
    return dict(logits=logits, S_logits=S, loss=loss, dlog=dlog, valid=valid)


def head_tols(h, lb):
    """Bounds of the softmax cross-entropy outputs, from the logit bound a =
    512 2^-23 S_logits (row maximum): a logit error d moves a probability by
    at most 2 d (|dp_i| = p_i |d_i - sum p_j d_j|), and the softmax's own
    arithmetic (a fast exp good to 2 ulp on a value <= 1 with an argument
    error |x| 2^-24 e^-|x| <= 2^-24 / e, a 10-term sum, one division) adds at
    most 16 2^-23 absolute; the loss is three fp32 terms of magnitude
    <= max|logit| + log 10 next to 2 a."""
    a = (N_FC2 * EPS * h["S_logits"]).max(1).values
    dlog_tol = ((2 * a + 16 * EPS) / lb)[:, None].expand(-1, 10)
    mag = h["logits"].abs().max(1).values + 2.31
    loss_tol = 2 * a + 8 * EPS * mag
    return dlog_tol, loss_tol


def head_dh(dlog, w4, hd, keep_prob, dt=F64):
    """dh = (dlog W4^T) / keep where hd > 0, else 0.  -> dh, S."""
    dlog, w4 = dlog.to(dt), w4.to(dt)
    act = (hd > 0).to(dt)
    d = (dlog @ w4.t()) / keep_prob * act
    S = (dlog.abs() @ w4.abs().t()) / keep_prob * act
    return d, S


def fc1_head(a2, w1, b3, w4, b4, labels, keep_mask, keep_prob, lb, hd_dev=None, dlog_dev=None, dt=F64):
    """The fc1 forward and the head in one call.  hd_dev / dlog_dev: the
    device's values of the stage inputs downstream (operand matching); None
    chains the reference's own.  -> dict(hd, S_hd, logits, S_logits, loss,
    dlog, dh, S_dh)."""
    hd, S_hd = fc1_fwd(a2, w1, b3, keep_mask, keep_prob, dt)
    hin = hd if hd_dev is None else hd_dev.to(dt)
    out = head_loss(hin, w4, b4, labels, lb, dt)
    din = out["dlog"] if dlog_dev is None else dlog_dev.to(dt)
    dh, S_dh = head_dh(din, w4, hin, keep_prob, dt)
    out.update(hd=hd, S_hd=S_hd, dh=dh, S_dh=S_dh)
    return out


def fc1_bwd(dh16, w1b, idx2, a2, a2t, dht, hd, dh, dlog, dt=F64):
    """fc1 backward.  dh16 / dht [B, 512], w1b [3136, 512] (shadow), idx2
    [B, 3136] codes, a2 / a2t [B, 3136], hd / dh [B, 512] fp32, dlog [B, 10].
    -> dict: dy2 [B, 14, 14, 64] (dX scattered through idx2, zero where
    a2 <= 0), S_dy2, live (bool: the one position of each window that may be
    non-zero), dW1 / S_dW1 [3136, 512], db3 / S_db3, dW4 / S_dW4, db4 / S_db4."""
    B = dh16.shape[0]
    d16, w = dh16.to(dt), w1b.to(dt)
    dx = d16 @ w.t()
    S = d16.abs() @ w.abs().t()
    act = (a2 > 0)
    dx = dx * act.to(dt)
    q = idx2.to(torch.int64).reshape(B, 7, 7, 64)
    onehot = F.one_hot(q.clamp(0, 3), 4).to(torch.bool) & act.reshape(B, 7, 7, 64, 1)  # [B,7,7,64,4]

    def scatter(v):  # [B, 3136] -> [B, 14, 14, 64]
        v = v.reshape(B, 7, 7, 64, 1) * onehot.to(dt)
        return v.reshape(B, 7, 7, 64, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 14, 14, 64)

    live = onehot.reshape(B, 7, 7, 64, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 14, 14, 64)
    at, dtr = a2t.to(dt), dht.to(dt)
    hd, dh, dlog = hd.to(dt), dh.to(dt), dlog.to(dt)
    return dict(dy2=scatter(dx), S_dy2=scatter(S), live=live,
                dW1=at.t() @ dtr, S_dW1=at.abs().t() @ dtr.abs(),
                db3=dh.sum(0), S_db3=dh.abs().sum(0),
                dW4=hd.t() @ dlog, S_dW4=hd.abs().t() @ dlog.abs(),
                db4=dlog.sum(0), S_db4=dlog.abs().sum(0))


def conv2_bwd_data(dy2, w2_taps, a1, dt=F64):
    """dA1 = [a1 > 0] conv2^T(dY2).  dy2 [B, 14, 14, 64], w2_taps [25, 32, 64]
    (w2b shadow), a1 [B, 14, 14, 32].  -> ref, S, mask (a1 > 0)."""
    w = w2_taps.to(dt).reshape(5, 5, 32, 64).permute(3, 2, 0, 1)  # [co, ci, kh, kw]
    d = dy2.to(dt).permute(0, 3, 1, 2)
    mask = a1 > 0
    ref = F.conv_transpose2d(d, w, padding=2).permute(0, 2, 3, 1) * mask.to(dt)
    S = F.conv_transpose2d(d.abs(), w.abs(), padding=2).permute(0, 2, 3, 1) * mask.to(dt)
    return ref, S, mask


def conv2_bwd_filter(a1_pad, dy2, dt=F64):
    """dW2[t, ci, co] = sum a1[n, y + kh - 2, x + kw - 2, ci] dY2[n, y, x, co],
    db2 = sum dY2.  a1_pad [B, 18, 18(+), 32] zero-bordered, dy2 [B, 14, 14, 64].
    -> dW2 [25, 32, 64], S, db2 [64], S_db2."""
    a, d = a1_pad.to(dt), dy2.to(dt)
    aa, da = a.abs(), d.abs()
    dW, S = torch.empty(25, 32, 64, dtype=dt), torch.empty(25, 32, 64, dtype=dt)
    for t in range(25):
        kh, kw = divmod(t, 5)
        dW[t] = torch.einsum("nyxc,nyxd->cd", a[:, kh:kh + 14, kw:kw + 14], d)
        S[t] = torch.einsum("nyxc,nyxd->cd", aa[:, kh:kh + 14, kw:kw + 14], da)
    return dW, S, d.sum((0, 1, 2)), da.sum((0, 1, 2))


def conv1_bwd_filter(da1m, idx1, x, dt=F64):
    """dW1c[t, co] = sum over pooled (n, py, px) of dA1m x[argmax pixel +
    tap], db1 = sum dA1m.  da1m [B, 14, 14, 32] fp32, idx1 [B, 14, 14, 32]
    codes, x [B, 28, 28] fp32 rows.  -> dW [25, 32], S, db1 [32], S_db1."""
    B = da1m.shape[0]
    g = da1m.to(dt)
    oh = F.one_hot(idx1.to(torch.int64).clamp(0, 3), 4).to(dt)  # [B,14,14,32,4]
    dz = (g[..., None] * oh).reshape(B, 14, 14, 32, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 28, 28, 32)
    xp = F.pad(x.to(dt).reshape(B, 28, 28), (2, 2, 2, 2))
    dW, S = torch.empty(25, 32, dtype=dt), torch.empty(25, 32, dtype=dt)
    dza, xa = dz.abs(), xp.abs()
    for t in range(25):
        kh, kw = divmod(t, 5)
        dW[t] = torch.einsum("nyx,nyxc->c", xp[:, kh:kh + 28, kw:kw + 28], dz)
        S[t] = torch.einsum("nyx,nyxc->c", xa[:, kh:kh + 28, kw:kw + 28], dza)
    return dW, S, g.sum((0, 1, 2)), g.abs().sum((0, 1, 2))


# --------------------------------------------------------- stage checks ----
# A snapshot `s` holds one step's buffers in logical form (the GPU test
# unpacks the device buffers into it, the CPU test fills it from a torch
# emulation): Bp, lb (logical batch), keep, x [Bp, 28, 28], labels [Bp], mask
# [Bp, 512] bool, p / g (name -> fp32 master parameter / gradient), the shadows
# w1t / w1b [3136, 512] and w2t / w2b [25, 32, 64], a1 [Bp, 14, 14, 32] (a1p
# interior), a1f [Bp, 18, 18, 32] (a1t, zero-bordered), idx1, a2 / a2t
# [Bp, 3136], idx2, hd / dh [Bp, 512], dlog [Bp, 10], loss [Bp], dh16 / dht
# [Bp, 512], dy2 (dy2p interior) / dy2f (dy2t columns 0..13) [Bp, 14, 14, 64],
# da1m [Bp, 14, 14, 32].  bf16 buffers as fp32 values.
#
# Every stage check returns {label: entry}; entry = ("tol", worst err / tol,
# elements over the bound, structural zeros violated), ("argmax", mismatches,
# codes out of range, share left out) or ("bits", elements that differ).
ARGMAX_CAP = {"idx1": 0.005, "idx2": 0.02}


def failures(res, caps=ARGMAX_CAP):
    bad = []
    for k, e in res.items():
        if e[0] == "tol" and (e[2] or e[3]):
            bad.append(f"{k}: {e[2]} over the bound (worst err / tol {e[1]:.3g}), "
                       f"{e[3]} non-zero structural zeros")
        elif e[0] == "argmax" and (e[1] or e[2] or e[3] > caps[k]):
            bad.append(f"{k}: {e[1]} argmax mismatches, {e[2]} codes out of 0..3, {e[3]:.4%} left out "
                       f"(cap {caps[k]:.2%})")
        elif e[0] == "bits" and e[1]:
            bad.append(f"{k}: {e[1]} elements differ bit for bit")
    return bad


def _t(*a, **k):
    return ("tol",) + check(*a, **k)


def same_bits(a, b):
    """fp32-held bf16 values (or any tensors) equal bit for bit (+0 != -0)."""
    a, b = a.contiguous(), b.contiguous()
    if a.dtype.is_floating_point:
        a, b = a.to(torch.float32).view(torch.int32), b.to(torch.float32).view(torch.int32)
    return ("bits", int((a != b).sum()))


def stage_shadows(s):
    p = s["p"]
    w1 = bf16_rne(p["fc1_weight"].reshape(3136, 512))
    w2 = bf16_rne(p["conv2_weight"].reshape(25, 32, 64))
    return {"w1b": same_bits(s["w1b"], w1), "w1t": same_bits(s["w1t"], w1),
            "w2tb": same_bits(s["w2t"], w2), "w2b": same_bits(s["w2b"], w2)}


def stage_conv1(s):
    ref, S, zq, Sq = conv1_pool(s["x"], s["p"]["conv1_weight"], s["p"]["conv1_bias"])
    return {"a1p": _t(s["a1"], ref, S, N_CONV1, bf16_out=True),
            "idx1": ("argmax",) + check_argmax(zq, N_CONV1 * EPS * Sq, s["idx1"])}


def stage_conv2(s):
    B = s["a2"].shape[0]
    ref, S, zq, Sq = conv2_pool(s["a1"][:B], s["w2t"], s["p"]["conv2_bias"])
    return {"a2h": _t(s["a2"], ref, S, N_CONV2, bf16_out=True),
            "idx2": ("argmax",) + check_argmax(zq, N_CONV2 * EPS * Sq, s["idx2"])}


def stage_fc1(s):
    """hd: ReLU and dropout are 1-Lipschitz, the 1 / keep scale follows."""
    ref, S = fc1_fwd(s["a2"], s["w1t"], s["p"]["fc1_bias"], s["mask"], s["keep"])
    return {"hd": _t(s["hd"], ref, S, N_FC1, scale=1.0 / s["keep"])}


def stage_head(s):
    p, lb = s["p"], s["lb"]
    h = head_loss(s["hd"], p["fc2_weight"], p["fc2_bias"], s["labels"], lb)
    dlog_tol, loss_tol = head_tols(h, lb)
    pad = ~h["valid"]

    def vs(got, ref, t, zero):
        got = got.to(F64)
        err = (got - ref).abs()
        return ("tol", float((err / t).max()), int((err > t).sum()) + int((~torch.isfinite(got)).sum()),
                int((got[zero] != 0).sum()))

    dh, S_dh = head_dh(s["dlog"], p["fc2_weight"], s["hd"], s["keep"])
    dead = ~(s["hd"] > 0) | pad[:, None]
    return {"dlog": vs(s["dlog"], h["dlog"], dlog_tol, pad[:, None].expand(-1, 10)),
            "loss_rows": vs(s["loss"], h["loss"], loss_tol, pad),
            "dh": _t(s["dh"], dh, S_dh, 10, zero=dead),
            "dh16": same_bits(s["dh16"], bf16_rne(s["dh"])),
            "dht16": same_bits(s["dht"], s["dh16"])}


def stage_fc1_bwd(s):
    Bp, lb, g = s["Bp"], s["lb"], s["g"]
    r = fc1_bwd(s["dh16"], s["w1b"], s["idx2"], s["a2"], s["a2t"][:lb], s["dht"][:lb], s["hd"][:lb],
                s["dh"][:lb], s["dlog"][:lb])
    live = r["live"].clone()
    live[lb:] = False  # pad rows: exactly zero
    return {"dy2p": _t(s["dy2"], r["dy2"], r["S_dy2"], N_DX, bf16_out=True, zero=~live),
            "g_fc1_weight": _t(g["fc1_weight"].reshape(3136, 512), r["dW1"], r["S_dW1"], n_dw1(Bp)),
            "g_fc1_bias": _t(g["fc1_bias"], r["db3"], r["S_db3"], Bp),
            "g_fc2_weight": _t(g["fc2_weight"].reshape(512, 10), r["dW4"], r["S_dW4"], Bp),
            "g_fc2_bias": _t(g["fc2_bias"], r["db4"], r["S_db4"], Bp)}


def stage_conv2_bwd_data(s):
    lb = s["lb"]
    ref, S, mask = conv2_bwd_data(s["dy2"], s["w2b"], s["a1"])
    dead = ~mask
    dead[lb:] = True
    return {"da1m": _t(s["da1m"], ref, S, N_BWD_DATA, zero=dead)}


def stage_conv2_bwd_filter(s, groups=None):
    """groups: a list of (n0, n1, dW2 slab [25, 32, 64]) checks the per-group
    slabs (K = the group's images) instead of the finished gradient."""
    Bp, lb, g = s["Bp"], s["lb"], s["g"]
    if groups is not None:
        out = {}
        for n0, n1, slab in groups:
            m = min(n1, lb)
            dW, S, _, _ = conv2_bwd_filter(s["a1f"][n0:m], s["dy2f"][n0:m])
            out[f"part2[{n0}:{n1}]"] = _t(slab, dW, S, n_dw2(n1 - n0))
        return out
    dW, S, db, S_db = conv2_bwd_filter(s["a1f"][:lb], s["dy2f"][:lb])
    return {"g_conv2_weight": _t(g["conv2_weight"].reshape(25, 32, 64), dW, S, n_dw2(Bp)),
            "g_conv2_bias": _t(g["conv2_bias"], db, S_db, n_dw2(Bp))}


def stage_conv1_bwd_filter(s):
    Bp, lb, g = s["Bp"], s["lb"], s["g"]
    dW, S, db, S_db = conv1_bwd_filter(s["da1m"][:lb], s["idx1"][:lb], s["x"][:lb])
    return {"g_conv1_weight": _t(g["conv1_weight"].reshape(25, 32), dW, S, n_conv1_filter(Bp)),
            "g_conv1_bias": _t(g["conv1_bias"], db, S_db, n_conv1_filter(Bp))}


STAGES = dict(shadows=stage_shadows, conv1=stage_conv1, conv2=stage_conv2, fc1=stage_fc1, head=stage_head,
              fc1_bwd=stage_fc1_bwd, conv2_bwd_data=stage_conv2_bwd_data,
              conv2_bwd_filter=stage_conv2_bwd_filter, conv1_bwd_filter=stage_conv1_bwd_filter)
