"""Float64 references of the small kernels every training step runs through:
the flat optimizer of csrc/kernels/sgd.hip and the non-conv tail of
csrc/kernels/ops_generic.hip (linear, cross-entropy, softmax, batch gather,
learning rate, stem re-layouts).  Plain torch / numpy, no GPU.  Each reference
comes with the error bound tests/test_step_kernels_gpu.py holds the kernel to;
tests/test_step_ref_cpu.py pins the references themselves.

exact mode (as in conv_ref.py): operands are small integers and dyadic
constants, every product and sum is an integer (or a dyadic fraction) fp32
holds exactly, so the kernel must equal the reference bit for bit whatever the
compiler contracts into an fma.

Layouts: linear W [K][N]; conv weights HWIO; the stem layouts are the comments
above stem_wt_kernel / s2d_stem_weight_kernel in ops_generic.hip, written here
as index loops."""

from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("conv_ref", os.path.join(_HERE, "conv_ref.py"))
CR = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CR)
_ROOT = os.path.dirname(os.path.dirname(_HERE))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
from mpi_tensorflow_amd.utils.data import batch_offset  # noqa: E402,F401  (reused, not re-derived)

EPS, guard_hits, bf16_bits = CR.EPS, CR.guard_hits, CR.bf16_bits
F64, F32 = torch.float64, torch.float32

# sgd.hip grid_for: 2048 blocks x 256 lanes, one float4 (or one word) a lane and pass
SGD_CAP_FLOATS = 2048 * 256 * 4
HASH_CAP_WORDS = 2048 * 256
# ops_generic.hip grid1d: 65536 blocks x 256 lanes, one element a lane and pass
GRID1D_CAP = 65536 * 256


def f32(v) -> float:
    """A host constant as the float the binding hands the kernel."""
    return float(np.float32(v))


# ------------------------------------------------------------- optimizer ----
def sgd_ref(w, g, m, l2_end, l2, momentum, gscale, lr):
    """g' = g gscale (+ l2 w on [0, l2_end)); m' = momentum m + g'; w' = w - lr m'
    -> (w', m') in float64.  l2, momentum, gscale, lr: the fp32 values."""
    w, g, m = w.to(F64), g.to(F64), m.to(F64)
    lc = torch.zeros_like(w)
    lc[:l2_end] = l2
    m2 = momentum * m + (g * gscale + lc * w)
    return w - lr * m2, m2


def sgd_tol(w, g, m, l2_end, l2, momentum, gscale, lr):
    """-> (bound of w', bound of m').  m' is three products and two sums, at
    most four roundings of magnitudes below |l2 w| + |g gscale| + |momentum m|:
    4 EPS of that.  w' = w - lr m': the error of m' times lr, the product's and
    the subtraction's rounding (2 EPS lr |m'|, EPS |w'|)."""
    w, g, m = w.to(F64), g.to(F64), m.to(F64)
    lc = torch.zeros_like(w)
    lc[:l2_end] = l2
    w2, m2 = sgd_ref(w, g, m, l2_end, l2, momentum, gscale, lr)
    tm = 4 * EPS * ((lc * w).abs() + (g * gscale).abs() + (momentum * m).abs())
    tw = EPS * w2.abs() + abs(lr) * tm + 2 * EPS * abs(lr) * m2.abs()
    return tw, tm


def l2_ends(n):
    """The L2 boundaries of a case: none, one float4, the middle, everything."""
    return sorted({0, 4, n // 2 // 4 * 4, n})


# ------------------------------------------------------- fully connected ----
def lin_groups(N):
    """K groups of linear_fwd_kernel: 256 / NT, NT = pow2 >= N, at most 64."""
    lg = 0
    while (1 << lg) < N and lg < 6:
        lg += 1
    return 256 >> lg


def linear_ref(x, w, b=None, relu=False, dt=F64):
    """y [M][N] = x [M][K] W [K][N] (+ b) (ReLU) -> (y, S, n): S the same on
    |operands|, n = K + the K groups summed on top (+ 1 for a bias)."""
    x, w = x.to(dt), w.to(dt)
    y, S, n = x @ w, x.abs() @ w.abs(), x.shape[1] + lin_groups(w.shape[1])
    if b is not None:
        y, S, n = y + b.to(dt), S + b.to(dt).abs(), n + 1
    if relu:
        y = y.clamp_min(0)
    return y, S, n


def linear_bwd_ref(x, w, y, dy, relu, dt=F64):
    """dy' = dy [y > 0] when the forward fused the ReLU (y: the very tensor the
    kernel reads); dW = x^T dy', db = sum_m dy', dX = dy' W^T.
    -> {"dw" | "db" | "dx": (ref, S, n)}, n = M, M, N."""
    x, w, g = x.to(dt), w.to(dt), dy.to(dt)
    if relu:
        g = torch.where(y.to(dt) <= 0, torch.zeros_like(g), g)
    M, N = g.shape
    return {"dw": (x.t() @ g, x.abs().t() @ g.abs(), M),
            "db": (g.sum(0), g.abs().sum(0), M),
            "dx": (g @ w.t(), g.abs() @ w.abs().t(), N)}


def lin_tol(S, n):
    return (n + 2) * EPS * S


# ------------------------------------------------------------------ loss ----
def xent_ref(logits, labels, dt=F64):
    """-> (loss rows, (softmax - onehot) / B, softmax, hits).  hits: rows whose
    lowest-index maximum is the label.  dt = float32 evaluates the kernels'
    own formula (max-subtracted exp, log of the sum) in fp32 on the host: the
    yardstick E of the GPU test."""
    z = logits.to(dt)
    B, C = z.shape
    lab = labels.to(torch.int64)
    mx = z.max(1, keepdim=True).values
    e = torch.exp(z - mx)
    se = e.sum(1, keepdim=True)
    p = e / se
    loss = torch.log(se[:, 0]) + mx[:, 0] - z[torch.arange(B), lab]
    onehot = torch.zeros(B, C, dtype=dt)
    onehot[torch.arange(B), lab] = 1
    am = np.argmax(logits.to(F64).numpy(), axis=1)  # numpy: the first maximum
    hits = int((torch.from_numpy(am) == lab).sum())
    return loss, (p - onehot) / B, p, hits


def xent_inputs(B, C, seed, shifted):
    """randn * 3 logits and labels; shifted: every row moved by +-80 and (C >=
    2) row 0 holding a +88 / -88 pair (e^88 is the last power fp32 holds,
    e^-176 underflows): without the max subtraction the sums of the wide +80
    rows overflow and the loss is inf."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, generator=g) * 3
    lab = torch.randint(0, C, (B,), generator=g).to(torch.int32)
    if shifted:
        sign = (torch.arange(B) % 2).to(F32) * 2 - 1
        z = z + 80 * sign[:, None]
        if C >= 2:
            z[0] = 0
            z[0, 0], z[0, C - 1] = 88.0, -88.0
    return z, lab


def tie_rows(C):
    """Rows of exactly representable logits whose maximum sits at two or three
    classes, with the label on the lowest of them (twice for the first two
    placements, so that a highest-index rule counts another total), on a later
    one and on none -> (logits [11, C], labels, the hit of each row).  C >= 4."""
    places = [(1, C - 1), (0, C // 2, C - 1), (C - 2, C - 1)]
    rows, labs, hits = [], [], []
    for i, at in enumerate(places):
        other = next(c for c in range(C) if c not in at)
        for lab, hit in ((at[0], 1), (at[-1], 0), (other, 0)) + (((at[0], 1),) if i < 2 else ()):
            r = -torch.arange(C, dtype=F32) * 0.25 - 1
            r[list(at)] = 2.5
            rows.append(r)
            labs.append(lab)
            hits.append(hit)
    return torch.stack(rows), torch.tensor(labs, dtype=torch.int32), hits


# --------------------------------------------------------------- staging ----
def lr_ref(step, n_local, batch, base, decay):
    """base decay^epoch, epoch = (step batch) // n_local, float64 (base and
    decay the fp32 values)."""
    return float(np.float64(f32(base)) * np.float64(f32(decay)) ** np.float64((step * batch) // n_local))


def lr_f32(step, n_local, batch, base, decay):
    """The same in numpy float32, as the kernel forms it: the yardstick of powf."""
    e = np.float32((step * batch) // n_local)
    with np.errstate(under="ignore"):
        return float(np.float32(base) * np.power(np.float32(decay), e, dtype=np.float32))


def gather_steps(n_local, batch):
    """Steps 0 and 1, the first step whose offset has wrapped, the first one
    whose offset is the largest the pair reaches (n_local - batch - 1 when
    batch and n_local - batch are coprime), and 2^33 (the 64-bit product)."""
    mod = n_local - batch
    offs = [batch_offset(s, n_local, batch) for s in range(mod + 1)]
    wrapped = next((s for s in range(1, mod + 1) if offs[s] < offs[s - 1]), 1)
    top = offs.index(max(offs))
    return sorted({0, 1, wrapped, top, 2 ** 33})


# ------------------------------------------------------ stem re-layouts ----
def im2col_layout(R, S, C):
    """(sc, seg, kp) of ops/functional.py _ConvIm2colFn: sc = S C floats per
    tap row, seg = sc rounded up to 8, kp = R seg rounded up to 64."""
    sc = S * C
    seg = (sc + 7) // 8 * 8
    return sc, seg, (R * seg + 63) // 64 * 64


def stem_wt_ref(w, R, sc, seg, kp, K):
    """HWIO [R][sc][K] -> [K][kp], k = kh seg + j (j < sc), zero elsewhere."""
    w = w.reshape(R, sc, K)
    out = torch.zeros(K, kp, dtype=w.dtype)
    for k in range(kp):
        kh, j = divmod(k, seg)
        if kh < R and j < sc:
            out[:, k] = w[kh, j, :]
    return out


def stem_pad_mask(R, sc, seg, kp):
    """True at the k of [kp] no filter tap maps to."""
    k = torch.arange(kp)
    return ~((k // seg < R) & (k % seg < sc))


def stem_wgrad_ref(gpad, R, sc, seg, K):
    """[kp][K] -> HWIO [R][sc][K]: gw[kh][j] = gpad[kh seg + j]."""
    gw = torch.zeros(R, sc, K, dtype=gpad.dtype)
    for kh in range(R):
        for j in range(sc):
            gw[kh, j] = gpad[kh * seg + j]
    return gw


def s2d_k(ky, kx, ci):
    """The k of wt8 [co][256] / dw8 [256][K] that filter tap (ky, kx, ci) of
    the 7x7 kernel sits at: k = (a 4 + b) 16 + (p 2 + q) 3 + ci with ky = 2a +
    p - 1, kx = 2b + q - 1 (a, b < 4 the 4x4 tap, p, q < 2 inside the 2x2 block)."""
    a, p = divmod(ky + 1, 2)
    b, q = divmod(kx + 1, 2)
    return (a * 4 + b) * 16 + (p * 2 + q) * 3 + ci


def s2d_weight_ref(w, K):
    """HWIO [7][7][3][K] -> wt8 [K][256], by the forward direction of the
    layout comment: every (a, b, p, q, ci), zero off the kernel and on the 4
    padding channels."""
    w = w.reshape(7, 7, 3, K)
    out = torch.zeros(K, 256, dtype=w.dtype)
    for a in range(4):
        for b in range(4):
            for p in range(2):
                for q in range(2):
                    ky, kx = 2 * a + p - 1, 2 * b + q - 1
                    if not (0 <= ky < 7 and 0 <= kx < 7):
                        continue
                    for ci in range(3):
                        out[:, (a * 4 + b) * 16 + (p * 2 + q) * 3 + ci] = w[ky, kx, ci]
    return out


def s2d_real_mask():
    """True at the 147 k of [256] a real filter tap sits at."""
    m = torch.zeros(256, dtype=torch.bool)
    for ky in range(7):
        for kx in range(7):
            for ci in range(3):
                m[s2d_k(ky, kx, ci)] = True
    return m


def s2d_wgrad_ref(dw8, K):
    """dw8 [256][K] -> HWIO [7][7][3][K]."""
    dw8 = dw8.reshape(256, K)
    gw = torch.zeros(7, 7, 3, K, dtype=dw8.dtype)
    for ky in range(7):
        for kx in range(7):
            for ci in range(3):
                gw[ky, kx, ci] = dw8[s2d_k(ky, kx, ci)]
    return gw
