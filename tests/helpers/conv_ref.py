"""Float64 references of the generic engine's convolutions (conv_bf16.hip,
conv_tiled.hip and the direct kernels of ops_generic.hip), plain torch, no GPU,
and the two ways tests/test_conv_routes_gpu.py compares a kernel with them.

rounded mode: the operands are seeded normals already rounded to bf16 (RNE, on
the host), so the reference multiplies the very numbers the kernel multiplies.
What is left between the two is the fp32 accumulation order plus, for a bf16
output, one rounding, and the bound per element is the derived `tol()` of
mnist_bf16_ref.py: n 2^-23 S, plus 2^-8 (|ref| + acc) for a bf16 store.

exact mode: the operands are small integers, thinned by a seeded mask until
every sum of absolute products (the `S` of each reference, and the sums of
squares of the statistics) stays below 2^24.  Every product and every partial
sum in any order is then an integer fp32 holds exactly: the kernel's result
must equal the reference bit for bit (after one RNE for a bf16 output)
whatever the tile, split or slab order.  A single dropped, doubled or
misplaced product changes an integer, however many terms the sum has.

Layouts: activations NHWC, weights HWIO.  Every reference returns (ref, S, n):
S the same operation on |operands|, n the products per output.  The
convolutions are written as one matrix product per filter tap over the shifted
image (BLAS in float64, or in float32 for exact mode, where it is exact too);
tests/test_conv_ref_cpu.py checks them against torch's own convolution."""

from __future__ import annotations

import importlib.util
import os

import torch
import torch.nn.functional as F

_spec = importlib.util.spec_from_file_location(
    "mnist_bf16_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mnist_bf16_ref.py"))
_M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_M)
tol, check, failures = _M.tol, _M.check, _M.failures
bf16_rne, bf16_bits, as_bits, bf16_trunc, bits_to_f32 = (_M.bf16_rne, _M.bf16_bits, _M.as_bits,
                                                         _M.bf16_trunc, _M.bits_to_f32)
same_bits, EPS, BF16_REL = _M.same_bits, _M.EPS, _M.BF16_REL

F64 = torch.float64
F32 = torch.float32
EXACT_MAX = 2 ** 24


def out_hw(H, W, R, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1


# ---------------------------------------------------------- convolutions ----
def _taps(x, w, stride, pad):
    """The padded image and, per tap, the slice of it that meets w[kh, kw]."""
    N, H, W, C = x.shape
    R, S = w.shape[0], w.shape[1]
    OH, OW = out_hw(H, W, R, stride, pad)
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    for kh in range(R):
        for kw in range(S):
            yield kh, kw, xp[:, kh:kh + stride * (OH - 1) + 1:stride, kw:kw + stride * (OW - 1) + 1:stride, :]


def _fwd(x, w, stride, pad):
    N, H, W, C = x.shape
    R, K = w.shape[0], w.shape[3]
    OH, OW = out_hw(H, W, R, stride, pad)
    y = torch.zeros(N * OH * OW, K, dtype=x.dtype)
    for kh, kw, xs in _taps(x, w, stride, pad):
        y += xs.reshape(-1, C) @ w[kh, kw]
    return y.reshape(N, OH, OW, K)


def _dgrad(dy, w, stride, pad, H, W):
    N, OH, OW, K = dy.shape
    R, S, C = w.shape[0], w.shape[1], w.shape[2]
    dxp = torch.zeros(N, H + 2 * pad, W + 2 * pad, C, dtype=dy.dtype)
    d = dy.reshape(-1, K)
    for kh in range(R):
        for kw in range(S):
            dxp[:, kh:kh + stride * (OH - 1) + 1:stride, kw:kw + stride * (OW - 1) + 1:stride, :] += \
                (d @ w[kh, kw].t()).reshape(N, OH, OW, C)
    return dxp[:, pad:pad + H, pad:pad + W, :].contiguous()


def _wgrad(x, dy, stride, pad, R):
    C, K = x.shape[3], dy.shape[3]
    dw = torch.zeros(R, R, C, K, dtype=x.dtype)
    d = dy.reshape(-1, K)
    for kh, kw, xs in _taps(x, dw, stride, pad):
        dw[kh, kw] = xs.reshape(-1, C).t() @ d
    return dw


def conv_fwd(x, w, stride, pad, bias=None, relu=False, addend=None, dt=F64):
    """y = conv(x, w) (+ bias) (ReLU) (+ addend).  A bias and an addend are one
    more term each; ReLU is 1-Lipschitz and leaves the bound as it is."""
    x, w = x.to(dt), w.to(dt)
    ref, S = _fwd(x, w, stride, pad), _fwd(x.abs(), w.abs(), stride, pad)
    n = w.shape[0] * w.shape[1] * w.shape[2]
    if bias is not None:
        ref, S, n = ref + bias.to(dt), S + bias.to(dt).abs(), n + 1
    if relu:
        ref = ref.clamp_min(0)
    if addend is not None:
        ref, S, n = ref + addend.to(dt), S + addend.to(dt).abs(), n + 1
    return ref, S, n


def conv_dgrad(dy, w, stride, pad, H, W, addend=None, dt=F64):
    """dX [N, H, W, C] = conv^T(dY, w) (+ addend)."""
    dy, w = dy.to(dt), w.to(dt)
    ref, S = _dgrad(dy, w, stride, pad, H, W), _dgrad(dy.abs(), w.abs(), stride, pad, H, W)
    n = w.shape[0] * w.shape[1] * w.shape[3]
    if addend is not None:
        ref, S, n = ref + addend.to(dt), S + addend.to(dt).abs(), n + 1
    return ref, S, n


def conv_wgrad(x, dy, stride, pad, R, dt=F64):
    """dW [R, R, C, K] = sum over the N OH OW output pixels of x (shifted) dY."""
    x, dy = x.to(dt), dy.to(dt)
    ref, S = _wgrad(x, dy, stride, pad, R), _wgrad(x.abs(), dy.abs(), stride, pad, R)
    return ref, S, dy.shape[0] * dy.shape[1] * dy.shape[2]


def bias_grad(dy, dt=F64):
    d = dy.to(dt).reshape(-1, dy.shape[-1])
    return d.sum(0), d.abs().sum(0), d.shape[0]


# ------------------------------------------------------------ statistics ----
def stats_fwd(yb, shift, dt=F64):
    """The BatchNorm forward sums a conv epilogue (or its slab reduction)
    writes: per channel sum (yb - shift) and sum (yb - shift)^2 over the rows,
    yb the bf16 outputs the kernel stored.  -> (s1, S1, s2, S2, n); n = rows
    + 2: the additions, one rounding of the subtraction, one of the square."""
    d = yb.to(dt).reshape(-1, yb.shape[-1]) - shift.to(dt)
    return d.sum(0), d.abs().sum(0), (d * d).sum(0), (d * d).sum(0), d.shape[0] + 2


def stats_bwd(dx, x, y, mean, rstd, relu, dt=F64):
    """The BatchNorm backward sums a dgrad epilogue (BnBwdStats) writes, from
    the kernel's own fp32 dX: d = dX [y > 0] (relu), s1 = sum d, s2 = sum d
    (x - mean) rstd.  -> (s1, S1, s2, S2, n1, n2).  n1 = rows (additions
    only); n2 = rows + 3: the epilogue rounds x - mean, the product with d and
    the product with rstd (`d * (xv - mu) * rs` in conv3_kernel's epilogue 2,
    dgrad3s2_kernel and slab_sum4_kernel) before each addition."""
    C = dx.shape[-1]
    d = dx.to(dt).reshape(-1, C)
    if relu:
        d = d * (y.to(dt).reshape(-1, C) > 0).to(dt)
    e = d * (x.to(dt).reshape(-1, C) - mean.to(dt)) * rstd.to(dt)
    return d.sum(0), d.abs().sum(0), e.sum(0), e.abs().sum(0), d.shape[0], d.shape[0] + 3


def part_sums(part, C, P):
    """The statistics table [2][C / 64][P][64] summed over its P partial rows
    (float64) -> (s1 [C], s2 [C])."""
    t = part.detach().cpu().to(F64).reshape(2, C // 64, P, 64).sum(2).reshape(2, C)
    return t[0], t[1]


# --------------------------------------------------------------- compare ----
def where_over(got, ref, S, n, bf16_out=False, limit=8):
    """Coordinates, values and bounds of the first elements over the bound."""
    t = tol(ref, S, n, bf16_out)
    err = (got.to(F64) - ref).abs()
    idx = (err > t).nonzero()[:limit]
    return [(tuple(int(v) for v in i), float(got[tuple(i)]), float(ref[tuple(i)]), float(t[tuple(i)]))
            for i in idx]


def exact_diff(got, ref, bf16_out=False):
    """exact mode: elements of got that differ from the reference (an integer
    table; one host RNE for a bf16 output), +0 == -0.  -> (count, first
    coordinates)."""
    ref = ref.to(F32)
    if bf16_out:
        ref = bf16_rne(ref)
    bad = got.detach().cpu().to(F32) != ref
    return int(bad.sum()), [tuple(int(v) for v in i) for i in bad.nonzero()[:8]]


def guard_hits(buf, n, canary):
    """Elements of the guard band buf[n:] that no longer hold the canary."""
    return int((buf.reshape(-1)[n:] != canary).sum())


# ------------------------------------------------------------- operands ----
def gen_rounded(seed, N, H, W, C, K, R, stride, pad, bias=False, addend=False):
    """Seeded normal operands already rounded to bf16 (fp32 tensors holding
    bf16 values); the filter scaled to unit output variance.  bias / addend
    stay plain fp32: the kernels add them in fp32."""
    g = torch.Generator().manual_seed(seed)
    OH, OW = out_hw(H, W, R, stride, pad)
    o = dict(x=bf16_rne(torch.randn(N, H, W, C, generator=g)),
             w=bf16_rne(torch.randn(R, R, C, K, generator=g) * (R * R * C) ** -0.5),
             dy=bf16_rne(torch.randn(N, OH, OW, K, generator=g)))
    if bias:
        o["bias"] = torch.randn(K, generator=g) * 0.1
    if addend:
        o["addend"] = torch.randn(N, H, W, C, generator=g)
    return o


def _ints(g, shape, lim, density):
    v = torch.randint(-lim, lim + 1, shape, generator=g).to(F32)
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density).to(F32)
    return v


def gen_exact(seed, N, H, W, C, K, R, stride, pad, bias=False, addend=False, relu=False, lim=3,
              density=1.0, also=None):
    """Integer operands in [-lim, lim], thinned by a seeded mask (density
    halved until it holds) so that the S of the forward, the backward-data and
    the filter gradient - the sum of |products| of every output, an upper bound
    of every partial sum in any order - is below 2^24.  also(o) -> an extra
    magnitude that has to stay below 2^24 too (sums of squares of statistics).
    -> the operands, with o["density"] the density that held."""
    OH, OW = out_hw(H, W, R, stride, pad)
    while True:
        g = torch.Generator().manual_seed(seed)
        o = dict(x=_ints(g, (N, H, W, C), lim, density), w=_ints(g, (R, R, C, K), lim, density),
                 dy=_ints(g, (N, OH, OW, K), lim, density), density=density)
        if bias:
            o["bias"] = _ints(g, (K,), 8, 1.0)
        if addend:
            o["addend"] = _ints(g, (N, H, W, C), 8, 1.0)
        # (kept: in exact mode these fp32 results are the references themselves)
        o["refs"] = dict(fwd=conv_fwd(o["x"], o["w"], stride, pad, o.get("bias"), relu, dt=F32),
                         dgrad=conv_dgrad(o["dy"], o["w"], stride, pad, H, W, o.get("addend"), dt=F32),
                         wgrad=conv_wgrad(o["x"], o["dy"], stride, pad, R, dt=F32))
        top = max(float(r[1].max()) for r in o["refs"].values())
        if also is not None:
            top = max(top, float(also(o)))
        if top < EXACT_MAX:
            assert_exact(top)
            return o
        density *= 0.5
        assert density > 1e-3, "exact mode: no density keeps the sums below 2^24"


def assert_exact(*mags):
    """The one condition of exact mode: every sum of magnitudes below 2^24."""
    for m in mags:
        assert float(m) < EXACT_MAX, f"exact mode needs every |sum| < 2^24, got {float(m):.4g}"
