"""Float64 references of the layers between the convs: the channel reductions
and BatchNorm of csrc/kernels/bn.hip, the max and average pooling of
csrc/kernels/ops_generic.hip.  Plain torch / numpy, no GPU.  The input
generators and the bounds tests/test_layer_kernels_gpu.py compares with live
here too, so tests/test_layer_ref_cpu.py can show on the CPU that a subtly
wrong kernel would fail them.

Two modes, per element and per output, never a norm:

  exact:   small-integer operands for which every intermediate the kernel
           forms is a value fp32 holds; `holds_f32` asserts it on the float64
           intermediates.  The kernel must match bit for bit (a bf16 output
           after one RNE), whatever the block plan or summation order.
  rounded: seeded normals (bf16-rounded where the kernel reads bf16); the
           bound is derived per element in float64 from the operands:
           k EPS S for an expression of k fp32 operations (S the expression
           over absolute values), n EPS S for an n-term sum, + BF16_REL |ref|
           for a bf16 store.  Used only where dropping one row moves the
           reference by at least 4x the bound (`drop_row_ratio`).

Applies are operand-matched: the forward apply is evaluated in float64 with
the mean / rstd the kernel wrote (k = 5), the backward apply with the kernel's
db / dg (k = 8), so neither bound grows with the number of rows.

Layouts: activations [rows, C] (NHWC flattened) or NHWC; the conv-epilogue
statistics table [2][C / 64][P][64] ("grp64"); partial_kernel's table
[2][C][P] (channel-major)."""

from __future__ import annotations

import importlib.util
import os

import numpy as np
import torch

_spec = importlib.util.spec_from_file_location(
    "mnist_bf16_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "mnist_bf16_ref.py"))
_M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_M)
tol, check, failures = _M.tol, _M.check, _M.failures
bf16_rne, bf16_bits, bf16_trunc, bits_to_f32, as_bits = (_M.bf16_rne, _M.bf16_bits, _M.bf16_trunc,
                                                         _M.bits_to_f32, _M.as_bits)
same_bits, EPS, BF16_REL = _M.same_bits, _M.EPS, _M.BF16_REL

F64, F32 = torch.float64, torch.float32
EXACT_MAX = 2 ** 24
BN_EPS = float(np.float32(1e-5))       # the values the kernels get (fp32 arguments)
BN_MOM = float(np.float32(0.1))
PT, FUSED_MAXC, FIN64_MAXP, FU = 1024, 1024, 128, 4


def holds_f32(**named):
    """Exact mode's own condition: every float64 intermediate is a value fp32
    holds (it survives the round trip)."""
    for k, v in named.items():
        v = torch.as_tensor(v, dtype=F64)
        assert torch.equal(v.to(F32).to(F64), v), f"exact mode: {k} is not an fp32 value"


def check_abs(got, ref, t, bf16_out=False):
    """`check` with the bound t given per element (t = n EPS S with n = 1)."""
    t = torch.as_tensor(t, dtype=F64).expand(ref.shape)
    return ("tol",) + check(got, ref, t / EPS, 1, bf16_out)


def f32r(v):
    """float64 -> the nearest fp32 (one rounding), as fp32."""
    return torch.as_tensor(v, dtype=F64).to(F32)


# ------------------------------------------------------ reduction plans ----
def row_lanes(C):
    """Row lanes of a pass-1 block (bn.hip: partial_kernel / partial1_kernel)."""
    if C % 4 == 0:
        rp = 1
        while rp * 2 * (C // 4) <= PT:
            rp *= 2
        return rp
    return 256 // C


def nblocks(rows, C):
    """Mirror of bn::nblocks."""
    rp = row_lanes(C)
    if C % 4 == 0:
        nb = min((rows + rp * 8 - 1) // (rp * 8), 256)
    else:
        nb = min((rows + rp * 16 - 1) // (rp * 16), 1024)
    return max(nb, 1)


def chan_reduce_ok(C):
    return (C % 4 == 0 and 4 <= C <= 1024) or 1 <= C <= 256


def ws_floats(rows, C):
    return nblocks(rows, C) * 2 * C if chan_reduce_ok(C) else 0


def reduce_plan(rows, C):
    """-> dict(nb, rpb, rp, live threads, empty = blocks that start past the
    end, short = rows of the last non-empty block)."""
    nb = nblocks(rows, C)
    rpb = (rows + nb - 1) // nb
    empty = sum(1 for k in range(nb) if k * rpb >= rows)
    last = (rows - 1) // rpb
    width = C // 4 if C % 4 == 0 else C
    return dict(nb=nb, rpb=rpb, rp=row_lanes(C), live=row_lanes(C) * width, empty=empty,
                short=rows - last * rpb, last=last)


def fused_plan(rows, C, grid_cap):
    """The FU-deep loop of the fused finalize + apply kernels: -> dict(grid,
    trips of the outer loop, partial = the last trip's unrolled group breaks
    early (i >= n4) for some thread that entered it)."""
    n4 = rows * C // 4
    grid = min(max(min((n4 + 255) // 256, 8192), 1), grid_cap)
    stride = grid * 256
    trips = (n4 + FU * stride - 1) // (FU * stride)
    base = (trips - 1) * FU * stride
    return dict(n4=n4, grid=grid, stride=stride, trips=trips, partial=0 < n4 - base < FU * stride,
                ragged=n4 % stride != 0)


# --------------------------------------------------- A. channel reductions ----
def colsum_operands(rows, C, seed):
    """Integers in [-8, 8], thinned until sum |a b| and sum a^2 stay below
    2^24 per channel: every partial sum in any order is an exact integer."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-8, 9, (rows, C), generator=g).to(F64)
    b = torch.randint(-8, 9, (rows, C), generator=g).to(F64)
    keep = 1.0
    while max(float((a * a).sum(0).max()), float((a * b).abs().sum(0).max())) >= EXACT_MAX:
        keep *= 0.5
        a = a * (torch.rand(rows, C, generator=g) < keep)
    return a, b


def colsum_ref(a, b, mode):
    """mode 0: (sum a, sum a^2); mode 1: (sum a, sum a b).  Exact mode only."""
    p = a * a if mode == 0 else a * b
    assert float(a.abs().sum(0).max()) < EXACT_MAX and float(p.abs().sum(0).max()) < EXACT_MAX
    s1, s2 = a.sum(0), p.sum(0)
    holds_f32(a=a, b=b, prod=p, s1=s1, s2=s2)
    return s1, s2


# ------------------------------------------------------ B. bn_fwd, training ----
def bn_stats(x, K, rm0=None, rv0=None, eps=BN_EPS, mom=BN_MOM, exact=False, sums=None, rows=None):
    """fin_channel in float64 on shifted sums (K = the shift: row 0 of x, or
    the running mean for the table form), with the bound of every output.
    sums = (s1, s2): reduce a statistics table instead of x.  exact: the sums
    themselves are exact (integer operands), only the epilogue rounds.
    -> dict of (ref, tol) pairs: mean, var, rstd, rmean, rvar (+ 'ms', 'q')."""
    if sums is None:
        rows = x.shape[0]
        d = x - K
        s1, s2, Sabs = d.sum(0), (d * d).sum(0), d.abs().sum(0)
    else:
        s1, s2 = sums
        Sabs = s1.abs()
    A1 = Sabs / rows
    pow2 = rows & (rows - 1) == 0
    ms, q = s1 / rows, s2 / rows
    var = (q - ms * ms).clamp_min(0.0)
    m = ms + K
    rstd = 1.0 / torch.sqrt(var + eps)
    acc = 0.0 if exact else rows * EPS
    # a * inv rounds twice unless rows is a power of two; the n-term bound's
    # slack covers it in rounded mode, exact mode has no such slack
    t_div = 0.0 if (pow2 or not exact) else EPS * ms.abs()
    t_ms = acc * A1 + EPS * ms.abs()
    t_m = acc * A1 + EPS * m.abs() + t_div
    t_var = acc * q + 2 * ms.abs() * t_ms + 3 * EPS * (q + ms * ms)
    t_rstd = 0.5 * rstd ** 3 * t_var + 2 * EPS * rstd
    out = dict(ms=ms, q=q, s1=s1, s2=s2, mean=(m, t_m), var=(var, t_var), rstd=(rstd, t_rstd))
    if rm0 is not None:
        f = rows / (rows - 1) if rows > 1 else 1.0  # torch: unbiased; rows = 1: fin_channel keeps var
        unb = var * f
        t_unb = t_var * f + (EPS * unb if rows > 1 else 0.0)
        rmean = (1 - mom) * rm0 + mom * m
        rvar = (1 - mom) * rv0 + mom * unb
        out["rmean"] = (rmean, mom * t_m + 2 * EPS * rmean.abs())
        out["rvar"] = (rvar, mom * t_unb + 2 * EPS * rvar.abs())
    if exact:
        holds_f32(s1=s1, s2=s2)
        assert float(Sabs.max()) < EXACT_MAX and float(s2.max()) < EXACT_MAX
        if pow2:
            holds_f32(ms=ms, q=q, mean=m)
    return out


def bn_apply(x, m, r, g, b, res=None, relu=False, k=5):
    """y = (x - m) r g + b (+ res) (relu) in float64 with the statistics given
    (the kernel's own: operand-matched) -> (ref, tol = k EPS S).  A ReLU is
    1-Lipschitz and keeps the bound.  Eval mode: r = rsqrt(rvar + eps), k = 6."""
    y = (x - m) * r * g + b
    S = (x.abs() + m.abs()) * (r * g).abs() + b.abs()
    if res is not None:
        y, S = y + res, S + res.abs()
    if relu:
        y = y.clamp_min(0.0)
    return y, k * EPS * S


def bn_fwd_operands(rows, C, seed, x_bf16=False, kind="normal"):
    """Rounded-mode operands.  Channel means of either sign, |mean| >= 1, std
    0.5, and a running mean of the channel mean's sign (so the momentum blend
    has no cancellation and its 2 EPS |value| term is a bound).
    kind: normal | large_mean (1e3 (1 + u), std 1) | outlier (row 0 sits 50
    sigma off) | constant (every channel constant)."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, (C,), generator=g).to(F32) * 2 - 1
    mu = sign * (1.0 + torch.rand(C, generator=g))
    sd = 0.5
    if kind == "large_mean":
        mu, sd = 1e3 * (1.0 + torch.rand(C, generator=g)), 1.0
    x = mu + sd * torch.randn(rows, C, generator=g)
    if kind == "outlier":
        x[0] = mu + 50 * sd * sign
    if kind == "constant":
        x = mu.expand(rows, C).clone()
    if x_bf16:
        x = bf16_rne(x)
    o = dict(x=x, g=0.5 + torch.rand(C, generator=g), b=torch.randn(C, generator=g),
             res=torch.randn(rows, C, generator=g),
             rm0=mu * (0.5 + torch.rand(C, generator=g)), rv0=0.5 + torch.rand(C, generator=g))
    assert bool((torch.sign(x.to(F64).mean(0)) == torch.sign(o["rm0"].to(F64))).all()), \
        "running mean and batch mean must share a sign"
    return o


def bn_fwd_exact_operands(rows, C, seed, x_bf16=False):
    """Integer x in [-3, 3] (bf16 values too): with K = row 0 the shifted sums
    stay below 2^24 up to 16384 rows; integer running mean, g in {1/2, 1, 2}."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (rows, C), generator=g).to(F32)
    return dict(x=x, g=torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)],
                b=torch.randint(-2, 3, (C,), generator=g).to(F32),
                res=torch.randint(-3, 4, (rows, C), generator=g).to(F32),
                rm0=torch.randint(1, 4, (C,), generator=g).to(F32),
                rv0=torch.randint(1, 3, (C,), generator=g).to(F32))


def drop_row_ratio(x, K, exact=False):
    """The 4x condition of rounded mode, for the mean: a pass 1 that loses row
    r delivers a shifted sum short of x_r - K, so the mean moves by
    |x_r - K| / rows.  -> over r >= 1, the smallest of the largest (over
    channels) move / tol.  (Row 0 is the shift itself: its term is exactly 0,
    and only the apply sees it.)"""
    rows = x.shape[0]
    if rows == 1:
        return float("inf")
    m, t = bn_stats(x, K, exact=exact)["mean"]
    moved = (x[1:] - K).abs() / rows
    return float((moved / t).max(1).values.min())


# ---------------------------------------------------------------- D. bn_bwd ----
def bn_bwd_ref(x, dy, y, mean, rstd, relu, exact=False):
    """db = sum dy', dg = sum dy' xhat, dy' = dy [y > 0] under a ReLU.
    -> dict(dyp, db=(ref, tol), dg=(ref, tol)); n-term sum bounds (the three
    operations inside a dg term are the + 3)."""
    rows = x.shape[0]
    dyp = torch.where(y > 0, dy, torch.zeros_like(dy)) if relu else dy  # +0 where masked, as the kernel
    xh = (x - mean) * rstd
    t = dyp * xh
    db, dg = dyp.sum(0), t.sum(0)
    Sb = dyp.abs().sum(0)
    Sg = (dyp.abs() * (x.abs() + mean.abs()) * rstd).sum(0)
    if exact:
        holds_f32(xh=xh, t=t, db=db, dg=dg)
        assert float(Sb.max()) < EXACT_MAX and float(t.abs().sum(0).max()) < EXACT_MAX
        assert float(db.abs().max()) < 2 ** 20 and float(dg.abs().max()) < 2 ** 20
        tb = tg = torch.zeros_like(db)
    else:
        tb, tg = rows * EPS * Sb, (rows + 3) * EPS * Sg
    return dict(dyp=dyp, db=(db, tb), dg=(dg, tg))


def bn_bwd_apply(x, dyp, mean, rstd, g, db, dg, rows, exact=False):
    """dx = g r (dy' - db / rows - xhat dg / rows) in float64 with the sums
    given (the kernel's own) -> (ref, tol = 8 EPS S).  exact: every
    intermediate of the kernel's expression is asserted to be an fp32 value."""
    inv = 1.0 / rows
    xh = (x - mean) * rstd
    dx = g * rstd * (dyp - db * inv - xh * dg * inv)
    S = (g * rstd).abs() * (dyp.abs() + db.abs() * inv + (x.abs() + mean.abs()) * rstd * dg.abs() * inv)
    if exact:
        assert rows & (rows - 1) == 0
        holds_f32(a=db * inv, xh=xh, xb=xh * dg, t=xh * dg * inv, u=dyp - db * inv,
                  v=dyp - db * inv - xh * dg * inv, gr=g * rstd, dx=dx)
    return dx, 8 * EPS * S


def bn_bwd_operands(rows, C, seed, exact, x_bf16=False):
    """exact: integer mean, rstd in {1/4, 1/2, 1, 2}, g in {1/2, 1, 2}, all
    per channel (a channel mix-up changes bits), integer x and dy, y a sign
    pattern with exact zeros.  rounded: normals; mean / rstd arbitrary (the
    backward takes them as operands)."""
    gen = torch.Generator().manual_seed(seed)
    y = torch.tensor([-1.0, 0.0, 0.0, 1.0, 2.0])[torch.randint(0, 5, (rows, C), generator=gen)]
    if exact:
        return dict(x=torch.randint(-3, 4, (rows, C), generator=gen).to(F32),
                    dy=torch.randint(-4, 5, (rows, C), generator=gen).to(F32), y=y,
                    mean=torch.randint(-1, 2, (C,), generator=gen).to(F32),
                    rstd=torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (C,), generator=gen)],
                    g=torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=gen)])
    x = 0.7 + 1.3 * torch.randn(rows, C, generator=gen)
    return dict(x=bf16_rne(x) if x_bf16 else x, dy=torch.randn(rows, C, generator=gen), y=y,
                mean=0.7 + 0.2 * torch.randn(C, generator=gen),
                rstd=0.4 + 0.6 * torch.rand(C, generator=gen),
                g=0.5 + torch.rand(C, generator=gen))


def drop_row_ratio_bwd(o, relu):
    """The 4x condition for db: as drop_row_ratio."""
    r = bn_bwd_ref(o["x"].to(F64), o["dy"].to(F64), o["y"].to(F64), o["mean"].to(F64),
                   o["rstd"].to(F64), relu)
    db, t = r["db"]
    moved = r["dyp"].abs()  # dropping row r moves db by |dy'_r|
    return float((moved / t).max(1).values.min())


# -------------------------------------------------------- E. partial tables ----
def table_operands(C, P, seed):
    """A grp64 table [2][C / 64][P][64] of distinct-looking integers: first
    moments in [-20, 20], second moments in [200, 400] (so the variance of a
    256-row layer is positive and no clamp hides an error)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.empty(2, C // 64, P, 64)
    t[0] = torch.randint(-20, 21, (C // 64, P, 64), generator=g).to(F32)
    t[1] = torch.randint(200, 401, (C // 64, P, 64), generator=g).to(F32)
    return t


def table_sums(t):
    """[2][C / 64][P][64] -> (s1 [C], s2 [C]) in float64; integer tables sum
    exactly in any order."""
    t = t.to(F64)
    assert float(t.abs().sum(2).max()) < EXACT_MAX
    s = t.sum(2).reshape(2, -1)
    holds_f32(s1=s[0], s2=s[1])
    return s[0], s[1]


def table_as_channel_major(t):
    """The wrong reading: the same floats taken as [2][C][P]."""
    two, G, P, _ = t.shape
    s = t.to(F64).reshape(2, G * 64, P).sum(2)
    return s[0], s[1]


# ------------------------------------------------------------ F. max pooling ----
def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def pool_data(N, H, W, C, mode, seed):
    """distinct: a seeded choice without repetition among the 32768 bf16
    values of either sign with magnitude in [2^-63, 2^65): no two elements of
    the tensor are equal, and the bf16 kernels read the same numbers;
    ties: values from {0, 0, 0, 1, 2}, as after a ReLU."""
    g = torch.Generator().manual_seed(seed)
    n = N * H * W * C
    if mode == "ties":
        return torch.tensor([0.0, 0.0, 0.0, 1.0, 2.0])[torch.randint(0, 5, (n,), generator=g)].reshape(N, H, W, C)
    bits = torch.arange(0x2000, 0x6000, dtype=torch.int64)
    bits = torch.cat([bits, bits + 0x8000])
    assert n <= bits.numel(), "distinct mode: more elements than values"
    pick = bits[torch.randperm(bits.numel(), generator=g)[:n]]
    v = bits_to_f32(torch.from_numpy(pick.numpy().astype(np.uint16).view(np.int16).copy()))
    assert v.unique().numel() == n
    return v.reshape(N, H, W, C)


def maxpool_ref(x, k, s, p, last_wins=False, wrap_pad=False, tap_shift=0):
    """Written out by hand: scan (kh, kw) in order, skip padding taps, a
    strictly greater value replaces the best (the first maximum wins).
    -> y [N, OH, OW, C] float64, tap32 (flat pixel index (n H + iy) W + ix,
    int32), tap8 (kh k + kw, uint8).  The keyword arguments are the mutants of
    the CPU file."""
    x = x.to(F64)
    N, H, W, C = x.shape
    OH, OW = out_hw(H, W, k, s, p)
    best = torch.full((N, OH, OW, C), -float("inf"), dtype=F64)
    tap32 = torch.full((N, OH, OW, C), -1, dtype=torch.int64)
    tap8 = torch.full((N, OH, OW, C), 255, dtype=torch.int64)
    flat = x.reshape(N * H * W, C)
    nn = torch.arange(N).reshape(N, 1, 1)
    for kh in range(k):
        for kw in range(k):
            iy = (torch.arange(OH) * s - p + kh + tap_shift).reshape(1, OH, 1)
            ix = (torch.arange(OW) * s - p + kw).reshape(1, 1, OW)
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            idx = (nn * H + iy) * W + ix
            if wrap_pad:  # a column tap off the row lands in the neighbouring row
                ok = (iy >= 0) & (iy < H) & (idx >= 0) & (idx < N * H * W)
            ok = ok.expand(N, OH, OW)
            idx = idx.expand(N, OH, OW)
            v = flat[idx.clamp(0, N * H * W - 1)]
            upd = ok.unsqueeze(-1) & ((v >= best) if last_wins else (v > best))
            best = torch.where(upd, v, best)
            tap32 = torch.where(upd, idx.unsqueeze(-1).expand_as(upd), tap32)
            tap8 = torch.where(upd, torch.full_like(tap8, kh * k + kw), tap8)
    return best, tap32.to(torch.int32), tap8.to(torch.uint8)


def tap8_to_pixel(tap8, N, H, W, k, s, p):
    """uint8 window tap -> the flat pixel index of the int32 form."""
    _, OH, OW, C = tap8.shape
    t = tap8.to(torch.int64)
    iy = torch.arange(OH).reshape(1, OH, 1, 1) * s - p + t // k
    ix = torch.arange(OW).reshape(1, 1, OW, 1) * s - p + t % k
    return (torch.arange(N).reshape(N, 1, 1, 1) * H + iy) * W + ix


def maxpool_bwd_ref(dy, tap32, N, H, W, all_ties=None):
    """dx[pixel] = the sum of the dy of the windows whose tap is this pixel.
    all_ties = (x, k, s, p): the mutant that routes the gradient to every tap
    that equals the maximum."""
    dy = dy.to(F64)
    C = dy.shape[-1]
    dx = torch.zeros(N * H * W * C, dtype=F64)
    c = torch.arange(C).expand_as(tap32)
    if all_ties is None:
        dx.index_add_(0, (tap32.to(torch.int64) * C + c).reshape(-1), dy.reshape(-1))
    else:
        x, k, s, p = all_ties
        y, _, _ = maxpool_ref(x, k, s, p)
        OH, OW = y.shape[1:3]
        flat = x.to(F64).reshape(N * H * W, C)
        for kh in range(k):
            for kw in range(k):
                iy = (torch.arange(OH) * s - p + kh).reshape(1, OH, 1)
                ix = (torch.arange(OW) * s - p + kw).reshape(1, 1, OW)
                ok = ((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)).expand(N, OH, OW)
                idx = ((torch.arange(N).reshape(N, 1, 1) * H + iy) * W + ix).expand(N, OH, OW)
                hit = ok.unsqueeze(-1) & (flat[idx.clamp(0, N * H * W - 1)] == y)
                dx.index_add_(0, (idx.unsqueeze(-1) * C + c).clamp(0, dx.numel() - 1)[hit], dy[hit])
    dx = dx.reshape(N, H, W, C)
    holds_f32(dx=dx)
    return dx


def pool_dy(N, OH, OW, C, seed):
    g = torch.Generator().manual_seed(seed + 77)
    return torch.randint(-4, 5, (N, OH, OW, C), generator=g).to(F32)


# ------------------------------------------------------ G. global average pool ----
def avgpool_operands(N, HW, C, seed):
    """Integers (exact mode) where HW is a power of two, normals otherwise."""
    g = torch.Generator().manual_seed(seed)
    if HW & (HW - 1) == 0:
        return torch.randint(-8, 9, (N, HW, C), generator=g).to(F32), True
    return torch.randn(N, HW, C, generator=g), False


def avgpool_ref(x, exact, drop_pixel=None, count=None):
    """-> (mean over HW, tol = (HW + 1) EPS S / HW: HW additions and the
    division).  drop_pixel / count: the mutants."""
    x = x.to(F64)
    HW = x.shape[1]
    xs = x if drop_pixel is None else torch.cat([x[:, :drop_pixel], x[:, drop_pixel + 1:]], 1)
    s = xs.sum(1)
    y = s / (HW if count is None else count)
    if exact and drop_pixel is None and count is None:
        holds_f32(s=s, y=y)
    return y, (HW + 1) * EPS * x.abs().sum(1) / HW


def avgpool_bwd_ref(dy, HW):
    """fp32(dy) * fp32(1 / HW), rounded once: the kernel's expression."""
    inv = float(np.float32(1.0) / np.float32(HW))
    N, C = dy.shape
    return f32r(dy.to(F64) * inv).reshape(N, 1, C).expand(N, HW, C)


# ------------------------------------------- the checks of a BatchNorm call ----
# Shared by the GPU file (on what the kernels wrote) and the CPU file (on
# simulated outputs and their mutants).
def _bits16(t):
    """bf16 tensor -> its int16 bit patterns (int16 bits pass through)."""
    return t.contiguous().view(torch.int16) if t.dtype == torch.bfloat16 else t


def check_apply(res, got, yref, t):
    """y and / or its bf16 twin against the operand-matched reference."""
    if got["y"] is not None:
        res["y"] = check_abs(got["y"], yref, t)
        if got["yb"] is not None:
            res["yb twin"] = same_bits(_bits16(got["yb"]), bf16_bits(got["y"]).reshape(yref.shape))
    else:
        res["yb"] = check_abs(got["yb"].to(F32), yref, t, bf16_out=True)


def check_bn_fwd(o, relu, res, got, exact, st=None):
    """Every output of a training-mode forward (got: fp32 tensors, yb a bf16
    tensor or None) against bn_stats and the operand-matched apply."""
    x = o["x"].to(F64)
    if st is None:
        st = bn_stats(x, x[0], o["rm0"].to(F64), o["rv0"].to(F64), exact=exact)
    out = {}
    rows = x.shape[0]
    if exact and rows & (rows - 1) == 0:
        out["mean"] = same_bits(got["mean"], st["mean"][0].to(F32))
    else:
        out["mean"] = check_abs(got["mean"], *st["mean"])
    for k in ("rstd", "rmean", "rvar"):
        out[k] = check_abs(got[k], *st[k])
    yref, t = bn_apply(x, got["mean"].to(F64), got["rstd"].to(F64), o["g"].to(F64), o["b"].to(F64),
                       o["res"].to(F64) if res else None, relu)
    check_apply(out, got, yref, t)
    return out


def check_bn_bwd(o, relu, got, exact, sums=None):
    """sums: the reference (db, dg) of a statistics table (the table form)."""
    x, dy, y, mean, rstd, g = (o[k].to(F64) for k in ("x", "dy", "y", "mean", "rstd", "g"))
    rows = x.shape[0]
    r = bn_bwd_ref(x, dy, y, mean, rstd, relu, exact=exact and sums is None)
    out = {}
    if sums is not None:
        out["db"], out["dg"] = same_bits(got["db"], sums[0].to(F32)), same_bits(got["dg"], sums[1].to(F32))
    elif exact:
        out["db"], out["dg"] = same_bits(got["db"], r["db"][0].to(F32)), same_bits(got["dg"], r["dg"][0].to(F32))
    else:
        out["db"], out["dg"] = check_abs(got["db"], *r["db"]), check_abs(got["dg"], *r["dg"])
    if got["dres"] is not None:
        out["dres"] = same_bits(got["dres"], r["dyp"].to(F32))
    bitwise = exact and sums is None
    dxr, t = bn_bwd_apply(x, r["dyp"], mean, rstd, g, got["db"].to(F64), got["dg"].to(F64), rows, exact=bitwise)
    if got["dx"] is not None:
        out["dx"] = same_bits(got["dx"], dxr.to(F32)) if bitwise else check_abs(got["dx"], dxr, t)
        if got["dxb"] is not None:
            out["dxb twin"] = same_bits(_bits16(got["dxb"]), bf16_bits(got["dx"]).reshape(dxr.shape))
    elif bitwise:
        out["dxb"] = same_bits(_bits16(got["dxb"]), bf16_bits(dxr.to(F32)).reshape(dxr.shape))
    else:
        out["dxb"] = check_abs(got["dxb"].to(F32), dxr, t, bf16_out=True)
    return out
