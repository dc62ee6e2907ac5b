"""The conv references and the two comparison modes of tests/helpers/conv_ref.py,
checked without a GPU: the per-tap references against torch's own convolution,
a torch emulation of a correct kernel (float64 on bf16-rounded operands, cast
through fp32, bf16 RNE store where the route has one; integers in exact mode)
against `check` / bit equality, and a list of planted faults - the mistakes
tile kernels make: ragged tiles, pad edges, store paths, split-K slabs, tap
and parity maps, structural zeros, stale weight copies, statistics rows, and
the 128-column tile on K % 128 == 64 - each of which has to fail.

For four of them the old criterion of tests/test_generic_ops_gpu.py, the norm
ratio < 1e-2 against fp32 torch on unrounded operands, is evaluated too, at
the sizes where the wide tiles run: it accepts three outright and misses the
fourth by a tenth of its bound, which is why tests/test_conv_routes_gpu.py
exists."""

import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("conv_ref", os.path.join(_HERE, "helpers", "conv_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)
F32, F64 = torch.float32, torch.float64


def _rel(a, b):  # the old criterion (tests/test_generic_ops_gpu.py)
    return ((a.float() - b.float()).norm() / max(1e-12, b.float().norm())).item()


def _torch_conv(x, w, stride, pad):
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), stride=stride,
                    padding=pad).permute(0, 2, 3, 1)


def _over(got, ref, S, n, **kw):
    worst, over, nzero = R.check(got, ref, S, n, **kw)
    return over + nzero


def bf16_half_away(x):
    """fp32 -> bf16 by adding half an ulp and truncating (ties away from zero:
    the wrong rounding)."""
    u = x.contiguous().view(torch.int32)
    return ((u + 0x8000) & ~0xFFFF).view(F32)


# ------------------------------------------------------------ references ----
@pytest.mark.parametrize("N,H,W,C,K,R_,stride,pad", [
    (2, 7, 9, 5, 6, 3, 1, 1), (2, 8, 8, 4, 6, 3, 2, 1), (2, 7, 7, 4, 6, 3, 2, 1), (2, 6, 8, 8, 4, 1, 2, 0),
    (1, 11, 9, 3, 8, 7, 2, 3), (2, 9, 7, 3, 4, 5, 1, 2), (2, 5, 5, 4, 4, 1, 1, 0)])
def test_references_equal_torch_convolution(N, H, W, C, K, R_, stride, pad):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, H, W, C, generator=g, dtype=F64).requires_grad_(True)
    w = torch.randn(R_, R_, C, K, generator=g, dtype=F64).requires_grad_(True)
    y = _torch_conv(x, w, stride, pad)
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    y.backward(dy)
    ref, S, n = R.conv_fwd(x.detach(), w.detach(), stride, pad)
    assert n == R_ * R_ * C and torch.allclose(ref, y.detach(), rtol=0, atol=1e-12)
    assert torch.allclose(S, _torch_conv(x.detach().abs(), w.detach().abs(), stride, pad), rtol=0, atol=1e-12)
    ref, S, n = R.conv_dgrad(dy, w.detach(), stride, pad, H, W)
    assert n == R_ * R_ * K and torch.allclose(ref, x.grad, rtol=0, atol=1e-12)
    ref, S, n = R.conv_wgrad(x.detach(), dy, stride, pad, R_)
    assert n == N * y.shape[1] * y.shape[2] and torch.allclose(ref, w.grad, rtol=0, atol=1e-12)
    assert (S >= ref.abs() - 1e-12).all()


def test_epilogue_terms_and_statistics_references():
    o = R.gen_rounded(3, 2, 6, 6, 8, 8, 3, 1, 1, bias=True, addend=True)
    a = o["addend"][:, :, :, :8]
    ref, S, n = R.conv_fwd(o["x"], o["w"], 1, 1, o["bias"], True, a)
    plain = _torch_conv(o["x"].double(), o["w"].double(), 1, 1)
    assert n == 74 and torch.allclose(ref, (plain + o["bias"].double()).clamp_min(0) + a.double(), atol=1e-12)
    yb = R.bf16_rne(ref.float())
    shift = torch.randn(8)
    s1, S1, s2, S2, ns = R.stats_fwd(yb, shift)
    d = yb.double().reshape(-1, 8) - shift.double()
    assert ns == 74 and torch.allclose(s1, d.sum(0)) and torch.allclose(s2, (d * d).sum(0))
    mean, rstd = torch.randn(8), torch.rand(8) + 0.5
    t1, T1, t2, T2, n1, n2 = R.stats_bwd(ref.float(), o["x"], yb, mean, rstd, True)
    dd = ref.float().double().reshape(-1, 8) * (yb.reshape(-1, 8) > 0)
    assert (n1, n2) == (72, 75) and torch.allclose(t1, dd.sum(0))
    assert torch.allclose(t2, (dd * (o["x"].double().reshape(-1, 8) - mean.double()) * rstd.double()).sum(0))
    # the table layout [2][C / 64][P][64]
    part = torch.arange(2 * 128 * 3, dtype=F32)
    p1, p2 = R.part_sums(part, 128, 3)
    assert p1[70] == sum(float(part[(1 * 3 + r) * 64 + 6]) for r in range(3))
    assert p2[5] == sum(float(part[128 * 3 + r * 64 + 5]) for r in range(3))


def test_generators_hold_their_conditions():
    o = R.gen_rounded(5, 2, 6, 6, 64, 64, 3, 1, 1)
    for k in ("x", "w", "dy"):
        assert torch.equal(R.bf16_rne(o[k]), o[k])  # already bf16 values: conversions are exact
    o = R.gen_exact(5, 2, 6, 6, 64, 64, 3, 1, 1, bias=True, addend=True)
    for k in ("x", "w", "dy", "bias", "addend"):
        assert torch.equal(o[k], o[k].round())
    assert o["density"] == 1.0 and max(float(r[1].max()) for r in o["refs"].values()) < 2 ** 24
    # exact mode's references are fp32 and equal torch's own fp32 convolution of the same integers
    x, w = o["x"].clone().requires_grad_(True), o["w"].clone().requires_grad_(True)
    y = _torch_conv(x, w, 1, 1) + o["bias"]
    y.backward(o["dy"])
    assert o["refs"]["fwd"][0].dtype == F32 and torch.equal(o["refs"]["fwd"][0], y.detach())
    assert torch.equal(o["refs"]["dgrad"][0], x.grad + o["addend"])
    assert torch.equal(o["refs"]["wgrad"][0], w.grad)
    # the largest filter gradient of the GPU tests (n = 100352 pixels) stays exact undiluted
    assert 100352 * 3 * 3 < 2 ** 24
    # a magnitude that cannot hold is thinned: the sum of squares of a statistic
    o = R.gen_exact(5, 2, 6, 6, 64, 64, 3, 1, 1,
                    also=lambda o: (o["refs"]["fwd"][0] ** 2).sum((0, 1, 2)).max() * 4000)
    assert o["density"] < 1.0
    with pytest.raises(AssertionError):
        R.assert_exact(2.0 ** 24)


# ----------------------------------------------- the table's base convs ----
class Base:
    """3x3 s1 64 -> 64 at N images of H x H: unrounded operands (the old
    criterion's reference), their bf16 roundings (what the kernel multiplies),
    the float64 reference of those and the emulated fp32 result."""

    def __init__(self, N, H):
        g = torch.Generator().manual_seed(7)
        self.x = torch.randn(N, H, H, 64, generator=g)
        self.w = torch.randn(3, 3, 64, 64, generator=g) * 0.1
        self.old = _torch_conv(self.x, self.w, 1, 1)  # fp32 torch, unrounded operands
        self.xb, self.wb = R.bf16_rne(self.x), R.bf16_rne(self.w)
        self.ref, self.S, self.n = R.conv_fwd(self.xb, self.wb, 1, 1)
        self.y = self.ref.to(F32)
        self.M = N * H * H

    def tap_rows(self, kh, kw):
        """[M, 64] activations that meet tap (kh, kw), zero where padded."""
        xp = F.pad(self.xb, (0, 0, 1, 1, 1, 1)).double()
        H = self.xb.shape[1]
        return xp[:, kh:kh + H, kw:kw + H, :].reshape(-1, 64)


@pytest.fixture(scope="module")
def small():
    return Base(1, 28)  # M = 784


@pytest.fixture(scope="module")
def wide():
    return Base(10, 56)  # M = 31360: the size that took 128-row tiles


def test_clean_conv_passes_both_criteria(small, wide):
    for b in (small, wide):
        assert _over(b.y, b.ref, b.S, b.n) == 0
        assert _over(R.bf16_rne(b.y), b.ref, b.S, b.n, bf16_out=True) == 0
        assert 2.0e-3 < _rel(b.y, b.old) < 2.7e-3  # operand rounding alone: 2.35e-3 of the 1e-2
    # fp32 accumulation in another order (torch's own fp32 conv on the same operands)
    y32 = _torch_conv(small.xb, small.wb, 1, 1)
    worst, over, _ = R.check(y32, small.ref, small.S, small.n)
    assert over == 0 and worst < 0.1


def test_fault_truncating_store_whole_tensor(small):
    got = R.bf16_trunc(small.y)
    assert _rel(got, small.old) < 1e-2  # the old criterion accepts it (4.1e-3)
    assert _over(got, small.ref, small.S, small.n, bf16_out=True) > 1000


def test_fault_cells_of_last_tile_never_stored(wide):
    got = wide.y.clone().reshape(-1, 64)
    got[wide.M - 8:, 16:32] = 0.0  # 8 x 16 cells the epilogue left out
    got = got.reshape(wide.y.shape)
    assert _rel(got, wide.old) < 1e-2  # accepted at M = 31360
    assert 100 <= _over(got, wide.ref, wide.S, wide.n) <= 128
    bad = R.where_over(got, wide.ref, wide.S, wide.n)
    assert bad and all(c[0] == 9 and c[1] == 55 and c[2] >= 48 and 16 <= c[3] < 32 for c, *_ in bad)


def test_fault_tap_reads_wrapped_neighbour_instead_of_padding(wide):
    # pixel (n 3, y 20, x 0), tap (kh 1, kw 0): ix = -1 is padding; the flat
    # pixel index one lower is the last pixel of the row above
    got = wide.y.clone()
    extra = wide.xb[3, 19, 55].double() @ wide.wb[1, 0].double()
    got[3, 20, 0] = (wide.ref[3, 20, 0] + extra).to(F32)
    assert _rel(got, wide.old) < 1e-2  # accepted at M = 31360
    assert 56 <= _over(got, wide.ref, wide.S, wide.n) <= 64


def test_fault_dropped_k_step_in_one_tile(wide, small):
    """One 16-channel K-step of one tap dropped in one 128-row tile.  At M =
    31360 the old criterion measures 1.1e-2: over its bound by a tenth (a
    fault of 128 x 64 elements, each short of 16 of its 576 products, in a
    tensor of 2 M elements); from M = 40768 on (13 images) the same fault is
    accepted outright, which the arithmetic below records without another
    convolution."""
    def drop(b, row0):
        got = b.ref.clone().reshape(-1, 64)
        rows = slice(row0, row0 + 128)
        got[rows] -= b.tap_rows(1, 1)[rows, 16:32] @ b.wb[1, 1, 16:32].double()
        return got.reshape(b.ref.shape).to(F32)

    got = drop(wide, 128 * 100)
    old = _rel(got, wide.old)
    assert 1.0e-2 <= old < 1.2e-2
    fault = ((got - wide.y).norm() / wide.old.norm()).item()
    clean = _rel(wide.y, wide.old)
    assert (fault ** 2 * 31360 / 40768 + clean ** 2) ** 0.5 < 1e-2  # accepted at 13 images
    assert _over(got, wide.ref, wide.S, wide.n) > 8000
    assert _rel(drop(small, 256), small.old) > 1e-2  # a small tensor shows it: 7e-2
    assert _over(drop(small, 256), small.ref, small.S, small.n) > 8000


def test_fault_pixel_group_dropped_from_a_filter_gradient_slab():
    """n = 25088 pixels: eight pixels less in one tap's 64 x 64 block is inside
    the rounding bound (and any norm criterion); exact mode sees it."""
    N, H = 8, 56
    o = R.gen_rounded(9, N, H, H, 64, 64, 3, 1, 1)
    ref, S, n = R.conv_wgrad(o["x"], o["dy"], 1, 1, 3)
    assert n == 25088
    px = slice(1000, 1008)
    delta = o["x"].double().reshape(-1, 64)[px].t() @ o["dy"].double().reshape(-1, 64)[px]  # centre tap
    got = ref.clone()
    got[1, 1] -= delta
    assert _over(got.to(F32), ref, S, n) == 0  # invisible to the bound
    e = R.gen_exact(9, N, H, H, 64, 64, 3, 1, 1)
    assert e["density"] == 1.0
    ref = e["refs"]["wgrad"][0]
    assert R.exact_diff(ref.clone(), ref)[0] == 0
    got = ref.clone()
    got[1, 1] -= e["x"].reshape(-1, 64)[px].t() @ e["dy"].reshape(-1, 64)[px]
    assert R.exact_diff(got, ref)[0] > 1000


# ------------------------------------------------------------ store paths ----
def test_exact_mode_sees_roundings_and_single_products():
    e = R.gen_exact(11, 2, 14, 14, 64, 128, 3, 2, 1)
    ref = e["refs"]["fwd"][0]
    assert float(ref.abs().max()) > 256  # real ties: odd integers above 256
    ties = int(((ref.abs() > 256) & (ref.abs() < 512) & (ref % 2 != 0)).sum())
    assert ties > 0
    yb = R.bf16_rne(ref)
    assert R.exact_diff(yb, ref, bf16_out=True)[0] == 0
    assert R.exact_diff(R.bf16_trunc(ref), ref, bf16_out=True)[0] > 0
    assert R.exact_diff(bf16_half_away(ref), ref, bf16_out=True)[0] > 0
    one = ref.clone()
    one[1, 3, 4, 77] += 4.0  # one product (2 x 2) added twice
    assert R.exact_diff(one, ref)[0] == 1


def test_fault_truncating_store_small_bf16_output():
    o = R.gen_rounded(13, 2, 14, 14, 64, 128, 3, 2, 1)
    ref, S, n = R.conv_fwd(o["x"], o["w"], 2, 1)
    y = ref.to(F32)
    assert _over(R.bf16_rne(y), ref, S, n, bf16_out=True) == 0
    assert _over(R.bf16_trunc(y), ref, S, n, bf16_out=True) > 0
    assert _over(bf16_half_away(y), ref, S, n, bf16_out=True) == 0  # only exact mode's ties see this one


# ---------------------------------------------------------- split-K slabs ----
def test_fault_split_k_slab_dropped_or_added_twice():
    """(2, 14, 14, 64 -> 128, 3x3 s2): the plan's two slabs of 5 + 4 K-steps."""
    for mode in ("rounded", "exact"):
        if mode == "rounded":
            o = R.gen_rounded(17, 2, 14, 14, 64, 128, 3, 2, 1)
            ref, S, n = R.conv_fwd(o["x"], o["w"], 2, 1)
        else:
            o = R.gen_exact(17, 2, 14, 14, 64, 128, 3, 2, 1)
            ref, S, n = o["refs"]["fwd"]
        wa, wb = o["w"].clone(), o["w"].clone()
        wa.reshape(9, 64, 128)[5:] = 0
        wb.reshape(9, 64, 128)[:5] = 0
        ya = R.conv_fwd(o["x"], wa, 2, 1)[0].to(F32)
        yb = R.conv_fwd(o["x"], wb, 2, 1)[0].to(F32)
        for got, wrong in ((ya + yb, False), (ya, True), (ya + yb + yb, True)):
            if mode == "rounded":
                assert (_over(got, ref, S, n) > 0) == wrong
            else:
                assert (R.exact_diff(got, ref)[0] > 0) == wrong


# -------------------------------------------------------- backward-data ----
def test_fault_unflipped_taps_in_stride1_dgrad():
    o = R.gen_rounded(19, 2, 9, 11, 64, 64, 3, 1, 1)
    ref, S, n = R.conv_dgrad(o["dy"], o["w"], 1, 1, 9, 11)
    assert _over(ref.to(F32), ref, S, n) == 0
    got = R.conv_dgrad(o["dy"], o["w"].flip(0, 1), 1, 1, 9, 11)[0].to(F32)
    assert _over(got, ref, S, n) > 0.9 * ref.numel()
    e = R.gen_exact(19, 2, 9, 11, 64, 64, 3, 1, 1)
    assert R.exact_diff(R.conv_dgrad(e["dy"], e["w"].flip(0, 1), 1, 1, 9, 11, dt=F32)[0],
                        e["refs"]["dgrad"][0])[0] > 0


def test_fault_wrong_parity_class_in_3x3_stride2_dgrad():
    o = R.gen_rounded(23, 2, 12, 12, 64, 64, 3, 2, 1)
    ref, S, n = R.conv_dgrad(o["dy"], o["w"], 2, 1, 12, 12)
    got = ref.to(F32)
    assert _over(got, ref, S, n) == 0
    a, b = got[:, 0::2, 1::2].clone(), got[:, 1::2, 0::2].clone()
    got[:, 0::2, 1::2], got[:, 1::2, 0::2] = b, a  # (even, odd) and (odd, even) classes exchanged
    assert _over(got, ref, S, n) > 0.4 * ref.numel()


def test_fault_zero_pixels_of_1x1_stride2_dgrad_unwritten():
    o = R.gen_rounded(29, 2, 8, 8, 128, 64, 1, 2, 0, addend=True)
    ref, S, n = R.conv_dgrad(o["dy"], o["w"], 2, 0, 8, 8)
    zero = torch.ones(ref.shape, dtype=torch.bool)
    zero[:, 0::2, 0::2] = False  # three of every 2 x 2 block receive no tap
    assert float(ref[zero].abs().max()) == 0 and float(S[zero].max()) == 0
    got = ref.to(F32)
    assert R.check(got, ref, S, n, zero=zero)[1:] == (0, 0)
    stale = got.clone()
    stale[zero] = 1e-30  # whatever the buffer held
    assert R.check(stale, ref, S, n, zero=zero)[2] == int(zero.sum())
    # with an addend the three pixels hold the addend exactly
    ref, S, n = R.conv_dgrad(o["dy"], o["w"], 2, 0, 8, 8, addend=o["addend"])
    assert torch.equal(ref[zero].to(F32), o["addend"][zero])
    got = ref.to(F32)
    got[zero] = 0.0
    assert _over(got, ref, S, n) > 0


# ---------------------------------------------------------- weight copies ----
def test_fault_stale_weight_copy():
    """The kernel reads the copy of the weights of the step before (an SGD
    step of lr 0.01 on a unit-scale gradient behind the master weights)."""
    g = torch.Generator().manual_seed(31)
    w_prev = torch.randn(3, 3, 64, 64, generator=g) * 0.05
    w_now = w_prev - 0.01 * torch.randn(3, 3, 64, 64, generator=g) * 0.05
    x = R.bf16_rne(torch.randn(2, 10, 10, 64, generator=g))
    ref, S, n = R.conv_fwd(x, R.bf16_rne(w_now), 1, 1)
    assert _over(ref.to(F32), ref, S, n) == 0
    got = R.conv_fwd(x, R.bf16_rne(w_prev), 1, 1)[0].to(F32)
    assert _over(got, ref, S, n) > 0.9 * ref.numel()


# -------------------------------------------------------------- statistics ----
def test_fault_statistics_partials_one_row_short():
    o = R.gen_rounded(37, 4, 14, 14, 64, 64, 3, 1, 1)
    ref, S, n = R.conv_fwd(o["x"], o["w"], 1, 1)
    yb = R.bf16_rne(ref.to(F32))
    shift = torch.randn(64, generator=torch.Generator().manual_seed(1)) * 0.3
    s1, S1, s2, S2, ns = R.stats_fwd(yb, shift)
    P = 26  # cdiv(784, 64) * 2 partial rows of 32 pixels (the last tile is ragged: row 25 is empty)
    keep = [p for p in range(P) if p != 7]
    d = (yb.reshape(-1, 64) - shift).to(F32)
    rows = [d[32 * p:32 * p + 32] for p in range(P)]
    assert sum(r.shape[0] for r in rows) == 784
    p1 = torch.stack([r.sum(0) for r in rows]).double()
    p2 = torch.stack([(r * r).sum(0) for r in rows]).double()
    assert _over(p1.sum(0), s1, S1, ns) == 0 and _over(p2.sum(0), s2, S2, ns) == 0
    assert _over(p1[keep].sum(0), s1, S1, ns) > 32 and _over(p2[keep].sum(0), s2, S2, ns) > 32
    # backward sums: the same, from the kernel's own dX
    dx = torch.randn(784, 64, generator=torch.Generator().manual_seed(2))
    mean, rstd = shift, torch.rand(64, generator=torch.Generator().manual_seed(3)) + 0.5
    t1, T1, t2, T2, n1, n2 = R.stats_bwd(dx, o["x"], yb, mean, rstd, True)
    dm = dx * (yb.reshape(-1, 64) > 0)
    e32 = dm * (o["x"].reshape(-1, 64) - mean) * rstd  # fp32, the epilogue's three roundings
    q1 = torch.stack([dm[32 * p:32 * p + 32].sum(0) for p in range(P)]).double()
    q2 = torch.stack([e32[32 * p:32 * p + 32].sum(0) for p in range(P)]).double()
    assert _over(q1.sum(0), t1, T1, n1) == 0 and _over(q2.sum(0), t2, T2, n2) == 0
    assert _over(q1[keep].sum(0), t1, T1, n1) > 32 and _over(q2[keep].sum(0), t2, T2, n2) > 32


# ------------------------------------------------- K % 128 == 64 (K = 192) ----
@pytest.mark.parametrize("order", ["stray_last", "owner_last", "mixed"])
def test_fault_128_column_tile_on_k192(order):
    """A 128-column tile at n0 = 128 of K = 192: its columns 192..255 read the
    clamped weight row 191 and store at y[m K + co], which is columns 0..63 of
    row m + 1 (racing the block that owns them) and, for the last row, 64
    floats past the tensor.  Whatever the store order, the value check or the
    guard band behind the tensor sees it."""
    N, H, C, K = 1, 12, 64, 192
    o = R.gen_rounded(41, N, H, H, C, K, 1, 1, 0)
    ref, S, n = R.conv_fwd(o["x"], o["w"], 1, 0)
    M, canary = N * H * H, -777.0
    y = ref.to(F32).reshape(M, K)
    buf = torch.full((M * K + 64,), canary)
    buf[:M * K] = y.reshape(-1)
    assert _over(buf[:M * K].reshape(ref.shape), ref, S, n) == 0 and R.guard_hits(buf, M * K, canary) == 0
    at = (torch.arange(M)[:, None] * K + torch.arange(192, 256)[None, :]).reshape(-1)  # flat targets
    stray = y[:, 191:192].expand(M, 64).reshape(-1)  # every clamped column computes column 191
    inside = at < M * K
    g = torch.Generator().manual_seed(0)
    wins = dict(stray_last=torch.ones(at.shape, dtype=torch.bool),
                owner_last=~inside,  # the owner overwrites what it owns; nothing owns the guard
                mixed=(torch.rand(at.shape, generator=g) < 0.5) | ~inside)[order]
    buf[at[wins]] = stray[wins]
    over = _over(buf[:M * K].reshape(ref.shape), ref, S, n)
    hits = R.guard_hits(buf, M * K, canary)
    assert hits == 64
    assert (over > 0) == (order != "owner_last")
    assert over + hits > 0
