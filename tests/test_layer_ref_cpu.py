"""tests/helpers/layer_ref.py on a CPU-only machine: (1) the float64 references
agree with torch's own BatchNorm (with autograd), pooling and mean; (2) the
input generators meet the conditions their modes rest on (exactness, the block
plans the GPU cases are named for, the 4x condition of rounded mode); (3) each
mutant of a reference output - what a subtly wrong kernel would write - fails
the same `check` / `same_bits` / `failures` that tests/test_layer_kernels_gpu.py
applies, in every mode it is claimed for, while the unmutated output passes."""

import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("layer_ref", os.path.join(_HERE, "helpers", "layer_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)
F32, F64 = torch.float32, torch.float64

POOL_SHAPES = [(2, 7, 5, 10, 3, 2, 1), (3, 12, 8, 6, 2, 2, 0), (2, 13, 9, 16, 3, 2, 1), (2, 7, 5, 8, 3, 1, 1),
               (2, 12, 8, 20, 2, 2, 0), (1, 1, 1, 4, 3, 2, 1), (2, 9, 6, 12, 5, 3, 2), (2, 14, 10, 64, 3, 2, 1),
               (2, 15, 9, 64, 3, 2, 1), (3, 2, 2, 64, 3, 2, 1), (2, 15, 10, 64, 3, 2, 1), (2, 14, 9, 64, 3, 2, 1)]


def fails(res):
    return bool(R.failures(res))


def close(a, b, rel=1e-11):
    return bool(((a - b).abs() <= rel * (1 + b.abs())).all())


# ------------------------------------------- 1. the references against torch ----
@pytest.mark.parametrize("relu,res", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("rows,C", [(37, 12), (210, 24)])
def test_batchnorm_reference_equals_torch(rows, C, relu, res):
    o = R.bn_fwd_operands(rows, C, seed=1)
    x = o["x"].to(F64).requires_grad_(True)
    g, b = o["g"].to(F64).requires_grad_(True), o["b"].to(F64).requires_grad_(True)
    rs = o["res"].to(F64).requires_grad_(True)
    rm, rv = o["rm0"].to(F64).clone(), o["rv0"].to(F64).clone()
    y = F.batch_norm(x, rm, rv, g, b, True, R.BN_MOM, R.BN_EPS)
    if res:
        y = y + rs
    if relu:
        y = y.relu()
    dy = torch.randn(rows, C, generator=torch.Generator().manual_seed(2), dtype=F64)
    y.backward(dy)
    xd, gd, bd = x.detach(), g.detach(), b.detach()
    st = R.bn_stats(xd, xd[0], o["rm0"].to(F64), o["rv0"].to(F64))
    assert close(st["mean"][0], xd.mean(0)) and close(st["var"][0], xd.var(0, unbiased=False), 1e-9)
    assert close(st["rmean"][0], rm) and close(st["rvar"][0], rv, 1e-9)
    yr, _ = R.bn_apply(xd, st["mean"][0], st["rstd"][0], gd, bd, rs.detach() if res else None, relu)
    assert close(yr, y.detach(), 1e-9)
    r = R.bn_bwd_ref(xd, dy, y.detach(), st["mean"][0], st["rstd"][0], relu)
    assert close(r["db"][0], b.grad, 1e-9) and close(r["dg"][0], g.grad, 1e-9)
    dx, _ = R.bn_bwd_apply(xd, r["dyp"], st["mean"][0], st["rstd"][0], gd, r["db"][0], r["dg"][0], rows)
    assert close(dx, x.grad, 1e-8)
    if res:
        assert torch.equal(r["dyp"], rs.grad)


def test_batchnorm_reference_single_row_keeps_biased_variance():
    x = torch.tensor([[1.0, -2.0, 3.0, 4.0]], dtype=F64)
    st = R.bn_stats(x, x[0], torch.ones(4, dtype=F64), torch.ones(4, dtype=F64))
    assert torch.equal(st["var"][0], torch.zeros(4, dtype=F64))
    assert close(st["rvar"][0], torch.full((4,), 1 - R.BN_MOM, dtype=F64))


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_reference_equals_torch(shape):
    N, H, W, C, k, s, p = shape
    x = R.pool_data(N, H, W, C, "distinct", seed=3)
    xr = x.to(F64).permute(0, 3, 1, 2).clone().requires_grad_(True)
    yt = F.max_pool2d(xr, k, s, p)
    y, t32, t8 = R.maxpool_ref(x, k, s, p)
    assert torch.equal(y, yt.detach().permute(0, 2, 3, 1))
    dy = R.pool_dy(N, y.shape[1], y.shape[2], C, seed=4)
    yt.backward(dy.to(F64).permute(0, 3, 1, 2))
    dx = R.maxpool_bwd_ref(dy, t32, N, H, W)
    assert torch.equal(dx, xr.grad.permute(0, 2, 3, 1))
    assert torch.equal(R.tap8_to_pixel(t8, N, H, W, k, s, p).to(torch.int32), t32)
    assert float(dx.sum()) == float(dy.to(F64).sum())
    # the bf16 kernels read the same numbers
    assert torch.equal(R.bf16_rne(x), x)


@pytest.mark.parametrize("HW", [1, 7, 8, 9, 16, 17, 24, 25, 49])
def test_avgpool_reference_equals_mean(HW):
    x, exact = R.avgpool_operands(3, HW, 33, seed=HW)
    y, t = R.avgpool_ref(x, exact)
    assert exact == (HW & (HW - 1) == 0)
    assert close(y, x.to(F64).mean(1), 1e-13)
    dy = torch.randn(3, 33)
    assert close(R.avgpool_bwd_ref(dy, HW).to(F64), (dy.to(F64) / HW).reshape(3, 1, 33).expand(3, HW, 33), 1e-6)


# ------------------------------------------ 2. the generators' own conditions ----
VEC = [(1, 4), (7, 4), (300, 12), (210, 24), (1000, 64), (129, 256), (8200, 516), (8200, 1024)]
SCALAR = [(100, 1), (50, 7), (500, 6), (500, 10), (300, 255), (16400, 255)]


@pytest.mark.parametrize("rows,C", VEC + SCALAR + [(1100, 70), (600, 258)])
def test_colsum_operands_are_exact(rows, C):
    a, b = R.colsum_operands(rows, C, seed=rows + C)
    for mode in (0, 1):
        R.colsum_ref(a, b, mode)  # asserts the sums of absolute values < 2^24 and the round trips
    assert float(a.abs().max()) <= 8 and float(b.abs().max()) <= 8


def test_reduction_plans_are_the_named_ones():
    assert R.reduce_plan(1, 4)["rp"] == 1024 and R.reduce_plan(7, 4)["rp"] > 7        # cq = 1, rows < RP
    assert R.reduce_plan(300, 12)["live"] == 768                                        # cq = 3
    assert R.reduce_plan(1000, 64)["nb"] == 2
    p = R.reduce_plan(129, 256)
    assert p["nb"] == 2 and p["short"] < p["rpb"]                                       # short second block
    for rows, C, cap in ((8200, 516, 256), (8200, 1024, 256), (16400, 255, 1024)):
        p = R.reduce_plan(rows, C)
        assert p["nb"] == cap and p["empty"] > 0, (rows, C, p)                          # cap, empty tail blocks
    p = R.reduce_plan(8200, 1024)
    assert (p["rpb"], p["last"], p["empty"]) == (33, 248, 7) and R.row_lanes(1024) == 4
    assert R.reduce_plan(8200, 516)["live"] == 516 and R.row_lanes(516) == 4            # cq = 129
    p = R.reduce_plan(16384, 1024)
    assert p["nb"] == 256 and p["empty"] == 0                                           # cap, no empty tail
    assert R.reduce_plan(300, 255)["rp"] == 1 and R.reduce_plan(100, 1)["rp"] == 256
    assert not R.chan_reduce_ok(258) and R.ws_floats(600, 258) == 0
    assert R.ws_floats(8200, 1024) == 256 * 2 * 1024


def test_fused_loop_tail_plans_are_partial():
    """An MI355X has 256 CUs: 2 blocks a CU cap the fused grid at 512."""
    for rows in (8200, 8192):
        p = R.fused_plan(rows, 516, 512)
        assert p["grid"] == 512 and p["trips"] == 3 and p["partial"] and p["ragged"], p
        base = 2 * R.FU * p["stride"]
        assert 0 < p["n4"] - base < p["stride"]  # the third trip: some threads enter, and break at u = 1


@pytest.mark.parametrize("rows,C", [(2048, 256), (16384, 1024), (4096, 516), (8200, 516)])
def test_bn_fwd_exact_operands_are_exact(rows, C):
    o = R.bn_fwd_exact_operands(rows, C, seed=rows + C)
    x = o["x"].to(F64)
    assert torch.equal(R.bf16_rne(o["x"]), o["x"])
    st = R.bn_stats(x, x[0], o["rm0"].to(F64), o["rv0"].to(F64), exact=True)  # asserts the round trips
    # the few-ulp bound of rstd does not grow with rows
    spread = float((st["q"] / (st["var"][0] + R.BN_EPS)).max())  # E[(x - K)^2] / var: a few units
    assert float((st["rstd"][1] / st["rstd"][0]).max()) < 16 * R.EPS * (1 + spread)


@pytest.mark.parametrize("rows,C", [(256, 4), (512, 12), (2048, 256), (4096, 1024), (8192, 516)])
def test_bn_bwd_exact_operands_are_exact(rows, C):
    o = {k: v.to(F64) for k, v in R.bn_bwd_operands(rows, C, seed=rows + C, exact=True).items()}
    assert bool((o["y"] == 0).any()) and bool((o["y"] > 0).any()) and bool((o["y"] < 0).any())
    assert o["mean"].unique().numel() > 1 and o["rstd"].unique().numel() > 1 and o["g"].unique().numel() > 1
    for relu in (False, True):
        r = R.bn_bwd_ref(o["x"], o["dy"], o["y"], o["mean"], o["rstd"], relu, exact=True)
        R.bn_bwd_apply(o["x"], r["dyp"], o["mean"], o["rstd"], o["g"], r["db"][0], r["dg"][0], rows, exact=True)


@pytest.mark.parametrize("x_bf16", [False, True])
@pytest.mark.parametrize("rows,C", [(210, 24), (37, 12), (2, 4), (392, 64)])
def test_rounded_fwd_cases_meet_the_4x_condition(rows, C, x_bf16):
    o = R.bn_fwd_operands(rows, C, seed=rows * 7 + C, x_bf16=x_bf16)
    x = o["x"].to(F64)
    assert R.drop_row_ratio(x, x[0]) >= 4.0


@pytest.mark.parametrize("rows,C", [(210, 24), (392, 64)])
def test_rounded_bwd_cases_meet_the_4x_condition(rows, C):
    for xb in (False, True):
        o = R.bn_bwd_operands(rows, C, seed=rows + C, exact=False, x_bf16=xb)
        for relu in (False, True):
            assert R.drop_row_ratio_bwd(o, relu) >= 4.0


def test_rounded_mode_would_not_hold_for_large_row_counts():
    """Why larger row counts use exact mode: at 16384 rows a dropped row moves
    the mean by less than the n-term bound."""
    o = R.bn_fwd_operands(16384, 4, seed=1)
    x = o["x"].to(F64)
    assert R.drop_row_ratio(x, x[0]) < 4.0


def test_table_operands_are_exact_and_grouped():
    for C, P in ((64, 1), (192, 129), (1024, 300)):
        t = R.table_operands(C, P, seed=C + P)
        assert t.shape == (2, C // 64, P, 64)
        s1, s2 = R.table_sums(t)
        assert s1.shape == (C,) and bool((s2 > 0).all())
        # channel c sits at [c // 64][p][c % 64]
        c = C - 3
        assert float(s1[c]) == float(t[0, c // 64, :, c % 64].to(F64).sum())


# ------------------------------------------------------------- 3. mutants ----
def _fwd_setup(mode):
    """A perfect kernel's outputs (the reference rounded once) for a forward
    case with residual and ReLU, and the operands."""
    if mode == "exact":
        rows, C = 2048, 256
        o = R.bn_fwd_exact_operands(rows, C, seed=9)
    else:
        rows, C = 210, 24
        o = R.bn_fwd_operands(rows, C, seed=9)
    x = o["x"].to(F64)
    st = R.bn_stats(x, x[0], o["rm0"].to(F64), o["rv0"].to(F64), exact=mode == "exact")
    got = {k: st[k][0].to(F32) for k in ("mean", "rstd", "rmean", "rvar")}
    return o, x, st, got


def _fwd_check(o, x, st, got, mode, relu=True, res=True, y=None, yb=None):
    """The GPU file's check of a forward call (R.check_bn_fwd) on a simulated
    output; y defaults to a perfect apply of the statistics in `got`."""
    if y is None:
        y = R.bn_apply(x, got["mean"].to(F64), got["rstd"].to(F64), o["g"].to(F64), o["b"].to(F64),
                       o["res"].to(F64) if res else None, relu)[0].to(F32)
    return R.check_bn_fwd(o, relu, res, dict(got, y=y, yb=yb), mode == "exact", st=st)


def _stats_from(x, K, o, keep=None, swap=False, chan_zero=None):
    """fin_channel on sums a wrong pass 1 would deliver, divided by the true rows."""
    rows = x.shape[0]
    d = x - K
    if keep is not None:
        d = d[keep]
    s1, s2 = d.sum(0), (d * d).sum(0)
    if swap:
        s1, s2 = s2, s1
    if chan_zero is not None:
        s1, s2 = s1.clone(), s2.clone()
        s1[chan_zero] = 0
        s2[chan_zero] = 0
    st = R.bn_stats(None, K, o["rm0"].to(F64), o["rv0"].to(F64), sums=(s1, s2), rows=rows)
    return {k: st[k][0].to(F32) for k in ("mean", "rstd", "rmean", "rvar")}


@pytest.mark.parametrize("mode", ["rounded", "exact"])
def test_forward_statistics_mutants_fail(mode):
    o, x, st, got = _fwd_setup(mode)
    rows, C = x.shape
    assert not fails(_fwd_check(o, x, st, got, mode))
    every = torch.ones(rows, dtype=torch.bool)
    # a dropped row (row 0 is the shift: its term is exactly 0)
    for r in (1, rows // 2, rows - 1):
        keep = every.clone()
        keep[r] = False
        assert fails(_fwd_check(o, x, st, _stats_from(x, x[0], o, keep=keep), mode)), f"row {r}"
    # the rows of the last block dropped
    p = R.reduce_plan(rows, C)
    keep = every.clone()
    keep[p["last"] * p["rpb"]:] = False
    assert fails(_fwd_check(o, x, st, _stats_from(x, x[0], o, keep=keep), mode))
    # the last channel quad dropped
    assert fails(_fwd_check(o, x, st, _stats_from(x, x[0], o, chan_zero=slice(C - 4, C)), mode))
    # s1 and s2 exchanged
    assert fails(_fwd_check(o, x, st, _stats_from(x, x[0], o, swap=True), mode))
    # biased running variance
    m = dict(got)
    m["rvar"] = ((1 - R.BN_MOM) * o["rv0"].to(F64) + R.BN_MOM * st["var"][0]).to(F32)
    assert fails(_fwd_check(o, x, st, m, mode))
    # momentum and its complement exchanged
    m = dict(got)
    m["rmean"] = (R.BN_MOM * o["rm0"].to(F64) + (1 - R.BN_MOM) * st["mean"][0]).to(F32)
    assert fails(_fwd_check(o, x, st, m, mode))
    # the shift not added back
    m = dict(got)
    m["mean"] = st["ms"].to(F32)
    assert fails(_fwd_check(o, x, st, m, mode))


@pytest.mark.parametrize("mode", ["rounded", "exact"])
def test_forward_apply_mutants_fail(mode):
    o, x, st, got = _fwd_setup(mode)
    g, b, rs = o["g"].to(F64), o["b"].to(F64), o["res"].to(F64)
    m64, r64 = got["mean"].to(F64), got["rstd"].to(F64)
    good, _ = R.bn_apply(x, m64, r64, g, b, rs, True)
    assert not fails(_fwd_check(o, x, st, got, mode, y=good.to(F32), yb=R.bf16_bits(good.to(F32)).reshape(good.shape)))
    # mean / rstd taken from the neighbouring quad
    y, _ = R.bn_apply(x, m64.roll(4), r64.roll(4), g, b, rs, True)
    assert fails(_fwd_check(o, x, st, got, mode, y=y.to(F32)))
    # residual added after the ReLU
    y = ((x - m64) * r64 * g + b).clamp_min(0) + rs
    assert fails(_fwd_check(o, x, st, got, mode, y=y.to(F32)))
    # bf16 truncation for RNE: the twin, and a lone bf16 output against its bound
    tr = R.bf16_trunc(good.to(F32))
    assert fails(_fwd_check(o, x, st, got, mode, y=good.to(F32), yb=R.bf16_bits(tr).reshape(good.shape)))
    if mode == "rounded":
        yr, t = R.bn_apply(x, m64, r64, g, b, rs, True)
        assert not fails({"yb": R.check_abs(R.bf16_rne(good.to(F32)), yr, t, bf16_out=True)})
        assert fails({"yb": R.check_abs(tr, yr, t, bf16_out=True)})


def _bwd_check(o, relu, got, exact):
    """The GPU file's check of a backward call on a simulated output."""
    return R.check_bn_bwd(o, relu, got, exact)


def _bwd_kernel(o, relu, ge=False, keep=None, neighbour=False, trunc=False):
    """A simulated backward; the keyword arguments are the mutations."""
    x, dy, y, mean, rstd, g = (o[k].to(F64) for k in ("x", "dy", "y", "mean", "rstd", "g"))
    rows = x.shape[0]
    mask = (y >= 0) if ge else (y > 0)
    dyp = torch.where(mask, dy, torch.zeros_like(dy)) if relu else dy
    xh = (x - mean) * rstd
    sel = slice(None) if keep is None else keep
    db, dg = dyp[sel].sum(0).to(F32), (dyp * xh)[sel].sum(0).to(F32)
    m2, r2 = (mean.roll(4), rstd.roll(4)) if neighbour else (mean, rstd)
    dx, _ = R.bn_bwd_apply(x, dyp, m2, r2, g, db.to(F64), dg.to(F64), rows)
    dx = dx.to(F32)
    dxb = R.bf16_bits(R.bf16_trunc(dx) if trunc else dx).reshape(dx.shape)
    return dict(db=db, dg=dg, dres=dyp.to(F32), dx=dx, dxb=dxb)


@pytest.mark.parametrize("mode", ["rounded", "exact"])
def test_backward_mutants_fail(mode):
    exact = mode == "exact"
    rows, C = (512, 12) if exact else (210, 24)
    o = R.bn_bwd_operands(rows, C, seed=rows + C, exact=exact)
    assert not fails(_bwd_check(o, True, _bwd_kernel(o, True), exact))
    assert not fails(_bwd_check(o, False, _bwd_kernel(o, False), exact))
    # ReLU mask >= for >
    assert fails(_bwd_check(o, True, _bwd_kernel(o, True, ge=True), exact))
    # a dropped row; the rows of the last block dropped
    keep = torch.ones(rows, dtype=torch.bool)
    keep[rows // 3] = False
    assert fails(_bwd_check(o, True, _bwd_kernel(o, True, keep=keep), exact))
    p = R.reduce_plan(rows, C)
    keep = torch.ones(rows, dtype=torch.bool)
    keep[p["last"] * p["rpb"]:] = False
    assert fails(_bwd_check(o, True, _bwd_kernel(o, True, keep=keep), exact))
    # mean / rstd taken from the neighbouring quad; bf16 truncation for RNE
    assert fails(_bwd_check(o, True, _bwd_kernel(o, True, neighbour=True), exact))
    assert fails(_bwd_check(o, True, _bwd_kernel(o, True, trunc=True), exact))


@pytest.mark.parametrize("rows,C", [(1000, 64), (8200, 1024), (16400, 255)])
def test_colsum_mutants_fail(rows, C):
    a, b = R.colsum_operands(rows, C, seed=rows + C)
    p = R.reduce_plan(rows, C)
    for mode in (0, 1):
        s1, s2 = R.colsum_ref(a, b, mode)
        prod = a * a if mode == 0 else a * b

        def res(keep=slice(None), swap=False, quad=False):
            g1, g2 = a[keep].sum(0).to(F32), prod[keep].sum(0).to(F32)
            if swap:
                g1, g2 = g2, g1
            if quad:
                g1[C - (4 if C % 4 == 0 else 1):] = 0
            return {"s1": R.same_bits(g1, s1.to(F32)), "s2": R.same_bits(g2, s2.to(F32))}
        assert not fails(res())
        keep = torch.ones(rows, dtype=torch.bool)
        nz = int((a[:, 0] != 0).nonzero()[0])
        keep[nz] = False
        assert fails(res(keep=keep))                                         # a dropped row
        keep = torch.ones(rows, dtype=torch.bool)
        keep[p["last"] * p["rpb"]:] = False
        assert fails(res(keep=keep))                                         # the last block's rows
        assert fails(res(quad=True)) and fails(res(swap=True))               # last quad; s1 <-> s2


@pytest.mark.parametrize("C,P", [(192, 3), (192, 129), (1024, 300)])
def test_table_mutants_fail(C, P):
    t = R.table_operands(C, P, seed=C + P)
    s1, s2 = R.table_sums(t)
    rm0 = torch.full((C,), 9.0, dtype=F64)
    rv0 = torch.ones(C, dtype=F64)

    def res(a, b):
        st = R.bn_stats(None, rm0, rm0, rv0, exact=True, sums=(s1, s2), rows=256)
        got = R.bn_stats(None, rm0, rm0, rv0, sums=(a, b), rows=256)
        return {"mean": R.same_bits(got["mean"][0].to(F32), st["mean"][0].to(F32)),
                "rstd": R.check_abs(got["rstd"][0].to(F32), *st["rstd"]),
                "db": R.same_bits(a.to(F32), s1.to(F32)), "dg": R.same_bits(b.to(F32), s2.to(F32))}
    assert not fails(res(s1, s2))
    short = t[:, :, :-1] if P > 1 else t * 0
    a, b = short.to(F64).sum(2).reshape(2, -1)
    assert fails(res(a, b))                                                  # one table row dropped
    a, b = R.table_as_channel_major(t)
    assert fails(res(a, b))                                                  # grp64 read as channel-major


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_mutants_fail(shape):
    N, H, W, C, k, s, p = shape
    one = H * W == 1
    for data in ("distinct", "ties"):
        x = R.pool_data(N, H, W, C, data, seed=H * W + C)
        y, t32, t8 = R.maxpool_ref(x, k, s, p)
        dy = R.pool_dy(N, y.shape[1], y.shape[2], C, seed=C)
        dx = R.maxpool_bwd_ref(dy, t32, N, H, W)

        def res(y2, a32, a8, dx2):
            return {"y": R.same_bits(y2.to(F32).reshape(-1), y.to(F32).reshape(-1)),
                    "tap32": R.same_bits(a32.reshape(-1), t32.reshape(-1)),
                    "tap8": R.same_bits(a8.reshape(-1), t8.reshape(-1)),
                    "dx": R.same_bits(dx2.to(F32), dx.to(F32))}
        assert not fails(res(y, t32, t8, dx))
        if one:
            continue  # a 1 x 1 map has one tap: nothing to confuse (the case is there for its empty taps)
        if data == "ties":
            y2, a32, a8 = R.maxpool_ref(x, k, s, p, last_wins=True)          # last maximum wins
            assert torch.equal(y2, y) and fails(res(y2, a32, a8, R.maxpool_bwd_ref(dy, a32, N, H, W)))
            dx2 = R.maxpool_bwd_ref(dy, t32, N, H, W, all_ties=(x, k, s, p))  # gradient to every tied tap
            assert fails(res(y, t32, t8, dx2))
        if H != W:                                                           # H and W exchanged
            y2, a32, a8 = R.maxpool_ref(x.reshape(N, W, H, C), k, s, p)
            if y2.numel() == y.numel():
                assert fails(res(y2, a32, a8, dx))
        if p > 0 and data == "distinct":                                     # a pad tap wrapped into the next row
            y2, a32, a8 = R.maxpool_ref(x, k, s, p, wrap_pad=True)
            assert fails(res(y2, a32, a8, dx))
        y2, a32, a8 = R.maxpool_ref(x, k, s, p, tap_shift=1)                 # window tap off by one
        assert fails(res(y2, a32, a8, R.maxpool_bwd_ref(dy, a32.clamp_min(0), N, H, W)))


@pytest.mark.parametrize("HW", [1, 7, 8, 9, 16, 17, 24, 25, 49])
def test_avgpool_mutants_fail(HW):
    x, exact = R.avgpool_operands(3, HW, 32, seed=HW * 100 + 32)
    y, t = R.avgpool_ref(x, exact)

    def res(got):
        return {"y": R.same_bits(got.to(F32), y.to(F32)) if exact else R.check_abs(got.to(F32), y, t)}
    assert not fails(res(y))
    for pix in range(max(0, HW - 8), HW):                                    # a pixel with p >= HW - 8 dropped
        assert fails(res(R.avgpool_ref(x, exact, drop_pixel=pix)[0])), pix
    for count in (HW + 1, 8 * ((HW + 7) // 8) + (8 if HW % 8 == 0 else 0)):  # division by the wrong count
        assert fails(res(R.avgpool_ref(x, exact, count=count)[0]))
    dy = torch.randn(3, 32, generator=torch.Generator().manual_seed(HW))
    good = R.avgpool_bwd_ref(dy, HW)
    assert not fails({"dx": R.same_bits(good, good.clone())})
    assert fails({"dx": R.same_bits(R.avgpool_bwd_ref(dy, HW + 1)[:, :HW], good)})
