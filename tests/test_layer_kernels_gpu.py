"""The layers between the convs, kernel by kernel: the channel reductions and
BatchNorm of csrc/kernels/bn.hip and the pooling of csrc/kernels/ops_generic.hip
against the float64 references of tests/helpers/layer_ref.py, through the raw
bindings on stream_handle() with no engine in between.

Every output and workspace buffer carries 64 sentinel elements behind it that
must survive the call, outputs start as NaN (an unwritten element fails), and
the workspace has exactly chan_reduce_ws_floats elements.  Comparisons are per
element and per output, in the two modes of layer_ref.py (exact: bit for bit;
rounded: derived bound); applies are operand-matched.  Where a call writes an
fp32 output and its bf16 twin, the twin's bits are bf16_bits of the fp32 one.
tests/test_layer_ref_cpu.py shows on the CPU that the listed mutants fail the
same checks.

case -> kernel
  test_colsum2[vec]       partial_kernel<SUM_SQ | SUM_PROD, false, false> + finalize_kernel
                          (cq = 1, 3, 129, 256; rows < RP; the 256-block cap with empty tail blocks)
  test_colsum2[scalar]    partial1_kernel + finalize_kernel (RP = 256 ... 1; the 1024-block cap)
  test_colsum2[fallback]  colsum2_kernel (atomics), without a workspace and with C = 258
  test_bn_fwd_*           partial_kernel<SUM_SQ, XB, false> + finalize_kernel + apply_kernel<XB>;
                          fused: finalize_apply_kernel<XB>, channel-major table, shift = row 0
                          of x (fp32 or bf16); test_bn_fwd_fused_loop_tail: its FU loop tail
  test_bn_fwd_eval        apply_kernel<XB>, eval
  test_bn_bwd_*           partial_kernel<BN_BWD, XB, YB> + finalize_kernel + bwd_apply_kernel<XB, YB>;
                          fused: finalize_bwd_apply_kernel<XB, YB>, channel-major table
  test_bn_fwd_partials    finalize64_kernel (P <= 128) | finalize_kernel grp64 (P > 128) +
                          apply_kernel<XB>; fused: finalize_apply_kernel<XB>, grp64 table
  test_bn_bwd_partials    the same finalizes + bwd_apply_kernel<true, true>; fused:
                          finalize_bwd_apply_kernel<true, true>, grp64 table
  test_maxpool_int32      maxpool_fwd_kernel / maxpool_bwd_kernel (C % 4 != 0),
                          maxpool_fwd4_kernel / maxpool_bwd4_kernel (C % 4 == 0)
  test_maxpool_uint8      maxpool_fwd4b_kernel<0,0,0,0 | 3,2,1,16, float4 | uint2>,
                          maxpool_bwd4b_kernel<0,0,0,0>, maxpool_bwd_k3s2_quad_kernel<16>,
                          maxpool_bwd_k3s2_kernel<16> (the `bwd` column of POOL_U8)
  test_avgpool            avgpool_fwd_kernel (C % 32 == 0), avgpool_fwd1_kernel, avgpool_bwd_kernel

MTA_STAGE_REPORT=<path>: the worst err / tol per (kernel variant, output) is
also written there as JSON (docs/ACCURACY.md holds a run's)."""

import importlib.util
import itertools
import json
import os

import pytest
import torch

from mpi_tensorflow_amd.ops import ptr, stream_handle

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("layer_ref", os.path.join(_HERE, "helpers", "layer_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16

REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    rows = {f"{variant} | {out}": v for (variant, out), v in sorted(REPORT.items())}
    for k, v in rows.items():
        print(f"[layer kernels] {k}: {v:.3g}")
    path = os.environ.get("MTA_STAGE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(rows, f, indent=1, sort_keys=True)


def _ops():
    from mpi_tensorflow_amd.ops import native

    return native().ops


def _settle(variant, res, where):
    """Record the worst err / tol of every bounded output, print each figure,
    then fail on anything over its bound or differing bit for bit."""
    for k, e in res.items():
        if e[0] == "tol":
            REPORT[(variant, k)] = max(REPORT.get((variant, k), 0.0), e[1])
    print(f"[{variant}] {where}: " + ", ".join(
        f"{k} {e[1]:.3g}" if e[0] == "tol" else f"{k} {e[1]} bits" for k, e in res.items()))
    bad = R.failures(res)
    assert not bad, f"{variant} {where}: " + "; ".join(bad)


# ------------------------------------------------------------- buffers ----
_PAT = {F32: (torch.int32, 0x5A5A5A5A), BF: (torch.int16, 0x5A5A), torch.int32: (torch.int32, 0x5A5A5A5A),
        torch.uint8: (torch.uint8, 0x5A)}
_UNWRITTEN = {torch.int32: -7, torch.uint8: 0x7B}  # no pixel index, no window tap


class Arena:
    """Output / workspace buffers of one call: n elements pre-filled with NaN
    (an impossible value for the integer taps) and 64 sentinel elements."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def out(self, n, dtype=F32):
        t = torch.empty(n + 64, dtype=dtype, device=self.dev)
        t[:n] = float("nan") if dtype.is_floating_point else _UNWRITTEN[dtype]
        it, pat = _PAT[dtype]
        t[n:].view(it).fill_(pat)
        self.bufs.append((t, n))
        return t

    def body(self, t):
        n = next(n for b, n in self.bufs if b is t)
        return t[:n].cpu()

    def intact(self):
        torch.cuda.synchronize()
        for t, n in self.bufs:
            it, pat = _PAT[t.dtype]
            assert bool((t[n:].view(it) == pat).all()), f"sentinel behind a {t.dtype} buffer of {n} overwritten"


def _bits(t):
    """bf16 buffer -> int16 bit patterns."""
    return t.contiguous().view(torch.int16)


def _dev_x(x, bf16, dev):
    """The device operand: fp32, or the bf16 buffer of an already rounded x."""
    return x.to(BF).to(dev) if bf16 else x.to(dev)


class _Fused:
    """bn_set_fused(on) for a block; always back to off / 2 blocks a CU."""

    def __init__(self, ops, on):
        self.ops, self.on = ops, on

    def __enter__(self):
        self.ops.bn_set_fused(self.on)
        self.ops.bn_set_fused_blocks_per_cu(2)

    def __exit__(self, *a):
        self.ops.bn_set_fused(False)
        self.ops.bn_set_fused_blocks_per_cu(2)
        return False


def _fused_equal(runs):
    """Every output of the fused run against the unfused one, bit for bit."""
    res = {}
    for k, a in runs[True].items():
        if a is not None:
            b = runs[False][k]
            res[f"{k} fused == unfused"] = R.same_bits(_bits(a), _bits(b)) if a.dtype == BF else R.same_bits(a, b)
    return res


# ------------------------------------------------- A. channel reductions ----
VEC = [(1, 4), (7, 4), (300, 12), (210, 24), (1000, 64), (129, 256), (8200, 516), (8200, 1024)]
SCALAR = [(100, 1), (50, 7), (500, 6), (500, 10), (300, 255), (16400, 255)]
FALLBACK = [(1100, 70, False), (600, 258, True)]
COLSUM = ([("vec", r, c, True) for r, c in VEC] + [("scalar", r, c, True) for r, c in SCALAR]
          + [("fallback", r, c, w) for r, c, w in FALLBACK])


@pytest.mark.parametrize("path,rows,C,with_ws", COLSUM, ids=[f"{p}-{r}x{c}" for p, r, c, _ in COLSUM])
def test_colsum2(cuda_dev, path, rows, C, with_ws):
    ops = _ops()
    assert ops.chan_reduce_ok(C) == R.chan_reduce_ok(C) == (path != "fallback" or not with_ws)
    assert ops.chan_reduce_ws_floats(rows, C) == R.ws_floats(rows, C)
    if (rows, C) in ((8200, 516), (8200, 1024), (16400, 255)):
        assert R.reduce_plan(rows, C)["empty"] > 0
    a, b = R.colsum_operands(rows, C, seed=rows + C)
    ad, bd = a.to(F32).to(cuda_dev), b.to(F32).to(cuda_dev)
    for mode in (0, 1):
        s1r, s2r = R.colsum_ref(a, b, mode)
        ar = Arena(cuda_dev)
        ws = ar.out(ops.chan_reduce_ws_floats(rows, C) if with_ws else 0)
        s1, s2 = ar.out(C), ar.out(C)
        ops.colsum2(ptr(ad), ptr(bd), rows, C, ptr(s1), ptr(s2), mode, ptr(ws) if with_ws else 0,
                    stream_handle())
        ar.intact()
        _settle(f"colsum2 {path}", {"s1": R.same_bits(ar.body(s1), s1r.to(F32)),
                                     "s2": R.same_bits(ar.body(s2), s2r.to(F32))}, f"{rows}x{C} mode {mode}")


# ------------------------------------------------------ B. bn_fwd, training ----
# (name, x bf16, y, yb, relu, res): a covering set
FWD_VARIANTS = [
    ("f32_y", False, True, False, False, False),
    ("f32_y_yb_relu_res", False, True, True, True, True),
    ("f32_yb_relu", False, False, True, True, False),
    ("bf16_y_res", True, True, False, False, True),
    ("bf16_yb_relu_res", True, False, True, True, True),
    ("bf16_y_yb_relu", True, True, True, True, False),
]
FV = {v[0]: v for v in FWD_VARIANTS}


def _run_bn_fwd(ops, dev, o, v, fused, training=True):
    _, xb, wy, wyb, relu, res = v
    rows, C = o["x"].shape
    ar = Arena(dev)
    x = _dev_x(o["x"], xb, dev)
    g, b = o["g"].to(dev), o["b"].to(dev)
    rs = o["res"].to(dev) if res else None
    y = ar.out(rows * C) if wy else None
    yb = ar.out(rows * C, BF) if wyb else None
    mean, rstd = ar.out(C), ar.out(C)
    ws = ar.out(ops.chan_reduce_ws_floats(rows, C))
    rm, rv = ar.out(C), ar.out(C)
    rm[:C], rv[:C] = o["rm0"].to(dev), o["rv0"].to(dev)
    with _Fused(ops, fused):
        ops.bn_fwd(ptr(x), rows, C, ptr(g), ptr(b), ptr(rs), ptr(y), ptr(mean), ptr(rstd), ptr(ws),
                   R.BN_EPS, R.BN_MOM, relu, training, ptr(rm), ptr(rv), stream_handle(), ptr(yb), xb)
        ar.intact()
    assert ops.bn_fused_error() == 0
    got = dict(mean=ar.body(mean), rstd=ar.body(rstd), rmean=ar.body(rm), rvar=ar.body(rv),
               y=ar.body(y).reshape(rows, C) if wy else None,
               yb=ar.body(yb).reshape(rows, C) if wyb else None)
    return got




def _bn_fwd_case(dev, o, v, exact, tag, label="bn_fwd", fused_only=False):
    ops = _ops()
    name = f"{label} {v[0]} {'exact' if exact else 'rounded'}"
    runs = {}
    for fused in ((True,) if fused_only else (False, True)):
        runs[fused] = _run_bn_fwd(ops, dev, o, v, fused)
        _settle(name + (" fused" if fused else ""), R.check_bn_fwd(o, v[4], v[5], runs[fused], exact), tag)
    if not fused_only:
        # the fused channel-major finalize documents finalize_kernel's order
        _settle(name, _fused_equal(runs), tag)
    return runs


FWD_ROUNDED = [(210, 24), (37, 12), (2, 4), (392, 64)]
FWD_EXACT = [((2048, 256), [v[0] for v in FWD_VARIANTS]),
             ((16384, 1024), ["f32_y_yb_relu_res", "bf16_yb_relu_res"]),
             ((4096, 516), ["f32_yb_relu", "bf16_y_res"])]


@pytest.mark.parametrize("rows,C", FWD_ROUNDED)
@pytest.mark.parametrize("vname", [v[0] for v in FWD_VARIANTS])
def test_bn_fwd_rounded(cuda_dev, vname, rows, C):
    v = FV[vname]
    o = R.bn_fwd_operands(rows, C, seed=rows * 7 + C, x_bf16=v[1])
    x = o["x"].to(F64)
    assert R.drop_row_ratio(x, x[0]) >= 4.0
    _bn_fwd_case(cuda_dev, o, v, False, f"{rows}x{C}")


@pytest.mark.parametrize("rows,C,vname", [(s[0], s[1], n) for s, names in FWD_EXACT for n in names])
def test_bn_fwd_exact(cuda_dev, rows, C, vname):
    v = FV[vname]
    o = R.bn_fwd_exact_operands(rows, C, seed=rows + C, x_bf16=v[1])
    if (rows, C) == (16384, 1024):
        p = R.reduce_plan(rows, C)
        assert p["nb"] == 256 and p["empty"] == 0
    _bn_fwd_case(cuda_dev, o, v, True, f"{rows}x{C}")


@pytest.mark.parametrize("vname", ["f32_y", "f32_y_yb_relu_res"])
def test_bn_fwd_large_channel_mean(cuda_dev, vname):
    """Mean 1e3 (1 + u), std 1: the shifted sums keep the variance's digits."""
    o = R.bn_fwd_operands(392, 64, seed=11, kind="large_mean")
    _bn_fwd_case(cuda_dev, o, FV[vname], False, "392x64", label="bn_fwd large_mean")


def test_bn_fwd_outlier_first_row(cuda_dev):
    """Row 0 sits 50 sigma off the channel mean: the shift is a poor sample,
    and the derived variance bound contains (mean - K)^2.  The err / tol of
    this case is in the report; above 1 is a finding."""
    o = R.bn_fwd_operands(392, 64, seed=12, kind="outlier")
    x = o["x"].to(F64)
    assert float(((x[0] - x[1:].mean(0)).abs() / x[1:].std(0)).min()) > 40
    _bn_fwd_case(cuda_dev, o, FV["f32_y"], False, "392x64", label="bn_fwd outlier_first_row")


@pytest.mark.parametrize("vname", ["f32_y_yb_relu_res", "bf16_y_res"])
def test_bn_fwd_constant_channel(cuda_dev, vname):
    """var is exactly 0, rstd = rsqrt(eps) within 2 ulp, y = beta (+ res) exactly."""
    ops = _ops()
    v = FV[vname]
    _, xb, wy, wyb, relu, res = v
    o = R.bn_fwd_operands(210, 24, seed=13, x_bf16=xb, kind="constant")
    x = o["x"].to(F64)
    runs = {f: _run_bn_fwd(ops, cuda_dev, o, v, f) for f in (False, True)}
    for fused, got in runs.items():
        want = o["b"].to(F64) + (o["res"].to(F64) if res else 0.0)
        want = R.f32r(want.clamp_min(0.0) if relu else want).expand(210, 24)
        r0 = 1.0 / torch.sqrt(torch.tensor(R.BN_EPS, dtype=F64))
        rv = (1 - R.BN_MOM) * o["rv0"].to(F64)
        rm = (1 - R.BN_MOM) * o["rm0"].to(F64) + R.BN_MOM * x[0]
        out = {"mean": R.same_bits(got["mean"], x[0].to(F32)),
               "rmean": R.check_abs(got["rmean"], rm, 2 * R.EPS * rm.abs()),
               "rstd": R.check_abs(got["rstd"], r0.expand(24), 2 * R.EPS * r0),
               "rvar": R.check_abs(got["rvar"], rv, 2 * R.EPS * rv),
               "y": R.same_bits(got["y"], want)}
        if wyb:
            out["yb twin"] = R.same_bits(_bits(got["yb"]), R.bf16_bits(got["y"]).reshape(210, 24))
        _settle(f"bn_fwd constant {vname}" + (" fused" if fused else ""), out, "210x24")


@pytest.mark.parametrize("vname", ["f32_y_yb_relu_res", "bf16_yb_relu_res"])
def test_bn_fwd_fused_loop_tail(cuda_dev, vname):
    """(8200, 516), fusing on: n4 is no multiple of the grid stride and the
    third trip of the FU loop is partial; the reduction has empty tail blocks."""
    ops = _ops()
    rows, C = 8200, 516
    with _Fused(ops, True):
        cap = ops.bn_fused_grid_cap()
    plan = R.fused_plan(rows, C, cap)
    assert cap > 0 and plan["partial"] and plan["ragged"] and plan["trips"] >= 2, plan
    assert R.reduce_plan(rows, C)["empty"] > 0
    o = R.bn_fwd_exact_operands(rows, C, seed=5, x_bf16=FV[vname][1])
    _bn_fwd_case(cuda_dev, o, FV[vname], True, f"{rows}x{C}", label="bn_fwd loop_tail")


# ---------------------------------------------------------- C. bn_fwd, eval ----
@pytest.mark.parametrize("rows,C", [(210, 24), (300, 1024)])
@pytest.mark.parametrize("vname", ["f32_y", "f32_y_yb_relu_res", "bf16_y_res", "bf16_y_yb_relu"])
def test_bn_fwd_eval(cuda_dev, vname, rows, C):
    ops = _ops()
    v = FV[vname]
    o = R.bn_fwd_operands(rows, C, seed=rows + 3 * C, x_bf16=v[1])
    got = _run_bn_fwd(ops, cuda_dev, o, v, False, training=False)
    rm, rv = o["rm0"].to(F64), o["rv0"].to(F64)
    r = 1.0 / torch.sqrt(rv + R.BN_EPS)
    yref, t = R.bn_apply(o["x"].to(F64), rm, r, o["g"].to(F64), o["b"].to(F64),
                         o["res"].to(F64) if v[5] else None, v[4], k=6)
    out = {"rmean unchanged": R.same_bits(got["rmean"], o["rm0"]),
           "rvar unchanged": R.same_bits(got["rvar"], o["rv0"])}
    R.check_apply(out, got, yref, t)
    _settle(f"bn_fwd eval {vname}", out, f"{rows}x{C}")


# ---------------------------------------------------------------- D. bn_bwd ----
def _run_bn_bwd(ops, dev, o, xb, yb, relu, wdx, wdxb, wdres, fused):
    rows, C = o["x"].shape
    ar = Arena(dev)
    x, y = _dev_x(o["x"], xb, dev), _dev_x(o["y"], yb, dev)
    dy, mean, rstd, g = (o[k].to(dev) for k in ("dy", "mean", "rstd", "g"))
    ws = ar.out(ops.chan_reduce_ws_floats(rows, C))
    dg, db = ar.out(C), ar.out(C)
    dx = ar.out(rows * C) if wdx else None
    dxb = ar.out(rows * C, BF) if wdxb else None
    dres = ar.out(rows * C) if wdres else None
    with _Fused(ops, fused):
        ops.bn_bwd(ptr(x), ptr(dy), ptr(y), ptr(mean), ptr(rstd), ptr(g), rows, C, relu, ptr(ws),
                   ptr(dg), ptr(db), ptr(dx), ptr(dres), stream_handle(), ptr(dxb), xb, yb)
        ar.intact()
    assert ops.bn_fused_error() == 0
    return dict(db=ar.body(db), dg=ar.body(dg), dx=ar.body(dx).reshape(rows, C) if wdx else None,
                dxb=ar.body(dxb).reshape(rows, C) if wdxb else None,
                dres=ar.body(dres).reshape(rows, C) if wdres else None)


_OUTS = [(True, False), (False, True), (True, True)]  # (dx, dxb)
# the four instantiations x relu x {dx, dxb, both}; dres on every other combination
BWD_COMBOS = [(xb, yb, relu, wdx, wdxb, i % 2 == 0) for i, (xb, yb, relu, (wdx, wdxb)) in enumerate(
    itertools.product((False, True), (False, True), (False, True), _OUTS))]


def _bn_bwd_case(dev, o_of, combos, exact, tag, fused_modes=(False, True)):
    ops = _ops()
    for xb, yb, relu, wdx, wdxb, wdres in combos:
        o = o_of(xb)
        name = (f"bn_bwd x{'bf16' if xb else 'f32'} y{'bf16' if yb else 'f32'}"
                f"{' relu' if relu else ''} {'exact' if exact else 'rounded'}")
        outs = "+".join(n for n, w in (("dx", wdx), ("dxb", wdxb), ("dres", wdres)) if w)
        runs = {}
        for fused in fused_modes:
            runs[fused] = _run_bn_bwd(ops, dev, o, xb, yb, relu, wdx, wdxb, wdres, fused)
            _settle(name + (" fused" if fused else ""), R.check_bn_bwd(o, relu, runs[fused], exact),
                    f"{tag} {outs}")
        if len(runs) == 2:
            _settle(name, _fused_equal(runs), f"{tag} {outs}")


def _bwd_ops(rows, C, exact):
    cache = {}

    def of(xb):
        if xb not in cache:
            cache[xb] = R.bn_bwd_operands(rows, C, seed=rows + C, exact=exact, x_bf16=xb)
        return cache[xb]
    return of


@pytest.mark.parametrize("rows,C", [(256, 4), (512, 12)])
def test_bn_bwd_exact_small(cuda_dev, rows, C):
    _bn_bwd_case(cuda_dev, _bwd_ops(rows, C, True), BWD_COMBOS, True, f"{rows}x{C}")


@pytest.mark.parametrize("rows,C,pick", [(2048, 256, [3 * j + j % 3 for j in range(8)]),
                                         (4096, 1024, [5, 7, 15, 23])])
def test_bn_bwd_exact_large(cuda_dev, rows, C, pick):
    """A covering subset: (2048, 256) every instantiation x relu, (4096, 1024)
    every instantiation; the outputs rotate."""
    combos = [BWD_COMBOS[i] for i in pick]
    assert {(c[0], c[1]) for c in combos} == set(itertools.product((False, True), repeat=2))
    _bn_bwd_case(cuda_dev, _bwd_ops(rows, C, True), combos, True, f"{rows}x{C}")


def test_bn_bwd_fused_loop_tail(cuda_dev):
    """(8192, 516), fusing on: the FU loop's third trip is partial."""
    ops = _ops()
    rows, C = 8192, 516
    with _Fused(ops, True):
        cap = ops.bn_fused_grid_cap()
    plan = R.fused_plan(rows, C, cap)
    assert cap > 0 and plan["partial"] and plan["trips"] >= 2, plan
    combos = [(False, False, True, True, True, True), (True, True, True, False, True, False)]
    _bn_bwd_case(cuda_dev, _bwd_ops(rows, C, True), combos, True, f"{rows}x{C}")


@pytest.mark.parametrize("rows,C", [(210, 24), (392, 64)])
def test_bn_bwd_rounded(cuda_dev, rows, C):
    of = _bwd_ops(rows, C, False)
    for relu in (False, True):
        assert R.drop_row_ratio_bwd(of(False), relu) >= 4.0
    _bn_bwd_case(cuda_dev, of, BWD_COMBOS, False, f"{rows}x{C}")


# -------------------------------------------------------- E. partial tables ----
TABLES = ([(192, P) for P in (1, 3, 127, 128, 129, 300)] + [(64, 1), (64, 128), (64, 129)]
          + [(1024, 3), (1024, 127), (1024, 300)])
TROWS = 256  # a power of two: the table is the operand, x need not agree with it


@pytest.mark.parametrize("C,P", TABLES)
def test_bn_fwd_partials(cuda_dev, C, P):
    ops = _ops()
    tab = R.table_operands(C, P, seed=C + P)
    s1, s2 = R.table_sums(tab)
    tabd = tab.to(cuda_dev)
    for vname in ("f32_y", "bf16_y_yb_relu_res"):
        xb = vname.startswith("bf16")
        v = (vname, xb, True, xb, xb, xb)
        o = R.bn_fwd_operands(TROWS, C, seed=C * 3 + P, x_bf16=xb)
        g = torch.Generator().manual_seed(P)
        o["rm0"] = torch.randint(8, 12, (C,), generator=g).to(F32) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
        st = R.bn_stats(None, o["rm0"].to(F64), o["rm0"].to(F64), o["rv0"].to(F64), exact=True,
                        sums=(s1, s2), rows=TROWS)
        assert bool((st["var"][0] > 0).all())
        assert bool((torch.sign(st["mean"][0]) == torch.sign(o["rm0"].to(F64))).all())
        runs = {}
        for fused in (False, True):
            ar = Arena(cuda_dev)
            x = _dev_x(o["x"], xb, cuda_dev)
            gd, bd = o["g"].to(cuda_dev), o["b"].to(cuda_dev)
            rs = o["res"].to(cuda_dev) if v[5] else None
            y = ar.out(TROWS * C)
            yb = ar.out(TROWS * C, BF) if v[3] else None
            mean, rstd, rm, rv = ar.out(C), ar.out(C), ar.out(C), ar.out(C)
            rm[:C], rv[:C] = o["rm0"].to(cuda_dev), o["rv0"].to(cuda_dev)
            with _Fused(ops, fused):
                ops.bn_fwd_partials(ptr(tabd), P, ptr(rm), ptr(x), TROWS, C, ptr(gd), ptr(bd), ptr(rs), ptr(y),
                                    ptr(mean), ptr(rstd), R.BN_EPS, R.BN_MOM, v[4], ptr(rm), ptr(rv),
                                    stream_handle(), ptr(yb), xb)
                ar.intact()
            assert ops.bn_fused_error() == 0
            got = dict(mean=ar.body(mean), rstd=ar.body(rstd), rmean=ar.body(rm), rvar=ar.body(rv),
                       y=ar.body(y).reshape(TROWS, C), yb=ar.body(yb).reshape(TROWS, C) if v[3] else None)
            runs[fused] = got
            _settle(f"bn_fwd_partials {'P<=128' if P <= R.FIN64_MAXP else 'P>128'} {vname}"
                    + (" fused" if fused else ""), R.check_bn_fwd(o, v[4], v[5], got, True, st=st), f"C={C} P={P}")
        if P > R.FIN64_MAXP:  # both forms sum in finalize_kernel's order
            _settle(f"bn_fwd_partials P>128 {vname}", _fused_equal(runs), f"C={C} P={P}")


@pytest.mark.parametrize("C,P", TABLES)
def test_bn_bwd_partials(cuda_dev, C, P):
    ops = _ops()
    tab = R.table_operands(C, P, seed=2 * C + P)
    sums = R.table_sums(tab)
    tabd = tab.to(cuda_dev)
    o = R.bn_bwd_operands(TROWS, C, seed=C + 5 * P, exact=False, x_bf16=True)
    for relu, wdx, wdres in ((True, True, True), (False, False, False)):
        runs = {}
        for fused in (False, True):
            ar = Arena(cuda_dev)
            x, y = _dev_x(o["x"], True, cuda_dev), _dev_x(o["y"], True, cuda_dev)
            dy, mean, rstd, g = (o[k].to(cuda_dev) for k in ("dy", "mean", "rstd", "g"))
            dg, db = ar.out(C), ar.out(C)
            dx = ar.out(TROWS * C) if wdx else None
            dxb = ar.out(TROWS * C, BF)
            dres = ar.out(TROWS * C) if wdres else None
            with _Fused(ops, fused):
                ops.bn_bwd_partials(ptr(tabd), P, ptr(x), ptr(dy), ptr(y), ptr(mean), ptr(rstd), ptr(g), TROWS,
                                    C, relu, ptr(dg), ptr(db), ptr(dx), ptr(dres), stream_handle(), ptr(dxb))
                ar.intact()
            assert ops.bn_fused_error() == 0
            got = dict(db=ar.body(db), dg=ar.body(dg), dx=ar.body(dx).reshape(TROWS, C) if wdx else None,
                       dxb=ar.body(dxb).reshape(TROWS, C), dres=ar.body(dres).reshape(TROWS, C) if wdres else None)
            runs[fused] = got
            name = f"bn_bwd_partials {'P<=128' if P <= R.FIN64_MAXP else 'P>128'}{' relu' if relu else ''}"
            _settle(name + (" fused" if fused else ""), R.check_bn_bwd(o, relu, got, False, sums=sums),
                    f"C={C} P={P}")
        if P > R.FIN64_MAXP:
            _settle(name, _fused_equal(runs), f"C={C} P={P}")


# ------------------------------------------------------------ F. max pooling ----
POOL_I32 = [("maxpool_fwd_kernel", (2, 7, 5, 10, 3, 2, 1)), ("maxpool_fwd_kernel", (3, 12, 8, 6, 2, 2, 0)),
            ("maxpool_fwd4_kernel", (2, 13, 9, 16, 3, 2, 1)), ("maxpool_fwd4_kernel", (2, 7, 5, 8, 3, 1, 1))]
G4, QUAD, K3S2 = "maxpool_bwd4b_kernel", "maxpool_bwd_k3s2_quad_kernel", "maxpool_bwd_k3s2_kernel"
POOL_U8 = [(G4, (2, 13, 9, 16, 3, 2, 1)), (G4, (2, 12, 8, 20, 2, 2, 0)), (G4, (2, 7, 5, 8, 3, 1, 1)),
           (G4, (1, 1, 1, 4, 3, 2, 1)), (G4, (2, 9, 6, 12, 5, 3, 2)),
           (QUAD, (2, 14, 10, 64, 3, 2, 1)), (QUAD, (3, 2, 2, 64, 3, 2, 1)),
           (K3S2, (2, 15, 9, 64, 3, 2, 1)), (K3S2, (2, 15, 10, 64, 3, 2, 1)), (K3S2, (2, 14, 9, 64, 3, 2, 1))]


def _bwd_kernel_of(N, H, W, C, k, s, p):
    """Mirror of maxpool_bwd_b8's dispatch."""
    if (k, s, p, C) == (3, 2, 1, 64):
        OH, OW = R.out_hw(H, W, k, s, p)
        return QUAD if H % 2 == 0 and W % 2 == 0 and OH == H // 2 and OW == W // 2 else K3S2
    return G4


@pytest.mark.parametrize("data", ["distinct", "ties"])
@pytest.mark.parametrize("kernel,shape", POOL_I32, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in POOL_I32])
def test_maxpool_int32(cuda_dev, kernel, shape, data):
    ops = _ops()
    N, H, W, C, k, s, p = shape
    assert (C % 4 == 0) == (kernel == "maxpool_fwd4_kernel")
    sh = ops.PoolShape(*shape)
    x = R.pool_data(N, H, W, C, data, seed=H * W + C)
    yr, t32, _ = R.maxpool_ref(x, k, s, p)
    assert (sh.OH, sh.OW) == tuple(yr.shape[1:3])
    dy = R.pool_dy(N, sh.OH, sh.OW, C, seed=C)
    dxr = R.maxpool_bwd_ref(dy, t32, N, H, W)
    ar = Arena(cuda_dev)
    n_out, n_in = yr.numel(), x.numel()
    y, arg, dx = ar.out(n_out), ar.out(n_out, torch.int32), ar.out(n_in)
    xd, dyd = x.to(cuda_dev), dy.to(cuda_dev)
    ops.maxpool_fwd(sh, ptr(xd), ptr(y), ptr(arg), stream_handle())
    ops.maxpool_bwd(sh, ptr(dyd), ptr(arg), ptr(dx), stream_handle())
    ar.intact()
    dxg = ar.body(dx).reshape(N, H, W, C)
    res = {"y": R.same_bits(ar.body(y).reshape(yr.shape), yr.to(F32)),
           "taps": R.same_bits(ar.body(arg).reshape(yr.shape), t32),
           "dx": R.same_bits(dxg, dxr.to(F32))}
    _settle(f"{kernel} + bwd {data}", res, "x".join(map(str, shape)))
    assert float(dxg.to(F64).sum()) == float(dy.to(F64).sum())


@pytest.mark.parametrize("data", ["distinct", "ties"])
@pytest.mark.parametrize("bwd,shape", POOL_U8, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in POOL_U8])
def test_maxpool_uint8(cuda_dev, bwd, shape, data):
    """fp32 input (maxpool_fwd_u8) and bf16 input (maxpool_fwd_b16: y only, yb
    only, both), then maxpool_bwd_b8 on the taps each forward recorded."""
    ops = _ops()
    N, H, W, C, k, s, p = shape
    assert _bwd_kernel_of(*shape) == bwd
    sh = ops.PoolShape(*shape)
    assert ops.maxpool_b16_ok(sh)
    x = R.pool_data(N, H, W, C, data, seed=H * W + C)  # bf16 values: both inputs read the same numbers
    yr, _, t8 = R.maxpool_ref(x, k, s, p)
    assert (sh.OH, sh.OW) == tuple(yr.shape[1:3])
    dy = R.pool_dy(N, sh.OH, sh.OW, C, seed=C)
    dxr = R.maxpool_bwd_ref(dy, R.tap8_to_pixel(t8, N, H, W, k, s, p), N, H, W)
    n_out, n_in = yr.numel(), x.numel()
    xd, xbd, dyd = x.to(cuda_dev), x.to(BF).to(cuda_dev), dy.to(cuda_dev)
    st = stream_handle()
    where = "x".join(map(str, shape))
    spec = "<3,2,1,16>" if (k, s, p, C) == (3, 2, 1, 64) else "<0,0,0,0>"
    for form in ("f32", "b16 y", "b16 yb", "b16 y+yb"):
        ar = Arena(cuda_dev)
        y = ar.out(n_out) if form != "b16 yb" else None
        yb = ar.out(n_out, BF) if "yb" in form else None
        arg, dx = ar.out(n_out, torch.uint8), ar.out(n_in)
        if form == "f32":
            ops.maxpool_fwd_u8(sh, ptr(xd), ptr(y), ptr(arg), st)
        else:
            ops.maxpool_fwd_b16(sh, ptr(xbd), ptr(y), ptr(yb), ptr(arg), st)
        ops.maxpool_bwd_b8(sh, ptr(dyd), ptr(arg), ptr(dx), st)
        ar.intact()
        dxg = ar.body(dx).reshape(N, H, W, C)
        res = {"taps": R.same_bits(ar.body(arg).reshape(yr.shape), t8), "dx": R.same_bits(dxg, dxr.to(F32))}
        if y is not None:
            res["y"] = R.same_bits(ar.body(y).reshape(yr.shape), yr.to(F32))
        if yb is not None:
            res["yb"] = R.same_bits(_bits(ar.body(yb)).reshape(yr.shape), R.bf16_bits(yr.to(F32)).reshape(yr.shape))
        _settle(f"maxpool_fwd4b_kernel{spec} {form} + {bwd} {data}", res, where)
        assert float(dxg.to(F64).sum()) == float(dy.to(F64).sum())


# ------------------------------------------------------ G. global average pool ----
@pytest.mark.parametrize("C", [32, 96, 33, 5])
def test_avgpool(cuda_dev, C):
    ops = _ops()
    N = 3
    kern = "avgpool_fwd_kernel" if C % 32 == 0 else "avgpool_fwd1_kernel"
    for HW in (1, 7, 8, 9, 16, 17, 24, 25, 49):
        x, exact = R.avgpool_operands(N, HW, C, seed=HW * 100 + C)
        yr, t = R.avgpool_ref(x, exact)
        g = torch.Generator().manual_seed(HW + C)
        dy = torch.randn(N, C, generator=g)
        ar = Arena(cuda_dev)
        y, dx = ar.out(N * C), ar.out(N * HW * C)
        xd, dyd = x.to(cuda_dev), dy.to(cuda_dev)
        ops.avgpool_fwd(ptr(xd), ptr(y), N, HW, C, stream_handle())
        ops.avgpool_bwd(ptr(dyd), ptr(dx), N, HW, C, stream_handle())
        ar.intact()
        yg = ar.body(y).reshape(N, C)
        res = {"y": R.same_bits(yg, yr.to(F32)) if exact else R.check_abs(yg, yr, t),
               "dx": R.same_bits(ar.body(dx).reshape(N, HW, C), R.avgpool_bwd_ref(dy, HW))}
        _settle(f"{kern} {'exact' if exact else 'rounded'} + avgpool_bwd_kernel", res, f"HW={HW} C={C}")
