"""The MFMA conv families of the generic engine (conv_bf16.hip, conv_tiled.hip,
the direct kernels of ops_generic.hip), route by route, against the references
of tests/helpers/conv_ref.py on the kernels' own operands.

Every case names the kernel, tile and split-K depth it is there for and
asserts them through `ops.conv_route`, which returns the plan that the
launcher of the same call executes (one planner per op, gops::plan_fwd /
plan_dgrad / plan_wgrad; its keyword flags say which operand copies,
statistics and workspace the call passes), so a plan change cannot move a case
onto another kernel and leave one untested.  The
kernels are driven through Fn.conv2d as the engine drives them: bf16 twins
attached to the inputs, bf16 dY where the route takes one, BatchNorm links
for the statistics epilogues, a GradJoin for the addend, the weight copies of
ConvWeightCopies.  Each case runs one forward and backward per mode:

  rounded: seeded normals already rounded to bf16; every output element within
           the derived bound `tol()` (n 2^-23 S, + 2^-8 (|ref| + acc) for a
           bf16 store) of the float64 reference; structural zeros exact;
  exact:   small integers whose every partial sum is below 2^24: bit equality
           with the reference whatever the tile, split or slab order.

tests/test_conv_ref_cpu.py shows on the CPU that dropped cells, K-steps,
slabs and pixel groups, wrapped pad taps, truncating stores, un-flipped taps,
exchanged parity classes, unwritten structural zeros, stale weight copies and
short statistics tables each fail these checks.

MTA_STAGE_REPORT=<path>: the worst err / tol per (route, output) of the
rounded mode is also written there as JSON (docs/ACCURACY.md holds a run's)."""

import dataclasses
import functools
import importlib.util
import json
import os
from typing import Optional

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("conv_ref", os.path.join(_HERE, "helpers", "conv_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16

REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    rows = {f"{route} | {out}": v for (route, out), v in sorted(REPORT.items())}
    for k, v in rows.items():
        print(f"[conv routes] {k}: {v:.3g}")
    path = os.environ.get("MTA_STAGE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(rows, f, indent=1, sort_keys=True)


def _ops():
    from mpi_tensorflow_amd.ops import native

    return native().ops


def _param(t):
    return Fn.Param(t.clone().requires_grad_(True), torch.zeros_like(t))


# ------------------------------------------------------------------ cases ----
# route = (kernel, bm, bn, z, halo) as ops.conv_route reports it
@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    shape: tuple                      # N, H, W, C, K, R, stride, pad
    fwd: tuple
    dgrad: Optional[tuple]
    wgrad: tuple
    modes: tuple = ("rounded", "exact")
    out_bf16: bool = False            # bf16 output, bf16 dY
    epi: bool = False                 # bias + ReLU forward epilogue
    stats: bool = False               # bn_out: the forward statistics
    bn_in: Optional[str] = None       # "relu" | "plain": the dgrad's BnBwdStats
    addend: bool = False              # GradJoin "final"
    copies: bool = True               # ConvWeightCopies (wcvt_batch) instead of the per-call convert
    stem: Optional[str] = None        # "im2col" | "implicit" | "s2d"
    preload: bool = True
    dgrad_family: str = "bf16"


H3 = "conv3_kernel"
FW = "fwd_kernel"
CASES = [
    # fwd_kernel 64 x 64, split-K 5 + 4 K-steps, M = 98 ragged; 3x3 s2 dgrad split
    Case("fwd64_split_f32", (2, 14, 14, 64, 128, 3, 2, 1), (FW, 64, 64, 2, False),
         ("dgrad3s2_kernel", 64, 64, 2, True), ("wgrad_kernel", 64, 128, 1, False), copies=False),
    Case("fwd64_split_bf16_stats", (2, 14, 14, 64, 128, 3, 2, 1), (FW, 64, 64, 2, False),
         ("dgrad3s2_kernel", 64, 64, 2, True), ("wgrad_kernel", 64, 128, 1, False),
         out_bf16=True, stats=True, bn_in="relu", addend=True),
    # the bias + ReLU epilogue forbids the split
    Case("fwd64_epilogue", (2, 14, 14, 64, 128, 3, 2, 1), (FW, 64, 64, 1, False),
         ("dgrad3s2_kernel", 64, 64, 2, True), ("wgrad_kernel", 64, 128, 1, False), epi=True),
    Case("fwd128x64", (8, 128, 128, 64, 64, 3, 2, 1), (FW, 128, 64, 1, False),
         ("dgrad3s2_kernel", 64, 64, 1, True), ("wgrad_kernel", 64, 64, 64, False),
         modes=("exact",), out_bf16=True),
    Case("fwd128x128", (4, 128, 128, 64, 256, 1, 2, 0), (FW, 128, 128, 1, False),
         (FW + "/ex2", 64, 64, 1, False), ("wgrad_kernel", 64, 128, 64, False)),
    # K % 128 == 64: 64-column tiles only (a 128-column tile stored past its row)
    Case("fwd_k192_bf16_stats", (3, 56, 56, 64, 192, 1, 1, 0), (FW, 64, 64, 1, False),
         (FW, 64, 64, 1, False), ("wgrad_kernel", 64, 64, 30, False), out_bf16=True, stats=True),
    Case("fwd_k192_epilogue", (3, 56, 56, 64, 192, 1, 1, 0), (FW, 64, 64, 1, False),
         (FW, 64, 64, 1, False), ("wgrad_kernel", 64, 64, 30, False), epi=True, copies=False),
    Case("dgrad_c192_addend", (3, 56, 56, 192, 64, 1, 1, 0), (FW, 64, 64, 1, False),
         (FW, 64, 64, 1, False), ("wgrad_kernel", 64, 64, 30, False), addend=True),
    # halo kernel: 128-row tiles need cdiv(M, 128) (K / 64) >= 256, i.e. 11 images of 56 x 56
    Case("conv3_128row", (11, 56, 56, 64, 64, 3, 1, 1), (H3, 128, 64, 1, True), (H3, 128, 64, 1, True),
         ("wgrad3_kernel", 128, 64, 154, True), modes=("exact",), out_bf16=True, bn_in="relu",
         addend=True),
    # (the sums of squares over 34496 rows need thinner operands: a case of its own)
    Case("conv3_128row_stats", (11, 56, 56, 64, 64, 3, 1, 1), (H3, 128, 64, 1, True),
         (H3, 128, 64, 1, True), ("wgrad3_kernel", 128, 64, 154, True), modes=("exact",), out_bf16=True,
         stats=True),
    Case("conv3_64row_f32", (4, 14, 14, 64, 64, 3, 1, 1), (H3, 64, 64, 1, True), (H3, 64, 64, 1, True),
         ("wgrad3_kernel", 64, 64, 16, True)),
    Case("conv3_64row_bf16_stats", (4, 14, 14, 64, 64, 3, 1, 1), (H3, 64, 64, 1, True),
         (H3, 64, 64, 1, True), ("wgrad3_kernel", 64, 64, 16, True), out_bf16=True, stats=True,
         bn_in="relu", addend=True),
    Case("conv3_split_bf16_stats", (3, 7, 7, 512, 512, 3, 1, 1), (H3, 64, 64, 8, True),
         (H3, 64, 64, 8, True), ("wgrad3_kernel", 64, 64, 3, True), out_bf16=True, stats=True,
         bn_in="plain", addend=True),
    Case("conv3_odd_image", (3, 11, 13, 64, 192, 3, 1, 1), (H3, 64, 64, 1, True), (H3, 64, 64, 3, True),
         ("wgrad3_kernel", 64, 64, 9, True), addend=True),
    Case("dgrad3s2_unsplit", (32, 56, 56, 64, 128, 3, 2, 1), (FW, 128, 64, 1, False),
         ("dgrad3s2_kernel", 64, 64, 1, True), ("wgrad_kernel", 64, 128, 56, False),
         modes=("exact",), out_bf16=True, bn_in="relu"),
    Case("dgrad3s2_split_bf16_stats", (2, 28, 28, 64, 128, 3, 2, 1), (FW, 64, 64, 2, False),
         ("dgrad3s2_kernel", 64, 64, 2, True), ("wgrad_kernel", 64, 128, 1, False),
         out_bf16=True, stats=True, bn_in="plain", addend=True),
    Case("dgrad1x1s2", (4, 14, 14, 128, 64, 1, 2, 0), (FW, 64, 64, 1, False),
         (FW + "/ex2", 64, 64, 1, False), ("wgrad_kernel", 128, 64, 1, False)),
    Case("dgrad1x1s2_addend", (4, 14, 14, 128, 64, 1, 2, 0), (FW, 64, 64, 1, False),
         (FW + "/ex2", 64, 64, 1, False), ("wgrad_kernel", 128, 64, 1, False), out_bf16=True,
         addend=True),
    # odd input, stride 2: the dgrad is not a bf16-family shape (tiled kernels, bf16 operands)
    Case("odd_s2_3x3", (2, 13, 13, 64, 128, 3, 2, 1), (FW, 64, 64, 2, False),
         ("data_kernel", 64, 64, 4, False), ("wgrad_kernel", 64, 128, 1, False), dgrad_family="tiled"),
    Case("odd_s2_1x1_bf16", (2, 13, 13, 64, 128, 1, 2, 0), (FW, 64, 64, 1, False),
         ("data_kernel", 64, 64, 1, False), ("wgrad_kernel", 64, 128, 1, False), out_bf16=True,
         dgrad_family="tiled"),
    Case("wgrad3_64px_split", (2, 14, 14, 256, 256, 3, 1, 1), (H3, 64, 64, 4, True), (H3, 64, 64, 4, True),
         ("wgrad3_kernel", 64, 64, 8, True)),
    Case("wgrad3_unsplit", (1, 7, 7, 512, 512, 3, 1, 1), (H3, 64, 64, 8, True), (H3, 64, 64, 8, True),
         ("wgrad3_kernel", 64, 64, 1, True), copies=False),
    Case("wgrad3_128px", (8, 56, 56, 64, 64, 3, 1, 1), (H3, 64, 64, 1, True), (H3, 64, 64, 1, True),
         ("wgrad3_kernel", 128, 64, 224, True), modes=("exact",)),
    Case("wgrad_128x128", (4, 14, 14, 128, 256, 1, 2, 0), (FW, 64, 64, 1, False),
         (FW + "/ex2", 64, 64, 1, False), ("wgrad_kernel", 128, 128, 1, False)),
    Case("wgrad_64x64_k192", (3, 9, 9, 64, 192, 1, 2, 0), (FW, 64, 64, 1, False),
         ("data_kernel", 64, 64, 1, False), ("wgrad_kernel", 64, 64, 1, False), dgrad_family="tiled"),
    # stems (no input gradient): materialised im2col, implicit loader, space-to-depth
    Case("stem_im2col_7x7", (2, 37, 41, 3, 64, 7, 2, 3), (FW, 64, 64, 1, False), None,
         ("wgrad_kernel", 64, 64, 3, False), stem="im2col"),
    Case("stem_im2col_5x5", (2, 37, 41, 3, 128, 5, 1, 2), (FW, 64, 64, 1, False), None,
         ("wgrad_kernel", 128, 128, 12, False), stem="im2col"),
    Case("stem_implicit_5x5", (2, 37, 41, 3, 128, 5, 1, 2), (FW + "/StemLoader", 128, 64, 1, False), None,
         ("wgrad_kernel/StemWgLoader", 128, 128, 12, False), out_bf16=True, stats=True, stem="implicit"),
    Case("stem_s2d_odd", (2, 37, 41, 3, 64, 7, 2, 3), (FW + "/S2dLoaderPre", 128, 64, 1, False), None,
         ("wgrad_kernel", 64, 64, 3, False), out_bf16=True, stats=True, stem="s2d"),
    Case("stem_s2d_odd_no_preload", (2, 37, 41, 3, 64, 7, 2, 3), (FW + "/S2dLoader", 128, 64, 1, False),
         None, ("wgrad_kernel", 64, 64, 3, False), out_bf16=True, stem="s2d", preload=False),
    Case("stem_s2d_even", (2, 32, 48, 3, 128, 7, 2, 3), (FW + "/S2dLoaderPre", 128, 64, 1, False), None,
         ("wgrad_kernel", 64, 128, 3, False), out_bf16=True, stats=True, stem="s2d"),
    Case("stem_s2d_even_no_preload", (2, 32, 48, 3, 128, 7, 2, 3), (FW + "/S2dLoader", 128, 64, 1, False),
         None, ("wgrad_kernel", 64, 128, 3, False), out_bf16=True, stem="s2d", preload=False),
]
RUNS = [(c, m) for c in CASES for m in c.modes]


def _as_tuple(d):
    return (d["kernel"], d["bm"], d["bn"], d["z"], d["halo"])


def routes_of(case, x_like=None):
    """The routes the launchers take for a case (bf16 conv mode must be on)."""
    ops = _ops()
    N, H, W, C, K, Rr, stride, pad = case.shape
    sh = ops.ConvShape(N, H, W, C, K, Rr, Rr, stride, pad)
    if case.stem:
        probe = x_like if x_like is not None else torch.zeros(1)
        kp = Fn._im2col_kp(sh, probe, False, False)
        assert kp > 0, "not a stem-route shape"
        s1 = ops.ConvShape(N, sh.OH, sh.OW, kp, K, 1, 1, 1, 0)
        if case.stem == "s2d":
            assert Fn._s2d_stem_ok(sh)
            si = Fn._s2d_shape(sh)
            f, g = ops.conv_route(si, "fwd", True, stem=2), ops.conv_route(si, "wgrad", True, stem=2)
        elif case.stem == "implicit":
            assert not Fn._s2d_stem_ok(sh)
            f, g = ops.conv_route(s1, "fwd", True, stem=1), ops.conv_route(s1, "wgrad", True, stem=1)
        else:
            f, g = ops.conv_route(s1, "fwd", True), ops.conv_route(s1, "wgrad", True)
        assert f["family"] == g["family"] == "bf16" and f["stem"] == (case.stem != "im2col")
        return _as_tuple(f), None, _as_tuple(g)
    f = ops.conv_route(sh, "fwd", True, case.epi)
    d = ops.conv_route(sh, "dgrad", True)
    g = ops.conv_route(sh, "wgrad", True)
    assert f["family"] == g["family"] == "bf16" and d["family"] == case.dgrad_family
    return _as_tuple(f), _as_tuple(d), _as_tuple(g)


# --------------------------------------------------------------- operands ----
def _extras(case, o, mode, seed):
    """Statistics operands: the forward shift, and the BatchNorm whose output
    the conv reads (its bf16 input bx, mean, rstd)."""
    N, H, W, C, K, Rr, stride, pad = case.shape
    g = torch.Generator().manual_seed(seed + 1000)
    if mode == "exact":
        o["shift"] = torch.randint(-2, 3, (K,), generator=g).to(F32)
        o["bx"] = torch.randint(-3, 4, (N, H, W, C), generator=g).to(F32)
        o["mean"] = torch.randint(-1, 2, (C,), generator=g).to(F32)
        o["rstd"] = torch.tensor([1.0, 2.0])[torch.randint(0, 2, (C,), generator=g)]
    else:
        o["shift"] = torch.randn(K, generator=g) * 0.3
        o["bx"] = R.bf16_rne(torch.randn(N, H, W, C, generator=g) * 2 + 0.5)
        o["mean"] = torch.randn(C, generator=g) * 0.3 + 0.5
        o["rstd"] = torch.rand(C, generator=g) * 0.5 + 0.3
    return o


@functools.lru_cache(maxsize=2)
def operands(case, mode):
    N, H, W, C, K, Rr, stride, pad = case.shape
    seed = 100 + [c.id for c in CASES].index(case.id)
    if mode == "rounded":
        return _extras(case, R.gen_rounded(seed, *case.shape, bias=case.epi, addend=case.addend), mode, seed)

    def also(o):
        """Exact statistics: the sums of |terms| of all four, from the references."""
        _extras(case, o, mode, seed)
        top = 0.0
        if case.stats:
            yb = R.bf16_rne(o["refs"]["fwd"][0])
            top = max(top, float(R.stats_fwd(yb, o["shift"], dt=F32)[3].max()))
        if case.bn_in:
            s = R.stats_bwd(o["refs"]["dgrad"][0], o["bx"], o["x"], o["mean"], o["rstd"],
                            case.bn_in == "relu", dt=F32)
            top = max(top, float(s[1].max()), float(s[3].max()))
        return top

    if case.epi:  # the ReLU mask reaches the gradients: references after the forward (run())
        o = R.gen_exact(seed, *case.shape, bias=True, relu=True)
        return _extras(case, o, mode, seed)
    return R.gen_exact(seed, *case.shape, addend=case.addend, also=also)


def _note(route, out, worst):
    key = (f"{route[0]} {route[1]}x{route[2]} z{route[3]}" if route[1] else route[0], out)
    REPORT[key] = max(REPORT.get(key, 0.0), worst)


def _compare(case, mode, route, out, got, ref, S, n, bf16_out=False, zero=None):
    got = got.detach().cpu()
    if mode == "exact":
        R.assert_exact(S.max())
        bad, at = R.exact_diff(got, ref, bf16_out)
        assert bad == 0, f"{case.id} {out} ({route}): {bad} elements differ from the integer reference, first at {at}"
        return
    ref, S = ref.to(F64), S.to(F64)
    worst, over, nzero = R.check(got, ref, S, n, bf16_out, zero)
    print(f"[conv routes] {case.id} {out}: worst err / tol {worst:.3g}, over {over}, zeros {nzero}")
    _note(route, out, worst)
    assert over == 0 and nzero == 0, (
        f"{case.id} {out} ({route}): {over} over the bound (worst err / tol {worst:.3g}), {nzero} "
        f"non-zero structural zeros; first (index, got, ref, tol): {R.where_over(got, ref, S, n, bf16_out)}")


# -------------------------------------------------------------------- run ----
@pytest.mark.parametrize("case,mode", RUNS, ids=[f"{c.id}-{m}" for c, m in RUNS])
def test_conv_route(cuda_dev, case, mode):
    ops = _ops()
    N, H, W, C, K, Rr, stride, pad = case.shape
    o = operands(case, mode)
    dt = F32 if mode == "exact" else F64
    dev = cuda_dev
    relu_in = case.bn_in == "relu"
    Fn.set_conv_bf16(True)
    ops.s2d_stem_set_preload(case.preload)
    try:
        xg = o["x"].to(dev).requires_grad_(case.stem is None)
        rf, rd, rg = routes_of(case, xg)
        assert (rf, rd, rg) == (case.fwd, case.dgrad, case.wgrad), f"{case.id}: the plan moved this case"
        if case.stem is None:
            Fn._attach_bf16(xg, o["x"].to(BF).to(dev))  # the bf16 twin: the same bits
        wp = _param(o["w"].to(dev))
        if case.copies and case.stem is None:
            Fn.ConvWeightCopies({"w": wp}, dev).refresh()
            assert wp.wtb is not None and wp.wtb_d is not None
        bp = _param(o["bias"].to(dev)) if case.epi else None
        lk_out = Fn.BnLink(o["shift"].to(dev)) if case.stats else None
        lk_in = None
        if case.bn_in:
            lk_in = Fn.BnLink()
            lk_in.bwd_src = (o["bx"].to(BF).to(dev), o["x"].to(BF).to(dev), o["mean"].to(dev),
                             o["rstd"].to(dev), relu_in)
        join = Fn.GradJoin() if case.addend else None
        y = Fn.conv2d(xg, wp, bp, stride, pad, case.epi, join, "final" if join else None,
                      out_bf16=case.out_bf16, bn_out=lk_out, bn_in=lk_in)
        assert y.dtype == (BF if case.out_bf16 else F32)
        if join is not None:
            join.stash(o["addend"].to(dev))
        dy = o["dy"].to(dev)
        y.backward(dy.to(BF) if case.out_bf16 else dy)
        torch.cuda.synchronize()
    finally:
        ops.s2d_stem_set_preload(True)
        Fn.set_conv_bf16(False)

    yc = y.detach().float().cpu()
    if case.epi:
        # the ReLU mask the backward saw is the kernel's own y > 0
        ref, S, n = (o["refs"]["fwd"] if mode == "exact" else
                     R.conv_fwd(o["x"], o["w"], stride, pad, o["bias"], True))
        _compare(case, mode, rf, "y", yc, ref, S, n)
        dym = o["dy"] * (yc > 0)
        _compare(case, mode, rd, "dX", xg.grad, *R.conv_dgrad(dym, o["w"], stride, pad, H, W, dt=dt))
        _compare(case, mode, rg, "dW", wp.grad_view, *R.conv_wgrad(o["x"], dym, stride, pad, Rr, dt=dt))
        _compare(case, mode, ("colsum2", 0, 0, 1, False), "db", bp.grad_view, *R.bias_grad(dym, dt=dt))
        return
    if mode == "exact":
        fwd, dgr, wgr = o["refs"]["fwd"], o["refs"]["dgrad"], o["refs"]["wgrad"]
    else:
        fwd = R.conv_fwd(o["x"], o["w"], stride, pad)
        dgr = R.conv_dgrad(o["dy"], o["w"], stride, pad, H, W, o.get("addend")) if case.stem is None else None
        wgr = R.conv_wgrad(o["x"], o["dy"], stride, pad, Rr)
    _compare(case, mode, rf, "y (bf16 store)" if case.out_bf16 else "y", yc, *fwd, bf16_out=case.out_bf16)
    _compare(case, mode, rg, "dW", wp.grad_view, *wgr)
    if case.stem is None:
        zero = None
        if Rr == 1 and stride == 2 and not case.addend:  # three structural zeros per 2 x 2 block
            zero = torch.ones(N, H, W, C, dtype=torch.bool)
            zero[:, 0::2, 0::2] = False
        _compare(case, mode, rd, "dX", xg.grad, *dgr, zero=zero)
    if case.stats:  # the partial rows summed, against the kernel's own bf16 output
        assert lk_out.fwd is not None
        part, P = lk_out.fwd
        g1, g2 = R.part_sums(part, K, P)
        s1, S1, s2, S2, ns = R.stats_fwd(yc, o["shift"], dt=dt)
        _compare(case, mode, rf, "stats sum", g1, s1, S1, ns)
        _compare(case, mode, rf, "stats sumsq", g2, s2, S2, ns)
    if case.bn_in:  # against the kernel's own fp32 dX
        assert lk_in.bwd is not None, "the dgrad did not write the BatchNorm backward sums"
        part, P, dx = lk_in.bwd
        assert dx.data_ptr() == xg.grad.data_ptr() or torch.equal(dx, xg.grad)
        g1, g2 = R.part_sums(part, C, P)
        t1, T1, t2, T2, n1, n2 = R.stats_bwd(xg.grad.cpu(), o["bx"], o["x"], o["mean"], o["rstd"], relu_in,
                                             dt=dt)
        _compare(case, mode, rd, "bwd stats sum", g1, t1, T1, n1)
        _compare(case, mode, rd, "bwd stats sum xhat", g2, t2, T2, n2)


# ------------------------------------------------- K % 128 == 64, guarded ----
def test_k192_forward_stays_inside_its_output(cuda_dev):
    """The forward of K = 192 at the size that used to pick a 128-column tile,
    called on an output that lies inside a larger buffer: the floats behind it
    keep their value (the 128-column tile stored 64 floats past the last row)."""
    from mpi_tensorflow_amd.ops import ptr, stream_handle

    ops = _ops()
    N, H, C, K = 3, 56, 64, 192
    sh = ops.ConvShape(N, H, H, C, K, 1, 1, 1, 0)
    r = ops.conv_route(sh, "fwd", True)
    assert (r["kernel"], r["bn"]) == ("fwd_kernel", 64)
    for c in (64, 192, 320, 448):  # no 128-column tile on any K % 128 == 64, at any M
        for n in (1, 3, 64):
            for op in ("fwd", "dgrad"):
                s = ops.ConvShape(n, H, H, c if op == "dgrad" else 64, 64 if op == "dgrad" else c, 1, 1, 1, 0)
                assert ops.conv_route(s, op, True)["bn"] == 64
    o = R.gen_exact(77, N, H, H, C, K, 1, 1, 0)
    M, canary = N * H * H, -777.0
    x, w = o["x"].to(cuda_dev), o["w"].to(cuda_dev)
    buf = torch.full((M * K + 4096,), canary, device=cuda_dev)
    ws = torch.zeros(max(int(ops.conv_ws_floats(sh, False)), 4), device=cuda_dev)
    ops.conv_fwd(sh, ptr(x), ptr(w), 0, ptr(buf), False, ptr(ws), stream_handle(), True)
    torch.cuda.synchronize()
    assert R.guard_hits(buf.cpu(), M * K, canary) == 0
    assert R.exact_diff(buf[:M * K].reshape(N, H, H, K), o["refs"]["fwd"][0])[0] == 0


# ------------------------- routes chosen by what the call passes, exact ----
def _direct(cuda_dev, shape, seed, also=None):
    """ConvShape, exact operands on the device and a zeroed workspace, for ops called directly."""
    ops = _ops()
    N, H, W, C, K, Rr, stride, pad = shape
    sh = ops.ConvShape(N, H, W, C, K, Rr, Rr, stride, pad)
    o = R.gen_exact(seed, *shape, also=also)
    R.assert_exact(*(r[1].max() for r in o["refs"].values()))
    d = {k: o[k].to(cuda_dev) for k in ("x", "w", "dy")}
    ws = torch.zeros(max(int(ops.conv_ws_floats(sh, False)), 4), device=cuda_dev)
    return ops, sh, o, d, ws


def test_fp32_forward_with_statistics_leaves_the_halo_kernel(cuda_dev):
    """fp32 forward with the weight copy passed: conv3f_kernel, but fwd_kernel
    once BatchNorm statistics are wanted (the forward of most 3x3 layers of
    ResNet-18 in fp32 training); output and both statistics sums to the bit."""
    from mpi_tensorflow_amd.ops import ptr, stream_handle

    shape = (2, 14, 14, 64, 64, 3, 1, 1)
    K = shape[4]
    g = torch.Generator().manual_seed(41)
    shift = torch.randint(-2, 3, (K,), generator=g).to(F32)
    ops, sh, o, d, ws = _direct(
        cuda_dev, shape, 81, also=lambda o: float(R.stats_fwd(o["refs"]["fwd"][0], shift, dt=F32)[3].max()))
    assert ops.conv_route(sh, "fwd", False, wcopy=True)["kernel"] == "conv3f_kernel"
    r = ops.conv_route(sh, "fwd", False, wcopy=True, stats=True)
    assert (r["family"], r["kernel"]) == ("tiled", "fwd_kernel")
    rows = ops.conv_fwd_stats_rows(sh, False)
    assert r["stats_rows"] == rows > 0
    wp = _param(d["w"])
    Fn.ConvWeightCopies({"w": wp}, cuda_dev, kind="f32flip").refresh()
    assert wp.wtb_d is not None
    y = torch.empty(sh.N, sh.OH, sh.OW, K, device=cuda_dev)
    part = torch.zeros(2 * K * rows, device=cuda_dev)
    sg = shift.to(cuda_dev)
    ops.conv_fwd(sh, ptr(d["x"]), ptr(d["w"]), 0, ptr(y), False, ptr(ws), stream_handle(), False, 0,
                 ptr(wp.wtb_d), 0, ptr(part), rows, ptr(sg))
    torch.cuda.synchronize()
    yc = y.cpu()
    assert R.exact_diff(yc, o["refs"]["fwd"][0])[0] == 0
    g1, g2 = R.part_sums(part, K, rows)
    s1, _, s2, S2, _ = R.stats_fwd(yc, shift, dt=F32)
    R.assert_exact(S2.max())
    assert torch.equal(g1.to(F32), s1) and torch.equal(g2.to(F32), s2)


def test_bf16_mode_without_operand_copies(cuda_dev):
    """bf16 conv mode with a bf16 operand copy left out: the forward without xb
    runs fwd_kernel (not conv3_kernel), the 3x3 stride-2 dgrad with the fp32 dY
    alone the tiled family's data_kernel, the filter gradient without dyb
    wgrad_kernel (not wgrad3_kernel); each to the bit."""
    from mpi_tensorflow_amd.ops import ptr, stream_handle

    st = stream_handle()
    ops, sh, o, d, ws = _direct(cuda_dev, (2, 14, 14, 64, 64, 3, 1, 1), 82)
    assert ops.conv_route(sh, "fwd", True)["kernel"] == "conv3_kernel"
    r = ops.conv_route(sh, "fwd", True, act16=False)
    assert (r["family"], r["kernel"]) == ("bf16", "fwd_kernel")
    y = torch.empty(sh.N, sh.OH, sh.OW, sh.K, device=cuda_dev)
    ops.conv_fwd(sh, ptr(d["x"]), ptr(d["w"]), 0, ptr(y), False, ptr(ws), st, True)
    torch.cuda.synchronize()
    assert R.exact_diff(y, o["refs"]["fwd"][0])[0] == 0

    ops, sh, o, d, ws = _direct(cuda_dev, (2, 14, 14, 64, 128, 3, 2, 1), 83)
    assert ops.conv_route(sh, "dgrad", True)["kernel"] == "dgrad3s2_kernel"
    r = ops.conv_route(sh, "dgrad", True, act16=False)
    assert (r["family"], r["kernel"]) == ("tiled", "data_kernel")
    dx = torch.empty(sh.N, sh.H, sh.W, sh.C, device=cuda_dev)
    ops.conv_bwd_data(sh, ptr(d["dy"]), ptr(d["w"]), ptr(dx), ptr(ws), st, True)
    torch.cuda.synchronize()
    assert R.exact_diff(dx, o["refs"]["dgrad"][0])[0] == 0

    ops, sh, o, d, ws = _direct(cuda_dev, (4, 14, 14, 64, 64, 3, 1, 1), 84)
    assert ops.conv_route(sh, "wgrad", True)["kernel"] == "wgrad3_kernel"
    r = ops.conv_route(sh, "wgrad", True, dy16=False)
    assert (r["family"], r["kernel"]) == ("bf16", "wgrad_kernel")
    xb = d["x"].to(BF)
    dw = torch.empty_like(d["w"])
    ops.conv_bwd_filter(sh, ptr(d["x"]), ptr(d["dy"]), ptr(ws), ptr(dw), st, True, ptr(xb), 0)
    torch.cuda.synchronize()
    assert R.exact_diff(dw, o["refs"]["wgrad"][0])[0] == 0


def test_fp32_filter_gradient_k_tile_depth(cuda_dev):
    """The fp32 64 x 128 filter tiles on 16-pixel K tiles (TiledPlan wg_bk16)
    and on 32-pixel ones: the route names the depth, the bits are equal."""
    from mpi_tensorflow_amd.ops import ptr, stream_handle

    ops, sh, o, d, ws = _direct(cuda_dev, (4, 28, 28, 64, 128, 3, 2, 1), 85)
    plan = ops.get_tiled_plan()
    got = []
    try:
        for on, bk in ((True, 16), (False, 32)):
            p = ops.get_tiled_plan()
            p.wg_bk16 = on
            ops.set_tiled_plan(p)
            r = ops.conv_route(sh, "wgrad", False)
            assert (r["kernel"], r["bm"], r["bn"], r["bk"]) == ("filter_kernel", 64, 128, bk)
            dw = torch.empty_like(d["w"])
            ops.conv_bwd_filter(sh, ptr(d["x"]), ptr(d["dy"]), ptr(ws), ptr(dw), stream_handle())
            torch.cuda.synchronize()
            assert R.exact_diff(dw, o["refs"]["wgrad"][0])[0] == 0
            got.append(dw.cpu())
    finally:
        ops.set_tiled_plan(plan)
    assert torch.equal(got[0].view(torch.int32), got[1].view(torch.int32))


# ----------------------------------------- fp32 tiled family, exact mode ----
# the shape lists of tests/test_generic_ops_gpu.py (test_conv_fwd_bwd,
# test_fp32_halo_conv3x3_fwd_and_dgrad, test_fp32_filter_grad_xcd_slice_order,
# test_fp32_dgrad3s2_halo) with their TiledPlan variants; (shape, relu, bias,
# weight copy, plan fields, routes) - routes as (family, kernel, bm, bn, z)
_cspec = importlib.util.spec_from_file_location("conv_plan_cases", os.path.join(_HERE, "helpers", "conv_plan_cases.py"))
PC = importlib.util.module_from_spec(_cspec)
_cspec.loader.exec_module(PC)
_halo_variants, FP32_SHAPES, HALO_SHAPES = PC._halo_variants, PC.FP32_SHAPES, PC.HALO_SHAPES
XCD_SHAPES, S2_SHAPES, XCD_VARIANTS, S2_VARIANTS = PC.XCD_SHAPES, PC.S2_SHAPES, PC.XCD_VARIANTS, PC.S2_VARIANTS

FP32_RUNS = ([(s[:8], s[8], s[9], False, [{}]) for s in FP32_SHAPES] +
             [((N, H, W, C, K, 3, 1, 1), False, False, True, _halo_variants()) for N, H, W, C, K in HALO_SHAPES] +
             [((N, H, H, C, K, Rr, st, pd), False, False, False, XCD_VARIANTS)
              for N, H, C, K, Rr, st, pd in XCD_SHAPES] +
             [((N, H, H, C, K, 3, 2, 1), False, False, False, S2_VARIANTS)
              for N, H, C, K in S2_SHAPES])


def _fp32_routes(ops, shape, epi, wcopy):
    N, H, W, C, K, Rr, stride, pad = shape
    sh = ops.ConvShape(N, H, W, C, K, Rr, Rr, stride, pad)
    out = []
    for op in ("fwd", "dgrad", "wgrad"):
        d = ops.conv_route(sh, op, False, epi and op == "fwd", wcopy)
        out.append((d["family"], d["kernel"], d["bm"], d["bn"], d["z"]))
    return tuple(out)


def _fp32_id(r):
    return "x".join(str(v) for v in r[0]) + ("_copy" if r[3] else "") + f"_{len(r[4])}plans"


@pytest.mark.parametrize("shape,relu,bias,wcopy,variants", FP32_RUNS, ids=[_fp32_id(r) for r in FP32_RUNS])
def test_fp32_family_exact(cuda_dev, shape, relu, bias, wcopy, variants):
    """fp32 operands, integers: every tile, split and plan variant of the
    tiled, halo, direct and gather kernels gives the integer result itself."""
    ops = _ops()
    N, H, W, C, K, Rr, stride, pad = shape
    key = "x".join(str(v) for v in shape) + ("_copy" if wcopy else "")
    o = R.gen_exact(300 + len(key) + sum(shape), *shape, bias=bias, relu=relu)
    plan = ops.get_tiled_plan()
    try:
        for vi, fields in enumerate(variants):
            p = ops.get_tiled_plan()
            for k, v in fields.items():
                setattr(p, k, v)
            ops.set_tiled_plan(p)
            routes = _fp32_routes(ops, shape, relu or bias, wcopy)
            assert routes == FP32_ROUTES[key][vi], f"{key} plan {vi}: the plan moved this case: {routes}"
            wp = _param(o["w"].to(cuda_dev))
            if wcopy:
                Fn.ConvWeightCopies({"w": wp}, cuda_dev, kind="f32flip").refresh()
                assert wp.wtb_d is not None
            bp = _param(o["bias"].to(cuda_dev)) if bias else None
            xg = o["x"].to(cuda_dev).requires_grad_(True)
            y = Fn.conv2d(xg, wp, bp, stride, pad, relu)
            y.backward(o["dy"].to(cuda_dev))
            torch.cuda.synchronize()
            yc = y.detach().cpu()
            where = f"{key} plan {vi} {routes}"
            assert torch.equal(yc, o["refs"]["fwd"][0]), where
            dym = o["dy"] * (yc > 0) if relu else o["dy"]
            dgr = R.conv_dgrad(dym, o["w"], stride, pad, H, W, dt=F32) if relu else o["refs"]["dgrad"]
            wgr = R.conv_wgrad(o["x"], dym, stride, pad, Rr, dt=F32) if relu else o["refs"]["wgrad"]
            R.assert_exact(dgr[1].max(), wgr[1].max())
            for name, got, ref in (("dX", xg.grad, dgr[0]), ("dW", wp.grad_view, wgr[0])):
                bad, at = R.exact_diff(got, ref)
                assert bad == 0, f"{where} {name}: {bad} elements differ, first at {at}"
            if bias:
                assert R.exact_diff(bp.grad_view, R.bias_grad(dym, dt=F32)[0])[0] == 0, where
    finally:
        ops.set_tiled_plan(plan)


# ------------------------------------------------------ conversions, bits ----
def _special_values(n, seed):
    """fp32 values whose bf16 rounding has to be right to the bit: ties (to
    even, both ways), values that round up into the next binade, fp32 and
    bf16 denormals, +-0, the largest finite value (rounds to infinity), the
    largest that stays finite, and seeded normals."""
    bits = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3FFFFFFF, 0x3FFF8000, 0x407FC000,
            0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x00800000, 0x0000FFFF,
            0x00000000, 0x80000000, 0x7F7FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0xFF7FFFFF, 0x7F800000,
            0x3F800000, 0xBF808000, 0xBF818000, 0x80008000]
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 8)
    sp = torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())
    idx = torch.randperm(n, generator=g)[:4 * len(bits)]
    v[idx] = sp.repeat(4)
    return v


def test_to_bf16_bits(cuda_dev):
    from mpi_tensorflow_amd.ops import ptr, stream_handle

    x = _special_values(8 * 1000 + 8 * 7, 5)
    xg = x.to(cuda_dev)
    y = torch.empty(x.numel(), dtype=BF, device=cuda_dev)
    _ops().to_bf16(ptr(xg), ptr(y), x.numel(), stream_handle())
    torch.cuda.synchronize()
    want, got = R.bf16_bits(x), R.as_bits(y)
    bad = (want != got).nonzero().reshape(-1)[:8]
    assert bad.numel() == 0, [(hex(int(x[i].view(torch.int32)) & 0xFFFFFFFF), hex(int(got[i]) & 0xFFFF),
                               hex(int(want[i]) & 0xFFFF)) for i in bad]


def test_wcvt_batch_modes_bits(cuda_dev):
    """wcvt_batch mode 0 (bf16 [tap][co][ci]), 1 (bf16 [taps - 1 - tap][ci][co])
    and 2 (fp32 [taps - 1 - tap][co][ci]) once each, bit for bit (the conv cases
    above check the layouts through their results)."""
    from mpi_tensorflow_amd.ops import ptr, stream_handle

    ops = _ops()
    taps, C, K = 9, 64, 96
    w = _special_values(taps * C * K, 6).reshape(taps, C, K)
    wg = w.to(cuda_dev)
    o0 = torch.empty(taps * C * K, dtype=BF, device=cuda_dev)
    o1 = torch.empty(taps * C * K, dtype=BF, device=cuda_dev)
    o2 = torch.empty(taps * C * K, dtype=F32, device=cuda_dev)
    nb = ops.wcvt_blocks(taps, C, K)
    jobs = torch.tensor([[ptr(wg), ptr(o0), taps, C, K, 0, 0, 0], [ptr(wg), ptr(o1), taps, C, K, 1, nb, 0],
                         [ptr(wg), ptr(o2), taps, C, K, 2, 2 * nb, 0]], dtype=torch.int64, device=cuda_dev)
    ops.wcvt_batch(ptr(jobs), 3, 3 * nb, stream_handle())
    torch.cuda.synchronize()
    assert torch.equal(R.as_bits(o0), R.bf16_bits(w.permute(0, 2, 1).contiguous()).reshape(-1))
    assert torch.equal(R.as_bits(o1), R.bf16_bits(w.flip(0).contiguous()).reshape(-1))
    assert torch.equal(o2.cpu().view(torch.int32), w.flip(0).permute(0, 2, 1).contiguous().reshape(-1).view(torch.int32))


# ----------------------------------------------- stem buffers: exact zeros ----
def test_stem_padding_is_exactly_zero(cuda_dev):
    """The im2col's padding columns (each tap row's tail up to seg, and R seg ..
    kp) and the taps the 8 x 8 extension adds to the 7 x 7 filter hold exact
    zeros, whatever the image and the filter hold."""
    from mpi_tensorflow_amd.ops import ptr, stream_handle

    ops = _ops()
    s = stream_handle()
    N, H, W, K, Rr = 2, 37, 41, 64, 7
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(N, H, W, 3, generator=g) + 1.0).to(cuda_dev)  # no zeros in the image
    sh = ops.ConvShape(N, H, W, 3, K, Rr, Rr, 2, 3)
    seg, kp = Fn._im2col_seg(sh), 192
    col = torch.full((N * sh.OH * sh.OW, kp), 7.0, dtype=BF, device=cuda_dev)
    ops.im2col_bf16(sh, ptr(x), kp, ptr(col), s)
    w = (torch.rand(7, 7, 3, K, generator=g) + 1.0).to(cuda_dev)  # nor in the filter
    wt8 = torch.full((K, 256), 7.0, dtype=BF, device=cuda_dev)
    ops.s2d_stem_weight(ptr(w), K, ptr(wt8), s)
    torch.cuda.synchronize()
    col = col.float().cpu()
    j = torch.arange(kp)
    padcol = (j >= Rr * seg) | (j % seg >= 7 * 3)
    assert int(padcol.sum()) == kp - 147 and float(col[:, padcol].abs().max()) == 0.0
    centre = ((sh.OH // 2) * sh.OW + sh.OW // 2)  # a pixel whose 7 x 7 window is inside the image
    assert int((col[centre] != 0).sum()) == 147
    wt8 = wt8.float().cpu()
    assert torch.equal((wt8 != 0).sum(1), torch.full((K,), 147))  # 256 - 147 added taps / channels: zero
    want = R.bf16_rne(w.cpu()).reshape(147, K).t().sort(1).values
    assert torch.equal(wt8.sort(1).values[:, 256 - 147:], want)


# key -> per plan variant, (family, kernel, bm, bn, z) of the forward, the backward-data and the filter
# gradient, as ops.conv_route reported them when the cases were written
FP32_ROUTES = {'10x56x56x64x64x3x1x1': [(('tiled', 'fwd_kernel', 64, 64, 3), ('tiled', 'conv3f_kernel', 128, 64, 4),
                           ('tiled', 'filter_kernel', 64, 64, 109))],
 '2x10x10x64x32x3x2x1': [(('tiled', 'fwd_kernel', 64, 64, 4), ('tiled', 'dgrad3s2f_kernel', 64, 64, 2),
                          ('tiled', 'filter_kernel', 64, 64, 2)),
                         (('tiled', 'fwd_kernel', 64, 64, 4), ('tiled', 'data_kernel', 64, 64, 1),
                          ('tiled', 'filter_kernel', 64, 64, 2))],
 '2x13x13x64x128x1x2x0': [(('tiled', 'fwd_kernel', 64, 64, 1), ('tiled', 'data_kernel', 64, 64, 1),
                           ('tiled', 'filter_kernel', 64, 128, 4))],
 '2x13x9x32x64x3x1x1_copy': [(('tiled', 'conv3f_kernel', 64, 64, 2), ('tiled', 'fwd_kernel', 64, 64, 4),
                              ('tiled', 'filter_kernel', 64, 64, 8)),
                             (('tiled', 'conv3f_kernel', 128, 64, 2), ('tiled', 'fwd_kernel', 64, 64, 4),
                              ('tiled', 'filter_kernel', 64, 64, 8)),
                             (('tiled', 'conv3f_kernel', 64, 64, 1), ('tiled', 'fwd_kernel', 64, 64, 4),
                              ('tiled', 'filter_kernel', 64, 64, 8)),
                             (('tiled', 'conv3f_kernel', 128, 64, 1), ('tiled', 'fwd_kernel', 64, 64, 4),
                              ('tiled', 'filter_kernel', 64, 64, 8)),
                             (('tiled', 'conv3f_kernel', 64, 64, 2), ('tiled', 'fwd_kernel', 64, 64, 4),
                              ('tiled', 'filter_kernel', 64, 64, 8)),
                             (('tiled', 'conv3f_kernel', 128, 64, 2), ('tiled', 'fwd_kernel', 64, 64, 4),
                              ('tiled', 'filter_kernel', 64, 64, 8)),
                             (('tiled', 'conv3f_kernel', 64, 64, 2), ('tiled', 'fwd_kernel', 64, 64, 4),
                              ('tiled', 'filter_kernel', 64, 64, 8)),
                             (('tiled', 'conv3f_kernel', 64, 64, 2), ('tiled', 'fwd_kernel', 64, 64, 4),
                              ('tiled', 'filter_kernel', 64, 64, 8)),
                             (('tiled', 'fwd_kernel', 64, 64, 2), ('tiled', 'fwd_kernel', 64, 64, 4),
                              ('tiled', 'filter_kernel', 64, 64, 8))],
 '2x14x14x64x128x3x2x1': [(('tiled', 'fwd_kernel', 64, 128, 4), ('tiled', 'dgrad3s2f_kernel', 64, 64, 8),
                           ('tiled', 'filter_kernel', 64, 128, 4))],
 '2x14x14x64x64x3x1x1': [(('tiled', 'fwd_kernel', 64, 64, 4), ('tiled', 'conv3f_kernel', 64, 64, 4),
                          ('tiled', 'filter_kernel', 64, 64, 13))],
 '2x15x15x5x72x5x1x2': [(('tiled', 'fwd_kernel/gather', 64, 128, 1), ('gather', 'conv_bwd_data_kernel', 64, 64, 19),
                         ('tiled', 'filter_gather_kernel', 64, 64, 15))],
 '2x16x16x3x64x7x2x3': [(('tiled', 'fwd_kernel/gather', 64, 64, 1), ('gather', 'conv_bwd_data_kernel', 64, 64, 25),
                         ('tiled', 'filter_gather_kernel', 64, 64, 4))],
 '2x28x28x128x256x3x2x1': [(('tiled', 'fwd_kernel', 64, 128, 9), ('tiled', 'dgrad3s2f_kernel', 64, 64, 16),
                            ('tiled', 'filter_kernel', 64, 128, 13)),
                           (('tiled', 'fwd_kernel', 64, 128, 9), ('tiled', 'data_kernel', 64, 64, 8),
                            ('tiled', 'filter_kernel', 64, 128, 13))],
 '2x40x40x3x64x7x2x3': [(('tiled', 'fwd_kernel/gather', 64, 64, 1), ('gather', 'conv_bwd_data_kernel', 64, 64, 20),
                         ('tiled', 'filter_gather_kernel', 64, 64, 32)),
                        (('tiled', 'fwd_kernel/gather', 64, 64, 1), ('gather', 'conv_bwd_data_kernel', 64, 64, 20),
                         ('tiled', 'filter_gather_kernel', 64, 64, 25)),
                        (('tiled', 'fwd_kernel/gather', 64, 64, 1), ('gather', 'conv_bwd_data_kernel', 64, 64, 20),
                         ('tiled', 'filter_gather_kernel', 64, 64, 25))],
 '2x56x56x64x64x3x1x1_copy': [(('tiled', 'conv3f_kernel', 64, 64, 4), ('tiled', 'conv3f_kernel', 64, 64, 4),
                               ('tiled', 'filter_kernel', 64, 64, 98)),
                              (('tiled', 'conv3f_kernel', 128, 64, 4), ('tiled', 'conv3f_kernel', 128, 64, 4),
                               ('tiled', 'filter_kernel', 64, 64, 98)),
                              (('tiled', 'conv3f_kernel', 64, 64, 2), ('tiled', 'conv3f_kernel', 64, 64, 2),
                               ('tiled', 'filter_kernel', 64, 64, 98)),
                              (('tiled', 'conv3f_kernel', 128, 64, 2), ('tiled', 'conv3f_kernel', 128, 64, 2),
                               ('tiled', 'filter_kernel', 64, 64, 98)),
                              (('tiled', 'conv3f_kernel', 64, 64, 4), ('tiled', 'conv3f_kernel', 64, 64, 4),
                               ('tiled', 'filter_kernel', 64, 64, 98)),
                              (('tiled', 'conv3f_kernel', 128, 64, 4), ('tiled', 'conv3f_kernel', 128, 64, 4),
                               ('tiled', 'filter_kernel', 64, 64, 98)),
                              (('tiled', 'conv3f_kernel', 64, 64, 4), ('tiled', 'conv3f_kernel', 64, 64, 4),
                               ('tiled', 'filter_kernel', 64, 64, 98)),
                              (('tiled', 'conv3f_kernel', 64, 64, 4), ('tiled', 'conv3f_kernel', 64, 64, 4),
                               ('tiled', 'filter_kernel', 64, 64, 98)),
                              (('tiled', 'fwd_kernel', 64, 64, 4), ('tiled', 'fwd_kernel', 64, 64, 4),
                               ('tiled', 'filter_kernel', 64, 64, 98))],
 '2x9x9x32x36x5x2x2': [(('tiled', 'fwd_kernel', 64, 64, 1), ('gather', 'conv_bwd_data_kernel', 64, 64, 8),
                        ('tiled', 'filter_kernel', 64, 64, 2))],
 '3x10x11x4x8x3x1x1': [(('direct', 'conv_fwd_direct_kernel', 0, 0, 1),
                        ('direct', 'conv_bwd_data_direct_kernel', 0, 0, 1), ('tiled', 'filter_kernel', 64, 64, 11))],
 '3x14x14x256x512x3x2x1': [(('tiled', 'fwd_kernel', 64, 128, 15), ('tiled', 'dgrad3s2f_kernel', 64, 64, 32),
                            ('tiled', 'filter_kernel', 64, 128, 5)),
                           (('tiled', 'fwd_kernel', 64, 128, 15), ('tiled', 'data_kernel', 64, 64, 16),
                            ('tiled', 'filter_kernel', 64, 128, 5))],
 '3x20x18x3x64x7x2x3': [(('tiled', 'fwd_kernel/gather', 64, 64, 1), ('gather', 'conv_bwd_data_kernel', 64, 64, 25),
                         ('tiled', 'filter_gather_kernel', 64, 64, 9))],
 '3x7x7x256x96x3x1x1': [(('tiled', 'fwd_kernel', 64, 128, 1), ('tiled', 'conv3f_kernel', 64, 64, 6),
                         ('tiled', 'filter_kernel', 64, 128, 5))],
 '3x7x7x512x512x3x1x1_copy': [(('tiled', 'conv3f_kernel', 64, 128, 32), ('tiled', 'conv3f_kernel', 64, 128, 32),
                               ('tiled', 'filter_kernel', 64, 128, 3)),
                              (('tiled', 'conv3f_kernel', 128, 128, 32), ('tiled', 'conv3f_kernel', 128, 128, 32),
                               ('tiled', 'filter_kernel', 64, 128, 3)),
                              (('tiled', 'conv3f_kernel', 64, 64, 16), ('tiled', 'conv3f_kernel', 64, 64, 16),
                               ('tiled', 'filter_kernel', 64, 128, 3)),
                              (('tiled', 'conv3f_kernel', 128, 64, 16), ('tiled', 'conv3f_kernel', 128, 64, 16),
                               ('tiled', 'filter_kernel', 64, 128, 3)),
                              (('tiled', 'conv3f_kernel', 64, 64, 32), ('tiled', 'conv3f_kernel', 64, 64, 32),
                               ('tiled', 'filter_kernel', 64, 128, 3)),
                              (('tiled', 'conv3f_kernel', 128, 64, 32), ('tiled', 'conv3f_kernel', 128, 64, 32),
                               ('tiled', 'filter_kernel', 64, 128, 3)),
                              (('tiled', 'conv3f_kernel', 64, 64, 32), ('tiled', 'conv3f_kernel', 64, 64, 32),
                               ('tiled', 'filter_kernel', 64, 128, 3)),
                              (('tiled', 'conv3f_kernel', 64, 64, 32), ('tiled', 'conv3f_kernel', 64, 64, 32),
                               ('tiled', 'filter_kernel', 64, 128, 3)),
                              (('tiled', 'fwd_kernel', 64, 128, 16), ('tiled', 'fwd_kernel', 64, 128, 16),
                               ('tiled', 'filter_kernel', 64, 128, 3))],
 '3x8x8x16x32x1x2x0': [(('direct', 'conv_fwd_direct_kernel', 0, 0, 1), ('tiled', 'data_kernel', 64, 64, 1),
                        ('tiled', 'filter_kernel', 64, 64, 2))],
 '4x12x12x8x16x3x2x1': [(('direct', 'conv_fwd_direct_kernel', 0, 0, 1),
                         ('direct', 'conv_bwd_data_direct_kernel', 0, 0, 1), ('tiled', 'filter_kernel', 64, 64, 5))],
 '4x14x14x256x256x3x1x1_copy': [(('tiled', 'conv3f_kernel', 64, 128, 16), ('tiled', 'conv3f_kernel', 64, 128, 16),
                                 ('tiled', 'filter_kernel', 64, 128, 13)),
                                (('tiled', 'conv3f_kernel', 128, 128, 16), ('tiled', 'conv3f_kernel', 128, 128, 16),
                                 ('tiled', 'filter_kernel', 64, 128, 13)),
                                (('tiled', 'conv3f_kernel', 64, 64, 8), ('tiled', 'conv3f_kernel', 64, 64, 8),
                                 ('tiled', 'filter_kernel', 64, 128, 13)),
                                (('tiled', 'conv3f_kernel', 128, 64, 8), ('tiled', 'conv3f_kernel', 128, 64, 8),
                                 ('tiled', 'filter_kernel', 64, 128, 13)),
                                (('tiled', 'conv3f_kernel', 64, 64, 16), ('tiled', 'conv3f_kernel', 64, 64, 16),
                                 ('tiled', 'filter_kernel', 64, 128, 13)),
                                (('tiled', 'conv3f_kernel', 128, 64, 16), ('tiled', 'conv3f_kernel', 128, 64, 16),
                                 ('tiled', 'filter_kernel', 64, 128, 13)),
                                (('tiled', 'conv3f_kernel', 64, 64, 16), ('tiled', 'conv3f_kernel', 64, 64, 16),
                                 ('tiled', 'filter_kernel', 64, 128, 13)),
                                (('tiled', 'conv3f_kernel', 64, 64, 16), ('tiled', 'conv3f_kernel', 64, 64, 16),
                                 ('tiled', 'filter_kernel', 64, 128, 13)),
                                (('tiled', 'fwd_kernel', 64, 128, 15), ('tiled', 'fwd_kernel', 64, 128, 15),
                                 ('tiled', 'filter_kernel', 64, 128, 13))],
 '4x14x14x6x16x5x1x0': [(('direct', 'conv_fwd_direct_kernel', 0, 0, 1),
                         ('direct', 'conv_bwd_data_direct_kernel', 0, 0, 1),
                         ('tiled', 'filter_gather_kernel', 64, 64, 13))],
 '4x28x28x128x128x3x1x1_copy': [(('tiled', 'conv3f_kernel', 64, 128, 8), ('tiled', 'conv3f_kernel', 64, 128, 8),
                                 ('tiled', 'filter_kernel', 64, 128, 49)),
                                (('tiled', 'conv3f_kernel', 128, 128, 8), ('tiled', 'conv3f_kernel', 128, 128, 8),
                                 ('tiled', 'filter_kernel', 64, 128, 49)),
                                (('tiled', 'conv3f_kernel', 64, 64, 4), ('tiled', 'conv3f_kernel', 64, 64, 4),
                                 ('tiled', 'filter_kernel', 64, 128, 49)),
                                (('tiled', 'conv3f_kernel', 128, 64, 4), ('tiled', 'conv3f_kernel', 128, 64, 4),
                                 ('tiled', 'filter_kernel', 64, 128, 49)),
                                (('tiled', 'conv3f_kernel', 64, 64, 8), ('tiled', 'conv3f_kernel', 64, 64, 8),
                                 ('tiled', 'filter_kernel', 64, 128, 49)),
                                (('tiled', 'conv3f_kernel', 128, 64, 8), ('tiled', 'conv3f_kernel', 128, 64, 8),
                                 ('tiled', 'filter_kernel', 64, 128, 49)),
                                (('tiled', 'conv3f_kernel', 64, 64, 8), ('tiled', 'conv3f_kernel', 64, 64, 8),
                                 ('tiled', 'filter_kernel', 64, 128, 49)),
                                (('tiled', 'conv3f_kernel', 64, 64, 8), ('tiled', 'conv3f_kernel', 64, 64, 8),
                                 ('tiled', 'filter_kernel', 64, 128, 49)),
                                (('tiled', 'fwd_kernel', 64, 128, 9), ('tiled', 'fwd_kernel', 64, 128, 9),
                                 ('tiled', 'filter_kernel', 64, 128, 49))],
 '4x28x28x64x128x1x2x0': [(('tiled', 'fwd_kernel', 64, 64, 1), ('tiled', 'data_kernel', 64, 64, 1),
                           ('tiled', 'filter_kernel', 64, 128, 32)),
                          (('tiled', 'fwd_kernel', 64, 64, 1), ('tiled', 'data_kernel', 64, 64, 1),
                           ('tiled', 'filter_kernel', 64, 128, 25)),
                          (('tiled', 'fwd_kernel', 64, 64, 1), ('tiled', 'data_kernel', 64, 64, 1),
                           ('tiled', 'filter_kernel', 64, 128, 25))],
 '4x28x28x64x128x3x2x1': [(('tiled', 'fwd_kernel', 64, 128, 4), ('tiled', 'dgrad3s2f_kernel', 64, 64, 8),
                           ('tiled', 'filter_kernel', 64, 128, 32)),
                          (('tiled', 'fwd_kernel', 64, 128, 4), ('tiled', 'dgrad3s2f_kernel', 64, 64, 8),
                           ('tiled', 'filter_kernel', 64, 128, 25)),
                          (('tiled', 'fwd_kernel', 64, 128, 4), ('tiled', 'dgrad3s2f_kernel', 64, 64, 8),
                           ('tiled', 'filter_kernel', 64, 128, 25))],
 '4x32x32x3x6x5x1x0': [(('direct', 'conv_fwd_direct_kernel', 0, 0, 1), ('gather', 'conv_bwd_data_kernel', 64, 64, 1),
                        ('gather', 'conv_bwd_filter_kernel', 64, 64, 49))],
 '4x56x56x64x128x3x2x1': [(('tiled', 'fwd_kernel', 64, 128, 4), ('tiled', 'dgrad3s2f_kernel', 64, 64, 8),
                           ('tiled', 'filter_kernel', 64, 128, 98)),
                          (('tiled', 'fwd_kernel', 64, 128, 4), ('tiled', 'data_kernel', 64, 64, 4),
                           ('tiled', 'filter_kernel', 64, 128, 98))],
 '4x9x7x5x6x3x1x1': [(('direct', 'conv_fwd_direct_kernel', 0, 0, 1), ('gather', 'conv_bwd_data_kernel', 64, 64, 1),
                      ('gather', 'conv_bwd_filter_kernel', 64, 64, 4))],
 '5x1x1x40x70x1x1x0': [(('gather', 'conv_fwd_kernel', 64, 64, 1), ('gather', 'conv_bwd_data_kernel', 64, 64, 1),
                        ('gather', 'conv_bwd_filter_kernel', 64, 64, 1))],
 '8x1x1x512x12x1x1x0': [(('tiled', 'fwd_kernel', 64, 64, 1), ('gather', 'conv_bwd_data_kernel', 64, 64, 1),
                         ('tiled', 'filter_kernel', 64, 64, 1))],
 '8x56x56x64x64x3x1x1': [(('tiled', 'fwd_kernel', 64, 64, 3), ('tiled', 'conv3f_kernel', 128, 64, 4),
                          ('tiled', 'filter_kernel', 64, 64, 112)),
                         (('tiled', 'fwd_kernel', 64, 64, 3), ('tiled', 'conv3f_kernel', 128, 64, 4),
                          ('tiled', 'filter_kernel', 64, 64, 112)),
                         (('tiled', 'fwd_kernel', 64, 64, 3), ('tiled', 'conv3f_kernel', 128, 64, 4),
                          ('tiled', 'filter_kernel', 64, 64, 112))],
 '8x56x56x64x64x3x1x1_copy': [(('tiled', 'conv3f_kernel', 64, 64, 2), ('tiled', 'conv3f_kernel', 64, 64, 2),
                               ('tiled', 'filter_kernel', 64, 64, 112)),
                              (('tiled', 'conv3f_kernel', 128, 64, 4), ('tiled', 'conv3f_kernel', 128, 64, 4),
                               ('tiled', 'filter_kernel', 64, 64, 112)),
                              (('tiled', 'conv3f_kernel', 64, 64, 2), ('tiled', 'conv3f_kernel', 64, 64, 2),
                               ('tiled', 'filter_kernel', 64, 64, 112)),
                              (('tiled', 'conv3f_kernel', 128, 64, 2), ('tiled', 'conv3f_kernel', 128, 64, 2),
                               ('tiled', 'filter_kernel', 64, 64, 112)),
                              (('tiled', 'conv3f_kernel', 64, 64, 2), ('tiled', 'conv3f_kernel', 64, 64, 2),
                               ('tiled', 'filter_kernel', 64, 64, 112)),
                              (('tiled', 'conv3f_kernel', 128, 64, 4), ('tiled', 'conv3f_kernel', 128, 64, 4),
                               ('tiled', 'filter_kernel', 64, 64, 112)),
                              (('tiled', 'conv3f_kernel', 128, 64, 4), ('tiled', 'conv3f_kernel', 128, 64, 4),
                               ('tiled', 'filter_kernel', 64, 64, 112)),
                              (('tiled', 'conv3f_kernel', 64, 64, 2), ('tiled', 'conv3f_kernel', 64, 64, 2),
                               ('tiled', 'filter_kernel', 64, 64, 112)),
                              (('tiled', 'fwd_kernel', 64, 64, 3), ('tiled', 'fwd_kernel', 64, 64, 3),
                               ('tiled', 'filter_kernel', 64, 64, 112))]}
