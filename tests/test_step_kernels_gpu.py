"""The small kernels of every training step, kernel by kernel: the flat
optimizer of csrc/kernels/sgd.hip (sgd_momentum, scale, to_bf16 / from_bf16,
hash_words) and the non-conv tail of csrc/kernels/ops_generic.hip (linear,
cross-entropy, softmax, batch gather, learning rate, ReLU backward, stem
re-layouts) against the float64 references of tests/helpers/step_ref.py,
through the raw bindings on stream_handle() with no engine in between.

Every output buffer carries 64 sentinel elements behind it that must survive
the call, and float outputs start as NaN (an unwritten element fails).  exact
mode: integer / dyadic operands, bit for bit.  rounded mode: the derived
bounds of step_ref.py, the worst err / bound printed.  The loss kernels
(__expf / logf) and the learning rate (powf) have no IEEE bound: they get 4 x
the error E of the same formula evaluated in fp32 on the host, on the same
inputs; both figures are printed (docs/ACCURACY.md holds a run's).
tests/test_step_ref_cpu.py pins the references on the CPU.

MTA_STAGE_REPORT=<path>: the printed figures are also written there as JSON."""

import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd.ops import ptr, stream_handle
from mpi_tensorflow_amd.parallel.sync import replica_hash

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("step_ref", os.path.join(_HERE, "helpers", "step_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)
F32, F64, BF, I32 = torch.float32, torch.float64, torch.bfloat16, torch.int32

GUARD = 64
CANARY = {F32: 12345.0, I32: 0x5A5A5A5A, torch.int16: 0x5A5A, torch.int64: 0x5A5A5A5A5A5A}
SGD_BIG = R.SGD_CAP_FLOATS + 1200  # a second grid-stride pass, ragged
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, v in sorted(REPORT.items()):
        print(f"[step kernels] {k}: {v}")
    path = os.environ.get("MTA_STAGE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def _C():
    from mpi_tensorflow_amd.ops import native

    return native()


def _worst(key, v):
    REPORT[key] = max(REPORT.get(key, 0.0), float(v))


# ------------------------------------------------------------- buffers ----
def out_buf(n, dev, dtype=F32, init=None):
    """n elements (init, or NaN / -7: unwritten) and GUARD sentinels."""
    t = torch.empty(n + GUARD, dtype=dtype, device=dev)
    if init is not None:
        t[:n] = init.reshape(-1).to(dev)
    else:
        t[:n] = float("nan") if dtype.is_floating_point else -7
    t[n:] = CANARY[dtype]
    return t


def intact(*bufs):
    """bufs: (tensor, n) pairs; no sentinel changed."""
    torch.cuda.synchronize()
    for i, (t, n) in enumerate(bufs):
        assert t.numel() == n + GUARD
        assert R.guard_hits(t, n, CANARY[t.dtype]) == 0, f"buffer {i}: sentinels overwritten"


def _ints(g, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g).to(F32)


def _ratio(got, ref, tol):
    """max err / bound over the elements (a zero bound wants a zero error)."""
    err = (got.detach().cpu().to(F64).reshape(ref.shape) - ref).abs()
    assert bool(torch.isfinite(err).all()), "non-finite output"
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, 1e9),
                                                                        torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


# ============================================================ optimizer ====
@pytest.mark.parametrize("n", [4, 1020, 4096, SGD_BIG])
def test_sgd_momentum_exact(cuda_dev, n):
    """Integers in +-64, momentum = l2 = gscale = 0.5, lr = 0.25: every product
    and sum is exact, so the update equals float64 bit for bit at every L2
    boundary, with lr from the device and as the constant, with and without
    the step bump."""
    O, s = _C().optim, stream_handle()
    g = torch.Generator().manual_seed(n)
    w, gr, m = (_ints(g, (n,), 64) for _ in range(3))
    gd = gr.to(cuda_dev)
    lr = torch.tensor([0.25], device=cuda_dev)
    for l2_end in R.l2_ends(n):
        w2, m2 = (t.to(F32).to(cuda_dev) for t in R.sgd_ref(w, gr, m, l2_end, 0.5, 0.5, 0.5, 0.25))
        for from_dev in (True, False):
            wb, mb = out_buf(n, cuda_dev, init=w), out_buf(n, cuda_dev, init=m)
            step = torch.zeros(1, dtype=torch.int64, device=cuda_dev)
            if from_dev:  # the pointers win over the constant; the step becomes 1
                O.sgd_momentum(ptr(wb), ptr(gd), ptr(mb), n, l2_end, 0.5, 0.5, 0.5, ptr(lr), 99.0, ptr(step), s)
            else:
                O.sgd_momentum(ptr(wb), ptr(gd), ptr(mb), n, l2_end, 0.5, 0.5, 0.5, 0, 0.25, 0, s)
            intact((wb, n), (mb, n))
            where = f"n {n} l2_end {l2_end} lr {'device' if from_dev else 'const'}"
            assert torch.equal(mb[:n], m2), f"momentum, {where}: {int((mb[:n] != m2).sum())} differ"
            assert torch.equal(wb[:n], w2), f"weights, {where}: {int((wb[:n] != w2).sum())} differ"
            assert int(step.item()) == (1 if from_dev else 0), where
    assert torch.equal(gd, gr.to(cuda_dev))


@pytest.mark.parametrize("n", [4096, SGD_BIG])
def test_sgd_momentum_rounded(cuda_dev, n):
    O, s = _C().optim, stream_handle()
    g = torch.Generator().manual_seed(n + 1)
    w, gr, m = (torch.randn(n, generator=g) for _ in range(3))
    l2_end = n // 2 // 4 * 4
    c = dict(l2=R.f32(5e-4), momentum=R.f32(0.9), gscale=R.f32(0.5), lr=R.f32(0.05))
    w2, m2 = R.sgd_ref(w, gr, m, l2_end, **c)
    tw, tm = R.sgd_tol(w, gr, m, l2_end, **c)
    wb, mb = out_buf(n, cuda_dev, init=w), out_buf(n, cuda_dev, init=m)
    lr = torch.tensor([0.05], device=cuda_dev)
    O.sgd_momentum(ptr(wb), ptr(gr.to(cuda_dev)), ptr(mb), n, l2_end, 5e-4, 0.9, 0.5, ptr(lr), 0.0, 0, s)
    intact((wb, n), (mb, n))
    rw, rm = _ratio(wb[:n], w2, tw), _ratio(mb[:n], m2, tm)
    print(f"[sgd_momentum] n {n}: w err/bound {rw:.3g}, m err/bound {rm:.3g}")
    _worst("sgd_momentum | w err/bound", rw)
    _worst("sgd_momentum | m err/bound", rm)
    assert rw <= 1.0 and rm <= 1.0


def test_sgd_and_scale_reject_ragged_lengths(cuda_dev):
    """The kernels move float4s: a length or an L2 boundary that is no
    multiple of 4 raises (as to_bf16 does) and leaves the buffers alone."""
    O, s = _C().optim, stream_handle()
    n = 4098
    g = torch.Generator().manual_seed(5)
    w, gr, m = (torch.randn(n + 2, generator=g) for _ in range(3))
    wb, mb, gd = out_buf(n + 2, cuda_dev, init=w), out_buf(n + 2, cuda_dev, init=m), gr.to(cuda_dev)
    lr = torch.tensor([0.05], device=cuda_dev)
    step = torch.zeros(1, dtype=torch.int64, device=cuda_dev)
    with pytest.raises(RuntimeError, match="sgd_momentum: n % 4 != 0"):
        O.sgd_momentum(ptr(wb), ptr(gd), ptr(mb), n, 1024, 5e-4, 0.9, 0.5, ptr(lr), 0.0, ptr(step), s)
    with pytest.raises(RuntimeError, match="sgd_momentum: l2_end % 4 != 0"):
        O.sgd_momentum(ptr(wb), ptr(gd), ptr(mb), 4096, 6, 5e-4, 0.9, 0.5, ptr(lr), 0.0, ptr(step), s)
    with pytest.raises(RuntimeError, match="scale: n % 4 != 0"):
        O.scale(ptr(wb), n, 0.5, s)
    intact((wb, n + 2), (mb, n + 2))
    assert torch.equal(wb[:n + 2].cpu(), w) and torch.equal(mb[:n + 2].cpu(), m) and int(step.item()) == 0


@pytest.mark.parametrize("n", [4, 1020, 4096, SGD_BIG])
def test_scale(cuda_dev, n):
    O, s = _C().optim, stream_handle()
    g = torch.Generator().manual_seed(n + 2)
    x = _ints(g, (n,), 1 << 20)
    xb = out_buf(n, cuda_dev, init=x)
    O.scale(ptr(xb), n, 0.125, s)
    intact((xb, n))
    assert torch.equal(xb[:n].cpu(), x * 0.125)
    x = torch.randn(n, generator=g)
    a = R.f32(1.0 / 3.0)
    xb = out_buf(n, cuda_dev, init=x)
    O.scale(ptr(xb), n, 1.0 / 3.0, s)
    intact((xb, n))
    ref = x.to(F64) * a
    r = _ratio(xb[:n], ref, R.EPS * ref.abs())
    print(f"[scale] n {n}: err/bound {r:.3g}")
    _worst("scale | err/bound", r)
    assert r <= 1.0


@pytest.mark.parametrize("n", [4, 65536, SGD_BIG])
def test_from_bf16_places_every_pattern(cuda_dev, n):
    """Every one of the 65,536 bf16 bit patterns (NaNs and infinities included)
    becomes the high half of an fp32 word."""
    O, s = _C().optim, stream_handle()
    pat = ((np.arange(n, dtype=np.uint64) * (1 if n >= 65536 else 0x3FC1)) & 0xFFFF).astype(np.uint32)
    x = torch.from_numpy(pat.astype(np.uint16).view(np.int16).copy()).to(cuda_dev)
    y = out_buf(n, cuda_dev)
    O.from_bf16(ptr(x), ptr(y), n, s)
    intact((y, n))
    want = torch.from_numpy((pat << 16).astype(np.uint32).view(np.int32).copy())
    assert torch.equal(y[:n].view(I32).cpu(), want)
    if n >= 65536:
        assert np.unique(pat).size == 65536


def _midpoints():
    """fp32 words at, just below and just above the round-to-even midpoints of
    bf16, for both parities of the kept bit, both signs, several exponents, and
    the largest finite bf16 (whose midpoint rounds to infinity)."""
    his = [0x3F80, 0x3F81, 0xBF80, 0xBF81, 0x4049, 0x404A, 0x0080, 0x0081, 0x7F7E, 0x7F7F, 0xFF7F, 0x00FF,
           0x3FFF, 0xC2FE]
    los = [0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF]
    u = np.array([(h << 16) | lo for h in his for lo in los], dtype=np.uint32)
    assert u.size % 4 == 0
    return torch.from_numpy(u.view(np.float32).copy())


def test_to_bf16_rounds_to_nearest_even(cuda_dev):
    O, s = _C().optim, stream_handle()
    g = torch.Generator().manual_seed(9)
    for x in (_midpoints(), torch.randn(4, generator=g), torch.randn(SGD_BIG, generator=g) * 100):
        n = x.numel()
        y = out_buf(n, cuda_dev, dtype=torch.int16)
        O.to_bf16(ptr(x.to(cuda_dev)), ptr(y), n, s)
        intact((y, n))
        want = x.to(BF).view(torch.int16)
        assert torch.equal(want, R.bf16_bits(x))  # torch's cast and the integer RNE agree
        bad = (y[:n].cpu() != want).nonzero().reshape(-1)
        assert bad.numel() == 0, f"n {n}: {bad.numel()} differ, first at {int(bad[0])}: " \
                                 f"{float(x[bad[0]]).hex()} -> {int(y[bad[0]]) & 0xFFFF:#06x}"
    y = out_buf(8, cuda_dev, dtype=torch.int16)
    x = torch.ones(8, device=cuda_dev)
    with pytest.raises(RuntimeError, match="to_bf16: n % 4 != 0"):
        O.to_bf16(ptr(x), ptr(y), 6, s)
    with pytest.raises(RuntimeError, match="from_bf16: n % 4 != 0"):
        O.from_bf16(ptr(y), ptr(x), 6, s)


@pytest.mark.parametrize("n", [1, 63, 64, 257, 1000003, R.HASH_CAP_WORDS + 5])
def test_hash_words_equals_the_host_hash(cuda_dev, n):
    """The device fingerprint of a buffer is replica_hash of its host copy
    (what makes the multi-rank divergence gates mean something)."""
    O, s = _C().optim, stream_handle()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    host = replica_hash(x)
    assert replica_hash(x.view(I32)) == host
    xd = x.to(cuda_dev)
    assert replica_hash(xd) == host and replica_hash(xd.view(I32)) == host

    def dev_hash(t):
        out = out_buf(1, cuda_dev, dtype=torch.int64)  # starts at -7: the launcher clears it
        O.hash_words(ptr(t), n, ptr(out), s)
        intact((out, 1))
        return int(out[0].item()) & (2 ** 64 - 1)
    assert dev_hash(xd) == host and dev_hash(xd) == host  # a second call repeats it
    flip = xd.clone()
    flip.view(I32)[n - 1] ^= -(2 ** 31)  # the sign bit of the last word
    assert dev_hash(flip) == replica_hash(flip.cpu()) != host
    if n > 1:
        i, j = 0, n - 1
        assert float(x[i]) != float(x[j])
        sw = xd.clone()
        sw[i], sw[j] = xd[j], xd[i]
        assert dev_hash(sw) == replica_hash(sw.cpu()) != host


# ====================================================== fully connected ====
LIN_SHAPES = [(1, 1, 1), (5, 3, 1), (7, 400, 64), (6, 130, 65), (130, 33, 10), (64, 512, 120)]
LIN_OPTS = [(True, True, True), (False, False, False)]  # bias, dx requested, db requested


def _lin_operands(M, K, N, exact):
    g = torch.Generator().manual_seed(M * 1000 + K + N)
    if not exact:
        return (torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) * K ** -0.5,
                torch.randn(N, generator=g) * 0.1, torch.randn(M, N, generator=g))
    x, w, b, dy = _ints(g, (M, K), 7), _ints(g, (K, N), 7), _ints(g, (N,), 8), _ints(g, (M, N), 7)
    if N > 1:  # outputs that are exactly 0: column 0
        w[:, 0], b[0] = 0, 0
    elif M > 1:  # ... row 0
        x[0], b[0] = 0, 0
    assert max(K, M, N) * 49 + 8 < 2 ** 24
    return x, w, b, dy


@pytest.mark.parametrize("exact", [False, True], ids=["rounded", "exact"])
@pytest.mark.parametrize("bias,want_dx,want_db", LIN_OPTS, ids=["all", "bare"])
@pytest.mark.parametrize("relu", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("M,K,N", LIN_SHAPES)
def test_linear(cuda_dev, M, K, N, relu, bias, want_dx, want_db, exact):
    ops, s = _C().ops, stream_handle()
    dt = F32 if exact else F64
    x, w, b, dy = _lin_operands(M, K, N, exact)
    if not bias:
        b = None
    xd, wd, dyd = x.to(cuda_dev), w.to(cuda_dev), dy.to(cuda_dev)
    bd = b.to(cuda_dev) if bias else None
    y_ref, S, n = R.linear_ref(x, w, b, relu, dt=dt)
    yb = out_buf(M * N, cuda_dev)
    ops.linear_fwd(ptr(xd), ptr(wd), ptr(bd), ptr(yb), M, K, N, relu, s)
    intact((yb, M * N))
    # the backward reads the y it is handed: the reference's, so both mask alike
    y_in = y_ref.to(F32)
    dw, db, dx = out_buf(K * N, cuda_dev), out_buf(N, cuda_dev), out_buf(M * K, cuda_dev)
    ops.linear_bwd(ptr(xd), ptr(wd), ptr(y_in.to(cuda_dev)), ptr(dyd), ptr(dw), ptr(db) if want_db else 0,
                   ptr(dx) if want_dx else 0, M, K, N, relu, s)
    intact((dw, K * N), (db, N), (dx, M * K))
    ref = R.linear_bwd_ref(x, w, y_in, dy, relu, dt=dt)
    got = {"y": (yb[:M * N], (y_ref, S, n)), "dw": (dw[:K * N], ref["dw"])}
    if want_db:
        got["db"] = (db[:N], ref["db"])
    else:
        assert bool(torch.isnan(db[:N]).all()), "db written through a null pointer's stand-in"
    if want_dx:
        got["dx"] = (dx[:M * K], ref["dx"])
    else:
        assert bool(torch.isnan(dx[:M * K]).all())
    where = f"M {M} K {K} N {N} relu {relu} bias {bias}"
    if exact:
        if relu and M * N > 1:  # the mask at y == 0: no gradient (the kernel tests y <= 0)
            assert bool((y_in == 0).any()) and bool((dy[y_in == 0] != 0).any())
        for k, (t, (r, _, _)) in got.items():
            r = r.to(F32)
            bad = (t.cpu().reshape(r.shape) != r).nonzero()
            assert bad.numel() == 0, f"{k}, {where}: {bad.shape[0]} differ, first at {bad[0].tolist()}"
        return
    fig = {}
    for k, (t, (r, S_, n_)) in got.items():
        fig[k] = _ratio(t, r, R.lin_tol(S_, n_))
        _worst(f"linear | {k} err/bound", fig[k])
    print(f"[linear] {where}: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))
    assert all(v <= 1.0 for v in fig.values()), fig


# ================================================================= loss ====
XENT_SHAPES = [(1, 1), (3, 10), (4, 64), (5, 65), (257, 1000)]


def _run_xent(ops, dev, z, lab, B, C, with_correct=True, zp=None, lp=None):
    """One call of xent and one of xent_mean on rows [B, C] -> outputs on the host."""
    s = stream_handle()
    zd, ld = (z.to(dev), lab.to(dev)) if zp is None else (None, None)
    zp, lp = (ptr(zd), ptr(ld)) if zp is None else (zp, lp)
    o = {}
    for name in ("xent", "mean"):
        loss, dl, mean = out_buf(B, dev), out_buf(B * C, dev), out_buf(1, dev)
        cor = out_buf(1, dev, dtype=I32, init=torch.zeros(1, dtype=I32))
        cp = ptr(cor) if with_correct else 0
        for _ in range(2):  # the counter accumulates over two calls
            if name == "xent":
                ops.xent(zp, lp, B, C, ptr(loss), ptr(dl), cp, s)
            else:
                ops.xent_mean(zp, lp, B, C, ptr(loss), ptr(dl), ptr(mean), cp, s)
        intact((loss, B), (dl, B * C), (cor, 1), (mean, 1))
        o[name] = dict(loss=loss[:B].cpu(), dl=dl[:B * C].cpu().reshape(B, C), mean=mean[:1].cpu(),
                       hits2=int(cor[0].item()))
    return o


@pytest.mark.parametrize("shifted", [False, True], ids=["randn3", "shifted"])
@pytest.mark.parametrize("B,C", XENT_SHAPES)
def test_xent_and_softmax(cuda_dev, B, C, shifted):
    ops, s = _C().ops, stream_handle()
    z, lab = R.xent_inputs(B, C, seed=B * 7 + C, shifted=shifted)
    loss, dl, p, hits = R.xent_ref(z, lab)
    l32, d32, p32, _ = R.xent_ref(z, lab, dt=F32)
    E = dict(loss=float((l32.to(F64) - loss).abs().max()), dl=float((d32.to(F64) - dl).abs().max()),
             p=float((p32.to(F64) - p).abs().max()), mean=abs(float(l32.mean()) - float(loss.mean())))
    o = _run_xent(ops, cuda_dev, z, lab, B, C)
    sm = out_buf(B * C, cuda_dev)
    ops.softmax_rows(ptr(z.to(cuda_dev)), ptr(sm), B, C, s)
    intact((sm, B * C))
    err = {}
    for name in ("xent", "mean"):
        for t in (o[name]["loss"], o[name]["dl"]):
            assert bool(torch.isfinite(t).all()), f"{name}: non-finite output"
        err[f"{name} loss"] = (float((o[name]["loss"].to(F64) - loss).abs().max()), E["loss"])
        err[f"{name} dlogits"] = (float((o[name]["dl"].to(F64) - dl).abs().max()), E["dl"])
        assert o[name]["hits2"] == 2 * hits, f"{name}: hit counter {o[name]['hits2']} for 2 x {hits}"
    assert np.isfinite(float(o["mean"]["mean"]))
    err["mean"] = (abs(float(o["mean"]["mean"]) - float(loss.mean())), E["mean"])
    smc = sm[:B * C].cpu().reshape(B, C)
    assert bool(torch.isfinite(smc).all())
    err["softmax"] = (float((smc.to(F64) - p).abs().max()), E["p"])
    tag = f"B {B} C {C} {'shifted' if shifted else 'randn3'}"
    print(f"[xent] {tag}: " + ", ".join(f"{k} {a:.3g} (E {e:.3g})" for k, (a, e) in err.items()))
    for k, (a, e) in err.items():
        REPORT[f"loss | {tag} | {k}"] = f"kernel {a:.3g}, host fp32 {e:.3g}"
    # the same rows without a counter: identical outputs
    o0 = _run_xent(ops, cuda_dev, z, lab, B, C, with_correct=False)
    for name in ("xent", "mean"):
        assert torch.equal(o0[name]["loss"], o[name]["loss"]) and torch.equal(o0[name]["dl"], o[name]["dl"])
    # xent and xent_mean evaluate the same per-row expressions
    assert torch.equal(o["xent"]["loss"], o["mean"]["loss"]), "xent / xent_mean loss rows differ"
    assert torch.equal(o["xent"]["dl"], o["mean"]["dl"]), "xent / xent_mean dlogits differ"
    over = {k: (a, e) for k, (a, e) in err.items() if a > 4 * e}
    assert not over, f"{tag}: over 4 E: {over}"


@pytest.mark.parametrize("C", [4, 10, 64, 65, 1000])
def test_xent_hit_counter_takes_the_lowest_maximum(cuda_dev, C):
    ops = _C().ops
    z, lab, hit_rows = R.tie_rows(C)
    B = z.shape[0]
    o = _run_xent(ops, cuda_dev, z, lab, B, C)
    assert o["xent"]["hits2"] == 2 * sum(hit_rows) and o["mean"]["hits2"] == 2 * sum(hit_rows)
    zd, ld = z.to(cuda_dev), lab.to(cuda_dev)
    for r in range(B):  # and row by row
        o = _run_xent(ops, cuda_dev, None, None, 1, C, zp=ptr(zd) + 4 * r * C, lp=ptr(ld) + 4 * r)
        assert o["xent"]["hits2"] == 2 * hit_rows[r], f"xent row {r}: label {int(lab[r])}"
        assert o["mean"]["hits2"] == 2 * hit_rows[r], f"xent_mean row {r}: label {int(lab[r])}"


# ============================================================== staging ====
GATHER = [(100, 1), (100, 7), (100, 64), (101, 64), (301, 256)]  # n_local, batch (n_local > batch)
LR_BASE, LR_DECAY = 0.01, 0.95
# (step, n_local, batch): both sides of epoch boundaries e -> e + 1 = (step batch) // n_local
LR_CASES = [(0, 100, 7), (14, 100, 7), (15, 100, 7), (28, 100, 7), (29, 100, 7), (242, 100, 7), (243, 100, 7),
            (9, 1000, 100), (10, 1000, 100), (937, 60000, 64), (938, 60000, 64), (15937, 60000, 64),
            (15938, 60000, 64), (152812, 60000, 64), (152813, 60000, 64)]
_POW = {}


def pow_yardstick():
    """E of the learning rate: the largest relative error of numpy float32
    power against float64 over every argument this file hands the kernels."""
    if not _POW:
        args = list(LR_CASES) + [(st, nl, b) for nl, b in GATHER for st in R.gather_steps(nl, b)]
        worst = 0.0
        for a in args:
            ref = R.lr_ref(*a, LR_BASE, LR_DECAY)
            if ref > 0:
                worst = max(worst, abs(R.lr_f32(*a, LR_BASE, LR_DECAY) - ref) / ref)
        _POW["E"] = worst
        REPORT["lr | host fp32 power rel. error E"] = f"{worst:.3g}"
    return _POW["E"]


def check_lr(got, args):
    ref, E = R.lr_ref(*args, LR_BASE, LR_DECAY), pow_yardstick()
    rel = abs(got - ref) / ref if ref > 0 else (0.0 if got == 0.0 else float("inf"))
    print(f"[lr] step {args[0]} n_local {args[1]} batch {args[2]}: rel. error {rel:.3g} (E {E:.3g})")
    REPORT["lr | kernel rel. error"] = f"{max(float(REPORT.get('lr | kernel rel. error', 0)), rel):.3g}"
    assert rel <= 4 * E, f"lr {got!r} for {ref!r} at {args}"


def test_lr_yardstick_sees_epoch_boundaries():
    pairs = [(a, b) for a, b in zip(LR_CASES, LR_CASES[1:]) if a[1:] == b[1:] and b[0] == a[0] + 1]
    rising = [(a[0] * a[2]) // a[1] + 1 == (b[0] * b[2]) // b[1] for a, b in pairs]
    assert len(pairs) == 7 and all(rising)


@pytest.mark.parametrize("row_elems", [4, 784, 3072])
@pytest.mark.parametrize("n_local,batch", GATHER)
def test_gather_batch(cuda_dev, n_local, batch, row_elems):
    ops, s = _C().ops, stream_handle()
    data = torch.arange(n_local * row_elems, dtype=F32).reshape(n_local, row_elems)  # distinct, exact
    labels = (torch.arange(n_local) * 3 + 1).to(I32)
    # `batch` rows of 1e30 / -1 behind the shard: an offset past n_local - batch shows them
    dd = torch.cat([data, torch.full((batch, row_elems), 1e30)]).to(cuda_dev)
    ld = torch.cat([labels, torch.full((batch,), -1, dtype=I32)]).to(cuda_dev)
    for step in R.gather_steps(n_local, batch):
        off = R.batch_offset(step, n_local, batch)
        sd = torch.tensor([step], dtype=torch.int64, device=cuda_dev)
        xb, yb, lr = out_buf(batch * row_elems, cuda_dev), out_buf(batch, cuda_dev, dtype=I32), out_buf(1, cuda_dev)
        ops.gather_batch(ptr(dd), ptr(ld), ptr(sd), n_local, batch, row_elems, ptr(xb), ptr(yb), s, LR_BASE,
                         LR_DECAY, ptr(lr))
        intact((xb, batch * row_elems), (yb, batch), (lr, 1))
        where = f"step {step} offset {off}"
        assert torch.equal(xb[:batch * row_elems].cpu().reshape(batch, row_elems), data[off:off + batch]), where
        assert torch.equal(yb[:batch].cpu(), labels[off:off + batch]), where
        check_lr(float(lr[0].item()), (step, n_local, batch))
        # the separate launch gives the same bits
        lr2 = out_buf(1, cuda_dev)
        ops.lr_from_step(ptr(sd), n_local, batch, LR_BASE, LR_DECAY, ptr(lr2), s)
        intact((lr2, 1))
        assert torch.equal(lr2[:1].view(I32), lr[:1].view(I32)), where
        # without a learning rate, and without a step pointer (step 0)
        xb2, yb2 = out_buf(batch * row_elems, cuda_dev), out_buf(batch, cuda_dev, dtype=I32)
        ops.gather_batch(ptr(dd), ptr(ld), 0, n_local, batch, row_elems, ptr(xb2), ptr(yb2), s)
        intact((xb2, batch * row_elems), (yb2, batch))
        assert torch.equal(xb2[:batch * row_elems].cpu().reshape(batch, row_elems), data[:batch])
        assert torch.equal(yb2[:batch].cpu(), labels[:batch])


def test_gather_rejects_unsupported_shapes(cuda_dev):
    """row_elems % 4, batch > 256, and a batch the shard does not exceed (the
    offset's modulus n_local - batch is then zero or negative)."""
    ops, s = _C().ops, stream_handle()
    data = torch.zeros(600 * 8, device=cuda_dev)
    labels = torch.zeros(600, dtype=I32, device=cuda_dev)
    lam = torch.zeros(600, device=cuda_dev)
    xb, yb, lb = out_buf(600 * 8, cuda_dev), out_buf(600, cuda_dev, dtype=I32), out_buf(600, cuda_dev)
    for n_local, batch, row in ((100, 7, 6), (600, 257, 8), (100, 100, 8), (100, 256, 8), (100, 0, 8)):
        with pytest.raises(RuntimeError, match="gather_batch: unsupported shape"):
            ops.gather_batch(ptr(data), ptr(labels), 0, n_local, batch, row, ptr(xb), ptr(yb), s)
    for n_local, batch in ((600, 257), (100, 100), (100, 256)):
        with pytest.raises(RuntimeError, match="gather_soft: unsupported shape"):
            ops.gather_soft(ptr(labels), ptr(lam), 0, n_local, batch, ptr(yb), ptr(lb), s)
    intact((xb, 600 * 8), (yb, 600), (lb, 600))
    assert bool(torch.isnan(xb[:600 * 8]).all()) and bool((yb[:600] == -7).all()) and bool(torch.isnan(lb[:600]).all())


@pytest.mark.parametrize("n_local,batch", GATHER)
def test_gather_soft(cuda_dev, n_local, batch):
    ops, s = _C().ops, stream_handle()
    labels2 = (torch.arange(n_local) * 5 + 2).to(I32)
    lam = torch.rand(n_local, generator=torch.Generator().manual_seed(n_local + batch))
    l2d = torch.cat([labels2, torch.full((batch,), -1, dtype=I32)]).to(cuda_dev)  # (as in test_gather_batch)
    lamd = torch.cat([lam, torch.full((batch,), 1e30)]).to(cuda_dev)
    for step in R.gather_steps(n_local, batch):
        off = R.batch_offset(step, n_local, batch)
        sd = torch.tensor([step], dtype=torch.int64, device=cuda_dev)
        y2b, lamb = out_buf(batch, cuda_dev, dtype=I32), out_buf(batch, cuda_dev)
        ops.gather_soft(ptr(l2d), ptr(lamd), ptr(sd), n_local, batch, ptr(y2b), ptr(lamb), s)
        intact((y2b, batch), (lamb, batch))
        assert torch.equal(y2b[:batch].cpu(), labels2[off:off + batch]), f"step {step}"
        assert torch.equal(lamb[:batch].cpu(), lam[off:off + batch]), f"step {step}"


def test_lr_from_step(cuda_dev):
    ops, s = _C().ops, stream_handle()
    for step, n_local, batch in LR_CASES + [(2 ** 33, 100, 256)]:
        sd = torch.tensor([step], dtype=torch.int64, device=cuda_dev)
        lr = out_buf(1, cuda_dev)
        ops.lr_from_step(ptr(sd), n_local, batch, LR_BASE, LR_DECAY, ptr(lr), s)
        intact((lr, 1))
        check_lr(float(lr[0].item()), (step, n_local, batch))


def _relu_patterns():
    u = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x3F800000, 0xBF800000, 0x7FC00000, 0xFFC00000,
                  0x7F800000, 0xFF800000, 0x00800000, 0x34000000, 0xC0490FDB], dtype=np.uint32)
    return torch.from_numpy(u.view(np.float32).copy())  # +-0, +-denormal, +-1, +-NaN, +-inf, small, -pi


@pytest.mark.parametrize("n", [1, 255, 257, R.GRID1D_CAP + 3])
def test_relu_bwd(cuda_dev, n):
    """dx = dy only where y > 0 (the smallest denormal included), else +0 with
    the sign bit clear (y = +-0, negatives, NaN)."""
    ops, s = _C().ops, stream_handle()
    pat = _relu_patterns().to(cuda_dev)
    idx = torch.arange(n, device=cuda_dev)
    dy = -((idx % 1021).to(F32) + 1.5)  # negative: a passed-through sign bit shows
    for shift in (range(pat.numel()) if n == 1 else (0,)):  # n = 1: every pattern in turn
        # moved on by one every 91 elements, so that the tail meets other patterns than the head
        y = pat[(idx + shift + idx // 91) % pat.numel()]
        dx = out_buf(n, cuda_dev)
        ops.relu_bwd(ptr(dy), ptr(y), ptr(dx), n, s)
        intact((dx, n))
        want = torch.where(y > 0, dy, torch.zeros_like(dy))  # (the device's comparison: checked on the host below)
        assert torch.equal(dx[:n].view(I32), want.view(I32))
        m = min(n, 4096)
        yh, dyh = y[-m:].cpu(), dy[-m:].cpu()
        wh = torch.where(yh > 0, dyh, torch.zeros(m))
        assert torch.equal(dx[n - m:n].cpu().view(I32), wh.view(I32)), f"shift {shift}"
        if n >= 255:
            got = dx[:n]
            assert int((got.view(I32) == 0).sum()) > 0 and int((got < 0).sum()) > 0


# ====================================================== stem re-layouts ====
STEM = [(7, 7, 3), (3, 3, 7)]  # R, S, C: (sc, seg, kp) = (21, 24, 192) and (21, 24, 128)


@pytest.mark.parametrize("K", [64, 8])
@pytest.mark.parametrize("R_,S,C", STEM)
def test_stem_weight_bf16(cuda_dev, R_, S, C, K):
    ops, s = _C().ops, stream_handle()
    sc, seg, kp = R.im2col_layout(R_, S, C)
    assert (sc, seg, kp) == ((21, 24, 192) if R_ == 7 else (21, 24, 128))
    w = torch.randn(R_, S, C, K, generator=torch.Generator().manual_seed(K + R_))
    out = out_buf(K * kp, cuda_dev, dtype=torch.int16)
    ops.stem_weight_bf16(ptr(w.to(cuda_dev)), R_, sc, seg, kp, K, ptr(out), s)
    intact((out, K * kp))
    want = R.stem_wt_ref(w, R_, sc, seg, kp, K).to(BF).view(torch.int16)
    got = out[:K * kp].cpu().reshape(K, kp)
    assert torch.equal(got, want)
    pad = R.stem_pad_mask(R_, sc, seg, kp)
    assert int(pad.sum()) == kp - R_ * sc and bool((got[:, pad] == 0).all())  # +0, sign bit clear


@pytest.mark.parametrize("K", [64, 8])
@pytest.mark.parametrize("R_,S,C", STEM)
def test_stem_wgrad(cuda_dev, R_, S, C, K):
    ops, s = _C().ops, stream_handle()
    sc, seg, kp = R.im2col_layout(R_, S, C)
    gpad = torch.arange(1, kp * K + 1, dtype=F32).reshape(kp, K)
    gpad[R.stem_pad_mask(R_, sc, seg, kp)] = 1e30
    gw = out_buf(R_ * sc * K, cuda_dev)
    ops.stem_wgrad(ptr(gpad.to(cuda_dev)), R_, sc, seg, K, ptr(gw), s)
    intact((gw, R_ * sc * K))
    got = gw[:R_ * sc * K].cpu().reshape(R_, sc, K)
    assert not bool((got == 1e30).any()), "a padded position of gpad reached gw"
    assert torch.equal(got, R.stem_wgrad_ref(gpad, R_, sc, seg, K))


@pytest.mark.parametrize("K", [64, 8])
def test_s2d_stem_wgrad(cuda_dev, K):
    ops, s = _C().ops, stream_handle()
    real = R.s2d_real_mask()
    dw8 = torch.arange(1, 256 * K + 1, dtype=F32).reshape(256, K)
    dw8[~real] = 1e30
    gw = out_buf(147 * K, cuda_dev)
    ops.s2d_stem_wgrad(ptr(dw8.to(cuda_dev)), K, ptr(gw), s)
    intact((gw, 147 * K))
    got = gw[:147 * K].cpu().reshape(7, 7, 3, K)
    assert not bool((got == 1e30).any()), "an off-kernel or padding-channel k reached gw"
    assert torch.equal(got, R.s2d_wgrad_ref(dw8, K))
    # round trip: s2d_stem_weight (bf16-exact integers) -> transpose -> s2d_stem_wgrad
    w = torch.randint(-127, 128, (7, 7, 3, K), generator=torch.Generator().manual_seed(K)).to(F32)
    wt8 = out_buf(K * 256, cuda_dev, dtype=torch.int16)
    ops.s2d_stem_weight(ptr(w.to(cuda_dev)), K, ptr(wt8), s)
    intact((wt8, K * 256))
    wt = wt8[:K * 256].view(BF).to(F32).reshape(K, 256)
    assert torch.equal(wt.cpu(), R.s2d_weight_ref(w, K))
    back = out_buf(147 * K, cuda_dev)
    ops.s2d_stem_wgrad(ptr(wt.t().contiguous()), K, ptr(back), s)
    intact((back, 147 * K))
    assert torch.equal(back[:147 * K].cpu().reshape(7, 7, 3, K), w)
