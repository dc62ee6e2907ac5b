"""The ResNet-18 bf16x3 inference forward (docs/ACCURACY.md): x3conv per loader and tile against
float64 and exactly, the small kernels against torch, Predictor against float64 and the bf16 one.
End to end on 3 rows, max |logits - fp64|: the figures are in docs/ACCURACY.md."""

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from helpers import lowp_conv as L

from mpi_tensorflow_amd.ops import functional as Fn
from mpi_tensorflow_amd.ops import native, ptr, stream_handle

pytestmark = pytest.mark.gpu

R, H_ = L.R, L.load("resnet_state")
F64, BF = L.F64, L.BF
# (N, H, W, C, K, R, stride, pad) -> (loader, bm) of ops.x3conv_route; the M rule is bm = 128
# from M = 8192 (the 128-row gather and stem tiles are the two cases with M = 8624 and 9408)
CASES = [((4, 14, 14, 64, 64, 3, 1, 1), ("halo", 64)), ((3, 56, 56, 64, 64, 3, 1, 1), ("halo", 128)),
         ((3, 11, 13, 64, 192, 3, 1, 1), ("halo", 64)), ((3, 7, 7, 512, 512, 3, 1, 1), ("halo", 64)),
         ((2, 14, 14, 64, 128, 3, 2, 1), ("gather", 64)), ((4, 14, 14, 128, 64, 1, 2, 0), ("gather", 64)),
         ((11, 56, 56, 64, 128, 1, 2, 0), ("gather", 128)), ((2, 37, 41, 3, 64, 7, 2, 3), ("stem", 64)),
         ((3, 112, 112, 3, 64, 7, 2, 3), ("stem", 128))]
IDS = [f"{r[0]}{r[1]}-{'x'.join(map(str, s))}" for s, r in CASES]
CANARY = -768.0


def split(v):
    hi = v.to(BF)
    return hi, (v - hi.float()).to(BF)


def planes(v, dev, tail=0):  # a split tensor as the kernels take it, `tail` canaries behind it
    return torch.cat([t.flatten() for t in split(v.float())] + [torch.full((tail,), CANARY, dtype=BF)]).to(dev)


def join(buf, n, shape):  # the fp64 values of the split tensor at the start of a host buffer
    return (buf[:n].to(F64) + buf[n:2 * n].to(F64)).reshape(shape)


def run_x3conv(dev, shape, route, x, w, a, b, res, relu):
    """x, w: fp32 NHWC / HWIO on the host -> the joined fp64 output and its buffer."""
    ops, s, (N, H, W, C, K, Rr, stride, pad) = native().ops, stream_handle(), shape
    sh = ops.ConvShape(N, H, W, C, K, Rr, Rr, stride, pad)
    run, M, wd = Fn._s2d_shape(sh) if C == 3 else sh, N * sh.OH * sh.OW, w.to(dev)
    r = ops.x3conv_route(run)
    assert (r["loader"], r["bm"], r["bn"], r["z"]) == route + (64, 1)
    wp = torch.empty(2 * (K * 256 if C == 3 else w.numel()), dtype=BF, device=dev)
    if C == 3:
        xp, xd = torch.empty(2 * N * run.H * run.W * 16, dtype=BF, device=dev), x.to(dev)
        ops.s2d_stem_input_x3(ptr(xd), N, H, W, sh.OH, sh.OW, ptr(xp), s)
        ops.s2d_stem_weight_x3(ptr(wd), K, ptr(wp), s)
    else:
        xp = planes(x, dev)
        jobs = torch.tensor([[ptr(wd), ptr(wp), Rr * Rr, C, K, 0, 0, 0]], dtype=torch.int64).to(dev)
        ops.wsplit_x3(ptr(jobs), 1, K // 32, s)
    y = torch.full((2 * M * K + 4096,), CANARY, dtype=BF, device=dev)
    t = [a.to(dev), b.to(dev), planes(res, dev) if res is not None else None]
    ops.x3conv(run, ptr(xp), ptr(wp), ptr(t[0]), ptr(t[1]), ptr(t[2]), relu, ptr(y), s)
    got = L.checked(y, 2 * M * K, CANARY)
    return join(got, M * K, (N, sh.OH, sh.OW, K)), got


@functools.lru_cache(maxsize=None)
def operands(i):
    """Unrounded fp32 operands (the lo planes carry weight), a, b, a residual, the fp64 conv."""
    N, H, W, C, K, Rr, stride, pad = CASES[i][0]
    g, n = torch.Generator().manual_seed(600 + i), Rr * Rr * C
    x = 3 * torch.randn(N, H, W, C, generator=g).clamp_min(0)
    w = torch.randn(Rr, Rr, C, K, generator=g) * (2 / n) ** 0.5
    g = torch.Generator().manual_seed(7)
    a = (torch.rand(K, generator=g) * 1.5 + 0.5) * (torch.randint(0, 2, (K,), generator=g) * 2 - 1)
    b = torch.rand(K, generator=g) * 2 - 1
    ref = R.conv_fwd(x, w, stride, pad)
    return x, w, a, b, torch.randn(ref[0].shape, generator=g), ref


@pytest.mark.parametrize("res,relu", [(True, True), (False, False)])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_x3conv_against_float64(cuda_dev, i, res, relu):
    """|join(y) - v64| <= 2^-15 |v64| + |a| (2^-14 + n 2^-23) S: each operand is within 2^-16 of
    its pair and the dropped xl wl is under 2^-16 |x w|, fp32 accumulation, a pair within 2^-16."""
    shape, route = CASES[i]
    x, w, a, b, rs, (ref, S, n) = operands(i)
    rs = rs if res and shape[3] != 3 else None
    rj = sum(t.to(F64) for t in split(rs)) if rs is not None else 0.0
    v = ref * a.to(F64) + b.to(F64) + rj
    v = v.clamp_min(0) if relu else v
    got, _ = run_x3conv(cuda_dev, shape, route, x, w, a, b, rs, relu)
    bound = 2.0 ** -15 * v.abs() + a.abs().to(F64) * (2.0 ** -14 + n * 2.0 ** -23) * S
    err = (got - v).abs()
    print(f"[x3conv] {route} {shape} res={res}: worst err / bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("wide", ["x", "w"])
@pytest.mark.parametrize("i", [0, 4], ids=[IDS[0], IDS[4]])
def test_x3conv_exact(cuda_dev, i, wide):
    """Integers: one side to 4095 (its lo plane works), the other to 2 (lo == 0); a = 1, integer b
    and residual, ReLU: the stored pair is split(the exact integer)."""
    shape, route = CASES[i]
    N, H, W, C, K, Rr, stride, pad = shape
    g, n = torch.Generator().manual_seed(40 + i), Rr * Rr * C
    lx, lw = (4095, 2) if wide == "x" else (2, 4095)
    x = torch.randint(-lx if wide == "x" else 0, lx + 1, (N, H, W, C), generator=g).float()
    w = torch.randint(-lw, lw + 1, (Rr, Rr, C, K), generator=g).float()
    assert n * float(x.abs().max()) * float(w.abs().max()) < 2 ** 24
    assert bool((split(x if wide == "x" else w)[1] != 0).any())
    ref = R.conv_fwd(x, w, stride, pad)[0]
    b = torch.randint(-9, 10, (K,), generator=g).float()
    rs = torch.randint(-4095, 4096, ref.shape, generator=g).float()
    v = (ref + b.to(F64) + rs.to(F64)).clamp_min(0)
    got, _ = run_x3conv(cuda_dev, shape, route, x, w, torch.ones(K), b, rs, True)
    assert torch.equal(got, sum(t.to(F64) for t in split(v.float())))


@pytest.mark.parametrize("n", [1, 7, 4097, 4104])  # 4104: the 16-byte stores of the lo plane
def test_x3_split_bits_with_poisoned_tails(cuda_dev, n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n + 64, generator=g) * torch.exp2(torch.randint(-20, 20, (n + 64,), generator=g).float())
    x[n:] = 1e30  # past the end: neither read nor split
    out = torch.full((2 * n + 64,), CANARY, dtype=BF, device=cuda_dev)
    xd = x.to(cuda_dev)
    native().ops.x3_split(ptr(xd), n, ptr(out), stream_handle())
    torch.cuda.synchronize()
    want = torch.cat(list(split(x[:n])) + [torch.full((64,), CANARY, dtype=BF)])
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


def test_maxpool_infer_x3(cuda_dev):
    ops, g = native().ops, torch.Generator().manual_seed(23)
    x = torch.randn(2, 9, 11, 64, generator=g) * 3
    p = ops.PoolShape(2, 9, 11, 64, 3, 2, 1)
    n, xd = 2 * p.OH * p.OW * 64, planes(x, cuda_dev)
    y = torch.full((2 * n + 256,), CANARY, dtype=BF, device=cuda_dev)
    ops.maxpool_infer_x3(p, ptr(xd), ptr(y), stream_handle())
    torch.cuda.synchronize()
    got, xin = y.cpu(), join(xd.cpu(), x.numel(), x.shape)
    assert R.guard_hits(got.float(), 2 * n, CANARY) == 0
    pool = lambda t: F.max_pool2d(t.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(join(got, n, (2, p.OH, p.OW, 64)), pool(xin))
    # a pair as one number, hi bits * 2^16 + lo bits: the output's is one of its window's
    key = lambda buf, m, shape: (buf[:m].view(torch.int16).to(F64) * 65536
                                 + (buf[m:2 * m].view(torch.int16).to(F64) + 32768)).reshape(shape)
    kin = F.pad(key(xd.cpu(), x.numel(), x.shape), (0, 0, 1, 1, 1, 1), value=-1e18)
    kout = key(got, n, (2, p.OH, p.OW, 64))
    hit = torch.zeros_like(kout, dtype=torch.bool)
    for kh in range(3):
        for kw in range(3):
            hit |= kin[:, kh:kh + 2 * p.OH - 1:2, kw:kw + 2 * p.OW - 1:2] == kout
    assert bool(hit.all())


@pytest.mark.parametrize("m", [1, 3])
def test_avgpool_fc_x3_against_float64(cuda_dev, m):
    g = torch.Generator().manual_seed(m)
    x = torch.randn(m, 49, 512, generator=g)
    w, b = torch.randn(512, 10, generator=g) * (2 / 512) ** 0.5, torch.randn(10, generator=g)
    xd, wd, bd = planes(x, cuda_dev), w.to(cuda_dev), b.to(cuda_dev)
    out = torch.zeros(m, 10, device=cuda_dev)
    native().ops.avgpool_fc_x3(ptr(xd), ptr(wd), ptr(bd), ptr(out), m, 49, 512, 10, stream_handle())
    ref = join(xd.cpu(), x.numel(), x.shape).mean(1) @ w.to(F64) + b.to(F64)
    assert float((out.cpu().to(F64) - ref).abs().max()) <= 1e-5


@pytest.fixture(scope="module")
def net(cuda_dev):
    """The shared state, 3 rows, their fp64 logits, and a Predictor of it per dtype."""
    from mpi_tensorflow_amd.runtime.predict import Predictor

    model, params, bn = H_.resnet_state()
    x = torch.randn(4, 224, 224, 3, generator=torch.Generator().manual_seed(5))[:3]
    pv = model.layout.views(params.double())
    P = {s.name: Fn.Param(pv[s.name], None) for s in model.layout.specs}
    with torch.no_grad(), Fn.oracle_mode():
        ref = model.forward(P, {k: (a.double(), b.double()) for k, (a, b) in bn.items()}, x.double(), False)
    pd, bd = params.to(cuda_dev), {k: (a.to(cuda_dev), b.to(cuda_dev)) for k, (a, b) in bn.items()}
    make = lambda dtype, backend="auto": Predictor("resnet18", pd, dtype=dtype, backend=backend, bn=bd)
    return make, model, params, bn, x.numpy(), ref


def test_end_to_end_against_float64_and_bf16(cuda_dev, net):
    make, _, _, _, x, ref = net
    pr = make("bf16x3")
    new = pr.predict(x).scores.clone()
    d = {k: float((p.predict(x).scores.cpu().to(F64) - ref).abs().max())
         for k, p in (("bf16x3", pr), ("bf16", make("bf16")), ("torch fp32", make("fp32", "torch")))}
    print("[resnet x3] max |logits - fp64|: " + ", ".join(f"{k} {v:.4g}" for k, v in d.items()))
    assert d["bf16x3"] <= d["bf16"] / 16
    for chunk in (1, 2, 3):  # a row's logits do not depend on its chunk; a second call repeats the first
        assert torch.equal(pr.predict(x, chunk=chunk).scores, new)
    ws, xd = pr._workspace(3), torch.from_numpy(x).to(cuda_dev)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        pr._forward_native(ptr(xd), 3, ws, stream_handle())
    for _ in range(3):
        ws["logits"].zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(ws["logits"][:30].view(3, 10), new)


def test_predict_main_agrees_with_the_api(cuda_dev, net, tmp_path):
    from mpi_tensorflow_amd import config as C
    from mpi_tensorflow_amd.runtime.predict import predict_main
    from mpi_tensorflow_amd.utils import checkpoint as ck

    make, model, params, bn, x, _ = net
    path, out, fx = (str(tmp_path / f) for f in ("r.npz", "o.npz", "x.npy"))
    np.save(fx, x)
    extra = {}
    for name, (rm, rv) in bn.items():
        extra[name + "/moving_mean"], extra[name + "/moving_variance"] = rm, rv
    ck.save(path, model.layout, params, torch.zeros_like(params), 0, meta={"model": "resnet18"}, extra=extra)
    rec = predict_main(C.TrainConfig(model="resnet18", dtype="bf16x3", resume=path, predict=fx,
                                     predict_out=out, predict_probs=True, device="cuda"))["predict"]
    api = make("bf16x3").predict(x, return_probs=True)
    assert (rec["dtype"], rec["n"]) == ("bf16x3", 3)
    assert np.array_equal(np.load(out)["probs"], api.probs.cpu().numpy())
