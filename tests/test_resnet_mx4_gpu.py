"""The ResNet-18 mxfp4 inference forward (docs/ACCURACY.md): mx4conv per loader form, wq_mx4
against the host packer, Predictor against the emulation of helpers/resnet_mx4_ref.py."""

import functools

import numpy as np
import pytest
import torch
from helpers import lowp_conv as L

from mpi_tensorflow_amd.ops import native, ptr, stream_handle

pytestmark = pytest.mark.gpu

R, H_, X = L.R, L.load("resnet_state"), L.load("resnet_mx4_ref")
E8, F64, BF, F8 = X.E8, L.F64, L.BF, L.F8
# test_resnet_fp8_gpu.py's five (deepest K; ragged M, three column tiles; the 128-row tile; 3x3
# stride 2; 1x1 stride 2) and a two-chunk halo shape: the single-buffered slab is staged again
SHAPES = [(3, 7, 7, 512, 512, 3, 1, 1), (3, 11, 13, 64, 192, 3, 1, 1), (11, 56, 56, 64, 64, 3, 1, 1),
          (2, 14, 14, 64, 128, 3, 2, 1), (4, 14, 14, 128, 64, 1, 2, 0), (2, 9, 9, 128, 64, 3, 1, 1)]
RUNS = [(s, f) for s in SHAPES for f in ((1, 2) if s[5] == 3 and s[6] == 1 else (1,))]
IDS = ["x".join(map(str, s)) + f"-form{f}" for s, f in RUNS]


def slabs(w):  # MX-exact weights -> the host packer's bytes
    q = X.mx4_quantise(w)
    assert torch.equal(X.mx4_dequant(*q), w.to(F64))
    return X.pack(*q)


@functools.lru_cache(maxsize=None)
def exact_ops(shape):
    """gen_exact's integers, each weight block times 2^e, e in [-2, 2] a function of (tap, k, c / 32)
    that differs between the halves of a chunk, between taps and between column groups."""
    C, K, Rr = shape[3:6]
    o = R.gen_exact(500 + SHAPES.index(shape), *shape, lim=3)
    tap, c, k = torch.meshgrid(torch.arange(Rr * Rr), torch.arange(C), torch.arange(K), indexing="ij")
    w = o["w"] * (2.0 ** ((tap + 2 * (c // 32) + k + k // 32) % 5 - 2)).reshape(Rr, Rr, C, K)
    ref, S, _ = R.conv_fwd(o["x"], w, *shape[6:], dt=torch.float32)
    R.assert_exact(S.max())
    return o["x"], slabs(w), ref


@functools.lru_cache(maxsize=None)
def epilogue_ops(shape):
    """test_resnet_fp8_gpu.py's epilogue operands with random MX-exact weights."""
    x, w, *rest = L.epilogue_ops(shape, 900 + SHAPES.index(shape), E8.q,
                                 lambda r, n: X.mx4_dequant(*X.mx4_quantise(r * 8 * n ** -0.5)))
    return (x, slabs(w), *rest)


def run_mx4conv(dev, shape, x, w, a2, b, res, s_res, inv, relu, out_bf16, form, canary):
    return L.run_byte_conv("mx4conv", dev, shape, x, w, a2, b, res, s_res, inv, relu, out_bf16, canary,
                           form=form)


@pytest.mark.parametrize("shape,form", RUNS, ids=IDS)
def test_mx4conv_exact(cuda_dev, shape, form):
    x, w, ref = exact_ops(shape)
    one, zero = torch.ones(shape[4]), torch.zeros(shape[4])
    got, plan = run_mx4conv(cuda_dev, shape, x, w, one, zero, None, 0.0, 1.0, False, True, form, -768.0)
    assert (plan["bm"], plan["form"]) == (128 if shape == SHAPES[2] else 64, form)
    assert R.exact_diff(got, ref, bf16_out=True)[0] == 0


@pytest.mark.parametrize("relu,clamp", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("shape,form", RUNS, ids=IDS)
def test_mx4conv_epilogue_against_float64(cuda_dev, shape, form, relu, clamp):
    """In code units, u = clamp(v inv_s_out, +-448): |got - u| <= 2^-4 |u| + 2^-10 + inv n EPS S |a2|."""
    x, w, a2, b, res, s_res, (ref, S, n) = epilogue_ops(shape)
    v = ref * a2.to(F64) + b.to(F64) + s_res * res
    v = v.clamp_min(0) if relu else v
    inv = float(np.float32(448.0 / float(v.abs().flatten().quantile(0.98)))) if clamp else 16.0
    u = (v * inv).clamp(-448.0, 448.0)
    if clamp:
        assert 0.005 <= float(((v * inv).abs() > 448.0).double().mean()) <= 0.05
    got, _ = run_mx4conv(cuda_dev, shape, x, w, a2, b, res, s_res, inv, relu, False, form, 0x7f)
    err = (got.view(F8).to(F64) - u).abs()
    bound = 2.0 ** -4 * u.abs() + 2.0 ** -10 + inv * n * R.EPS * S * a2.abs().to(F64)
    print(f"[mx4conv] {shape} form {form}: worst err / bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())


def test_wq_mx4_bits(cuda_dev):
    """3x3 C = 64 and 1x1 C = 192 in one launch: an all-zero block, an amax of exactly 6 2^-7, a tie."""
    ops, g, dev = native().ops, torch.Generator().manual_seed(21), cuda_dev
    ws = [torch.randn(3, 3, 64, 64, generator=g) * 0.05, torch.randn(1, 1, 192, 128, generator=g) * 3]
    ws[0][1, 2, 32:, 5] = 0.0
    ws[0][2, 0, :32, 6] = ws[0][2, 0, :32, 6].clamp(-0.04, 0.04)
    ws[0][2, 0, 3, 6] = -6.0 * 2.0 ** -7
    ws[1][0, 0, 64:96, 70] = ws[1][0, 0, 64:96, 70].clamp(-5.0, 5.0)
    ws[1][0, 0, 64:67, 70] = torch.tensor([6.0, 2.5, -0.25])  # E = 0: 2.5 -> 2, -0.25 -> -0
    wd = [w.to(dev) for w in ws]
    ref = [X.pack(*X.mx4_quantise(w)) for w in ws]
    out = [torch.full((r.numel() + 64,), 0x55, dtype=torch.uint8, device=dev) for r in ref]
    jobs = torch.tensor([[ptr(wd[0]), ptr(out[0]), 9, 64, 64, 0, 0, 0],
                         [ptr(wd[1]), ptr(out[1]), 1, 192, 128, 0, 1, 0]], dtype=torch.int64).to(dev)
    ops.wq_mx4(ptr(jobs), 2, 1 + 6, stream_handle())
    torch.cuda.synchronize()
    for r, o in zip(ref, out):
        assert torch.equal(o.cpu()[:r.numel()], r) and R.guard_hits(o.cpu(), r.numel(), 0x55) == 0


def test_end_to_end_against_the_float64_emulation(cuda_dev, tmp_path):
    """max |native - fp64| <= 2 E, E = max |emulation - fp64| (figures: docs/ACCURACY.md); chunks, a
    ragged tail, graph replays and a second predict give the same bits; predict_main's record."""
    from mpi_tensorflow_amd import config as C
    from mpi_tensorflow_amd.runtime.predict import Predictor, predict_main
    from mpi_tensorflow_amd.utils import checkpoint as ck

    model, params, bn = H_.resnet_state()
    x4 = torch.randn(4, 224, 224, 3, generator=torch.Generator().manual_seed(5))
    x, x4 = x4[:3], x4.numpy()
    pr = Predictor("resnet18", params.to(cuda_dev), dtype="mxfp4",
                   bn={k: (a.to(cuda_dev), b.to(cuda_dev)) for k, (a, b) in bn.items()})
    with pytest.raises(RuntimeError, match="not calibrated"):
        pr._forward_native(1, 1, pr._workspace(3), stream_handle())
    assert pr.calibrate(x) == 3
    amax = pr._amax.cpu().tolist()
    ref = E8.emulate(model, params, bn, x, amax, quantise=False)  # the float64 forward
    emu, emu8 = X.emulate(model, params, bn, x, amax), E8.emulate(model, params, bn, x, amax)
    new = pr.predict(x).scores.clone()
    e_ref, e_dev = float((emu - ref).abs().max()), float((new.cpu().to(F64) - ref).abs().max())
    print(f"[resnet mxfp4] max |logits - fp64|: emulation E {e_ref:.4g}, native {e_dev:.4g}, fp8's E "
          f"{float((emu8 - ref).abs().max()):.4g}; native vs emulation "
          f"{float((new.cpu().to(F64) - emu).abs().max()):.4g}")
    assert e_dev <= 2 * e_ref
    assert torch.equal(pr.predict(x, chunk=2).scores, new)
    assert torch.equal(pr.predict(x).scores, new)  # no recalibration: the same bits
    x28 = np.concatenate([x4 * (1 + 0.1 * i) for i in range(7)])
    assert torch.equal(pr.predict(x28, chunk=24).scores[24:], pr.predict(x28[24:]).scores)
    ws, xd, gr = pr._workspace(3), x.to(cuda_dev), torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        pr._forward_native(ptr(xd), 3, ws, stream_handle())
    for _ in range(3):
        ws["logits"].zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(ws["logits"][:30].view(3, 10), new)
    path, fx = str(tmp_path / "r.npz"), str(tmp_path / "x.npy")
    np.save(fx, x4)
    extra = {n + s: t for n, (rm, rv) in bn.items() for s, t in (("/moving_mean", rm), ("/moving_variance", rv))}
    ck.save(path, model.layout, params, torch.zeros_like(params), 0, meta={"model": "resnet18"}, extra=extra)
    rec = predict_main(C.TrainConfig(model="resnet18", dtype="mxfp4", resume=path, predict=fx,
                                     predict_calib=3, device="cuda"))["predict"]
    assert (rec["dtype"], rec["calib_rows"], rec["n"]) == ("mxfp4", 3, 4)
