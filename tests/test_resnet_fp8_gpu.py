"""The ResNet-18 fp8 inference forward (docs/ACCURACY.md): f8conv per loader and MFMA form, the
small kernels against torch, Predictor against the emulation of helpers/resnet_fp8_ref.py."""

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from helpers import lowp_conv as L

from mpi_tensorflow_amd.ops import native, ptr, stream_handle

pytestmark = pytest.mark.gpu

R, H_, E = L.R, L.load("resnet_state"), L.load("resnet_fp8_ref")
F64, BF, F8 = L.F64, L.BF, L.F8
# deepest K; ragged M, odd width, three column tiles; the 128-row tile; 3x3 stride 2; 1x1 stride 2
SHAPES = [(3, 7, 7, 512, 512, 3, 1, 1), (3, 11, 13, 64, 192, 3, 1, 1), (11, 56, 56, 64, 64, 3, 1, 1),
          (2, 14, 14, 64, 128, 3, 2, 1), (4, 14, 14, 128, 64, 1, 2, 0)]
# every eligible (loader form, MFMA form) of a shape: gather 1 / halo 2 x 32x32x64 1 / 32x32x16 2
RUNS = [(s, f, m) for s in SHAPES for f in ((1, 2) if s[5] == 3 and s[6] == 1 else (1,)) for m in (1, 2)]
IDS = ["x".join(map(str, s)) + f"-form{f}-mfma{m}" for s, f, m in RUNS]


def wcodes(w, dev):  # e4m3-exact HWIO weights -> the codes of [tap][k][c]
    return L.codes(w.permute(0, 1, 3, 2).reshape(-1, w.shape[3], w.shape[2]).contiguous(), dev)


@functools.lru_cache(maxsize=None)
def exact_ops(shape):
    return R.gen_exact(500 + SHAPES.index(shape), *shape, lim=3)


@functools.lru_cache(maxsize=None)
def epilogue_ops(shape):
    """Random e4m3-exact operands, a2, b, an e4m3 residual with its scale, and the fp64 conv."""
    return L.epilogue_ops(shape, 900 + SHAPES.index(shape), E.q,
                          lambda r, n: E.q(r.to(F64) * 8 * n ** -0.5))


def run_f8conv(dev, shape, x, w, a2, b, res, s_res, inv, relu, out_bf16, form, mfma, canary):
    return L.run_byte_conv("f8conv", dev, shape, x, wcodes(w, dev), a2, b, res, s_res, inv, relu,
                           out_bf16, canary, form=form, mfma=mfma)


@pytest.mark.parametrize("shape,form,mfma", RUNS, ids=IDS)
def test_f8conv_exact(cuda_dev, shape, form, mfma):
    o, K = exact_ops(shape), shape[4]
    got, plan = run_f8conv(cuda_dev, shape, o["x"], o["w"], torch.ones(K), torch.zeros(K), None, 0.0,
                           1.0, False, True, form, mfma, -768.0)
    assert (plan["bm"], plan["form"]) == (128 if shape == SHAPES[2] else 64, form)
    assert R.exact_diff(got, o["refs"]["fwd"][0], bf16_out=True)[0] == 0


@pytest.mark.parametrize("relu,clamp", [(True, False), (False, False), (True, True)])
@pytest.mark.parametrize("shape,form,mfma", RUNS[::2] + RUNS[1:2], ids=IDS[::2] + IDS[1:2])
def test_f8conv_epilogue_against_float64(cuda_dev, shape, form, mfma, relu, clamp):
    """In code units, u = clamp(v inv_s_out, +-448): |got - u| <= 2^-4 |u| + 2^-10 + inv n EPS S |a2|."""
    x, w, a2, b, res, s_res, (ref, S, n) = epilogue_ops(shape)
    v = ref * a2.to(F64) + b.to(F64) + s_res * res
    v = v.clamp_min(0) if relu else v
    inv = float(np.float32(448.0 / float(v.abs().flatten().quantile(0.98)))) if clamp else 16.0
    u = (v * inv).clamp(-448.0, 448.0)
    if clamp:
        assert 0.005 <= float(((v * inv).abs() > 448.0).double().mean()) <= 0.05
    got, _ = run_f8conv(cuda_dev, shape, x, w, a2, b, res, s_res, inv, relu, False, form, mfma, 0x7f)
    got = got.view(F8).to(F64)
    bound = 2.0 ** -4 * u.abs() + 2.0 ** -10 + inv * n * R.EPS * S * a2.abs().to(F64)
    err = (got - u).abs()
    print(f"[f8conv] {shape} form {form} mfma {mfma}: worst err / bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())


def test_wq_f8_bits(cuda_dev):
    """C = 64 (3x3) and 192 (1x1), an all-zero channel, channels whose amax is exactly 448 2^j."""
    ops, g, dev = native().ops, torch.Generator().manual_seed(21), cuda_dev
    ws = [torch.randn(3, 3, 64, 64, generator=g) * 0.05, torch.randn(1, 1, 192, 128, generator=g) * 3]
    ws[0][..., 5] = 0.0
    ws[0][..., 6] = ws[0][..., 6].clamp(-0.4, 0.4)
    ws[0][1, 2, 3, 6] = -448.0 * 2.0 ** -10
    ws[1][0, 0, 7, 9] = 448.0 * 2.0 ** 3
    wd = [w.to(dev) for w in ws]
    out = [torch.full((w.numel(),), 0x55, dtype=torch.uint8, device=dev) for w in ws]
    sw = torch.zeros(64 + 128, device=dev)
    jobs = torch.tensor([[ptr(wd[0]), ptr(out[0]), 9, 64, 64, 0, 0, 0],
                         [ptr(wd[1]), ptr(out[1]), 1, 192, 128, 64, 2, 0]], dtype=torch.int64).to(dev)
    ops.wq_f8(ptr(jobs), 2, 2 + 4, ptr(sw), stream_handle())
    torch.cuda.synchronize()
    for w, o, off in zip(ws, out, (0, 64)):
        s_ref, c_ref = E.quantise_weight(w)
        assert torch.equal(sw[off:off + w.shape[3]].cpu().to(F64), s_ref)
        assert torch.equal(o.cpu(), c_ref.to(torch.float32).to(F8).view(torch.uint8).flatten())
    assert float(sw[5]) == 1.0 and float(sw[6]) == 2.0 ** -10 and float(sw[64 + 9]) == 8.0


def test_maxpool_infer_f8_bits(cuda_dev):
    ops, g = native().ops, torch.Generator().manual_seed(22)
    x = (torch.randn(2, 7, 9, 64, generator=g) * 3).to(BF)
    p = ops.PoolShape(2, 7, 9, 64, 3, 2, 1)
    n = 2 * p.OH * p.OW * 64
    y = torch.full((n + 256,), 0x7f, dtype=torch.uint8, device=cuda_dev)
    xd, inv = x.to(cuda_dev), torch.tensor([8.0], device=cuda_dev)
    ops.maxpool_infer_f8(p, ptr(xd), ptr(inv), ptr(y), stream_handle())
    torch.cuda.synchronize()
    ref = F.max_pool2d(x.to(F64).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(y.cpu()[:n], E.q(ref * 8.0).to(torch.float32).to(F8).view(torch.uint8).flatten())
    assert R.guard_hits(y.cpu(), n, 0x7f) == 0


# around one block's 2048 values, the 16-byte vector and the 1024-block grid cap
@pytest.mark.parametrize("n", [1, 7, 2047, 2048, 2057, 1024 * 2048 - 5, 1024 * 2048 + 2048 + 3])
def test_amax_b16_with_a_poisoned_tail(cuda_dev, n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n + 64, generator=g).to(BF)
    x[n:] = 1e30  # past the end: must not be read into the result
    x[int(torch.randint(0, n, (1,), generator=g))] = -37.5
    xd, slot = x.to(cuda_dev), torch.tensor([0.0, 1e9], device=cuda_dev)
    for s in (0, 1):  # an empty slot, and one that already holds more
        native().ops.amax_b16(ptr(xd), n, ptr(slot) + 4 * s, stream_handle())
    torch.cuda.synchronize()
    assert slot.cpu().tolist() == [float(x[:n].float().abs().max()), 1e9]


@pytest.fixture(scope="module")
def net(cuda_dev):
    """A calibrated fp8 Predictor on the shared state, 4 rows, the fp64 logits of the first 3."""
    from mpi_tensorflow_amd.ops import functional as Fn
    from mpi_tensorflow_amd.runtime.predict import Predictor

    model, params, bn = H_.resnet_state()
    x = torch.randn(4, 224, 224, 3, generator=torch.Generator().manual_seed(5))
    pv = model.layout.views(params.double())
    P = {s.name: Fn.Param(pv[s.name], None) for s in model.layout.specs}
    with torch.no_grad(), Fn.oracle_mode():
        ref = model.forward(P, {k: (a.double(), b.double()) for k, (a, b) in bn.items()},
                            x[:3].double(), False)
    pr = Predictor("resnet18", params.to(cuda_dev), dtype="fp8",
                   bn={k: (a.to(cuda_dev), b.to(cuda_dev)) for k, (a, b) in bn.items()})
    with pytest.raises(RuntimeError, match="not calibrated"):
        pr._forward_native(1, 1, pr._workspace(3), stream_handle())
    assert pr.calibrate(x[:3].numpy()) == 3
    return pr, model, params, bn, x.numpy(), ref


def test_end_to_end_against_the_float64_emulation(cuda_dev, net):
    """max |native - fp64| <= 2 E, E = max |emulation - fp64| (figures: docs/ACCURACY.md)."""
    pr, model, params, bn, x4, ref = net
    x = x4[:3]
    emu = E.emulate(model, params, bn, torch.from_numpy(x), pr._amax.cpu().tolist())
    new = pr.predict(x).scores.clone()
    e_ref, e_dev = float((emu - ref).abs().max()), float((new.cpu().to(F64) - ref).abs().max())
    print(f"[resnet fp8] max |logits - fp64|: emulation E {e_ref:.4g}, native {e_dev:.4g}; "
          f"native vs emulation {float((new.cpu().to(F64) - emu).abs().max()):.4g}")
    assert e_dev <= 2 * e_ref
    assert torch.equal(pr.predict(x, chunk=2).scores, new)
    assert torch.equal(pr.predict(x).scores, new)  # no recalibration: the same bits
    x28 = np.concatenate([x4 * (1 + 0.1 * i) for i in range(7)])
    assert torch.equal(pr.predict(x28, chunk=24).scores[24:], pr.predict(x28[24:]).scores)
    ws, xd = pr._workspace(3), torch.from_numpy(x).to(cuda_dev)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        pr._forward_native(ptr(xd), 3, ws, stream_handle())
    for _ in range(3):
        ws["logits"].zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(ws["logits"][:30].view(3, 10), new)


def test_predict_main_records_dtype_and_calibration_rows(cuda_dev, net, tmp_path):
    from mpi_tensorflow_amd import config as C
    from mpi_tensorflow_amd.runtime.predict import predict_main
    from mpi_tensorflow_amd.utils import checkpoint as ck

    pr, model, params, bn, x4, _ = net
    path, fx = str(tmp_path / "r.npz"), str(tmp_path / "x.npy")
    np.save(fx, x4)
    extra = {}
    for name, (rm, rv) in bn.items():
        extra[name + "/moving_mean"], extra[name + "/moving_variance"] = rm, rv
    ck.save(path, model.layout, params, torch.zeros_like(params), 0, meta={"model": "resnet18"},
            extra=extra)
    rec = predict_main(C.TrainConfig(model="resnet18", dtype="fp8", resume=path, predict=fx,
                                     predict_calib=3, device="cuda"))["predict"]
    assert (rec["dtype"], rec["calib_rows"], rec["n"]) == ("fp8", 3, 4)
