"""The ResNet-18 bf16 inference forward (csrc/resnet_infer.cpp): the affine conv epilogues per
route, bn_fold and the head against float64, the forward through Predictor and predict_main.
End to end on 3 rows, max |logits - fp64| measured on an MI355X: engine.evaluate (bf16) 0.2437,
this forward 0.2765 (bound: twice the former)."""

import importlib.util
import os

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd.ops import functional as Fn
from mpi_tensorflow_amd.ops import native, ptr, stream_handle

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R, H_ = _load("conv_ref"), _load("resnet_state")
F64, BF = torch.float64, torch.bfloat16
H3, FW = "conv3_kernel", "fwd_kernel"
# (N, H, W, C, K, R, stride, pad) -> (kernel, bm, bn, z, halo) of ops.conv_route
CASES = [((4, 14, 14, 64, 64, 3, 1, 1), (H3, 64, 64, 1, True)),
         ((11, 56, 56, 64, 64, 3, 1, 1), (H3, 128, 64, 1, True)),
         ((3, 11, 13, 64, 192, 3, 1, 1), (H3, 64, 64, 1, True)),
         ((3, 7, 7, 512, 512, 3, 1, 1), (H3, 64, 64, 8, True)),
         ((2, 14, 14, 64, 128, 3, 2, 1), (FW, 64, 64, 2, False)),
         ((4, 14, 14, 128, 64, 1, 2, 0), (FW, 64, 64, 1, False)),
         ((4, 128, 128, 64, 256, 1, 2, 0), (FW, 128, 128, 1, False)),
         ((2, 37, 41, 3, 64, 7, 2, 3), (FW + "/S2dLoaderPre", 128, 64, 1, False))]


@pytest.mark.parametrize("res,relu", [(True, True), (False, False)])
@pytest.mark.parametrize("shape,route", CASES, ids=[f"{r[0]}-{'x'.join(map(str, s))}" for s, r in CASES])
def test_affine_conv_against_float64(cuda_dev, shape, route, res, relu):
    ops, s, dev = native().ops, stream_handle(), cuda_dev
    N, H, W, C, K, Rr, stride, pad = shape
    stem = C == 3
    sh = ops.ConvShape(N, H, W, C, K, Rr, Rr, stride, pad)
    si = Fn._s2d_shape(sh) if stem else None
    r = ops.conv_route(si, "fwd", True, stem=2) if stem else ops.conv_route(sh, "fwd", True)
    assert (r["kernel"], r["bm"], r["bn"], r["z"], r["halo"]) == route
    o = R.gen_rounded(300 + CASES.index((shape, route)), *shape)
    g = torch.Generator().manual_seed(7)
    a = (torch.rand(K, generator=g) * 1.5 + 0.5) * (torch.randint(0, 2, (K,), generator=g) * 2 - 1)
    b = torch.rand(K, generator=g) * 2 - 1
    rs = R.bf16_rne(torch.randn(N, sh.OH, sh.OW, K, generator=g)) if res and not stem else None
    ref, S, n = R.conv_fwd(o["x"], o["w"], stride, pad)
    v = ref * a.to(F64) + b.to(F64) + (rs.to(F64) if rs is not None else 0.0)
    v = v.clamp_min(0) if relu else v
    bound = 2.0 ** -8 * v.abs() + n * R.EPS * S * a.abs().to(F64)
    M, canary = N * sh.OH * sh.OW, -768.0
    yb = torch.full((M * K + 4096,), canary, dtype=BF, device=dev)
    ad, bd, wd = a.to(dev), b.to(dev), o["w"].to(dev)
    if stem:
        xd = o["x"].to(dev)
        xs = torch.empty(N * si.H * si.W * 16, dtype=BF, device=dev)
        wt8 = torch.empty(K * 256, dtype=BF, device=dev)
        ops.s2d_stem_input(ptr(xd), N, H, W, sh.OH, sh.OW, ptr(xs), s)
        ops.s2d_stem_weight(ptr(wd), K, ptr(wt8), s)
        ops.conv_fwd_s2d_stem_affine_bf16(si, ptr(xs), ptr(wt8), ptr(ad), ptr(bd), relu, ptr(yb), s)
    else:
        xd = o["x"].to(BF).to(dev)
        wtb = torch.empty(wd.numel(), dtype=BF, device=dev)
        jobs = torch.tensor([[ptr(wd), ptr(wtb), Rr * Rr, C, K, 0, 0, 0]], dtype=torch.int64).to(dev)
        ops.wcvt_batch(ptr(jobs), 1, ops.wcvt_blocks(Rr * Rr, C, K), s)
        ws = torch.zeros(max(int(r["ws_floats"]), 4), device=dev)
        rd = rs.to(BF).to(dev) if rs is not None else None
        ops.conv_fwd_affine_bf16(sh, ptr(xd), ptr(wtb), ptr(ad), ptr(bd), ptr(rd), relu, ptr(yb),
                                 ptr(ws), s)
    torch.cuda.synchronize()
    got = yb.cpu()
    assert R.guard_hits(got.float(), M * K, canary) == 0
    err = (got[:M * K].to(F64).reshape(v.shape) - v).abs()
    print(f"[affine conv] {route} res={res}: worst err / bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())


def test_bn_fold_against_float64(cuda_dev):
    g = torch.Generator().manual_seed(11)
    jobs, off, want = [], 0, []
    for c in (64, 192):  # gamma, beta, rm, rv in [1e-3, 4], and their device copies
        t = [torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g),
             torch.randn(c, generator=g), torch.rand(c, generator=g) * (4 - 1e-3) + 1e-3]
        want.append(t + [[x.to(cuda_dev) for x in t]])
        jobs.append([ptr(x) for x in want[-1][4]] + [c, off, 0, 0])
        off += c
    out = torch.zeros(2 * off, device=cuda_dev)
    jd = torch.tensor(jobs, dtype=torch.int64).to(cuda_dev)
    native().ops.bn_fold(ptr(jd), 2, off, 1e-5, ptr(out), stream_handle())
    got, o = out.cpu().to(F64), 0
    for gm, beta, rm, rv, _ in want:
        c = gm.numel()
        a = gm.to(F64) / torch.sqrt(rv.to(F64) + float(np.float32(1e-5)))
        bb = beta.to(F64) - rm.to(F64) * a
        assert bool(((got[o:o + c] - a).abs() <= 1e-6 * a.abs()).all())
        assert bool(((got[off + o:off + o + c] - bb).abs() <= 1e-6 * (1 + (rm.to(F64) * a).abs())).all())
        o += c


@pytest.mark.parametrize("m", [1, 3])
def test_avgpool_fc_against_float64(cuda_dev, m):
    g = torch.Generator().manual_seed(m)
    x = torch.randn(m, 49, 512, generator=g).to(BF)
    w, b = torch.randn(512, 10, generator=g) * (2 / 512) ** 0.5, torch.randn(10, generator=g)
    xd, wd, bd = x.to(cuda_dev), w.to(cuda_dev), b.to(cuda_dev)
    out = torch.zeros(m, 10, device=cuda_dev)
    native().ops.avgpool_fc(ptr(xd), ptr(wd), ptr(bd), ptr(out), m, 49, 512, 10, stream_handle())
    ref = x.to(F64).mean(1) @ w.to(F64) + b.to(F64)
    assert float((out.cpu().to(F64) - ref).abs().max()) <= 1e-5


@pytest.fixture(scope="module")
def engine(cuda_dev):
    """A bf16 GenericEngine holding the shared state, 4 rows and the fp64 logits of the first 3."""
    from mpi_tensorflow_amd import config as C
    from mpi_tensorflow_amd.runtime.generic_engine import GenericEngine

    model, params, bn = H_.resnet_state()
    cfg = C.TrainConfig(model="resnet18", dtype="bf16", batch_size=2, graph=False).validate()
    eng = GenericEngine(cfg, np.zeros((4, 224, 224, 3), np.float32), np.zeros(4, np.int64), cuda_dev)
    with torch.no_grad():
        eng.params.copy_(params)
        for name, (rm, rv) in bn.items():
            eng.bn[name][0].copy_(rm)
            eng.bn[name][1].copy_(rv)
    x = torch.randn(4, 224, 224, 3, generator=torch.Generator().manual_seed(5))
    pv = model.layout.views(params.double())
    P = {s.name: Fn.Param(pv[s.name], None) for s in model.layout.specs}
    with torch.no_grad(), Fn.oracle_mode():
        ref = model.forward(P, {k: (a.double(), b.double()) for k, (a, b) in bn.items()},
                            x[:3].double(), False)
    return eng, x.numpy(), ref


def test_end_to_end_against_float64_and_the_engine(cuda_dev, engine):
    from mpi_tensorflow_amd.runtime.predict import Predictor

    eng, x4, ref = engine
    x = x4[:3]
    old = eng.evaluate(x, np.zeros(3, np.int64), return_logits=True)[1].cpu().to(F64)
    pr = Predictor.from_engine(eng)
    assert (pr.backend, pr.dtype) == ("native", "bf16")
    assert pr.bn["bn1"][1].data_ptr() == eng.bn["bn1"][1].data_ptr()
    new = pr.predict(x).scores.clone()
    dev_old, dev_new = float((old - ref).abs().max()), float((new.cpu().to(F64) - ref).abs().max())
    print(f"[resnet infer] max |logits - fp64|: engine.evaluate {dev_old:.4g}, ResnetInfer {dev_new:.4g}")
    assert dev_new <= 2 * dev_old
    assert torch.equal(pr.predict(x, chunk=2).scores, new)
    # buffers sized at a chunk whose layer4 does not split K (24 rows), then a tail whose does (4)
    RI = native().ResnetInfer
    assert RI.ws_bytes(pr.ptrs, 256)[3] >= RI.ws_bytes(pr.ptrs, 40)[3] > RI.ws_bytes(pr.ptrs, 4)[3] // 2
    x28 = np.concatenate([x4 * (1 + 0.1 * i) for i in range(7)])
    alone = Predictor.from_engine(eng).predict(x28[24:]).scores.clone()
    assert torch.equal(pr.predict(x28, chunk=24).scores[24:], alone)
    w24 = pr._workspace(24)
    with pytest.raises(RuntimeError, match="workspace"):
        RI.eval_chunk(pr.ptrs, ptr(w24["xv"]), 4, ptr(w24["act0"]), ptr(w24["act1"]), ptr(w24["act2"]),
                      ptr(w24["conv_ws"]), 4, ptr(w24["logits"]), stream_handle())
    # the captured chain, replayed, against the eager launch
    ws, xd = pr._workspace(3), torch.from_numpy(x).to(cuda_dev)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        pr._forward_native(ptr(xd), 3, ws, stream_handle())
    for _ in range(3):
        ws["logits"].zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(ws["logits"][:30].view(3, 10), new)
    rv = eng.bn["l2b0n1"][1]
    keep = rv.clone()
    rv.mul_(4.0)
    try:
        assert not torch.equal(pr.predict(x).scores, new)  # the fold is re-derived
    finally:
        rv.copy_(keep)


def test_predict_main_on_a_saved_checkpoint(cuda_dev, engine, tmp_path):
    from mpi_tensorflow_amd import config as C
    from mpi_tensorflow_amd.runtime.predict import Predictor, predict_main
    from mpi_tensorflow_amd.utils import checkpoint as ck

    eng, x, _ = engine
    y = np.arange(4, dtype=np.int64)
    path, out, fx, fy = (str(tmp_path / f) for f in ("r.npz", "o.npz", "x.npy", "y.npy"))
    np.save(fx, x)
    np.save(fy, y)
    extra = eng.extra_state()
    ck.save(path, eng.layout, eng.params, eng.mom, 0, meta={"model": "resnet18"}, extra=extra)
    cfg = C.TrainConfig(model="resnet18", dtype="bf16", resume=path, predict=fx, predict_labels=fy,
                        predict_out=out, device="cuda")
    rec = predict_main(cfg)["predict"]
    api = Predictor.from_checkpoint(path, dtype="bf16", device="cuda").predict(x, labels=y)
    assert (rec["n"], rec["error"]) == (4, api.metrics.error)
    assert np.array_equal(np.load(out)["pred"], api.pred.cpu().numpy())
    with pytest.raises(ValueError, match="--dtype bf16"):
        Predictor.from_checkpoint(path, dtype="fp32", device="cuda", backend="native")
    del extra["bn1/moving_variance"]
    ck.save(path, eng.layout, eng.params, eng.mom, 0, meta={"model": "resnet18"}, extra=extra)
    with pytest.raises(ValueError, match="bn1/moving_variance"):
        Predictor.from_checkpoint(path, dtype="bf16", device="cuda")
