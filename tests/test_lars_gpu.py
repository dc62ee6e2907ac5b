"""--optimizer lars on the GPU: optim.lars_step on a synthetic segment table against the
float64 definition (docs/ACCURACY.md "LARS" derives the bounds), the generic engine against
the CPU torch engine and graph against eager, ResNet-18 bf16's conv weight copies."""

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.runtime.generic_engine import GenericEngine
from mpi_tensorflow_amd.runtime.lars import LarsState, adapted, lars_update_
from mpi_tensorflow_amd.utils.data import synthetic_rows

pytestmark = pytest.mark.gpu

# (numel, adapted, zeroed buffer): every chunk-count and float4-tail case of the kernels
TENSORS = [(1, True, None), (63, False, None), (64, True, "w"), (4095, True, None),
           (4096, False, None), (4097, True, "g"), (3 * 4096 + 5, True, None)]
PAD_BITS = 0x7FC12345  # a quiet NaN with a payload: poisons any norm that reads it
EPS, SLACK = 2.0 ** -24, 1 + 2.0 ** -10
LR, MU = float(np.float32(0.0123)), float(np.float32(0.9))  # the kernel's fp32 operands


@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
@pytest.mark.parametrize("nesterov", [False, True])
def test_lars_step_kernels(cuda_dev, nesterov, wd, gscale):
    opt = C.OptimizerSpec("lars", 0.001, wd, nesterov)
    opt32 = C.OptimizerSpec("lars", 0.001, float(np.float32(wd)), nesterov)  # the update's fp32 wd
    offs = np.cumsum([0] + [-(-n // 64) * 64 for n, _, _ in TENSORS]).tolist()
    segs, total = [(o, n, ad) for o, (n, ad, _) in zip(offs, TENSORS)], offs[-1]
    gen = torch.Generator().manual_seed(11)
    w0, g0, m0 = (torch.randn(total, generator=gen) for _ in range(3))
    pad = torch.ones(total, dtype=torch.bool)
    for (o, n, _), (_, _, zero) in zip(segs, TENSORS):
        pad[o:o + n] = False
        if zero is not None:
            (w0 if zero == "w" else g0)[o:o + n] = 0.0
    g0[pad] = 1e30
    w0.view(torch.int32)[pad] = PAD_BITS
    m0.view(torch.int32)[pad] = PAD_BITS
    st, st2 = LarsState(segs, opt, cuda_dev), LarsState(segs, opt, cuda_dev)
    assert st.nchunks == 5 + 2 + 4
    lr, g = torch.tensor([LR]).to(cuda_dev), g0.to(cuda_dev)
    w, m, step = w0.to(cuda_dev), m0.to(cuda_dev), torch.zeros(1, dtype=torch.int64).to(cuda_dev)
    st.step(w, g, m, MU, gscale, lr, step)
    torch.cuda.synchronize()
    ratio, w1, m1 = st.ratio.cpu().double(), w.cpu(), m.cpu()
    assert int(step.item()) == 1
    assert all(bool((t.view(torch.int32)[pad] == PAD_BITS).all()) for t in (w1, m1))
    for (o, n, ad), (_, _, zero), rk in zip(segs, TENSORS, ratio.tolist()):
        W, G, M = (t[o:o + n].double() for t in (w0, g0, m0))
        r = float(lars_update_(W.clone(), G, M.clone(), ad, opt, LR, MU, gscale))
        assert abs(rk - r) <= 2.0 ** -18 * r and (ad and zero is None or r == rk == 1.0)
        # w and m with the kernel's ratio as the operand: g', e = fma(wd, w, g'), u = r e,
        # m = fma(mu, m, u), [d = fma(mu, m, u)], w = fma(-lr, d or m, w), 2^-24 relative each
        gp = G * gscale
        e = gp + (opt32.wd * W if ad else 0.0)
        u = rk * e
        lars_update_(W, G, M, ad, opt32, LR, MU, gscale, r=rk)
        du = EPS * (rk * gp.abs() + rk * e.abs() + u.abs())
        dm = du + EPS * M.abs()
        dw = LR * (MU * dm + du + EPS * (u + MU * M).abs() if nesterov else dm) + EPS * W.abs()
        em, ew = (m1[o:o + n].double() - M).abs(), (w1[o:o + n].double() - W).abs()
        assert bool((em <= dm * SLACK).all()) and bool((ew <= dw * SLACK).all())
    # three eager steps against one captured step replayed three times, bit for bit
    for _ in range(2):
        st.step(w, g, m, MU, gscale, lr, step)
    w2, m2, step2 = w0.to(cuda_dev), m0.to(cuda_dev), torch.zeros_like(step)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st2.step(w2, g, m2, MU, gscale, lr, step2)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(step.item()) == int(step2.item()) == 3
    for a, b in ((w, w2), (m, m2), (st.ratio, st2.ratio)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _lenet(device, **kw):
    cfg = C.TrainConfig(**{**dict(model="lenet5", batch_size=8, graph=False, device=device.type,
                                  optimizer="lars:0.01,wd:5e-4"), **kw}).validate()
    return GenericEngine(cfg, *synthetic_rows("train", 0, 64, shape=(32, 32, 3)), device)


def test_generic_engine_lenet(cuda_dev):
    """Per step from the same state, against the CPU torch engine: the bounds of
    test_generic_ops_gpu.py::test_model_grads_native_vs_oracle (loss 1e-4, gradients 1e-3 per
    tensor, weights 1e-4); a ratio follows its gradient norm, so 1e-3 too.  Then graph == eager."""
    gpu, cpu = _lenet(cuda_dev), _lenet(torch.device("cpu"))
    rel = lambda a, b: ((a.cpu() - b).norm() / max(1e-12, b.norm())).item()  # noqa: E731
    for s in range(3):
        cpu.params.data.copy_(gpu.params.detach().cpu())
        cpu.mom.copy_(gpu.mom.cpu())
        gpu.train(1)
        cpu.train(1)
        torch.cuda.synchronize()
        assert abs(gpu.loss_value() - cpu.loss_value()) < 1e-4 * max(1.0, cpu.loss_value())
        gv, cv = gpu.layout.views(gpu.grads), cpu.layout.views(cpu.grads)
        for sp, rg, rc in zip(gpu.layout.specs, gpu.ratio.tolist(), cpu.ratio.tolist()):
            assert rel(gv[sp.name], cv[sp.name]) < 1e-3, (s, sp.name)
            assert abs(rg - rc) < 1.01e-3 * rc and (adapted(sp) or rg == 1.0)
        assert rel(gpu.params.detach(), cpu.params.detach()) < 1e-4
    assert int(gpu.step_dev.item()) == 3 and bool((gpu.ratio != 1.0).any())
    a, b = _lenet(cuda_dev, graph=True, graph_steps=2), _lenet(cuda_dev)
    a.train(7)  # 3 eager warm-up steps + 2 replays of the 2-step graph
    b.train(7)
    torch.cuda.synchronize()
    assert a.step == b.step == int(a.step_dev.item()) == 7
    assert all(torch.equal(getattr(a, k).detach(), getattr(b, k).detach()) for k in ("params", "mom", "ratio"))


def test_resnet18_bf16_step_and_native_engine_refusals(cuda_dev):
    """One bf16 step at the smallest batch the suite trains a bf16 ResNet-18 at."""
    from mpi_tensorflow_amd.runtime.lenet_engine import NativeLenetEngine
    from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine

    x, y = synthetic_rows("train", 0, 16, shape=(32, 32, 3))
    eng = GenericEngine(C.TrainConfig(model="resnet18", batch_size=8, dtype="bf16", graph=False,
                                      optimizer="lars,wd:5e-4").validate(), x, y, cuda_dev)
    w0 = eng.params.detach().clone()
    eng.train(1)
    copies = eng.wcache.buf.clone()
    eng.wcache.refresh()
    torch.cuda.synchronize()
    assert torch.equal(copies.view(torch.int16), eng.wcache.buf.view(torch.int16))
    ratio = eng.ratio.cpu()
    assert ratio.shape == (62,) and bool(torch.isfinite(ratio).all()) and bool((ratio != 1).any())
    assert all(adapted(sp) or r == 1.0 for r, sp in zip(ratio.tolist(), eng.layout.specs))
    assert not torch.equal(w0, eng.params.detach())
    with pytest.raises(ValueError, match="momentum SGD"):
        NativeLenetEngine(C.TrainConfig(model="lenet5", optimizer="lars").validate(), x, y, cuda_dev)
    with pytest.raises(ValueError, match="momentum SGD"):  # (validate() already refuses mnist_cnn)
        NativeMnistEngine(C.TrainConfig(optimizer="lars"), *synthetic_rows("train", 0, 128), cuda_dev)
