"""--dtype fp8 without a GPU: the refusals, and the emulation helper at zero quantisation."""

import importlib.util
import os

import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


E, H_ = _load("resnet_fp8_ref"), _load("resnet_state")
F64 = torch.float64


@pytest.mark.parametrize("kw,flag", [
    (dict(dtype="fp8", model="resnet18"), "--predict"),
    (dict(dtype="fp8", model="lenet5", predict="test", resume="c.npz"), "resnet18"),
    (dict(dtype="fp8", model="mnist_cnn", predict="test", resume="c.npz"), "resnet18"),
    (dict(dtype="fp8", model="resnet18", predict="test", resume="c.npz", device="cpu"), "--device cpu"),
    (dict(dtype="fp8", model="resnet18", predict="test", resume="c.npz", backend="torch"), "--backend torch"),
    (dict(dtype="bf16", model="resnet18", predict="test", resume="c.npz", predict_calib=64), "--predict-calib"),
    (dict(dtype="fp8", model="resnet18", predict="test", resume="c.npz", predict_calib=0), "--predict-calib"),
])
def test_refusals(kw, flag):
    from mpi_tensorflow_amd import config as C

    with pytest.raises(ValueError, match=flag):
        C.TrainConfig(**kw).validate()
    cfg = C.config_from_args(["--model", "resnet18", "--dtype", "fp8", "--resume", "c.npz",
                              "--predict", "test", "--predict-calib", "64"])
    assert (cfg.dtype, cfg.predict_calib) == ("fp8", 64)


def test_emulation_at_zero_quantisation_is_the_float64_forward():
    """An integer conv with unit scales (nothing rounds), then the net with q the identity."""
    from mpi_tensorflow_amd.ops import functional as Fn

    g = torch.Generator().manual_seed(2)
    x = torch.randint(-3, 4, (1, 5, 5, 4), generator=g).to(F64)
    w = torch.randint(-3, 4, (3, 3, 4, 2), generator=g).float()
    w[0, 0, 0] = 448.0  # sw = 1 for both channels
    one, zero = torch.ones(2, dtype=F64), torch.zeros(2, dtype=F64)
    got = E.f8_conv(x, 1.0, w, one, zero, 1, 1, s_out=None)
    assert torch.equal(got, E.conv(x, w.to(F64), 1, 1))
    sw, codes = E.quantise_weight(w)
    assert sw.tolist() == [1.0, 1.0] and torch.equal(codes[4], w[1, 1].t().to(F64))
    model, params, bn = H_.resnet_state()
    xi = torch.randn(1, 32, 32, 3, generator=g)
    pv = model.layout.views(params.double())
    P = {s.name: Fn.Param(pv[s.name], None) for s in model.layout.specs}
    with torch.no_grad(), Fn.oracle_mode():
        ref = model.forward(P, {k: (a.double(), b.double()) for k, (a, b) in bn.items()},
                            xi.double(), False)
    amax = [0.37 * (i + 1) for i in range(20)]  # any scales: they cancel exactly
    emu = E.emulate(model, params, bn, xi, amax, quantise=False)
    assert float((emu - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
    assert float((E.emulate(model, params, bn, xi, amax) - ref).abs().max()) > 1e-6
