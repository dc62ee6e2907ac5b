"""--dtype mxfp4 without a GPU: the refusals, and the MXFP4 quantiser reference on hand-worked blocks."""

import importlib.util
import os

import pytest
import torch

_spec = importlib.util.spec_from_file_location("resnet_mx4_ref", os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "helpers", "resnet_mx4_ref.py"))
X = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(X)
OK = dict(dtype="mxfp4", model="resnet18", predict="test", resume="c.npz")


@pytest.mark.parametrize("kw,msg", [
    (dict(dtype="mxfp4", model="resnet18"), "--dtype mxfp4 is inference only: it needs --predict"),
    (dict(OK, model="lenet5"), "--dtype mxfp4 supports --model resnet18 only, not lenet5"),
    (dict(OK, model="mnist_cnn"), "--dtype mxfp4 supports --model resnet18 only, not mnist_cnn"),
    (dict(OK, device="cpu"), "--dtype mxfp4 runs on the native GPU forward only: not with --backend"),
    (dict(OK, backend="torch"), "--dtype mxfp4 runs on the native GPU forward only: not with --backend"),
    (dict(OK, predict_calib=0), "--predict-calib must be positive"),
])
def test_refusals(kw, msg):
    from mpi_tensorflow_amd import config as C

    with pytest.raises(ValueError, match=msg):
        C.TrainConfig(**kw).validate()
    cfg = C.config_from_args(["--model", "resnet18", "--dtype", "mxfp4", "--resume", "c.npz",
                              "--predict", "test", "--predict-calib", "64"])
    assert (cfg.dtype, cfg.predict_calib) == ("mxfp4", 64)


@pytest.mark.parametrize("vals,E,codes", [
    ([0.0], 0, [0.0]),  # an all-zero block: scale byte 127
    ([6.0 * 2.0 ** -7, -1.0 * 2.0 ** -7], -7, [6.0, -1.0]),  # amax exactly 6 2^j
    ([6.0 * 2.0 ** 5 * (1 + 2.0 ** -20), 2.0 ** 6], 6, [3.0, 1.0]),  # just above: the next exponent
    ([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0], 0, [6.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]),  # the ties
    ([-6.0, -0.25, -0.75, -2.5, -5.0, 0.26, -2.51], 0, [-6.0, -0.0, -1.0, -2.0, -4.0, 0.5, -3.0]),  # signs
    ([4.1], 0, [4.0]),  # 3 < amax < 6: E comes from the amax, not from the largest code
])
def test_quantiser_reference_on_hand_worked_blocks(vals, E, codes):
    """One MX block (a [1, 1, 32, 1] filter) that starts with vals, zeros behind them."""
    w = torch.zeros(1, 1, 32, 1)
    w[0, 0, :len(vals), 0] = torch.tensor(vals)
    q = X.mx4_quantise(w)
    got = q[0].flatten().tolist()
    assert int(q[1]) == E and got[:len(codes)] == codes and not any(got[len(codes):])
    assert [torch.tensor(v).signbit().item() for v in got[:len(codes)]] == [v < 0 for v in vals]
    assert torch.equal(X.mx4_dequant(*X.mx4_quantise(X.mx4_dequant(*q))), X.mx4_dequant(*q))  # idempotent
    sc = X.pack(*X.mx4_quantise(torch.zeros(1, 1, 64, 64)))
    assert sc.numel() == 2176 and not sc[:2048].any() and bool((sc[2048:] == 127).all())
