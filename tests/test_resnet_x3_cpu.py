"""--dtype bf16x3 without a GPU: what the configuration accepts and refuses, and the identities of
the hi / lo split (docs/ACCURACY.md "ResNet-18 bf16x3 inference") written in torch."""

import pytest
import torch

BF = torch.bfloat16
OK = dict(dtype="bf16x3", model="resnet18", predict="test", resume="c.npz")


def split(v):
    hi = v.to(BF).float()
    return hi, (v - hi).to(BF).float()


@pytest.mark.parametrize("kw,flag", [
    (dict(OK, predict=None), "--predict"),
    (dict(OK, model="lenet5"), "resnet18"),
    (dict(OK, model="mnist_cnn"), "resnet18"),
    (dict(OK, device="cpu"), "--device cpu"),
    (dict(OK, backend="torch"), "--backend torch"),
    (dict(OK, predict_calib=64), "--predict-calib"),
])
def test_config_accepts_and_refuses(kw, flag):
    from mpi_tensorflow_amd import config as C

    with pytest.raises(ValueError, match=flag):
        C.TrainConfig(**kw).validate()
    cfg = C.config_from_args(["--model", "resnet18", "--dtype", "bf16x3", "--resume", "X",
                              "--predict", "test"])
    assert (cfg.dtype, cfg.predict, cfg.resume) == ("bf16x3", "test", "X")


def test_split_identities():
    g = torch.Generator().manual_seed(1)
    v = torch.randn(4096, generator=g) * torch.exp2(torch.randint(-20, 20, (4096,), generator=g).float())
    hi, lo = split(v)
    join = hi + lo
    assert torch.equal(join.double(), hi.double() + lo.double())  # the fp32 sum is exact
    assert bool(((v.double() - join.double()).abs() <= 2.0 ** -16 * v.double().abs()).all())
    # split(join) moves hi only where lo is exactly half an ulp of hi and the tie goes the other
    # way: lo rounds onto that value for about 2^-9 of the inputs, so a sixteenth is far off
    h2, l2 = split(join)
    ties = int(((h2 != hi) | (l2 != lo)).sum())
    print(f"[x3 split] split(join) != (hi, lo) on {ties} of 4096 values")
    assert torch.equal(h2 + l2, join) and ties < 4096 // 16
