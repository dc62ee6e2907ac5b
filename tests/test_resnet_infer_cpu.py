"""ResNet-18 --predict without a GPU: the flags, and the torch-backend
Predictor with the BatchNorm statistics of a checkpoint."""

import importlib.util
import os

import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("resnet_state", os.path.join(_HERE, "helpers", "resnet_state.py"))
_H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_H)
_resnet_state = _H.resnet_state


def test_flags(tmp_path):
    from mpi_tensorflow_amd import config as C

    ck = str(tmp_path / "c.npz")
    cfg = C.config_from_args(["--model", "resnet18", "--dtype", "bf16", "--resume", ck,
                              "--predict", "test", "--predict-topk", "5"])
    assert (cfg.model, cfg.predict, cfg.dtype) == ("resnet18", "test", "bf16")
    C.TrainConfig(model="resnet18", predict="test", resume=ck, device="cpu").validate()
    with pytest.raises(ValueError, match="--dtype bf16"):
        C.TrainConfig(model="resnet18", predict="test", resume=ck).validate()
    with pytest.raises(ValueError, match="resnet18.*BatchNorm"):
        C.config_from_args(["--model", "resnet18", "--ema", "0.999"])


def test_predict_test_is_the_trainers_test_shard():
    import numpy as np

    from mpi_tensorflow_amd import config as C
    from mpi_tensorflow_amd.runtime.predict import load_source
    from mpi_tensorflow_amd.utils.data import synthetic_images_torch

    cfg = C.TrainConfig(model="resnet18", dtype="bf16", resume="c.npz", predict="test", seed=3)
    n, a, x, y, _ = load_source(cfg, rank=1, world=2)
    per = C.RESNET_SYNTH_ROWS[1]  # as Trainer generates rank 1's test rows
    tx, ty = synthetic_images_torch(per, (224, 224, 3), seed=3, split="test", start=per)
    assert (n, a) == (2 * per, per) and np.array_equal(x, tx.numpy()) and np.array_equal(y, ty.numpy())


def test_torch_predictor_reads_the_batchnorm_statistics(tmp_path):
    from mpi_tensorflow_amd.ops import functional as Fn
    from mpi_tensorflow_amd.runtime.predict import Predictor
    from mpi_tensorflow_amd.utils import checkpoint as ck

    model, params, bn = _resnet_state()
    extra = {}
    for name, (rm, rv) in bn.items():
        extra[name + "/moving_mean"], extra[name + "/moving_variance"] = rm, rv
    path = str(tmp_path / "r18.npz")
    ck.save(path, model.layout, params, torch.zeros_like(params), 7, meta={"model": "resnet18"},
            extra=extra)
    pr = Predictor.from_checkpoint(path, device="cpu")
    assert (pr.model, pr.backend, pr.dtype, pr.step) == ("resnet18", "torch", "fp32", 7)
    x = torch.randn(2, 224, 224, 3, generator=torch.Generator().manual_seed(1))
    pv = model.layout.views(params)
    P = {s.name: Fn.Param(pv[s.name], None) for s in model.layout.specs}
    with torch.no_grad(), Fn.oracle_mode():
        ref = model.forward(P, bn, x, False)
        plain = model.forward(P, model.make_bn_state("cpu"), x, False)
    got = pr.predict(x.numpy(), topk=2).scores
    assert torch.equal(got, ref)
    assert not torch.equal(got, plain)  # the statistics are in the result
    with pytest.raises(NotImplementedError, match="bf16"):
        Predictor.from_checkpoint(path, device="cpu", dtype="bf16")
    del extra["l3b0nd/moving_variance"]
    ck.save(path, model.layout, params, torch.zeros_like(params), 7, meta={"model": "resnet18"},
            extra=extra)
    with pytest.raises(ValueError, match="l3b0nd/moving_variance"):
        Predictor.from_checkpoint(path, device="cpu")
