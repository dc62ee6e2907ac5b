"""--ema on the CPU: the spec parser, the torch implementation of
Fn.ema_update against hand-worked rows, the torch engines against the float64
recurrence (tests/helpers/ema_ref.py has the definition and the derived
bound), checkpoint save / resume, the command line with its metrics records
and --predict-weights, two gloo ranks, and the validation errors.

Definition: config.parse_ema, ops/functional.py ema_update, docs/ACCURACY.md
(TF1's tf.train.ExponentialMovingAverage with num_updates, the companion of
the reference's MomentumOptimizer, /root/reference/mpipy.py:59-66)."""

import importlib.util
import json
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.ops import functional as Fn
from mpi_tensorflow_amd.runtime.mnist_engine import TorchMnistEngine
from mpi_tensorflow_amd.utils import checkpoint as ckpt
from mpi_tensorflow_amd.utils.data import synthetic_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("ema_ref")
CPU = torch.device("cpu")


# ------------------------------------------------------------------ 1: spec --
def test_parse_ema_accepts_the_spec_in_either_order():
    assert C.parse_ema("0.999") == (0.999, 1)
    assert C.parse_ema("0.99,every:4") == (0.99, 4)
    assert C.parse_ema("every:4,0.99") == (0.99, 4)
    assert C.parse_ema(" 0.5 , every:1 ") == (0.5, 1)


@pytest.mark.parametrize("spec", ["0", "1", "-0.1", "nan", "0.9,every:0", "0.9,0.8",
                                  "0.9,every:2,every:3", "0.9,warm", "0.9,span:3", "every:2", "",
                                  "0.9,every:1.5", "1.5"])
def test_parse_ema_rejects(spec):
    with pytest.raises(ValueError, match="ema"):
        C.parse_ema(spec)
    with pytest.raises(ValueError):
        C.TrainConfig(ema=spec).validate()


# ------------------------------------------------------------ 2: the oracle --
def _rows():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(64, generator=g) * 0.3 + 0.1
    e = torch.randn(64, generator=g) * 0.2 - 0.4
    return w, e


def _f32(x):
    return float(np.float32(x))


def test_oracle_hand_worked_rows():
    w, e0 = _rows()
    # t = 1: u = 0, d = 1 / 10 whatever DECAY >= 0.1
    for decay in (0.1, 0.5, 0.999):
        assert Fn.ema_decay(1, decay) == _f32(np.float32(1) / np.float32(10))
        e = e0.clone()
        assert Fn.ema_update(e, w, 1, decay) is e
        want = e0.double() + (1.0 - 0.1) * (w.double() - e0.double())
        R.assert_within(e, want, R.ONE_UPDATE * torch.maximum(w.abs(), e0.abs()).double(),
                        f"t = 1, decay {decay}")
    # t = 10^6: (1 + u) / (10 + u) is past any DECAY < 0.99999
    assert Fn.ema_decay(10 ** 6, 0.999) == _f32(0.999)
    e = e0.clone()
    Fn.ema_update(e, w, 10 ** 6, 0.999)
    want = e0.double() + (1.0 - _f32(0.999)) * (w.double() - e0.double())
    R.assert_within(e, want, R.ONE_UPDATE * torch.maximum(w.abs(), e0.abs()).double(), "t = 10^6")
    # a decay below the warm-up value wins at once
    assert Fn.ema_decay(1, 0.05) == _f32(0.05)


def test_oracle_every_k_skips_and_counts_updates():
    w, e0 = _rows()
    e = e0.clone()
    Fn.ema_update(e, w, 5, 0.9, 4)  # 5 % 4 != 0
    assert torch.equal(e, e0) and Fn.ema_decay(5, 0.9, 4) is None
    Fn.ema_update(e, w, torch.tensor([8]), 0.9, 4)  # u = 8 / 4 - 1 = 1: d = 2 / 11
    assert Fn.ema_decay(8, 0.9, 4) == _f32(np.float32(2) / np.float32(11))
    want = e0.double() + (1.0 - 2.0 / 11.0) * (w.double() - e0.double())
    R.assert_within(e, want, R.ONE_UPDATE * torch.maximum(w.abs(), e0.abs()).double(), "K = 4, t = 8")
    assert not torch.equal(e, e0)
    # the float64 reference agrees with itself on the same rows
    assert R.decay64(5, 0.9, 4) is None and R.decay64(8, 0.9, 4) == 2.0 / 11.0
    with pytest.raises(ValueError):
        Fn.ema_update(e, w[:32], 1, 0.9)
    with pytest.raises(ValueError):
        Fn.ema_update(e, w, 1, 0.9, 0)


# ----------------------------------------------------------- 3: torch engine --
def _cfg(**kw):
    kw.setdefault("batch_size", 8)
    kw.setdefault("device", "cpu")
    kw.setdefault("backend", "torch")
    return C.TrainConfig(**kw).validate()


@pytest.fixture(scope="module")
def shard24():
    return synthetic_rows("train", 0, 24)


@pytest.fixture(scope="module")
def seven_steps(shard24):
    """Seven train(1) calls with --ema 0.9: (initial params, params after each, ema)."""
    eng = TorchMnistEngine(_cfg(ema="0.9"), *shard24, CPU)
    p0 = eng.params.clone()
    assert torch.equal(eng.ema, p0) and eng.ema.data_ptr() != eng.params.data_ptr()
    rec = []
    for _ in range(7):
        eng.train(1)
        rec.append(eng.params.clone())
    return p0, rec, eng.ema.clone()


def test_engine_without_the_flag_keeps_no_average(shard24):
    eng = TorchMnistEngine(_cfg(), *shard24, CPU)
    eng.train(1)
    assert eng.ema is None


def test_torch_engine_follows_the_recurrence(seven_steps):
    p0, rec, ema = seven_steps
    want, bound = R.recurrence(p0, rec, 0.9)
    R.assert_within(ema, want, bound, "TorchMnistEngine, 7 steps, --ema 0.9")
    assert not torch.equal(ema, p0) and not torch.equal(ema, rec[-1])


def test_torch_engine_one_call_of_seven_is_bit_identical(shard24, seven_steps):
    _, rec, ema = seven_steps
    eng = TorchMnistEngine(_cfg(ema="0.9"), *shard24, CPU)
    eng.train(7)
    assert torch.equal(eng.params, rec[-1]) and torch.equal(eng.ema, ema)


def test_torch_engine_every_two_waits_for_the_second_step(shard24, seven_steps):
    p0, rec, _ = seven_steps
    eng = TorchMnistEngine(_cfg(ema="0.9,every:2"), *shard24, CPU)
    eng.train(1)
    assert torch.equal(eng.ema, p0)
    eng.train(3)
    want, bound = R.recurrence(p0, rec[:4], 0.9, K=2)
    R.assert_within(eng.ema, want, bound, "every:2, 4 steps")


def test_lenet5_torch_path_follows_the_recurrence():
    from mpi_tensorflow_amd.runtime.generic_engine import make_image_engine

    x, y = synthetic_rows("train", 0, 24, shape=(32, 32, 3))
    eng = make_image_engine(_cfg(model="lenet5", ema="0.9"), x, y, CPU)
    p0 = eng.params.detach().clone()
    assert torch.equal(eng.ema, p0) and not eng.ema.requires_grad
    rec = []
    for _ in range(3):
        eng.train(1)
        rec.append(eng.params.detach().clone())
    want, bound = R.recurrence(p0, rec, 0.9)
    R.assert_within(eng.ema, want, bound, "LeNet-5 torch path, 3 steps")
    assert not torch.equal(eng.ema, p0)


# ------------------------------------------------------------- 4: checkpoint --
def _trainer(tmp_path, **kw):
    from mpi_tensorflow_amd.runtime.trainer import Trainer

    kw.setdefault("synthetic", True)
    kw.setdefault("quiet", True)
    tr = Trainer(_cfg(**kw))
    return tr


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    """train(3) with and without --ema, saved; and train(6) in one go."""
    d = tmp_path_factory.mktemp("ema_ckpt")
    with_ema, plain = str(d / "ema.npz"), str(d / "plain.npz")
    tr = _trainer(d, ema="0.9")
    tr.engine.train(3)
    tr.save_checkpoint(with_ema)
    tr.engine.train(3)
    six = (tr.engine.params.clone(), tr.engine.mom.clone(), tr.engine.ema.clone())
    tr.watchdog.stop()
    tp = _trainer(d)
    tp.engine.train(3)
    tp.save_checkpoint(plain)
    tp.watchdog.stop()
    return with_ema, plain, six


def test_checkpoint_key_names(ckpts):
    from mpi_tensorflow_amd.models import mnist_cnn as M

    with_ema, plain, _ = ckpts
    names = [s.tf_name for s in M.layout().specs]
    with np.load(with_ema, allow_pickle=False) as z:
        for n, s in zip(names, M.layout().specs):
            key = n + "/ExponentialMovingAverage"
            assert key in z.files and z[key].shape == tuple(s.shape) and z[key].dtype == np.float32
        assert str(z["__meta__/ema"]) == "0.9"
        assert not np.array_equal(z["Variable_4/ExponentialMovingAverage"], z["Variable_4"])
    with np.load(plain, allow_pickle=False) as z:
        assert not [k for k in z.files if "ExponentialMovingAverage" in k or k == "__meta__/ema"]


def test_resume_continues_the_same_sequence(tmp_path, ckpts):
    with_ema, _, (p6, m6, e6) = ckpts
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tr = _trainer(tmp_path, ema="0.9", resume=with_ema)
    assert tr.engine.step == 3 and not torch.equal(tr.engine.ema, tr.engine.params)
    tr.engine.train(3)
    tr.watchdog.stop()
    assert torch.equal(tr.engine.params, p6) and torch.equal(tr.engine.mom, m6)
    assert torch.equal(tr.engine.ema, e6)


def test_resume_from_a_checkpoint_without_the_average_warns(tmp_path, ckpts):
    _, plain, _ = ckpts
    with pytest.warns(UserWarning, match="no moving average"):
        tr = _trainer(tmp_path, ema="0.9", resume=plain)
    tr.watchdog.stop()
    assert torch.equal(tr.engine.ema, tr.engine.params)
    assert tr.engine.ema.data_ptr() != tr.engine.params.data_ptr()


def test_resume_with_another_spec_warns_and_without_the_flag_ignores(tmp_path, ckpts):
    with_ema, _, _ = ckpts
    with pytest.warns(UserWarning, match="saved ema=0.9"):
        tr = _trainer(tmp_path, ema="0.99,every:2", resume=with_ema)
    tr.watchdog.stop()
    with np.load(with_ema, allow_pickle=False) as z:
        saved = torch.from_numpy(z["Variable_4/ExponentialMovingAverage"])
    assert torch.equal(tr.engine.layout.views(tr.engine.ema)["fc1_weight"], saved)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tp = _trainer(tmp_path, resume=with_ema)
    tp.watchdog.stop()
    assert tp.engine.ema is None and tp.engine.step == 3


def test_load_ema_reports_a_partial_set(tmp_path, ckpts):
    from mpi_tensorflow_amd.models import mnist_cnn as M

    with_ema, plain, _ = ckpts
    buf = torch.zeros(M.layout().total)
    assert ckpt.load_ema(plain, M.layout(), buf) == (False, None) and float(buf.abs().sum()) == 0.0
    assert ckpt.load_ema(with_ema, M.layout(), buf) == (True, "0.9") and float(buf.abs().sum()) > 0
    with np.load(with_ema, allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files if k != "Variable_7/ExponentialMovingAverage"}
    broken = str(tmp_path / "broken.npz")
    np.savez(broken, **arrays)
    with pytest.raises(ValueError, match="Variable_7/ExponentialMovingAverage"):
        ckpt.load_ema(broken, M.layout(), buf)


# ------------------------------------------------------------ 5: command line --
def _mpipy(*args, timeout=600):
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="",
               HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, "mpipy.py", "--synthetic", "--backend", "torch", "--device", "cpu", *args]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def _json_line(out, key):
    return json.loads([ln for ln in out.splitlines() if ln.startswith('{"%s"' % key)][-1])[key]


def _records(path):
    with open(path) as f:
        return [json.loads(ln) for ln in f if ln.strip()]


def test_cli_reports_saves_and_predicts_the_average(tmp_path):
    ck, mj, mj0 = str(tmp_path / "c.npz"), str(tmp_path / "m.jsonl"), str(tmp_path / "m0.jsonl")
    # (one logged eval event at step 2, then the final one at step 3)
    common = ("--batch-size", "8", "--max-steps", "4", "--eval-every", "2")
    out = _mpipy(*common, "--ema", "0.99", "--metrics-jsonl", mj, "--ckpt", ck)
    recs = _records(mj)
    events = [r for r in recs if not r.get("final")]
    assert [r["step"] for r in events] == [2] and "ema_test_error" in events[0]
    assert "ema_test_loss" not in events[0]  # (--eval-metrics adds those)
    assert "[ema] step 2: test error %.2f%%" % events[0]["ema_test_error"] in out
    # the reference's own log line is what it always was
    assert "0  process at  2 with test error: " in out
    final = recs[-1]
    assert final["final"] and final["ema_test_error"] == final["final_ema_test_error_local"]
    assert final["final_ema_test_error_global"] == pytest.approx(
        final["final_ema_test_error_local"], abs=1e-9)  # world 1
    summ = _json_line(out, "summary")
    assert summ["final_ema_test_error_local"] == final["final_ema_test_error_local"]
    # the same run without the flag has neither key
    out0 = _mpipy(*common, "--metrics-jsonl", mj0)
    for r in _records(mj0):
        assert r.get("ema_test_error") is None and r.get("final_ema_test_error_local") is None
    assert "[ema]" not in out0
    assert _json_line(out0, "summary").get("final_ema_test_error_local") is None
    assert _records(mj0)[-1]["final_test_error_local"] == final["final_test_error_local"]
    # --predict on the checkpoint: the average and the raw weights
    pe = _json_line(_mpipy("--resume", ck, "--predict", "test", "--predict-weights", "ema"),
                    "predict")
    assert pe["weights"] == "ema" and pe["error"] == final["final_ema_test_error_local"]
    pr = _json_line(_mpipy("--resume", ck, "--predict", "test", "--predict-weights", "raw"),
                    "predict")
    assert pr["weights"] == "raw" and pr["error"] == final["final_test_error_local"]
    assert pe["confusion"] != pr["confusion"]


def test_trainer_eval_metrics_adds_the_global_keys(tmp_path):
    mj = str(tmp_path / "m.jsonl")
    tr = _trainer(tmp_path, ema="0.9,every:2", eval_metrics=True, max_steps=2, eval_every=0,
                  metrics_jsonl=mj, check_replicas=True)
    summ = tr.run()
    final = _records(mj)[-1]
    for key in ("ema_test_error", "ema_test_loss", "ema_test_error_global", "ema_val_error",
                "ema_val_loss"):
        assert isinstance(final[key], float), key
    assert final["ema_test_error_global"] == final["ema_test_error"]  # world 1
    assert summ.final_ema_test_error_local == final["ema_test_error"]
    assert summ.as_dict()["final_ema_test_error_global"] == pytest.approx(final["ema_test_error"],
                                                                         abs=1e-9)
    # the average is evaluated by a Predictor on engine.ema itself, kept for the next event
    pred = tr._ema_predictor["test"]
    assert pred.weights == "ema" and pred.params.data_ptr() == tr.engine.ema.data_ptr()
    tr._ema_event(1, True)
    assert tr._ema_predictor["test"] is pred


# --------------------------------------------------------- 6: two gloo ranks --
def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker_ema(rank, world, port, out_dir, steps):
    torch.set_num_threads(2)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    for k in ("OMPI_COMM_WORLD_RANK", "PMI_RANK", "SLURM_PROCID"):
        os.environ.pop(k, None)
    from mpi_tensorflow_amd.parallel import dist as D
    from mpi_tensorflow_amd.parallel.comm import make_comm
    from mpi_tensorflow_amd.parallel.sync import replicas_identical

    di = D.init("cpu")
    comm = make_comm(di, CPU)
    x, y = synthetic_rows("train", rank * 24, (rank + 1) * 24)
    eng = TorchMnistEngine(_cfg(ema="0.9"), x, y, CPU, rank, world, comm)
    assert eng.grad_sync
    eng.train(steps)
    same = replicas_identical(eng.ema) and replicas_identical(eng.params)
    np.save(os.path.join(out_dir, f"e{rank}.npy"), eng.ema.numpy())
    np.save(os.path.join(out_dir, f"p{rank}.npy"), eng.params.numpy())
    with open(os.path.join(out_dir, f"same{rank}"), "w") as f:
        f.write(str(same))
    D.shutdown()


def test_two_ranks_grad_sync_keep_the_average_identical(tmp_path):
    world, port = 2, _free_port()
    mp.spawn(_worker_ema, args=(world, port, str(tmp_path), 3), nprocs=world, join=True)
    e0, e1 = np.load(tmp_path / "e0.npy"), np.load(tmp_path / "e1.npy")
    assert np.array_equal(e0, e1), "the averages diverged under per-step gradient all-reduce"
    assert np.array_equal(np.load(tmp_path / "p0.npy"), np.load(tmp_path / "p1.npy"))
    assert not np.array_equal(e0, np.load(tmp_path / "p0.npy"))
    assert open(tmp_path / "same0").read() == "True" and open(tmp_path / "same1").read() == "True"


# -------------------------------------------------------------- 7: validation --
def test_ema_rejects_resnet18():
    with pytest.raises(ValueError, match="resnet18.*BatchNorm"):
        C.TrainConfig(model="resnet18", ema="0.999").validate()
    with pytest.raises(ValueError, match="resnet18"):
        C.config_from_args(["--model", "resnet18", "--ema", "0.999"])
    assert C.config_from_args(["--model", "lenet5", "--ema", "0.999,every:2"]).ema == "0.999,every:2"


def test_predict_weights_needs_predict_and_the_arrays(ckpts):
    from mpi_tensorflow_amd.runtime.predict import Predictor

    with_ema, plain, _ = ckpts
    for w in ("raw", "ema"):
        with pytest.raises(ValueError, match="--predict-weights needs --predict"):
            C.TrainConfig(predict_weights=w).validate()
    with pytest.raises(ValueError, match="predict weights"):
        C.TrainConfig(predict="test", resume=plain, predict_weights="mean").validate()
    with pytest.raises(ValueError, match=r"missing Variable(_\d)?/ExponentialMovingAverage"):
        Predictor.from_checkpoint(plain, device="cpu", weights="ema")
    with pytest.raises(ValueError, match="weights"):
        Predictor.from_checkpoint(with_ema, device="cpu", weights="mean")
    pe = Predictor.from_checkpoint(with_ema, device="cpu", weights="ema")
    pr = Predictor.from_checkpoint(with_ema, device="cpu")
    assert (pe.weights, pr.weights) == ("ema", "raw") and not torch.equal(pe.params, pr.params)
    with np.load(with_ema, allow_pickle=False) as z:
        assert torch.equal(pe.layout.views(pe.params)["fc2_bias"],
                           torch.from_numpy(z["Variable_7/ExponentialMovingAverage"]))
    # the command line reports the missing key too
    from mpi_tensorflow_amd.runtime.predict import predict_main

    cfg = C.TrainConfig(device="cpu", backend="torch", synthetic=True, resume=plain, predict="val",
                        predict_weights="ema")
    with pytest.raises(ValueError, match="ExponentialMovingAverage.*without --ema"):
        predict_main(cfg)


def test_predictor_from_engine_shares_the_average(shard24):
    from mpi_tensorflow_amd.runtime.predict import Predictor

    eng = TorchMnistEngine(_cfg(ema="0.9"), *shard24, CPU)
    eng.train(2)
    pe = Predictor.from_engine(eng, weights="ema")
    assert pe.params.data_ptr() == eng.ema.data_ptr() and pe.backend == "torch"
    x, y = synthetic_rows("test", 0, 40)
    m1 = pe.evaluate(x, y)
    m2 = pe.predict(x, labels=y).metrics
    assert m1.error == m2.error and m1.loss == m2.loss and m1.n == 40
    plain = TorchMnistEngine(_cfg(), *shard24, CPU)
    with pytest.raises(ValueError, match="without --ema"):
        Predictor.from_engine(plain, weights="ema")
