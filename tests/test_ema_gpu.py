"""--ema on the GPU: the ema.hip kernel against the float64 definition, the
native engines (MNIST fp32 / bf16, LeNet-5) against the float64 recurrence
and graph replay against eager launches, the discarded steps of the sync tune
and the pre-warm, the Trainer's evaluation of the average, and two ranks under
every gradient-sync schedule (tests/helpers/ema_sync_ranks.py).

tests/helpers/ema_ref.py has the definition and the derived bound: one update
within 2^-21 max(|w|, |ema|) per element, k updates within k times that.

The kernel is held to the bound only, not to bit equality with the torch path
of Fn.ema_update: that path forms the fma as an exact float64 product and sum
rounded to float32, which differs from the kernel's single rounding wherever
the float64 sum lands on a float32 rounding tie (rare, but not never)."""

import importlib.util
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.ops import functional as Fn
from mpi_tensorflow_amd.utils.data import synthetic_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HERE = os.path.dirname(os.path.abspath(__file__))
HELPER = os.path.join(ROOT, "tests", "helpers", "ema_sync_ranks.py")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("ema_ref")

TAIL = 64  # poisoned floats behind each buffer
POISON = 0x7FC0DEAD  # a NaN no arithmetic produces
SWEEP = 2048 * 256 * 4  # floats one pass of the capped grid covers


# ---------------------------------------------------------------- 1: kernel --
def _buffers(n, dev, seed):
    """(w, ema) of n floats on asymmetric random data, each the head of a
    buffer whose TAIL floats behind it hold POISON."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, generator=g) * 0.3 + 0.1
    e = torch.randn(n, generator=g) * 0.02 - 0.4
    out = []
    for t in (w, e):
        buf = torch.empty(n + TAIL, device=dev)
        buf[n:].view(torch.int32).fill_(POISON)
        buf[:n].copy_(t)
        out.append(buf)
    return out


def _tail_ok(buf, n):
    return bool((buf[n:].view(torch.int32) == POISON).all())


@pytest.mark.parametrize("n", [4, 1008, 1024, SWEEP + 1028])
@pytest.mark.parametrize("step_on_device", [True, False])
def test_kernel_matches_the_definition(cuda_dev, n, step_on_device):
    wb, eb = _buffers(n, cuda_dev, 3 + n % 7)
    w0, e0 = wb[:n].clone().cpu(), eb[:n].clone().cpu()
    M = torch.maximum(w0.abs(), e0.abs()).double()

    def step(t):
        return torch.tensor([t], dtype=torch.int64, device=cuda_dev) if step_on_device else t

    # t = 5 with K = 4: nothing happens
    Fn.ema_update(eb[:n], wb[:n], step(5), 0.9, 4)
    torch.cuda.synchronize()
    assert torch.equal(eb[:n].cpu(), e0), "K = 4, t = 5 changed the average"
    # t = 8 with K = 4 (u = 1, d = 2 / 11), t = 1 (d = 0.1) and t = 10^6 (d = DECAY),
    # each from the same start
    for t, decay, K, d in ((8, 0.9, 4, 2.0 / 11.0), (1, 0.999, 1, 0.1),
                           (10 ** 6, 0.999, 1, float(np.float32(0.999)))):
        assert R.decay64(t, decay, K) == d
        eb[:n].copy_(e0)
        Fn.ema_update(eb[:n], wb[:n], step(t), decay, K)
        torch.cuda.synchronize()
        want = R.update64(e0.double(), w0, t, decay, K)
        R.assert_within(eb[:n], want, R.ONE_UPDATE * M, f"n = {n}, t = {t}, K = {K}")
        assert not torch.equal(eb[:n].cpu(), e0)
        assert torch.equal(wb[:n].cpu(), w0), "the kernel wrote the weights"
        assert _tail_ok(eb, n) and _tail_ok(wb, n), "the kernel wrote past the buffer"


def test_kernel_rejects_a_length_that_is_no_multiple_of_four(cuda_dev):
    w, e = torch.ones(6, device=cuda_dev), torch.zeros(6, device=cuda_dev)
    with pytest.raises(RuntimeError, match="n % 4"):
        Fn.ema_update(e, w, 1, 0.9)
    torch.cuda.synchronize()
    assert float(e.abs().sum()) == 0.0


# --------------------------------------------------------------- 2: engines --
def _engine(kind, dev, **kw):
    """A native engine on a 96-row synthetic shard, B = 32."""
    kw.setdefault("batch_size", 32)
    if kind == "lenet5":
        from mpi_tensorflow_amd.runtime.lenet_engine import NativeLenetEngine

        x, y = synthetic_rows("train", 0, 96, shape=(32, 32, 3))
        return NativeLenetEngine(C.TrainConfig(model="lenet5", **kw).validate(), x, y, dev)
    from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine

    x, y = synthetic_rows("train", 0, 96)
    return NativeMnistEngine(C.TrainConfig(dtype=kind, **kw).validate(), x, y, dev)


@pytest.mark.parametrize("kind", ["fp32", "bf16", "lenet5"])
def test_native_engine_follows_the_recurrence_and_replays_it(cuda_dev, kind):
    eng = _engine(kind, cuda_dev, graph=False, ema="0.9")
    p0 = eng.params.clone()
    assert torch.equal(eng.ema, p0) and eng.ema.data_ptr() != eng.params.data_ptr()
    rec = []
    for _ in range(7):  # eager single steps
        eng.train(1)
        torch.cuda.synchronize()
        rec.append(eng.params.clone())
    want, bound = R.recurrence(p0, rec, 0.9)
    R.assert_within(eng.ema, want, bound, f"{kind}: 7 eager steps, --ema 0.9")
    assert not torch.equal(eng.ema, p0) and not torch.equal(eng.ema, rec[-1])
    # graphs of 3, 3 and 1 steps from the same start
    rep = _engine(kind, cuda_dev, graph=True, graph_steps=3, ema="0.9")
    rep.train(7)
    torch.cuda.synchronize()
    assert rep.use_graph and len(rep._graphs) == 2, "expected the 3-step and the 1-step graph"
    assert torch.equal(rep.params, rec[-1]), "graph replay: other parameters than eager"
    assert torch.equal(rep.ema, eng.ema), "graph replay: another average than eager"
    # every:2 leaves the first step alone
    two = _engine(kind, cuda_dev, graph=False, ema="0.9,every:2")
    two.train(1)
    torch.cuda.synchronize()
    assert torch.equal(two.ema, p0) and torch.equal(two.params, rec[0])
    two.train(1)
    torch.cuda.synchronize()
    want2, bound2 = R.recurrence(p0, rec[:2], 0.9, K=2)
    R.assert_within(two.ema, want2, bound2, f"{kind}: every:2 after 2 steps")
    assert not torch.equal(two.ema, p0)


def test_engine_without_the_flag_allocates_and_launches_nothing(cuda_dev):
    eng = _engine("fp32", cuda_dev, graph=False)
    eng.train(1)
    assert eng.ema is None


# ------------------------------------------------- 3: discarded trial steps --
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_tune_and_prewarm_leave_the_average_alone(cuda_dev, dtype):
    from mpi_tensorflow_amd.parallel.comm import EmulatedDeviceComm
    from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine

    x, y = synthetic_rows("train", 0, 256)
    comm = EmulatedDeviceComm(8, lat_us=10.0, busbw_gbps=150.0, blocks=32)
    cfg = C.TrainConfig(dtype=dtype, graph=True, graph_steps=2, ema="0.9").validate()
    eng = NativeMnistEngine(cfg, x, y, cuda_dev, comm=comm, force_sync=True)
    e0, p0 = eng.ema.clone(), eng.params.clone()
    assert eng.tune_schedule() > 0  # (before the first step, as in a run)
    torch.cuda.synchronize()
    # the candidates whose FC update ends on the comm stream were timed, with the average
    want = {"buckets", "serial", "sharded"} | ({"factors", "defer"} if dtype == "fp32" else set())
    assert set(eng.tune_log) == want and all(v is not None for v in eng.tune_log.values()), eng.tune_log
    assert torch.equal(eng.ema, e0) and torch.equal(eng.params, p0)
    assert eng.step == int(eng.step_dev.item()) == 0
    assert eng.prewarm_train(1.0) > 0
    torch.cuda.synchronize()
    assert torch.equal(eng.ema, e0) and torch.equal(eng.params, p0)
    assert int(eng.step_dev.item()) == 0
    eng.train(2)
    torch.cuda.synchronize()
    assert not torch.equal(eng.ema, e0) and int(eng.step_dev.item()) == 2
    # a tune after steps restores an average that is no longer the parameters
    eng._tuned = False
    e2 = eng.ema.clone()
    assert not torch.equal(e2, eng.params)
    assert eng.tune_schedule() > 0
    torch.cuda.synchronize()
    assert torch.equal(eng.ema, e2) and int(eng.step_dev.item()) == 2


def test_lenet_tune_leaves_the_average_alone(cuda_dev):
    from mpi_tensorflow_amd.parallel.comm import EmulatedDeviceComm, XgmiDeviceComm
    from mpi_tensorflow_amd.runtime.lenet_engine import NativeLenetEngine

    x, y = synthetic_rows("train", 0, 256, shape=(32, 32, 3))
    comm = EmulatedDeviceComm(8, lat_us=10.0, busbw_gbps=150.0, blocks=32)
    xc = XgmiDeviceComm.emulated(8, lat_us=2.0, link_gbps=64.0)
    cfg = C.TrainConfig(model="lenet5", graph=True, graph_steps=2, ema="0.9").validate()
    eng = NativeLenetEngine(cfg, x, y, cuda_dev, comm=comm, force_sync=True, xcomm=xc)
    eng.train(2)  # (tunes first; then the average differs from the parameters)
    torch.cuda.synchronize()
    assert eng.tune_log and int(eng.step_dev.item()) == 2
    e2, p2 = eng.ema.clone(), eng.params.clone()
    assert not torch.equal(e2, p2)
    eng._tuned = False
    assert eng.tune_schedule() > 0
    torch.cuda.synchronize()
    assert torch.equal(eng.ema, e2) and torch.equal(eng.params, p2)
    assert int(eng.step_dev.item()) == 2


# --------------------------------------------------------------- 4: trainer --
def test_trainer_evaluates_the_saved_average_without_new_buffers(cuda_dev, tmp_path):
    from mpi_tensorflow_amd.runtime.predict import Predictor
    from mpi_tensorflow_amd.runtime.trainer import Trainer

    ck, mj = str(tmp_path / "c.npz"), str(tmp_path / "m.jsonl")
    cfg = C.TrainConfig(synthetic=True, quiet=True, ema="0.9", eval_metrics=True, max_steps=4,
                        eval_every=2, graph_steps=2, ckpt=ck, metrics_jsonl=mj).validate()
    tr = Trainer(cfg)
    assert tr.engine.kind == "native"
    summ = tr.run()
    with open(mj) as f:
        recs = [json.loads(ln) for ln in f if ln.strip()]
    assert [r.get("step") for r in recs if not r.get("final")] == [2]
    final = recs[-1]
    for r in recs:
        for key in ("ema_test_error", "ema_test_loss", "ema_test_error_global", "ema_val_error",
                    "ema_val_loss"):
            assert isinstance(r[key], float), key
    assert summ.final_ema_test_error_local == final["ema_test_error"]
    # (wrong / n from the summed counts against 100 (err n / 100) / n: one rounding apart)
    assert summ.final_ema_test_error_global == pytest.approx(final["ema_test_error_global"], abs=1e-9)
    # the checkpoint's average gives the same error on the same split
    pe = Predictor.from_checkpoint(ck, device=cuda_dev, weights="ema")
    assert torch.equal(pe.params, tr.engine.ema)
    got = pe.predict(tr.shard.test_x, labels=tr.shard.test_y).metrics
    print(f"ema test error {final['ema_test_error']} (raw {final['final_test_error_local']}), "
          f"from the checkpoint {got.error}")
    assert got.error == final["ema_test_error"]
    assert got.loss == pytest.approx(final["ema_test_loss"], rel=1e-9)
    raw = Predictor.from_checkpoint(ck, device=cuda_dev).predict(tr.shard.test_x,
                                                                labels=tr.shard.test_y).metrics
    assert raw.error == final["final_test_error_local"]
    # a later eval event reuses the Predictor, its workspaces and its result buffers
    pred = tr._ema_predictor["test"]
    assert pred.params.data_ptr() == tr.engine.ema.data_ptr() and pred.backend == "native"
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(cuda_dev)["allocation.all.allocated"]
    rec, _ = tr._ema_event(3, True)
    torch.cuda.synchronize()
    after = torch.cuda.memory_stats(cuda_dev)["allocation.all.allocated"]
    assert after == before, f"{after - before} device allocations in a repeated ema evaluation"
    assert tr._ema_predictor["test"] is pred and rec["ema_test_error"] == final["ema_test_error"]


# ------------------------------------------------------------- 5: two ranks --
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(*args, timeout=240):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), HELPER] + list(args)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_ranks_every_shm_schedule(dtype):
    """buckets, sharded, split, serial (fp32: + factors, defer) over the
    shared-memory communicator, captured."""
    out = _run("mnist", dtype)
    assert f"EMA_SYNC_OK mnist {dtype} world=2" in out, out[-2000:]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_ranks_every_xgmi_schedule(dtype):
    """xgmi, serial (fp32: + xgmi-step, xgmi-fac) over the peer-to-peer communicator."""
    out = _run("xgmi", dtype)
    assert f"EMA_SYNC_OK xgmi {dtype} world=2" in out, out[-2000:]


@pytest.mark.parametrize("kind", ["shm", "xgmi", "xgmipush", "xgmipull"])
def test_two_ranks_lenet5(kind):
    out = _run("lenet", kind)
    assert f"EMA_SYNC_OK lenet {kind} world=2" in out, out[-2000:]
