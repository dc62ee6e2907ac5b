"""The native MNIST engine at batch sizes that are no multiple of 32.

The fused kernels tile the batch in groups of 32 images, so the step runs on
Bp = ceil(B / 32) * 32 rows; the head kernel seeds the backward pass with
exact zeros for the Bp - B pad rows, and everything the model defines in terms
of the batch (offset, LR epoch, the 1 / B of the mean loss) uses the logical
B.  Each test compares against the plain-PyTorch fp32 oracle
(`TorchMnistEngine`), which has no notion of padding, or against a second
native run bit for bit.  Tolerances are the ones the multiple-of-32 tests
already use (tests/test_native_mnist_gpu.py, tests/test_mnist_bf16_gpu.py).
"""

import math

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.runtime.mnist_engine import (XGMI_STEP_RTOL, NativeMnistEngine,
                                                     TorchMnistEngine)
from mpi_tensorflow_amd.utils.data import batch_offset, synthetic_rows

pytestmark = pytest.mark.gpu


def _rel(a, b):  # as tests/test_native_mnist_gpu.py
    return (a - b).abs().max().item() / max(1e-6, b.abs().max().item())


def _nrel(a, b):  # as tests/test_mnist_bf16_gpu.py
    return ((a.float() - b.float()).norm() / max(1e-12, b.float().norm())).item()


@pytest.fixture(scope="module")
def data():
    return synthetic_rows("train", 0, 1024)


def _cfg(**kw):
    return C.TrainConfig(graph=kw.pop("graph", False), **kw).validate()


def _check_grads_fp32(nat, ref, step):
    """One native forward + backward at `step` against the oracle's, with the
    bounds of test_forward_backward_grads_match_oracle."""
    nat.set_step(step)
    ref.set_step(step)
    nat.forward_backward_only()
    ref.forward_backward(step)
    torch.cuda.synchronize()
    loss = nat.bufs["loss_rows"][:nat.B].sum().item() / nat.B
    nv, rv = nat.layout.views(nat.grads), ref.layout.views(ref.grads)
    errs = {s.name: _rel(nv[s.name], rv[s.name]) for s in nat.layout.specs}
    print(f"B={nat.B} step={step} loss={loss:.6f} ref={ref.last_loss:.6f}",
          {k: f"{v:.1e}" for k, v in errs.items()})
    assert abs(loss - ref.last_loss) < 1e-4
    for name, err in errs.items():
        assert err < 2e-4, (name, err)


@pytest.mark.parametrize("algo", ["winograd", "direct"])
@pytest.mark.parametrize("batch", [1, 33, 50, 100])
def test_grads_match_oracle_any_batch(cuda_dev, data, batch, algo):
    """Bp = 32, 64, 64, 128: a single valid row, the largest pad, and two
    ordinary sizes."""
    x, y = data
    cfg = _cfg(batch_size=batch, conv_algo=algo)
    nat = NativeMnistEngine(cfg, x, y, cuda_dev)
    assert nat.B == batch and nat.Bp == (batch + 31) // 32 * 32
    _check_grads_fp32(nat, TorchMnistEngine(cfg, x, y, cuda_dev), 7)
    # the pad rows' seed is exactly zero and their loss rows do not count
    assert float(nat.bufs["dlog"].view(nat.Bp, 10)[batch:].abs().sum()) == 0.0
    assert float(nat.bufs["dh"].view(nat.Bp, -1)[batch:].abs().sum()) == 0.0
    assert float(nat.bufs["loss_rows"][batch:].abs().sum()) == 0.0


def test_bf16_grads_match_oracle_b50(cuda_dev, data):
    """bf16 engine at B = 50, bounds of test_bf16_grads_match_fp32_oracle; then
    one train step from zero momentum (the single-launch conv1 + conv2 forward
    of the train path): mom = g + l2 * w, against the oracle's g."""
    x, y = data
    nat = NativeMnistEngine(_cfg(batch_size=50, dtype="bf16"), x, y, cuda_dev)
    ref = TorchMnistEngine(_cfg(batch_size=50), x, y, cuda_dev)
    nat.set_step(3)
    ref.set_step(3)
    nat.forward_backward_only()
    ref.forward_backward(3)
    torch.cuda.synchronize()
    loss = nat.bufs["loss_rows"][:50].sum().item() / 50
    nv, rv = nat.layout.views(nat.grads), ref.layout.views(ref.grads)
    errs = {s.name: _nrel(nv[s.name], rv[s.name]) for s in nat.layout.specs}
    print(f"bf16 loss={loss:.5f} ref={ref.last_loss:.5f}", {k: f"{v:.1e}" for k, v in errs.items()})
    assert abs(loss - ref.last_loss) < 2e-2 * max(1, ref.last_loss)
    for name, e in errs.items():
        assert e < 6e-2, (name, e)
    assert float(nat.bufs["dh16"].float().view(-1, nat.Bp, 16)[:, 50:].abs().sum()) == 0.0
    assert float(nat.bufs["dht16"].float().view(nat.Bp // 16, -1, 16)[3, :, 2:].abs().sum()) == 0.0
    want = ref.grads.clone()
    l2_end = ref.layout.l2_range()[1]
    want[:l2_end] += ref.cfg.l2 * ref.params[:l2_end]
    nat.train(1)
    torch.cuda.synchronize()
    mv, wv = nat.layout.views(nat.mom), nat.layout.views(want)
    errs = {s.name: _nrel(mv[s.name], wv[s.name]) for s in nat.layout.specs}
    print("bf16 train(1) momentum", {k: f"{v:.1e}" for k, v in errs.items()})
    for name, e in errs.items():
        assert e < 6e-2, (name, e)
    assert int(nat.step_dev.item()) == 4


@pytest.mark.parametrize("step", [0, 9])
def test_shard_shorter_than_padded_batch(cuda_dev, data, step):
    """60 rows, B = 50: Bp = 64 > n_local, so at every offset the pad rows read
    past the shard's end (the engine's device copy carries Bp - B zero rows)."""
    x, y = data
    x, y = x[:60], y[:60]
    cfg = _cfg(batch_size=50)
    nat = NativeMnistEngine(cfg, x, y, cuda_dev)
    assert nat.n_local == 60 and nat.Bp == 64
    assert nat.train_x.shape[0] == 60 + 14 and nat.train_y.shape[0] == 60 + 14
    _check_grads_fp32(nat, TorchMnistEngine(cfg, x, y, cuda_dev), step)


def test_pad_rows_are_inert_bit_for_bit(cuda_dev, data):
    """Two shards that differ only in the rows (and labels) the pad rows of
    step 3 read: the same gradients, parameters and momentum, bit for bit."""
    x, y = data
    off = batch_offset(3, 1024, 50)
    x2, y2 = x.copy(), y.copy()
    rows = slice(off + 50, off + 64)
    x2[rows] = x[600:614] * 1.5 + 0.25
    y2[rows] = (y[rows] + 3) % 10
    assert not np.array_equal(x2[rows], x[rows])
    cfg = _cfg(batch_size=50)
    a = NativeMnistEngine(cfg, x, y, cuda_dev)
    b = NativeMnistEngine(cfg, x2, y2, cuda_dev)
    for e in (a, b):
        e.set_step(3)
        e.forward_backward_only()
    torch.cuda.synchronize()
    assert float(a.grads.abs().max()) > 0
    assert torch.equal(a.grads, b.grads)
    for e in (a, b):
        e.train(1)
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params)
    assert torch.equal(a.mom, b.mom)
    assert a.loss_value() == b.loss_value()


def test_schedule_quantities_use_logical_batch(cuda_dev, data):
    """30 eager steps at B = 50 on 1024 rows (the LR decays once, at step 21:
    21 * 50 >= 1024; with Bp = 64 it would decay at step 16 and again at 32)
    against the oracle on the CPU, as test_training_trajectory_matches_oracle."""
    x, y = data
    cfg = _cfg(batch_size=50)
    nat = NativeMnistEngine(cfg, x, y, cuda_dev)
    nthreads = torch.get_num_threads()
    torch.set_num_threads(4)
    try:
        ref = TorchMnistEngine(cfg, x, y, torch.device("cpu"))
        nat.train(30)
        ref.train(30)
        torch.cuda.synchronize()
    finally:
        torch.set_num_threads(nthreads)
    assert nat.step == int(nat.step_dev.item()) == 30
    assert ref.lr(29) < ref.lr(20) == ref.lr(0)
    print(f"lr device={nat.device_lr():.9g} ref={ref.lr(29):.9g} "
          f"loss native={nat.loss_value():.6f} ref={ref.loss_value():.6f}")
    assert abs(nat.device_lr() - ref.lr(29)) < 1e-9
    a, b = nat.loss_value(), ref.loss_value()
    assert abs(a - b) < 2e-2 * max(1.0, abs(b))


@pytest.mark.parametrize("algo,max_ties,tie_err", [("direct", 2, 5e-3), ("winograd", 4, 1e-2)])
def test_per_step_grads_along_native_trajectory_b50(cuda_dev, data, algo, max_ties, tie_err):
    """test_per_step_grads_along_native_trajectory at B = 50, 6 steps: at
    every step the native grads equal the oracle's at the native parameters."""
    x, y = data
    cfg = _cfg(batch_size=50, conv_algo=algo)
    nat, ref = NativeMnistEngine(cfg, x, y, cuda_dev), TorchMnistEngine(cfg, x, y, cuda_dev)
    ties = 0
    for step in range(6):
        ref.params.copy_(nat.params)
        ref.set_step(step)
        nat.forward_backward_only()
        ref.forward_backward(step)
        torch.cuda.synchronize()
        nv, rv = nat.layout.views(nat.grads), ref.layout.views(ref.grads)
        errs = {s.name: ((nv[s.name] - rv[s.name]).norm() / rv[s.name].norm()).item()
                for s in nat.layout.specs}
        print(step, {k: f"{v:.1e}" for k, v in errs.items()})
        assert max(errs.values()) < tie_err, (step, errs)
        assert max(v for k, v in errs.items() if k.startswith("fc")) < 1e-4, (step, errs)
        if max(errs.values()) > 1e-4:
            ties += 1
        nat.train(1)
    assert ties <= max_ties, ties


def test_graph_replay_equals_eager_b50(cuda_dev, data):
    x, y = data
    eager = NativeMnistEngine(_cfg(batch_size=50), x, y, cuda_dev)
    graphed = NativeMnistEngine(_cfg(batch_size=50, graph=True, graph_steps=4), x, y, cuda_dev)
    eager.train(10)
    graphed.train(10)  # 2 replays of a 4-step graph + a 2-step graph
    torch.cuda.synchronize()
    assert torch.equal(eager.params, graphed.params)
    assert torch.equal(eager.mom, graphed.mom)


def test_trainer_runs_batch_50(cuda_dev):
    from mpi_tensorflow_amd.runtime.trainer import Trainer

    s = Trainer(C.TrainConfig(batch_size=50, synthetic=True, max_steps=20, eval_every=0,
                              quiet=True)).run()
    assert s.batch == 50 and s.steps == 20 and s.images == 1000
    assert s.engine == "native"
    assert math.isfinite(s.final_loss)


def test_factor_schedule_exchanges_padded_rows(cuda_dev, data):
    """The factor schedule gathers Bp rows a rank and forms the FC gradients
    over all of them; 3 steps must give the serial schedule's update (an
    update-versus-update comparison: XGMI_STEP_RTOL of the largest update).
    The communicator is the one-GPU stand-in of
    test_sync_schedule_autotune_with_emulated_ring (8 slots, rank 0's filled:
    the other slots are zero rows like the pad rows)."""
    from mpi_tensorflow_amd.parallel.comm import EmulatedDeviceComm

    x, y = data
    outs = {}
    for sched in ("factors", "serial"):
        comm = EmulatedDeviceComm(8, lat_us=10.0, busbw_gbps=150.0, blocks=32)
        eng = NativeMnistEngine(_cfg(batch_size=50, sync_schedule=sched), x, y, cuda_dev, comm=comm,
                                force_sync=True)
        assert eng.sync_schedule == sched
        p0 = eng.params.clone()
        eng.train(3)
        torch.cuda.synchronize()
        assert int(eng.step_dev.item()) == 3
        outs[sched] = eng.params - p0
    ref = float(outs["serial"].abs().max())
    err = float((outs["factors"] - outs["serial"]).abs().max())
    print(f"factors vs serial: max|d update|={err:.3e} max|update|={ref:.3e}")
    assert ref > 0 and math.isfinite(err)
    assert err <= XGMI_STEP_RTOL * ref


def test_xgmi_factor_schedule_exchanges_padded_rows(cuda_dev, data):
    """The same over the peer-to-peer communicator: `xgmi-fac` copies Bp factor
    rows a rank out of the peers' buffers (one-GPU stand-in of
    test_xgmi_emulated_eight_ranks_trains, whose peers hold zero rows) and
    must give the update of the serial schedule at the same rank count."""
    from mpi_tensorflow_amd.parallel.comm import EmulatedDeviceComm, XgmiDeviceComm

    x, y = data
    xc = XgmiDeviceComm.emulated(2, lat_us=0.0, link_gbps=0.0)
    fac = NativeMnistEngine(_cfg(batch_size=50, sync_schedule="xgmi-fac"), x, y, cuda_dev, 0, 1, xc,
                            force_sync=True)
    ser = NativeMnistEngine(_cfg(batch_size=50, sync_schedule="serial"), x, y, cuda_dev,
                            comm=EmulatedDeviceComm(2, lat_us=1.0, busbw_gbps=150.0, blocks=32),
                            force_sync=True)
    assert fac.sync_schedule == "xgmi-fac" and ser.sync_schedule == "serial"
    p0 = fac.params.clone()
    assert torch.equal(p0, ser.params)
    fac.train(3)
    ser.train(3)
    torch.cuda.synchronize()
    assert xc.error() == 0
    assert int(fac.step_dev.item()) == 3
    d_fac, d_ser = fac.params - p0, ser.params - p0
    ref = float(d_ser.abs().max())
    err = float((d_fac - d_ser).abs().max())
    print(f"xgmi-fac vs serial: max|d update|={err:.3e} max|update|={ref:.3e}")
    assert ref > 0 and math.isfinite(err)
    assert err <= XGMI_STEP_RTOL * ref
