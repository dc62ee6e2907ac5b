"""Worker for tests/test_ema_gpu.py: 2 ranks share ONE GPU and train with
--ema under every gradient-sync schedule the two-rank tests of
captured_sync_ranks.py exercise.  Per schedule:

  * four graph-replayed steps (one 4-step graph): the moving average is
    bit-identical across the ranks, and so are the parameters;
  * the state is restored and four single-step runs record the parameters
    after each step: the average of the 4-step graph lies within the derived
    bound (ema_ref.py) of the float64 recurrence over them.

The second check is what an average that read the parameters too early would
miss: under the sharded, split and defer schedules the FC update finishes on
the comm stream, and a launch that did not wait for it would average the FC
parameters of the step before.

usage: ema_sync_ranks.py SCENARIO [ARG]
  mnist DTYPE  - native MNIST executor over the shared-memory communicator:
                 buckets / sharded / split / serial (/ factors, defer: fp32)
  xgmi DTYPE   - the same engine over the xGMI peer-to-peer communicator:
                 xgmi / serial (/ xgmi-step, xgmi-fac: fp32)
  lenet COMM   - the fused LeNet-5 executor: shm (all-reduce), xgmi
                 (two-phase), xgmipush, xgmipull
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mpi_tensorflow_amd import config as C  # noqa: E402
from mpi_tensorflow_amd.parallel import dist as D  # noqa: E402
from mpi_tensorflow_amd.parallel.comm import ShmDeviceComm, XgmiDeviceComm  # noqa: E402
from mpi_tensorflow_amd.parallel.sync import replicas_identical  # noqa: E402
from mpi_tensorflow_amd.runtime.engine_common import StateSnapshot  # noqa: E402
from mpi_tensorflow_amd.runtime.trainer import comm_capacity_bytes  # noqa: E402
from mpi_tensorflow_amd.utils.data import synthetic_rows  # noqa: E402

import ema_ref as R  # noqa: E402

STEPS, DECAY = 4, 0.9
ROWS = 256


def check(eng, what):
    """The two checks of the module docstring on a freshly built engine."""
    assert eng.grad_sync and eng.use_graph and eng.ema is not None, what
    torch.cuda.synchronize()
    snap = StateSnapshot(eng.params, eng.mom, eng.step_dev, eng.ema)
    p0 = eng.params.detach().clone().cpu()
    assert torch.equal(eng.ema.cpu(), p0), f"{what}: the average does not start at the parameters"
    eng.train(STEPS)
    torch.cuda.synchronize()
    assert len(eng._graphs) >= 1 and eng.use_graph, f"{what}: the steps were not captured"
    assert int(eng.step_dev.item()) == STEPS
    assert replicas_identical(eng.params.detach()), f"{what}: the parameters differ across the ranks"
    assert replicas_identical(eng.ema), f"{what}: the average differs across the ranks"
    ema4 = eng.ema.clone().cpu()
    assert not torch.equal(ema4, p0), f"{what}: the average never moved"
    # the same start again, one step per run
    snap.restore(sync=True)
    eng.set_step(0)
    rec = []
    for _ in range(STEPS):
        eng.train(1)
        torch.cuda.synchronize()
        rec.append(eng.params.detach().clone().cpu())
    want, bound = R.recurrence(p0, rec, DECAY)
    R.assert_within(ema4, want, bound, f"{what}: 4-step graph vs the recurrence")
    same = torch.equal(eng.ema.cpu(), ema4)
    print(f"{what}: single-step runs give the same average bit for bit: {same}", flush=True)
    xc = getattr(eng, "xcomm", None)
    if xc is not None:
        assert xc.error() == 0, f"{what}: an xgmi barrier timed out"


def mnist_engine(di, sched, dtype, comm):
    from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine

    cfg = C.TrainConfig(sync_schedule=sched, dtype=dtype, batch_size=32, graph=True,
                        graph_steps=STEPS, ema=str(DECAY)).validate()
    x, y = synthetic_rows("train", di.rank * ROWS, (di.rank + 1) * ROWS)
    eng = NativeMnistEngine(cfg, x, y, torch.device("cuda"), di.rank, di.world, comm)
    assert eng.sync_schedule == sched, (eng.sync_schedule, sched)
    return eng


def scenario_mnist(di, dtype):
    scheds = ["buckets", "sharded", "split", "serial"] + (["factors", "defer"] if dtype == "fp32" else [])
    for sched in scheds:
        cfg = C.TrainConfig(batch_size=32).validate()
        comm = ShmDeviceComm(di, comm_capacity_bytes(cfg), timeout_s=60.0)
        check(mnist_engine(di, sched, dtype, comm), f"mnist {dtype} {sched}")
    return ",".join(scheds)


def scenario_xgmi(di, dtype):
    scheds = ["xgmi", "serial"] + (["xgmi-step", "xgmi-fac"] if dtype == "fp32" else [])
    for sched in scheds:
        comm = XgmiDeviceComm(di, timeout_s=20.0)
        eng = mnist_engine(di, sched, dtype, comm)
        assert eng.xcomm is comm
        check(eng, f"mnist {dtype} over xgmi, {sched}")
    return ",".join(scheds)


def scenario_lenet(di, kind):
    from mpi_tensorflow_amd.models.generic import model_input_shape
    from mpi_tensorflow_amd.runtime.lenet_engine import NativeLenetEngine
    from mpi_tensorflow_amd.utils.data import synthetic_images_torch

    mode = {"shm": "two-phase", "xgmi": "two-phase", "xgmipush": "push", "xgmipull": "pull"}[kind]
    B = 64
    cfg = C.TrainConfig(model="lenet5", batch_size=B, graph=True, graph_steps=STEPS, xgmi_mode=mode,
                        ema=str(DECAY)).validate()
    x, y = synthetic_images_torch(4 * B, model_input_shape("lenet5"), seed=cfg.seed,
                                  start=di.rank * 4 * B)
    if kind == "shm":
        comm = ShmDeviceComm(di, comm_capacity_bytes(cfg), timeout_s=60.0)
    else:
        comm = XgmiDeviceComm(di, timeout_s=20.0)
    eng = NativeLenetEngine(cfg, x.numpy(), y.numpy(), torch.device("cuda"), di.rank, di.world, comm)
    want = {"shm": "all-reduce", "xgmi": "xgmi", "xgmipush": "xgmi-push", "xgmipull": "xgmi-pull"}
    assert eng.sync_schedule == want[kind], eng.sync_schedule
    check(eng, f"lenet5 {kind}")
    return eng.sync_schedule


def main():
    di = D.init("cuda")
    scen = sys.argv[1]
    arg = sys.argv[2] if len(sys.argv) > 2 else ""
    if scen == "mnist":
        msg = scenario_mnist(di, arg or "fp32")
    elif scen == "xgmi":
        msg = scenario_xgmi(di, arg or "fp32")
    elif scen == "lenet":
        msg = scenario_lenet(di, arg or "shm")
    else:
        raise SystemExit(f"unknown scenario {scen}")
    D.barrier()
    if di.rank == 0:
        print(f"EMA_SYNC_OK {scen} {arg} world={di.world} {msg}", flush=True)
    D.shutdown()


if __name__ == "__main__":
    main()
