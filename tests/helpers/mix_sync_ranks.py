"""Worker for tests/test_mix_gpu.py: 2 ranks share ONE GPU, each runs the native
MNIST executor under --mix mixup:50 --label-smoothing 0.1 with a host-staged gloo
communicator (real cross-rank data), and checks
  * the ranks drew different partners (each mixes inside its own shard with its
    own key);
  * buckets == a SERIAL emulation of data parallelism on rank 0 (both ranks'
    soft-target gradients by the same kernels, summed, one SGD with gscale 1/N):
    bit-identical params and momentum, as tests/helpers/native_sync_ranks.py;
  * the factor schedule - it forms the FC gradients from dlog, which is what the
    soft target changes - keeps the replicas bit-identical and matches the serial
    emulation at that helper's bounds for factors (params 1e-3, momentum 1e-2 of
    the largest).
Launch: RANK / WORLD_SIZE / MASTER_PORT in the environment, one process a rank."""
import sys

import torch
import torch.distributed as dist

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.ops import native, ptr, stream_handle
from mpi_tensorflow_amd.parallel import dist as D
from mpi_tensorflow_amd.parallel.comm import HostStagedComm
from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine
from mpi_tensorflow_amd.utils.data import load_mnist_shard

ROWS = 512
FLAGS = dict(mix="mixup:50", label_smoothing=0.1)


def _shard(rank, world, seed):
    sh = load_mnist_shard(rank, world, synthetic=True, seed=seed)
    return sh.train_x[:ROWS], sh.train_y[:ROWS]


def run(schedule, steps, di):
    cfg = C.TrainConfig(sync_schedule=schedule, graph=False, **FLAGS).validate()
    x, y = _shard(di.rank, di.world, cfg.seed)
    eng = NativeMnistEngine(cfg, x, y, torch.device("cuda"), di.rank, di.world, HostStagedComm(di))
    assert eng.grad_sync and eng.sync_schedule == schedule, eng.sync_schedule
    assert eng.ptrs.train_lam != 0 and eng.ptrs.label_smoothing > 0
    eng.train(steps)
    eng.sync_optimizer_state()
    torch.cuda.synchronize()
    return eng.params.cpu(), eng.mom.cpu(), eng.shuffler.work_lam[:ROWS].cpu()


def serial(steps, world):
    """One process plays every rank: same kernels, summed grads, one SGD."""
    C_ = native()
    cfg = C.TrainConfig(graph=False, **FLAGS).validate()
    engs = []
    for r in range(world):
        x, y = _shard(r, world, cfg.seed)
        engs.append(NativeMnistEngine(cfg, x, y, torch.device("cuda"), r, world, None))
    lead = engs[0]
    gsum = torch.empty_like(lead.grads)
    hi = lead.layout.l2_range()[1]
    s = stream_handle()
    for _ in range(steps):
        for e in engs:
            if e is not lead:
                e.params.copy_(lead.params)
                e.step_dev.copy_(lead.step_dev)
                e.step = lead.step
            e.forward_backward_only()
        gsum.copy_(engs[0].grads)
        for e in engs[1:]:
            gsum.add_(e.grads)
        C_.optim.sgd_momentum(ptr(lead.params), ptr(gsum), ptr(lead.mom), lead.layout.total, hi,
                              cfg.l2, cfg.momentum, 1.0 / world, ptr(lead.lr_dev), 0.0,
                              ptr(lead.step_dev), s)
        lead.step += 1
    torch.cuda.synchronize()
    return lead.params.cpu(), lead.mom.cpu()


def main():
    di = D.init("cuda")
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    pb, mb, lam = run("buckets", steps, di)
    pf, mf, _ = run("factors", steps, di)
    for tag, t in (("buckets", pb), ("factors", pf)):
        ref = t.clone()
        dist.broadcast(ref, 0)
        assert torch.equal(ref, t), f"{tag}: replicas diverged"
    other = lam.clone()  # a pure function of (key, row): equal keys would give equal shares
    dist.broadcast(other, 0)
    if di.rank == 1:
        assert not torch.equal(other, lam), "both ranks drew with the same key"
    assert float(pb.abs().sum()) > 0 and float(mb.abs().sum()) > 0
    if di.rank == 0:
        p1, m1 = serial(steps, di.world)
        assert torch.equal(pb, p1), f"buckets vs serial: params {(pb - p1).abs().max().item()}"
        assert torch.equal(mb, m1), f"buckets vs serial: momentum {(mb - m1).abs().max().item()}"
        dp = (pf - p1).abs().max().item() / p1.abs().max().item()
        dm = (mf - m1).abs().max().item() / m1.abs().max().item()
        assert dp < 1e-3 and dm < 1e-2, f"factors vs serial: rel params {dp:.2e}, momentum {dm:.2e}"
        print(f"MIX_SYNC_OK world={di.world} steps={steps} factors-rel={dp:.2e}", flush=True)
    D.barrier()
    D.shutdown()


if __name__ == "__main__":
    main()
