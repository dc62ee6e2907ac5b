"""--optimizer lars without a GPU: parser and refusals, the torch update by hand, the CPU
engine against the recurrence written out, two gloo ranks, the command line's record."""

import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.ops import functional as Fn
from mpi_tensorflow_amd.runtime.generic_engine import GenericEngine
from mpi_tensorflow_amd.runtime.lars import lars_update_
from mpi_tensorflow_amd.utils.data import batch_offset, synthetic_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
Opt = C.OptimizerSpec


@pytest.mark.parametrize("spec,want", [
    ("momentum", Opt("momentum")), ("lars", Opt("lars", 0.001, 0.0, False)),
    ("lars:0.02,wd:5e-4", Opt("lars", 0.02, 5e-4, False)),
    ("lars:1, nesterov ,wd:0", Opt("lars", 1.0, 0.0, True))])
def test_parse_optimizer(spec, want):
    assert C.parse_optimizer(spec) == want and C.TrainConfig().optimizer == "momentum"


@pytest.mark.parametrize("spec,msg", [
    ("", "empty optimizer spec"), ("adam", "bad item"), ("lars:", "bad item"),
    ("wd:1,lars", "bad item"), ("lars,wd", "bad item"), ("lars,nesterov:1", "bad item"),
    ("lars:nan", "bad item"), ("lars,wd:1,wd:2", "twice"), ("lars,nesterov,nesterov", "twice"),
    ("lars:0", r"eta must be in \(0, 1\]"), ("lars:1.5", r"eta must be in \(0, 1\]"),
    ("lars,wd:-1", "wd must be at least 0"), ("momentum,nesterov", "momentum takes no items")])
def test_refusals(spec, msg):
    with pytest.raises(ValueError, match=msg):
        C.parse_optimizer(spec)
    with pytest.raises(ValueError, match="separate piece of work"):
        C.TrainConfig(model="mnist_cnn", optimizer="lars").validate()
    with pytest.raises(ValueError, match="training-only"):
        C.TrainConfig(model="lenet5", optimizer="lars", predict="test", resume="x.npz").validate()


@pytest.mark.parametrize("nesterov,w_want", [(False, [2.97, 3.96]), (True, [2.955, 3.94])])
def test_update_by_hand(nesterov, w_want):
    """|w| = 5, |g'| = 1, eta 0.1, wd 0.2: r = 0.5 / (1 + 1) = 0.25, u = 0.25 (g' + 0.2 w) =
    (0.3, 0.4); from m = 0 with mu 0.5, lr 0.1: m = u, w -= 0.1 m, or 0.1 (u + 0.5 m)."""
    opt, f64 = Opt("lars", 0.1, 0.2, nesterov), torch.float64
    w, m = torch.tensor([[3.0], [4.0]], dtype=f64), torch.zeros(2, 1, dtype=f64)
    r = lars_update_(w, torch.tensor([[1.2], [1.6]], dtype=f64), m, True, opt, 0.1, 0.5, gscale=0.5)
    assert float(r) == pytest.approx(0.25, rel=1e-15)
    torch.testing.assert_close(m.flatten(), torch.tensor([0.3, 0.4], dtype=f64))
    torch.testing.assert_close(w.flatten(), torch.tensor(w_want, dtype=f64))
    # a 1-D tensor: r = 1, no decay; zero weights or a zero gradient: r = 1
    w1, m1 = torch.tensor([3.0, 4.0]), torch.tensor([1.0, 1.0])
    assert lars_update_(w1, torch.tensor([0.5, 1.0]), m1, False, opt, lr=0.5, mu=0.5) == 1.0
    assert m1.tolist() == [1.0, 1.5] and w1.tolist() == ([2.5, 3.125] if nesterov else [2.5, 3.25])
    for wz, gz in (([0.0, 0.0], [3.0, 4.0]), ([3.0, 4.0], [0.0, 0.0])):
        assert lars_update_(torch.tensor([wz]), torch.tensor([gz]), torch.zeros(1, 2), True, opt,
                            lr=0.1, mu=0.5) == 1.0


def _engine(rank=0, world=1, comm=None, **kw):
    cfg = C.TrainConfig(**{**dict(model="lenet5", device="cpu", batch_size=8,
                                  optimizer="lars:0.01,wd:5e-4"), **kw}).validate()
    x, y = synthetic_rows("train", rank * 64, (rank + 1) * 64, shape=(32, 32, 3))
    return GenericEngine(cfg, x, y, CPU, rank, world, comm)


def test_cpu_engine_follows_the_recurrence():
    eng, ref = _engine(), _engine()
    m = torch.zeros_like(ref.mom)
    for s in range(3):
        eng.train(1)
        z = slice(batch_offset(s, ref.n_local, 8), batch_offset(s, ref.n_local, 8) + 8)
        ref.params.grad = None
        Fn.cross_entropy(ref.model.forward(ref.P, ref.bn, ref.train_x[z], True), ref.train_y[z]).backward()
        with torch.no_grad():
            for i, sp in enumerate(ref.layout.specs):
                a, b = ref.layout.segment(sp.name)
                w, u, r = ref.params[a:b], ref.params.grad[a:b], 1.0
                if len(sp.shape) >= 2:
                    nw, ng = float(w.double().norm()), float(u.double().norm())
                    r = 0.01 * nw / (ng + 5e-4 * nw)
                    u = r * (u + 5e-4 * w)
                m[a:b] = 0.9 * m[a:b] + u
                w -= ref.lr(s) * m[a:b]
                assert float(eng.ratio[i]) == pytest.approx(r, rel=1e-5)
    torch.testing.assert_close(eng.params, ref.params, rtol=1e-5, atol=1e-7)
    assert _engine(optimizer="momentum").ratio is None


def _worker(rank, world, port):
    torch.set_num_threads(2)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from mpi_tensorflow_amd.parallel import dist as D
    from mpi_tensorflow_amd.parallel.comm import make_comm
    from mpi_tensorflow_amd.parallel.sync import replicas_identical

    eng = _engine(rank, world, make_comm(D.init("cpu"), CPU))
    eng.train(3)
    assert all(replicas_identical(t) for t in (eng.params.detach(), eng.mom, eng.ratio))
    assert bool((eng.ratio != 1).any())
    D.shutdown()


def test_two_gloo_ranks_stay_bit_identical():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(2, port), nprocs=2, join=True)  # (a worker's assert fails the spawn)


def test_cli_record_names_the_optimizer(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="",
               HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, "mpipy.py", "--synthetic", "--device", "cpu", "--model", "lenet5",
           "--max-steps", "2", "--batch-size", "8", "--eval-every", "0", "--metrics-jsonl"]
    for extra, want in ((["--optimizer", "lars"], "lars"), ([], None)):
        mj = str(tmp_path / f"m{len(extra)}.jsonl")
        r = subprocess.run(cmd + [mj] + extra, cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
        summ = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"summary"')][-1])
        with open(mj) as f:
            final = [json.loads(ln) for ln in f if ln.strip()][-1]
        assert summ["summary"].get("optimizer") == final.get("optimizer") == want
