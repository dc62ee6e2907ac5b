"""runtime/engine_common.py on the CPU: the graph step driver on a fake engine
(expected launch logs written out by hand), the tune's state snapshot, and
the attribute surface bench.py and the Trainer probe on the engine classes."""

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd.runtime.engine_common import GraphStepDriver, StateSnapshot
from mpi_tensorflow_amd.runtime.generic_engine import GenericEngine
from mpi_tensorflow_amd.runtime.lenet_engine import NativeLenetEngine
from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine, TorchMnistEngine
from mpi_tensorflow_amd.runtime.shuffle import PassShuffler
from mpi_tensorflow_amd.utils.data import pass_of


class _Replay:
    def __init__(self, log, n):
        self.log, self.n = log, n

    def replay(self):
        self.log.append(self.n)


class FakeEngine(GraphStepDriver):
    """Logs "e" per eager step and n per replay of an n-step graph; `broken`:
    the graph lengths whose capture fails (None), `sticky`: a failed capture
    also ends the use of graphs."""

    def __init__(self, G, broken=(), sticky=False, shuffler=None):
        self.use_graph, self.graph_steps, self._tuned, self.step = True, G, True, 0
        self.shuffler = shuffler
        self.broken, self.sticky = set(broken), sticky
        self.log, self.requested = [], []

    def _launch_one(self):
        self.log.append("e")

    def _graph(self, n):
        self.requested.append(n)
        if n in self.broken:
            self.use_graph = self.use_graph and not self.sticky
            return None
        return _Replay(self.log, n)


@pytest.mark.parametrize("k,log", [(0, []), (1, [1]), (3, [3]), (7, [3, 3, 1])])
def test_run_steps_full_graphs_then_remainder(k, log):
    eng = FakeEngine(3)
    eng._run_steps(k)
    assert eng.log == log


@pytest.mark.parametrize("k,sizes", [(7, {3, 1}), (2, {2})])
def test_capture_requests_the_sizes_train_replays(k, sizes):
    eng = FakeEngine(3)
    eng.capture(k)
    assert set(eng.requested) == sizes and len(eng.requested) == len(sizes)
    assert eng.log == []


def test_capture_unavailable_runs_every_step_eagerly():
    eng = FakeEngine(3, broken={1, 2, 3}, sticky=True)
    eng._run_steps(7)
    assert eng.log == ["e"] * 7 and not eng.use_graph


def test_failed_remainder_capture_does_not_repeat_replayed_steps():
    eng = FakeEngine(3, broken={1})
    eng._run_steps(7)
    assert eng.log == [3, 3, "e"]


def test_train_cuts_at_pass_boundaries():
    n, B = 10, 4
    assert [s for s in range(7) if s == 0 or pass_of(s, n, B) != pass_of(s - 1, n, B)] == [0, 2, 3, 5, 6]
    x = torch.arange(n, dtype=torch.float32).reshape(n, 1, 1, 1)
    shuf = PassShuffler(0, 0, n, B, x, torch.arange(n, dtype=torch.int32), native=None)
    eng = FakeEngine(3, shuffler=shuf)
    load = shuf.load
    shuf.load = lambda p: (eng.log.append(("load", p)), load(p))
    eng.train(6)
    assert eng.log == [("load", 0), 2, ("load", 1), 1, ("load", 2), 2, ("load", 3), 1]
    assert eng.step == 6 and shuf.loaded == 3


def test_snapshot_restores_values_in_place():
    a = torch.arange(6, dtype=torch.float32).requires_grad_(True)  # (as the generic params)
    b = torch.tensor([7], dtype=torch.int64)
    want = [a.detach().clone(), b.clone()]
    ptrs = [a.data_ptr(), b.data_ptr()]
    snap = StateSnapshot(a, b)
    with torch.no_grad():
        a.mul_(3.0).add_(float("nan"))
        b.add_(5)
    snap.restore()
    assert np.array_equal(a.detach().numpy(), want[0].numpy()) and torch.equal(b, want[1])
    assert [a.data_ptr(), b.data_ptr()] == ptrs and a.requires_grad


def test_engine_classes_keep_their_surface():
    """bench.py and the Trainer pick their path by hasattr: a shared base must
    not hand an engine a method it did not have."""
    for cls in (NativeLenetEngine, GenericEngine, TorchMnistEngine):
        assert not hasattr(cls, "prewarm_train"), cls
    assert hasattr(NativeMnistEngine, "prewarm_train")
    for name in ("tune_schedule", "capture"):
        assert not hasattr(TorchMnistEngine, name), name
        for cls in (NativeMnistEngine, NativeLenetEngine, GenericEngine):
            assert hasattr(cls, name), (cls, name)
    assert hasattr(GenericEngine, "collective_graph_nodes")
    for cls in (NativeMnistEngine, NativeLenetEngine, TorchMnistEngine):
        assert not hasattr(cls, "collective_graph_nodes"), cls
    for cls in (NativeMnistEngine, NativeLenetEngine, GenericEngine):
        assert isinstance(cls.sync_schedule, property) and hasattr(cls, "_graph"), cls
    for name in ("_set_schedule", "_tune_candidates"):
        assert hasattr(NativeMnistEngine, name), name
    assert {c.kind for c in (TorchMnistEngine, NativeMnistEngine, NativeLenetEngine, GenericEngine)} \
        == {"torch", "native", "native-lenet5", "generic"}
