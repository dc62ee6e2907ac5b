"""bench.py's plain run, --full and --dump-outputs, in-process on the CPU
(PyTorch oracle engines): the result line's keys, the number of timed steps,
what a plain run leaves out, and the dumped arrays of two identical runs."""
import json
import os

import numpy as np
import pytest

import bench

KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")


def _bench(capsys, *args):
    assert bench.main(["--gpus", "1", "--prewarm-ms", "0"] + list(args)) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.fixture
def on_cpu(monkeypatch):
    """bench.py picks the device itself; these tests pin its CPU path."""
    import torch

    from mpi_tensorflow_amd.parallel import dist as D

    monkeypatch.setattr(D, "resolve_device", lambda device="auto": torch.device("cpu"))


def test_plain_run_times_exactly_the_steps_and_skips_the_rest(capsys, on_cpu):
    j = _bench(capsys, "--model", "lenet5", "--steps", "3", "--warmup", "2")
    for k in KEYS:
        assert k in j, k
    assert j["steps"] == 3 and j["warmup"] == 2 and j["full"] is False
    assert j["test_eval_after_steps"] == 5  # warm-up + timed steps, nothing after them
    assert j["final_test_accuracy"] is None and j["outputs"] is None
    assert j["unit"] == "images/sec" and j["higher_is_better"] is True and j["dtype"] == "fp32"
    assert j["ms_per_step"] > 0
    # value and ms_per_step describe the same window
    assert j["value"] == pytest.approx(64 * 1000.0 / j["ms_per_step"], rel=1e-3)


def test_full_run_adds_the_evaluation(capsys, on_cpu):
    j = _bench(capsys, "--model", "lenet5", "--steps", "3", "--warmup", "2", "--full")
    assert j["full"] is True and j["steps"] == 3
    assert j["final_test_accuracy"] is not None and 0.0 <= j["final_test_accuracy"] <= 100.0
    j = _bench(capsys, "--model", "lenet5", "--steps", "1", "--warmup", "0", "--full", "--no-eval")
    assert j["full"] is True and j["final_test_accuracy"] is None


def test_dump_outputs_same_arguments_same_arrays(capsys, tmp_path, on_cpu):
    outs = []
    for d in ("a", "b"):
        j = _bench(capsys, "--model", "lenet5", "--steps", "3", "--warmup", "1",
                   "--dump-outputs", str(tmp_path / d))
        outs.append(j["outputs"])
    assert outs[0] == outs[1] and set(outs[0]) == {"params", "momentum", "grads", "loss"}
    total = 0
    for name, n in outs[0].items():
        a, b = (np.load(tmp_path / d / (name + ".npy")) for d in ("a", "b"))
        assert a.dtype == (np.float64 if name == "loss" else np.float32) and a.shape == (n,)
        assert np.isfinite(a).all() and np.array_equal(a, b), name
        total += os.path.getsize(tmp_path / "a" / (name + ".npy"))
    assert total <= 64 << 20
    assert np.abs(np.load(tmp_path / "a" / "momentum.npy")).max() > 0  # the steps ran
    # one more timed step gives other weights: the dump is the last step's
    _bench(capsys, "--model", "lenet5", "--steps", "4", "--warmup", "1",
           "--dump-outputs", str(tmp_path / "c"))
    assert not np.array_equal(np.load(tmp_path / "a" / "params.npy"),
                              np.load(tmp_path / "c" / "params.npy"))


def test_dump_outputs_samples_large_buffers_the_same_way(tmp_path, monkeypatch):
    """A flat buffer above its share of the byte budget is stored as the same
    sorted index sample every time."""
    import torch

    class Eng:
        def __init__(self, seed):
            g = torch.Generator().manual_seed(seed)
            self.params = torch.randn(1000, generator=g)
            self.mom = torch.zeros(50)
            self.grads = torch.arange(1000, dtype=torch.float32)

        def extra_state(self):
            return {"bn/moving_mean": torch.ones(7)}

        def loss_value(self):
            return 1.5

    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 3 * 100)  # 100 elements a flat buffer
    s1 = bench.dump_outputs(Eng(0), str(tmp_path / "x"))
    s2 = bench.dump_outputs(Eng(1), str(tmp_path / "y"))
    assert s1 == s2 == {"params": 100, "momentum": 50, "grads": 100, "state.bn.moving_mean": 7,
                        "loss": 1}
    idx = np.load(tmp_path / "x" / "grads.npy").astype(np.int64)  # grads hold their own index
    assert np.all(np.diff(idx) > 0) and np.array_equal(idx, np.load(tmp_path / "y" / "grads.npy"))
    assert np.array_equal(np.load(tmp_path / "x" / "params.npy"), Eng(0).params.numpy()[idx])
    assert np.load(tmp_path / "x" / "loss.npy").dtype == np.float64
