"""Evaluation metrics, CPU side: the fp64 torch oracle of Fn.eval_metrics on
hand-worked rows (tie rule, ignored labels), EvalMetrics arithmetic, the
--eval-metrics / --ckpt-best flags through mpipy.py (new record keys with the
flag, the old key set without it) and the sum over two gloo ranks."""

import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EVENT_KEYS = {"test_loss", "test_error_global", "test_top3_error", "val_error", "val_loss"}
FINAL_KEYS = {"test_confusion", "test_rank_hist", "val_confusion", "test_per_class_recall",
              "final_test_loss", "final_val_error", "final_val_loss"}
BEST_KEYS = {"best_val_error", "best_step"}


def _lse(row):
    m = max(row)
    return m + np.log(sum(np.exp(np.array(row, np.float64) - m)))


# ------------------------------------------------------------ the oracle --
def test_oracle_hand_worked_rows():
    from mpi_tensorflow_amd.ops import functional as Fn

    rows = [
        [1.0, 3.0, 3.0, 0.0, 3.0],   # three-way tie at 1, 2, 4; label 4
        [2.0, 2.0, 2.0, 2.0, 2.0],   # all equal; label 3
        [0.0, 1.0, 5.0, 1.0, -1.0],  # label 9: outside [0, 5)
        [0.0, 1.0, 5.0, 1.0, -1.0],  # label -1: outside too
        [4.0, 1.0, 0.0, 1.0, 2.0],   # plain: label 3 ties with 1 behind 0 and 4
    ]
    labels = [4, 3, 9, -1, 3]
    m = Fn.eval_metrics(torch.tensor(rows, dtype=torch.float32), torch.tensor(labels))
    assert m.confusion.dtype == np.int64 and m.rank_hist.dtype == np.int64
    want = np.zeros((5, 5), np.int64)
    want[4, 1] += 1  # the lowest index among the maximal logits
    want[3, 0] += 1  # all equal: class 0
    want[3, 0] += 1  # the plain row predicts 0
    assert np.array_equal(m.confusion, want)
    # ranks: row 0 -> the equal classes 1 and 2 come first: 2; row 1 -> classes
    # 0..2 equal and lower: 3; last row -> 0 and 4 greater, 1 equal and lower: 3
    assert m.rank_hist.tolist() == [0, 0, 1, 2, 0]
    assert m.ignored == 2 and m.n == 3
    loss = (_lse(rows[0]) - 3.0) + (_lse(rows[1]) - 2.0) + (_lse(rows[4]) - 1.0)
    assert abs(m.loss_sum - loss) <= 1e-12 * abs(loss)
    assert m.error == 100.0 and m.topk_error(3) == pytest.approx(200.0 / 3)


def test_oracle_accumulates_into_out_and_handles_no_rows():
    from mpi_tensorflow_amd.ops import functional as Fn

    g = torch.Generator().manual_seed(3)
    x = torch.randn(37, 7, generator=g)
    y = torch.randint(0, 7, (37,), generator=g)
    whole = Fn.eval_metrics(x, y)
    out = Fn.EvalMetricsOut(7, x.device)
    for a, b in ((0, 20), (20, 20), (20, 37)):
        assert Fn.eval_metrics(x[a:b], y[a:b], out=out) is out
    got = out.result()
    assert np.array_equal(got.confusion, whole.confusion)
    assert np.array_equal(got.rank_hist, whole.rank_hist)
    assert got.n == whole.n == 37 and got.loss_sum == pytest.approx(whole.loss_sum, rel=1e-12)
    assert whole.wrong == int((x.double().argmax(1) != y).sum())  # no ties in randn
    with pytest.raises(ValueError):
        Fn.eval_metrics(torch.zeros(2, 65), torch.zeros(2, dtype=torch.int64))


# ------------------------------------------------------------ EvalMetrics --
def test_eval_metrics_arithmetic():
    from mpi_tensorflow_amd.ops import functional as Fn
    from mpi_tensorflow_amd.utils.metrics import EvalMetrics

    conf = np.array([[5, 1, 0], [2, 2, 0], [0, 3, 7]])
    m = EvalMetrics(20, 1, 8.0, conf, np.array([14, 4, 2]))
    assert m.error == 100.0 * 6 / 20 and m.loss == 0.4
    assert m.topk_error(1) == m.error and m.topk_error(2) == 10.0 and m.topk_error(3) == 0.0
    assert np.allclose(m.per_class_recall, [5 / 6, 0.5, 0.7])
    j = json.loads(json.dumps(m.to_json()))
    assert j["confusion"] == conf.tolist() and j["rank_hist"] == [14, 4, 2] and j["n"] == 20
    with pytest.raises(ValueError):
        m.topk_error(0)

    g = torch.Generator().manual_seed(5)
    x = torch.randint(-2, 3, (60, 6), generator=g).float()  # many ties
    y = torch.randint(-1, 7, (60,), generator=g)  # some labels outside [0, 6)
    a, b, ab = Fn.eval_metrics(x[:25], y[:25]), Fn.eval_metrics(x[25:], y[25:]), Fn.eval_metrics(x, y)
    s = a + b
    assert np.array_equal(s.confusion, ab.confusion) and np.array_equal(s.rank_hist, ab.rank_hist)
    assert (s.n, s.ignored) == (ab.n, ab.ignored) and ab.ignored > 0 and ab.n + ab.ignored == 60
    assert s.loss_sum == pytest.approx(ab.loss_sum, rel=1e-12)
    assert int(ab.rank_hist[0]) == int(np.trace(ab.confusion))  # rank 0 = top-1 correct
    ints, sums = ab.pack()
    back = EvalMetrics.unpack(ints, sums, 6)
    assert np.array_equal(back.confusion, ab.confusion) and back.n == ab.n


def test_allreduce_sum_host_array_world_1():
    from mpi_tensorflow_amd.parallel import dist as D

    a = D.allreduce_sum_host_array(np.array([[1, 2], [3, 4]], np.int32))
    assert a.dtype == np.int64 and a.tolist() == [[1, 2], [3, 4]]
    f = D.allreduce_sum_host_array(np.array([0.5], np.float32))
    assert f.dtype == np.float64 and f[0] == 0.5


# ------------------------------------------------------------------ flags --
def test_ckpt_best_flag_validation():
    from mpi_tensorflow_amd import config as C

    cfg = C.config_from_args(["--ckpt-best", "b.npz"])
    assert cfg.eval_metrics and cfg.ckpt_best == "b.npz"
    assert not C.config_from_args([]).eval_metrics
    assert C.config_from_args(["--eval-metrics"]).eval_metrics
    for model in ("lenet5", "resnet18"):  # shards without validation rows
        with pytest.raises(ValueError):
            C.config_from_args(["--ckpt-best", "b.npz", "--model", model])
    with pytest.raises(ValueError):
        C.config_from_args(["--ckpt-best", "b.npz", "--eval-every", "0"])


def test_evaluate_metrics_rejects_an_empty_or_unknown_split():
    from types import SimpleNamespace

    from mpi_tensorflow_amd.runtime.trainer import Trainer

    tr = Trainer.__new__(Trainer)  # the check comes before anything else is touched
    tr.shard = SimpleNamespace(val_x=np.zeros((0, 28, 28, 1), np.float32), val_y=np.zeros(0, np.int64))
    with pytest.raises(ValueError, match="empty"):
        tr.evaluate_metrics("val")
    with pytest.raises(ValueError, match="unknown split"):
        tr.evaluate_metrics("train")


# ------------------------------------------------------------- mpipy runs --
def _mpipy(*args, timeout=600):
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="",
               HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, "mpipy.py", "--synthetic", "--backend", "torch", "--device", "cpu",
           "--max-steps", "4", "--eval-every", "2", *args]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def _records(path):
    return [json.loads(line) for line in open(path)]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("eval_metrics")
    out_a = _mpipy("--eval-metrics", "--metrics-jsonl", str(d / "a.jsonl"))
    out_b = _mpipy("--metrics-jsonl", str(d / "b.jsonl"))
    return out_a, _records(d / "a.jsonl"), out_b, _records(d / "b.jsonl")


def test_run_with_eval_metrics_writes_the_new_keys(runs):
    out_a, a, _, _ = runs
    assert [r.get("step") for r in a[:-1]] == [2] and a[-1]["final"]
    assert EVENT_KEYS <= set(a[0]) and not (FINAL_KEYS | BEST_KEYS) & set(a[0])
    fin = a[-1]
    assert EVENT_KEYS | FINAL_KEYS <= set(fin) and not BEST_KEYS & set(fin)
    conf = np.array(fin["test_confusion"])
    assert conf.shape == (10, 10) and conf.sum() == 10000  # the whole synthetic test split
    assert 100.0 * (1.0 - np.trace(conf) / conf.sum()) == pytest.approx(
        fin["final_test_error_global"], abs=1e-9)
    assert fin["test_error_global"] == pytest.approx(fin["final_test_error_global"], abs=1e-9)
    assert sum(fin["test_rank_hist"]) == 10000 and fin["test_rank_hist"][0] == np.trace(conf)
    assert np.array(fin["val_confusion"]).sum() == 5000
    assert np.isfinite(fin["test_loss"]) and fin["final_test_loss"] == fin["test_loss"]
    assert fin["final_val_error"] == fin["val_error"] and fin["final_val_loss"] == fin["val_loss"]
    assert 0.0 <= fin["test_top3_error"] <= fin["test_error_global"]
    assert len(fin["test_per_class_recall"]) == 10
    # the reference-format lines are still there; rank 0 adds one line per event
    lines = out_a.splitlines()
    assert "Process ID: 0  training session starts!" in lines
    assert any(l.startswith("0  process at  2 with test error: ") for l in lines)
    assert len([l for l in lines if l.startswith("[metrics] step ")]) == 2


def test_run_without_the_flag_keeps_its_key_set_and_lines(runs):
    out_a, a, out_b, b = runs
    new = EVENT_KEYS | FINAL_KEYS | BEST_KEYS
    assert len(a) == len(b) == 2
    for ra, rb in zip(a, b):
        assert not new & set(rb)
        assert set(rb) == set(ra) - new  # nothing else came or went
    assert "[metrics]" not in out_b
    strip = lambda out: [l for l in out.splitlines()  # noqa: E731
                         if not l.startswith(("[metrics]", '{"summary"'))]
    assert strip(out_a) == strip(out_b)  # the reference-format lines, byte for byte
    summ = json.loads([l for l in out_b.splitlines() if l.startswith('{"summary"')][-1])["summary"]
    assert not new & set(summ)


def test_ckpt_best_writes_a_checkpoint_that_resumes(tmp_path):
    best = tmp_path / "best.npz"
    _mpipy("--ckpt-best", str(best), "--metrics-jsonl", str(tmp_path / "m.jsonl"), "--quiet")
    assert best.exists()
    recs = _records(tmp_path / "m.jsonl")
    steps = []
    for r in recs:
        assert EVENT_KEYS | BEST_KEYS <= set(r)
        steps.append(r["step"] if "step" in r else 3)  # the final evaluation: after step 3
        assert r["best_step"] in steps and r["best_val_error"] <= r["val_error"]
    assert steps == [2, 3]
    # strictly lower only: the best error is the minimum, at its first occurrence
    errs = [r["val_error"] for r in recs]
    assert recs[-1]["best_val_error"] == min(errs)
    assert recs[-1]["best_step"] == steps[errs.index(min(errs))]
    out = _mpipy("--resume", str(best), "--max-steps", "5", "--eval-every", "0")
    summ = json.loads([l for l in out.splitlines() if l.startswith('{"summary"')][-1])["summary"]
    assert summ["steps"] == 5 - (recs[-1]["best_step"] + 1)


def test_a_model_without_validation_rows_reports_test_metrics_only(tmp_path):
    """LeNet-5 through the op-by-op oracle engine: evaluate_metrics is the
    engine's eval logits through Fn.eval_metrics, whatever the engine."""
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="",
               HIP_VISIBLE_DEVICES="")
    path = tmp_path / "m.jsonl"
    r = subprocess.run([sys.executable, "mpipy.py", "--model", "lenet5", "--device", "cpu",
                        "--max-steps", "2", "--eval-every", "0", "--eval-metrics", "--quiet",
                        "--metrics-jsonl", str(path)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "[metrics]" not in r.stdout  # --quiet silences the extra line too
    (fin,) = _records(path)
    assert {"test_loss", "test_top3_error", "test_confusion", "final_test_loss"} <= set(fin)
    assert not {"val_error", "val_loss", "val_confusion", "final_val_error"} & set(fin)
    conf = np.array(fin["test_confusion"])
    assert conf.sum() == 2048
    assert 100.0 * (1.0 - np.trace(conf) / conf.sum()) == pytest.approx(
        fin["final_test_error_global"], abs=1e-9)


# ------------------------------------------------------------ gloo, world 2 --
def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker_metrics(rank, world, port, out_dir):
    torch.set_num_threads(2)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    for k in ("OMPI_COMM_WORLD_RANK", "PMI_RANK", "SLURM_PROCID"):
        os.environ.pop(k, None)
    from mpi_tensorflow_amd import config as C
    from mpi_tensorflow_amd.parallel import dist as D
    from mpi_tensorflow_amd.runtime.trainer import Trainer

    cfg = C.TrainConfig(device="cpu", backend="torch", synthetic=True, max_steps=4, eval_every=2,
                        quiet=True, ckpt_best=os.path.join(out_dir, "best.npz"),
                        collective_timeout_s=120.0)
    tr = Trainer(cfg)
    tr.run()
    local = tr.evaluate_metrics("test")
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), local=local.confusion,
             glob=tr.last_metrics["test"].confusion, val=tr.last_metrics["val"].confusion,
             best_step=tr.best_step, best_err=tr.best_val_error)
    D.barrier()
    D.shutdown()


def test_two_ranks_sum_their_metrics_and_agree_on_the_best_step(tmp_path):
    world, port = 2, _free_port()
    mp.spawn(_worker_metrics, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = np.load(tmp_path / "r0.npz"), np.load(tmp_path / "r1.npz")
    assert r0["local"].sum() == r1["local"].sum() == 5000
    assert not np.array_equal(r0["local"], r1["local"])  # different shards
    assert np.array_equal(r0["glob"], r0["local"] + r1["local"])
    assert np.array_equal(r1["glob"], r0["glob"]) and np.array_equal(r1["val"], r0["val"])
    assert r0["val"].sum() == 5000
    assert int(r0["best_step"]) == int(r1["best_step"]) and int(r0["best_step"]) in (2, 3)
    assert float(r0["best_err"]) == float(r1["best_err"])
    assert (tmp_path / "best.npz").exists()
