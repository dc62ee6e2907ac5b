"""The evaluation-metrics kernel (csrc/kernels/eval_metrics.hip) against the
fp64 torch oracle of the same definitions (Fn.eval_metrics on the CPU):
counts exactly, losses within the fp32 kernel tolerance; accumulation over
chunks and reproducibility; the engines' own error counters against the
confusion matrix of the same logits; --eval-metrics through the trainer with
the evaluation sets resident on the device.

Measured on an MI355X (precise expf / logf), in units of 1 + |ref| against
the bound of 1e-5: largest row loss error 1.0e-7 (4.3e-8 on the +-80 row),
largest loss_sum error 1.5e-8 (docs/ACCURACY.md)."""

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.ops import functional as Fn
from mpi_tensorflow_amd.utils.data import synthetic_rows

pytestmark = pytest.mark.gpu

# the project's fp32-kernel-against-fp64 tolerance: |dev - ref| <= TOL (1 + |ref|)
TOL = 1e-5
CASES = [(1, 10), (3, 10), (257, 10), (64, 3), (130, 64)]


def _case(n, c):
    """randn * 3 logits with: row 0 = +-80 alternating, labelled with a -80
    class (a softmax that is not max-subtracted overflows; its 80s also tie),
    row 1 all equal, every third row from 2 on small integers (ties); random
    labels, two of the 257 rows labelled outside [0, C).  (n = 1 has room for
    the +-80 row only.)"""
    g = torch.Generator().manual_seed(1000 * n + c)
    x = torch.randn(n, c, generator=g) * 3
    y = torch.randint(0, c, (n,), generator=g)
    x[0] = torch.tensor([80.0 if j % 2 == 0 else -80.0 for j in range(c)])
    y[0] = 1
    if n > 1:
        x[1] = 1.5
    for i in range(2, n, 3):
        x[i] = torch.randint(-2, 3, (c,), generator=g).float()
    if n == 257:
        y[5], y[200] = c, -3
    return x, y


def _row_losses_ref(x, y):
    c = x.shape[1]
    ok = (y >= 0) & (y < c)
    x64 = x.double()
    picked = x64.gather(1, y.clamp(0, c - 1)[:, None])[:, 0]
    return torch.where(ok, torch.logsumexp(x64, 1) - picked, torch.zeros_like(picked))


def _same_counts(a, b):
    assert np.array_equal(a.confusion, b.confusion)
    assert np.array_equal(a.rank_hist, b.rank_hist)
    assert (a.n, a.ignored) == (b.n, b.ignored)


@pytest.mark.parametrize("n,c", CASES)
def test_kernel_matches_the_fp64_oracle(cuda_dev, n, c):
    x, y = _case(n, c)
    ref = Fn.eval_metrics(x, y)  # CPU: the fp64 oracle
    rows = torch.full((n,), -1.0, device=cuda_dev)
    out = Fn.EvalMetricsOut(c, cuda_dev)
    Fn.eval_metrics(x.to(cuda_dev), y.to(cuda_dev), out=out, loss_rows=rows)
    got = out.result()
    _same_counts(got, ref)  # the same fp32 comparisons: exact, every row
    assert got.n + got.ignored == n and got.ignored == (2 if n == 257 else 0)
    assert int(got.rank_hist[0]) == int(np.trace(got.confusion))
    want = _row_losses_ref(x, y)
    err = (rows.cpu().double() - want).abs() / (1.0 + want.abs())
    sum_err = abs(got.loss_sum - ref.loss_sum) / (n + float(want.abs().sum()))
    print(f"eval_metrics n={n} C={c}: max row loss error {err.max().item():.3e} "
          f"(row 0, +-80: {err[0].item():.3e}), loss_sum error {sum_err:.3e}, in units of (1 + |ref|)")
    assert want[0].item() > 159.0  # the +-80 row is there
    assert err.max().item() <= TOL
    assert abs(got.loss_sum - float(want.sum())) <= TOL * (n + float(want.abs().sum()))
    assert sum_err <= TOL
    # a single-row call gives that row's loss as the sum
    one = Fn.eval_metrics(x[:1].to(cuda_dev), y[:1].to(cuda_dev))
    assert abs(one.loss_sum - want[0].item()) <= TOL * (1.0 + want[0].item())


def test_chunks_accumulate_and_the_sum_is_reproducible(cuda_dev):
    x, y = _case(257, 10)
    xd, yd = x.to(cuda_dev), y.to(cuda_dev)
    whole = Fn.eval_metrics(xd, yd)
    out = Fn.EvalMetricsOut(10, cuda_dev)
    for a, b in ((0, 100), (100, 200), (200, 257), (257, 257)):  # the last: no rows, no launch
        Fn.eval_metrics(xd[a:b], yd[a:b], out=out)
    parts = out.result()
    _same_counts(parts, whole)
    # an fp64 sum of the same fp32 terms in another order
    assert abs(parts.loss_sum - whole.loss_sum) <= 1e-12 * abs(whole.loss_sum)
    again = Fn.eval_metrics(xd, yd)
    assert again.loss_sum == whole.loss_sum  # bit for bit
    assert out.zero_().result().n == 0 and out.result().loss_sum == 0.0


def test_oracle_mode_on_device_tensors(cuda_dev):
    x, y = _case(64, 3)
    with Fn.oracle_mode():
        a = Fn.eval_metrics(x.to(cuda_dev), y.to(cuda_dev))
    _same_counts(a, Fn.eval_metrics(x, y))


# ---------------------------------------------------------------- engines --
def _engine(kind, dev):
    if kind == "lenet5":
        from mpi_tensorflow_amd.runtime.lenet_engine import NativeLenetEngine

        shape = (32, 32, 3)
        x, y = synthetic_rows("train", 0, 256, shape=shape)
        eng = NativeLenetEngine(C.TrainConfig(model="lenet5").validate(), x, y, dev)
        return eng, synthetic_rows("test", 0, 100, shape=shape)
    from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine

    x, y = synthetic_rows("train", 0, 256)
    eng = NativeMnistEngine(C.TrainConfig(dtype=kind, graph=False).validate(), x, y, dev)
    return eng, synthetic_rows("test", 0, 100)


@pytest.mark.parametrize("kind", ["fp32", "bf16", "lenet5"])
def test_engine_error_counter_equals_the_confusion_matrix(cuda_dev, kind):
    """Random-init weights, 100 rows in chunks of 32 (four chunks, a tail of 4):
    the engine's own count of wrong rows and the metrics of the same call's
    logits agree as integers - the tie rule and the chunk offsets."""
    eng, (tx, ty) = _engine(kind, cuda_dev)
    err, logits = eng.evaluate(tx, ty, chunk=32, return_logits=True)
    m = Fn.eval_metrics(logits, torch.from_numpy(np.asarray(ty)))
    n = len(ty)
    wrong = err * n / 100.0  # evaluate() returns the percentage
    assert n == 100 and m.n == n and m.ignored == 0
    assert abs(wrong - round(wrong)) < 1e-9 and int(round(wrong)) == m.wrong, (err, m.wrong)
    assert int(m.confusion.sum()) == 100 and int(m.rank_hist.sum()) == 100
    assert np.array_equal(m.confusion.sum(1), np.bincount(np.asarray(ty), minlength=10))


# ---------------------------------------------------------------- trainer --
def test_trainer_eval_metrics_with_resident_eval_sets(cuda_dev, tmp_path):
    import json

    from mpi_tensorflow_amd.runtime.trainer import Trainer

    path = tmp_path / "m.jsonl"
    cfg = C.TrainConfig(model="mnist_cnn", synthetic=True, max_steps=4, eval_every=2,
                        eval_metrics=True, quiet=True, metrics_jsonl=str(path)).validate()
    tr = Trainer(cfg)
    summ = tr.run()
    assert np.isfinite(summ.final_test_loss) and np.isfinite(summ.final_val_loss)
    # two eval events (step 2, the end) x two splits: one upload each, then hits
    for split in ("test", "val"):
        cache = tr.eval_cache[split]
        assert cache.misses == 1 and cache.hits >= 1, (split, cache.misses, cache.hits)
    held = tr.eval_cache["test"].get(tr.shard.test_x, tr.device)
    err = tr.evaluate()  # evaluate() runs on the resident copy too, same float as the run's
    assert tr.eval_cache["test"].get(tr.shard.test_x, tr.device) is held
    assert tr.eval_cache["test"].misses == 1
    assert err == summ.final_test_error_local
    # the oracle on the same logits, moved to the CPU
    _, logits = tr.engine.evaluate(tr.shard.test_x, tr.shard.test_y, return_logits=True)
    ref = Fn.eval_metrics(logits.cpu(), torch.from_numpy(np.asarray(tr.shard.test_y)))
    assert abs(summ.final_test_loss - ref.loss) <= 1e-4 * abs(ref.loss)
    got = tr.last_metrics["test"]
    assert np.array_equal(got.confusion, ref.confusion) and got.error == err
    recs = [json.loads(line) for line in open(path)]
    assert recs[0]["step"] == 2 and "test_loss" in recs[0] and "val_error" in recs[0]
    assert np.array(recs[-1]["test_confusion"]).sum() == tr.shard.test_x.shape[0]
    with pytest.raises(ValueError):
        tr.evaluate_metrics("train")
