"""Per-pass shuffled training batches (--shuffle), host side: the permutation
(utils/rng.py shuffle_key / shuffle_perm), the pass bookkeeping
(utils/data.py pass_of, runtime/shuffle.py) and the PyTorch engines on the CPU.
"""

import dataclasses

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.runtime.mnist_engine import TorchMnistEngine
from mpi_tensorflow_amd.runtime.shuffle import PassShuffler, batch_rows
from mpi_tensorflow_amd.utils import checkpoint as ckpt_mod
from mpi_tensorflow_amd.utils import rng
from mpi_tensorflow_amd.utils.data import batch_offset, pass_of, synthetic_rows

BIJECTION_N = (2, 3, 33, 64, 65, 97, 1000, 6875, 8192, 27500, 50000, 55000)


@pytest.mark.parametrize("args,n,key,first", [
    ((1, 0, 0), 10, 0xde56f3b3, [6, 0, 2, 9, 4, 5, 1, 8, 7, 3]),
    ((1, 0, 1), 10, 0xa0fb72af, [5, 2, 8, 9, 1, 3, 6, 7, 4, 0]),
    ((1, 3, 2), 97, 0x69d1cfab, [50, 6, 0, 34, 24, 23, 2, 88, 70, 1]),
])
def test_golden_values(args, n, key, first):
    assert rng.SHUFFLE_SALT == 0x2545F491
    assert rng.shuffle_key(*args) == key
    assert rng.shuffle_key(*args) == rng.dropout_key(*args, rng.SHUFFLE_SALT)
    assert rng.shuffle_perm(key, n)[:10].tolist() == first


@pytest.mark.parametrize("n", BIJECTION_N)
def test_perm_is_a_bijection(n):
    p = rng.shuffle_perm(rng.shuffle_key(1, 0, 0), n)
    assert p.shape == (n,)
    assert np.array_equal(np.sort(p), np.arange(n))


def test_perm_differs_between_passes_and_ranks():
    n = 55000
    p0 = rng.shuffle_perm(rng.shuffle_key(1, 0, 0), n)
    p1 = rng.shuffle_perm(rng.shuffle_key(1, 0, 1), n)
    r1 = rng.shuffle_perm(rng.shuffle_key(1, 1, 0), n)
    assert int((p0 == p1).sum()) == 0  # passes 0 and 1 of one rank share no position
    # two independent uniform permutations agree at about one position
    assert int((p0 == r1).sum()) < 10
    assert int((p0 == np.arange(n)).sum()) < 10


def test_same_order_on_all_ranks_under_reference_quirks():
    x, y = synthetic_rows("train", 0, 200)
    dev = torch.device("cpu")
    for quirks, same in ((True, True), (False, False)):
        cfg = C.TrainConfig(batch_size=50, shuffle=True, reference_quirks=quirks).validate()
        a = TorchMnistEngine(cfg, x, y, dev, rank=0, world=1)
        b = TorchMnistEngine(cfg, x, y, dev, rank=3, world=1)
        assert np.array_equal(a.shuffler.perm(1), b.shuffler.perm(1)) == same
        for e in (a, b):
            e.forward_backward(0)
        assert torch.equal(a.train_x, b.train_x) == same


@pytest.mark.parametrize("n_local,batch", [(200, 50), (55000, 64)])
def test_pass_of_changes_exactly_where_the_offset_wraps(n_local, batch):
    steps = 3 * (n_local // batch) + 5
    assert pass_of(0, n_local, batch) == 0
    seen = 0
    for s in range(1, steps):
        wrapped = batch_offset(s, n_local, batch) < batch_offset(s - 1, n_local, batch) + batch
        assert pass_of(s, n_local, batch) - pass_of(s - 1, n_local, batch) == (1 if wrapped else 0)
        seen += wrapped
    assert seen == pass_of(steps - 1, n_local, batch) >= 2
    with pytest.raises(ValueError):
        pass_of(0, batch, batch)


def test_segments_cut_at_pass_boundaries():
    x = torch.zeros(200, 2)
    y = torch.zeros(200, dtype=torch.int64)
    sh = PassShuffler(1, 0, 200, 50, x, y)
    assert list(sh.segments(0, 7)) == [(0, 3), (1, 3), (2, 1)]  # 150 rows a pass: 3 steps
    assert list(sh.segments(2, 2)) == [(0, 1), (1, 1)]
    assert list(sh.segments(3, 3)) == [(1, 3)]
    for step, k in ((0, 40), (5, 1), (17, 23)):
        segs = list(sh.segments(step, k))
        assert sum(m for _, m in segs) == k
        s = step
        for p, m in segs:
            assert all(pass_of(t, 200, 50) == p for t in range(s, s + m))
            s += m
    sh = PassShuffler(1, 0, 55000, 64, torch.zeros(55000, 1), torch.zeros(55000, dtype=torch.int64))
    assert list(sh.segments(0, 2000)) == [(0, 859), (1, 858), (2, 283)]


@pytest.fixture(scope="module")
def data200():
    return synthetic_rows("train", 0, 200)


def _cfg(**kw):
    return C.TrainConfig(batch_size=50, device="cpu", **kw).validate()


def _hand_loop(x, y, steps, seed=1):
    """The shuffled run spelled out: for every step a shuffle-off engine on
    x[perm_p], p the step's pass, continuing from the previous state."""
    dev = torch.device("cpu")
    state, eng, loaded = None, None, None
    for s in range(steps):
        p = pass_of(s, 200, 50)
        if p != loaded:
            perm = rng.shuffle_perm(rng.shuffle_key(seed, 0, p), 200)
            nxt = TorchMnistEngine(_cfg(), x[perm], y[perm], dev)
            if eng is not None:
                nxt.params.copy_(eng.params)
                nxt.mom.copy_(eng.mom)
                nxt.set_step(eng.step)
            eng, loaded = nxt, p
        eng.train(1)
    return eng


def test_torch_engine_equals_hand_loop_bit_for_bit(data200):
    """200 rows, B = 50: 3 steps to a pass, 7 steps cross two boundaries."""
    x, y = data200
    eng = TorchMnistEngine(_cfg(shuffle=True), x, y, torch.device("cpu"))
    eng.train(7)
    ref = _hand_loop(x, y, 7)
    assert eng.step == ref.step == 7
    assert torch.equal(eng.params, ref.params)
    assert torch.equal(eng.mom, ref.mom)
    # and the order matters: the file-order run ends elsewhere
    plain = TorchMnistEngine(_cfg(), x, y, torch.device("cpu"))
    plain.train(7)
    assert not torch.equal(plain.params, eng.params)


def test_resume_across_a_boundary_is_bit_identical(data200, tmp_path):
    """Stopped after step 4 (inside pass 1), checkpointed and resumed in a new
    engine: no checkpoint state beyond the step is needed."""
    x, y = data200
    dev = torch.device("cpu")
    whole = TorchMnistEngine(_cfg(shuffle=True), x, y, dev)
    whole.train(7)
    first = TorchMnistEngine(_cfg(shuffle=True), x, y, dev)
    first.train(5)
    path = str(tmp_path / "ck.npz")
    ckpt_mod.save(path, first.layout, first.params, first.mom, first.step)
    second = TorchMnistEngine(_cfg(shuffle=True), x, y, dev)
    step, _ = ckpt_mod.load(path, second.layout, second.params, second.mom)
    assert step == 5
    second.set_step(step)
    second.train(2)
    assert torch.equal(second.params, whole.params)
    assert torch.equal(second.mom, whole.mom)


def test_oracle_forward_backward_reads_the_pass_of_its_step(data200):
    x, y = data200
    dev = torch.device("cpu")
    eng = TorchMnistEngine(_cfg(shuffle=True), x, y, dev)
    for step in (4, 0, 6):  # passes 1, 0, 2: in any order
        eng.forward_backward(step)
        perm = rng.shuffle_perm(rng.shuffle_key(1, 0, pass_of(step, 200, 50)), 200)
        ref = TorchMnistEngine(_cfg(), x[perm], y[perm], dev)
        ref.forward_backward(step)
        assert torch.equal(eng.grads, ref.grads)
        assert np.array_equal(batch_rows(1, 0, step, 200, 50),
                              perm[batch_offset(step, 200, 50):][:50])


def test_shuffle_off_allocates_nothing(data200):
    x, y = data200
    assert C.TrainConfig().shuffle is False
    assert C.config_from_args([]).shuffle is False
    assert C.config_from_args(["--shuffle"]).shuffle is True
    eng = TorchMnistEngine(_cfg(), x, y, torch.device("cpu"))
    assert eng.shuffler is None
    eng.train(4)
    assert np.array_equal(eng.train_x.numpy(), x)
    assert np.array_equal(eng.train_y.numpy(), y)


def test_trainer_lenet5_shuffle_across_a_boundary():
    """8192 rows, B = 2048: a pass is 3 steps; 4 steps cross one boundary."""
    from mpi_tensorflow_amd.ops import functional as Fn
    from mpi_tensorflow_amd.runtime.trainer import Trainer

    cfg = C.TrainConfig(model="lenet5", device="cpu", batch_size=2048, shuffle=True, max_steps=4,
                        eval_every=0, quiet=True).validate()
    tr = Trainer(cfg)
    s = tr.run()
    eng, sh = tr.engine, tr.shard
    assert s.steps == 4 and eng.step == 4 and np.isfinite(s.final_loss)
    assert eng.shuffler.loaded == 1 == pass_of(3, 8192, 2048)
    # the working copy is the pristine shard in the order of pass 1
    perm = rng.shuffle_perm(rng.shuffle_key(cfg.seed, 0, 1), 8192)
    assert np.array_equal(eng.train_x.numpy(), sh.train_x[perm])
    assert np.array_equal(eng.train_y.numpy(), sh.train_y[perm].astype(np.int32))
    # train_prediction(): the rows step 4 reads (pass 1, offset 2048)
    off = batch_offset(4, 8192, 2048)
    assert pass_of(4, 8192, 2048) == 1 and off == 2048
    rows = perm[off:off + 2048]
    assert not np.array_equal(rows, np.arange(off, off + 2048))
    _, logits = eng.evaluate(sh.train_x[rows], np.zeros(2048, np.int64), dropout=True,
                             return_logits=True)
    assert torch.equal(tr.train_prediction(), Fn.softmax(logits))
    # ... which are not the rows of the file-order run
    plain = dataclasses.replace(cfg, shuffle=False)
    _, other = eng.evaluate(sh.train_x[off:off + 2048], np.zeros(2048, np.int64), dropout=True,
                            return_logits=True)
    assert plain.shuffle is False and not torch.equal(other, logits)
