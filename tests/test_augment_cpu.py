"""Per-pass shift / flip augmentation (--augment), host side: the spec
(config.parse_augment), the draws and the transform (utils/rng.py
augment_key / augment_params / augment_np, the definition the device mirrors),
and the PyTorch engines and the Trainer on the CPU.
"""

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.ops import functional as Fn
from mpi_tensorflow_amd.runtime.mnist_engine import TorchMnistEngine
from mpi_tensorflow_amd.runtime.shuffle import PassShuffler, batch_rows, make_shuffler
from mpi_tensorflow_amd.utils import rng
from mpi_tensorflow_amd.utils.data import batch_offset, pass_of, synthetic_rows

N, B = 200, 50  # 150 rows a pass: 3 steps


# ---------------------------------------------------------------- the spec --
def test_spec_parsing():
    assert C.parse_augment("shift:2") == (2, False, -0.5)
    assert C.parse_augment("shift:4,flip", "lenet5") == (4, True, 0.0)
    assert C.parse_augment("flip", "resnet18") == (0, True, 0.0)
    assert C.parse_augment("shift:2,fill:0") == (2, False, 0.0)
    assert C.parse_augment(" flip , shift:3 ", "mnist_cnn") == (3, True, -0.5)
    for bad in ("shift:0", "shift:-1", "shift:x", "crop", "", "shift:2,shift:3", "flip,flip",
                "fill:1", "flip:1", "shift", "shift:2,fill:nan"):
        with pytest.raises(ValueError):
            C.parse_augment(bad)
        with pytest.raises(ValueError):
            C.TrainConfig(augment=bad).validate()
    # the default fill is per model: the normalised raw 0 pixel on MNIST, else zero padding
    assert [C.parse_augment("shift:1", m)[2] for m in C.MODELS] == [-0.5, 0.0, 0.0]
    assert C.TrainConfig().augment is None and C.config_from_args([]).augment is None
    cfg = C.config_from_args(["--augment", "shift:4,flip", "--model", "lenet5"])
    assert cfg.augment == "shift:4,flip"


# --------------------------------------------------------------- the draws --
def test_augment_key_is_the_dropout_key_with_its_own_salt():
    assert rng.AUGMENT_SALT not in (0, rng.EVAL_SALT, rng.SHUFFLE_SALT)
    assert rng.augment_key(1, 3, 2) == rng.dropout_key(1, 3, 2, rng.AUGMENT_SALT)
    assert rng.augment_key(1, 0, 0) != rng.shuffle_key(1, 0, 0)


def test_augment_params_golden_values():
    """The draw written out with Python integers for a few rows."""
    def mix(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)

    key, K = rng.augment_key(1, 0, 1), 2
    rows = [0, 1, 54999, 0x7FFFFFFE]
    dy, dx, fl = rng.augment_params(key, rows, K, True)
    for j, s in enumerate(rows):
        h0 = mix(key ^ s)
        h1 = mix(h0 + rng.GOLDEN)
        h2 = mix(h1 + rng.GOLDEN)
        assert (dy[j], dx[j], fl[j]) == (h0 % 5 - 2, h1 % 5 - 2, bool(h2 >> 31))


def test_augment_params_are_pure_and_cover_their_range():
    key = rng.augment_key(1, 0, 0)
    rows = np.arange(10000)
    dy, dx, fl = rng.augment_params(key, rows, 2, True)
    # pure in (key, row): any order, any grouping
    order = np.random.default_rng(5).permutation(10000)
    for got, want in zip(rng.augment_params(key, rows[order], 2, True), (dy, dx, fl)):
        assert np.array_equal(got, want[order])
    for a, b in ((0, 17), (17, 5000), (5000, 10000)):
        for got, want in zip(rng.augment_params(key, rows[a:b], 2, True), (dy, dx, fl)):
            assert np.array_equal(got, want[a:b])
    # every shift in [-2, 2] and both flip values occur
    assert set(dy.tolist()) == set(dx.tolist()) == {-2, -1, 0, 1, 2}
    assert set(fl.tolist()) == {False, True}
    # no flip in the spec: no row is flipped, the shifts are the same
    dy2, dx2, fl2 = rng.augment_params(key, rows, 2, False)
    assert not fl2.any() and np.array_equal(dy2, dy) and np.array_equal(dx2, dx)
    # flip only: no shift
    dy0, dx0, fl0 = rng.augment_params(key, rows, 0, True)
    assert not dy0.any() and not dx0.any() and np.array_equal(fl0, fl)
    # other passes and other ranks draw differently
    for other in (rng.augment_key(1, 0, 1), rng.augment_key(1, 1, 0), rng.augment_key(2, 0, 0)):
        assert other != key
        assert not np.array_equal(rng.augment_params(other, rows, 2, True)[0], dy)


def test_ranks_agree_under_reference_quirks(data200):
    x, y = data200
    dev = torch.device("cpu")
    for quirks, same in ((True, True), (False, False)):
        cfg = C.TrainConfig(batch_size=B, augment="shift:2", reference_quirks=quirks).validate()
        a = TorchMnistEngine(cfg, x, y, dev, rank=0, world=1)
        b = TorchMnistEngine(cfg, x, y, dev, rank=3, world=1)
        assert (a.shuffler.augment_key(1) == b.shuffler.augment_key(1)) == same
        for e in (a, b):
            e.forward_backward(0)
        assert torch.equal(a.train_x, b.train_x) == same


# ----------------------------------------------------------- the transform --
def _naive(x, dy, dx, fl, fill):
    n, H, W, Cn = x.shape
    out = np.full_like(x, fill)
    for i in range(n):
        for yy in range(H):
            for xx in range(W):
                sy = yy + dy[i]
                sx = (W - 1 - xx if fl[i] else xx) + dx[i]
                if 0 <= sy < H and 0 <= sx < W:
                    out[i, yy, xx] = x[i, sy, sx]
    return out


@pytest.mark.parametrize("shape", [(3, 5, 1), (5, 7, 3)])
def test_augment_np_equals_naive_loops(shape):
    H, W, _ = shape
    K = min(H, W) - 1  # whole lines and columns of fill
    g = np.random.default_rng(H * W)
    # every (dy, dx, flip) combination once
    combos = [(a, b, f) for a in range(-K, K + 1) for b in range(-K, K + 1) for f in (False, True)]
    dy, dx, fl = (np.array(v) for v in zip(*combos))
    x = g.standard_normal((len(combos),) + shape).astype(np.float32)
    keep = x.copy()
    for fill in (-0.5, 0.0):
        want = _naive(x, dy, dx, fl, fill)
        got = rng.augment_np(x, dy, dx, fl, fill)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert (want == np.float32(fill)).all(axis=(1, 2, 3)).sum() == 0  # K < min(H, W)
        tw = rng.augment_torch(torch.from_numpy(x), dy, dx, fl, fill)
        assert tw.dtype == torch.float32 and np.array_equal(tw.numpy(), want)
    assert np.array_equal(x, keep)
    # drawn parameters as well
    pdy, pdx, pfl = rng.augment_params(0xde56f3b3, np.arange(len(combos)), K, True)
    assert np.array_equal(rng.augment_np(x, pdy, pdx, pfl, 1.5), _naive(x, pdy, pdx, pfl, 1.5))
    # no shift, no flip: the identity; a flip twice: the identity
    zero, no, yes = np.zeros(len(combos), np.int64), np.zeros(len(combos), bool), np.ones(len(combos), bool)
    assert np.array_equal(rng.augment_np(x, zero, zero, no, 9.0), x)
    once = rng.augment_np(x, zero, zero, yes, 9.0)
    assert not np.array_equal(once, x) and np.array_equal(once, x[:, :, ::-1])
    assert np.array_equal(rng.augment_np(once, zero, zero, yes, 9.0), x)


# ------------------------------------------------------------- the engines --
@pytest.fixture(scope="module")
def data200():
    return synthetic_rows("train", 0, N)


def _cfg(**kw):
    return C.TrainConfig(batch_size=B, device="cpu", **kw).validate()


def _host_pass(x, y, p, shuffle, spec="shift:2", model="mnist_cnn", seed=1, rank=0):
    """Rows and labels of pass p as the definition gives them."""
    n = x.shape[0]
    rows = rng.shuffle_perm(rng.shuffle_key(seed, rank, p), n) if shuffle else np.arange(n)
    K, flip, fill = C.parse_augment(spec, model)
    dy, dx, fl = rng.augment_params(rng.augment_key(seed, rank, p), rows, K, flip)
    return rng.augment_np(x[rows], dy, dx, fl, fill), y[rows]


@pytest.mark.parametrize("shuffle", [False, True], ids=["file-order", "shuffle"])
def test_torch_engine_working_copy_is_the_host_transform(data200, shuffle):
    x, y = data200
    eng = TorchMnistEngine(_cfg(augment="shift:2", shuffle=shuffle), x, y, torch.device("cpu"))
    assert eng.shuffler is not None and eng.shuffler.shuffle is shuffle
    seen = []
    for step in (0, 3, 4):  # passes 0, 1, 1
        eng.forward_backward(step)
        p = pass_of(step, N, B)
        hx, hy = _host_pass(x, y, p, shuffle)
        assert eng.shuffler.loaded == p
        assert np.array_equal(eng.train_x.numpy(), hx) and np.array_equal(eng.train_y.numpy(), hy)
        # ... and the gradients are those of a plain engine on these rows
        plain = TorchMnistEngine(_cfg(), hx, hy, torch.device("cpu"))
        plain.forward_backward(step)
        assert torch.equal(eng.grads, plain.grads)
        seen.append(hx)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], x)  # pass 0 too
    assert np.array_equal(eng.shuffler.src_x.numpy(), x)  # the pristine copy


@pytest.mark.parametrize("shuffle", [False, True], ids=["file-order", "shuffle"])
def test_torch_engine_train_cuts_and_resume(data200, shuffle):
    x, y = data200
    dev = torch.device("cpu")
    cfg = _cfg(augment="shift:2", shuffle=shuffle)
    whole = TorchMnistEngine(cfg, x, y, dev)
    whole.train(4)
    at4 = (whole.params.clone(), whole.mom.clone())
    whole.train(3)
    cut = TorchMnistEngine(cfg, x, y, dev)
    for k in (2, 2, 3):
        cut.train(k)
    assert cut.step == whole.step == 7
    assert torch.equal(cut.params, whole.params) and torch.equal(cut.mom, whole.mom)
    # resumed inside pass 1 from the step-4 state alone
    tail = TorchMnistEngine(cfg, x, y, dev)
    tail.params.copy_(at4[0])
    tail.mom.copy_(at4[1])
    tail.set_step(4)
    tail.train(3)
    assert torch.equal(tail.params, whole.params) and torch.equal(tail.mom, whole.mom)
    # the augmentation matters
    plain = TorchMnistEngine(_cfg(shuffle=shuffle), x, y, dev)
    plain.train(7)
    assert not torch.equal(plain.params, whole.params)


def test_make_shuffler_off_and_checks(data200):
    x, y = data200
    tx, ty = torch.from_numpy(x), torch.from_numpy(y)
    assert make_shuffler(_cfg(), 0, N, tx, ty) is None
    assert make_shuffler(_cfg(), 0, N, tx, ty, image_shape=(28, 28, 1)) is None
    eng = TorchMnistEngine(_cfg(), x, y, torch.device("cpu"))
    assert eng.shuffler is None
    only_shuffle = make_shuffler(_cfg(shuffle=True), 0, N, tx, ty)
    assert only_shuffle.augment is None and only_shuffle.shuffle
    both = make_shuffler(_cfg(shuffle=True, augment="shift:2,flip"), 0, N, tx, ty,
                         image_shape=(28, 28, 1))
    assert both.augment == (2, True, -0.5, (28, 28, 1)) and both.shuffle
    only_aug = make_shuffler(_cfg(augment="flip,fill:1"), 0, N, tx, ty, image_shape=(28, 28, 1))
    assert only_aug.augment == (0, True, 1.0, (28, 28, 1)) and not only_aug.shuffle
    assert np.array_equal(only_aug.perm(3), np.arange(N))
    with pytest.raises(ValueError):  # the shape of a row is needed
        make_shuffler(_cfg(augment="shift:2"), 0, N, tx, ty)
    with pytest.raises(ValueError):  # K >= min(H, W)
        TorchMnistEngine(_cfg(augment="shift:28"), x, y, torch.device("cpu"))
    with pytest.raises(ValueError):
        PassShuffler(1, 0, N, B, tx, ty, augment=(2, False, 0.0, (28, 14, 2)))


def test_mpipy_augment_through_the_trainer():
    """`mpipy.py --synthetic --device cpu --augment shift:2 --max-steps 4
    --eval-every 0`: main() builds this config and runs this Trainer."""
    from mpi_tensorflow_amd.runtime.trainer import Trainer

    cfg = C.config_from_args(["--synthetic", "--device", "cpu", "--augment", "shift:2",
                              "--max-steps", "4", "--eval-every", "0", "--quiet"])
    assert cfg.augment == "shift:2" and not cfg.shuffle
    tr = Trainer(cfg)
    s = tr.run()
    eng, sh = tr.engine, tr.shard
    n = sh.train_x.shape[0]
    assert s.steps == 4 and eng.step == 4 and np.isfinite(s.final_loss)
    assert eng.shuffler.loaded == 0 == pass_of(3, n, cfg.batch_size)
    hx, hy = _host_pass(sh.train_x, sh.train_y, 0, False, seed=cfg.seed)
    assert np.array_equal(eng.train_x.numpy(), hx) and np.array_equal(eng.train_y.numpy(), hy)
    # train_prediction(): the augmented rows step 4 reads
    off = batch_offset(4, n, cfg.batch_size)
    batch = hx[off:off + cfg.batch_size]
    assert not np.array_equal(batch, sh.train_x[off:off + cfg.batch_size])
    assert torch.equal(tr.train_prediction(), tr.eval_prediction(batch, dropout=True))
    _, other = eng.evaluate(sh.train_x[off:off + cfg.batch_size], np.zeros(cfg.batch_size, np.int64),
                            dropout=True, return_logits=True)
    assert not torch.equal(tr.train_prediction(), Fn.softmax(other))


def test_trainer_lenet5_augment_and_shuffle_across_a_boundary():
    """8192 rows, B = 2048: a pass is 3 steps; step 4 reads pass 1."""
    from mpi_tensorflow_amd.runtime.trainer import Trainer

    cfg = C.TrainConfig(model="lenet5", device="cpu", batch_size=2048, shuffle=True,
                        augment="shift:4,flip", max_steps=4, eval_every=0, quiet=True).validate()
    tr = Trainer(cfg)
    tr.run()
    eng, sh = tr.engine, tr.shard
    assert eng.step == 4 and eng.shuffler.loaded == 1
    hx, hy = _host_pass(sh.train_x, sh.train_y, 1, True, "shift:4,flip", "lenet5", seed=cfg.seed)
    assert np.array_equal(eng.train_x.numpy(), hx)
    assert np.array_equal(eng.train_y.numpy(), hy.astype(np.int32))
    off = batch_offset(4, 8192, 2048)
    assert np.array_equal(batch_rows(cfg.seed, 0, 4, 8192, 2048),
                          rng.shuffle_perm(rng.shuffle_key(cfg.seed, 0, 1), 8192)[off:off + 2048])
    assert torch.equal(tr.train_prediction(),
                       tr.eval_prediction(hx[off:off + 2048], dropout=True))
