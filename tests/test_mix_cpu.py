"""--mix and --label-smoothing without a GPU: the parsers, the table and the
draws of the definition (docs/ACCURACY.md) worked by hand, the numpy / torch
oracles, the PyTorch engines of the three models against engines fed host-mixed
rows, resume, the command line and two gloo ranks."""

import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.ops import functional as Fn
from mpi_tensorflow_amd.runtime.mnist_engine import TorchMnistEngine
from mpi_tensorflow_amd.runtime.shuffle import make_shuffler
from mpi_tensorflow_amd.utils import rng
from mpi_tensorflow_amd.utils.data import batch_offset, pass_of, synthetic_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
M32 = 0xFFFFFFFF


# ----------------------------------------------------------------- parsers ----
def test_parse_mix_accepts():
    assert C.parse_mix("mixup:50") == ("mixup", 50.0)
    assert C.parse_mix("cutmix:12.5") == ("cutmix", 12.5)
    assert C.parse_mix(" mixup:1e-3 ") == ("mixup", 1e-3)


@pytest.mark.parametrize("spec,names", [
    ("", "empty"), (None, "empty"), ("mixup", "'mixup'"), ("mixup:", "'mixup:'"),
    ("mixup:x", "'mixup:x'"), ("blend:10", "'blend:10'"), ("mixup:nan", "'mixup:nan'"),
    ("mixup:inf", "'mixup:inf'"), ("mixup:10,mixup:20", "twice"),
    ("mixup:10,cutmix:10", "both"), ("mixup:0", "(0, 50]"), ("cutmix:50.5", "(0, 50]"),
    ("mixup:-3", "(0, 50]"),
])
def test_parse_mix_rejects_and_names_the_item(spec, names):
    with pytest.raises(ValueError) as e:
        C.parse_mix(spec)
    assert names in str(e.value)


def test_label_smoothing_range():
    assert C.TrainConfig(label_smoothing=0.0).validate().label_smoothing == 0.0
    assert C.TrainConfig(label_smoothing=0.999).validate().label_smoothing == 0.999
    for bad in (1.0, -0.1, float("nan"), 2.0):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            C.TrainConfig(label_smoothing=bad).validate()
    with pytest.raises(ValueError, match="mix spec"):
        C.TrainConfig(mix="mixup").validate()


def test_command_line_flags_and_predict_refuses_them(tmp_path):
    cfg = C.config_from_args(["--mix", "cutmix:25", "--label-smoothing", "0.1"])
    assert cfg.mix == "cutmix:25" and cfg.label_smoothing == 0.1
    plain = C.config_from_args([])
    assert plain.mix is None and plain.label_smoothing == 0.0
    ck = str(tmp_path / "c.npz")
    for extra in (["--mix", "mixup:50"], ["--label-smoothing", "0.1"]):
        with pytest.raises(ValueError, match="training-only"):
            C.config_from_args(["--resume", ck, "--predict", "test"] + extra)


# -------------------------------------------------------------- the table ----
def test_table_mixup():
    t = rng.mix_table("mixup", 50, 28, 28)
    assert t.shape == (3, 129) and t.dtype == np.int32
    assert tuple(t[:, 0]) == (0, 0, 0)
    assert (np.diff(t[0]) >= 0).all() and t[0].max() <= 32768 + 1
    assert t[0, 128] == 32768 and not t[1:].any()
    for M_ in (10, 12.5, 33.3):
        Mq = int(np.rint(65536 * M_ / 100))
        t = rng.mix_table("mixup", M_, 5, 7)
        assert t[0, 128] == Mq  # (Mq 128 + 64) >> 7
        assert [int(v) for v in t[0]] == [(Mq * l + 64) >> 7 for l in range(129)]


def test_table_cutmix():
    for (H, W), M_ in (((28, 28), 50), ((32, 32), 10), ((5, 7), 50)):
        t = rng.mix_table("cutmix", M_, H, W).astype(np.int64)
        assert tuple(t[:, 0]) == (0, 0, 0)
        assert (t[1] <= H).all() and (t[2] <= W).all() and (np.diff(t[1]) >= 0).all()
        assert np.array_equal(t[0], np.rint(65536.0 * t[1] * t[2] / (H * W)).astype(np.int64))
    # 4 x 4 at M = 50 by hand: a = 256 l; the side is floor(4 sqrt(l / 256) + 0.5)
    t = rng.mix_table("cutmix", 50, 4, 4)
    assert int(np.rint(65536 * 50 / 100)) == 32768
    for l, side in ((0, 0), (3, 0), (4, 1), (35, 1), (36, 2), (99, 2), (100, 3), (128, 3)):
        assert math.floor(4 * math.sqrt(l / 256) + 0.5) == side
        assert (t[1, l], t[2, l]) == (side, side), l
        assert t[0, l] == round(65536 * side * side / 16)
    # 28 x 28 at M = 50: level 128 is a = 32768, side floor(28 sqrt(.5) + .5) = 20
    t = rng.mix_table("cutmix", 50, 28, 28)
    assert (t[1, 128], t[2, 128], t[0, 128]) == (20, 20, round(65536 * 400 / 784))
    assert (t[1, 64], t[2, 64]) == (14, 14) and t[0, 64] == 16384


# --------------------------------------------------------------- the draws ----
def _mix_py(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def _feistel_py(x, h, rk):
    mask = (1 << h) - 1
    l, r = x >> h, x & mask
    for k in rk:
        l, r = r, l ^ (_mix_py(r ^ k) & mask)
    return (l << h) | r


def test_salts_and_key():
    salts = [rng.EVAL_SALT, rng.SHUFFLE_SALT, rng.AUGMENT_SALT, rng.MIX_SALT]
    assert len(set(salts)) == 4
    assert rng.mix_key(1, 0, 3) == rng.dropout_key(1, 0, 3, rng.MIX_SALT)
    keys = {rng.mix_key(1, 0, 3), rng.augment_key(1, 0, 3), rng.shuffle_key(1, 0, 3),
            rng.mix_key(1, 1, 3), rng.mix_key(1, 0, 4), rng.mix_key(2, 0, 3)}
    assert len(keys) == 6


@pytest.mark.parametrize("kind", ["mixup", "cutmix"])
def test_draws_with_python_integers(kind):
    n, H, W, key = 5, 28, 20, 0xde56f3b3
    tab = rng.mix_table(kind, 50, H, W)
    j, lamq, cy, cx, bh, bw = rng.mix_params(key, n, tab, H, W)
    pkey = _mix_py(key ^ rng.GOLDEN)
    rk = [_mix_py((pkey + r * rng.GOLDEN) & M32) for r in range(4)]
    bits = 4  # n - 1 = 4 has 3 bits, made even
    for i in range(n):
        g0 = _mix_py(key ^ i)
        g1 = _mix_py((g0 + rng.GOLDEN) & M32)
        g2 = _mix_py((g1 + rng.GOLDEN) & M32)
        level = g0 % 129
        assert lamq[i] == 65536 - int(tab[0, level])
        assert (bh[i], bw[i]) == (tab[1, level], tab[2, level])
        assert cy[i] == g1 % (H - int(bh[i]) + 1) and cx[i] == g2 % (W - int(bw[i]) + 1)
        x = _feistel_py(i, bits // 2, rk)
        while x >= n:
            x = _feistel_py(x, bits // 2, rk)
        assert j[i] == x
    assert sorted(j.tolist()) == list(range(n))
    assert np.array_equal(j, rng.shuffle_perm(pkey, n))


# ------------------------------------------------------- hand-worked cases ----
def test_mixup_of_two_images_by_hand():
    A = np.array([[1.0, 2.0, 3.0, 4.0], [10.0, 20.0, 30.0, 40.0]], np.float32).reshape(2, 2, 2, 1)
    y = np.array([7, 3])
    z = np.zeros(2, np.int64)
    # row 0 keeps 3/4 of itself (wq = 16384), row 1 is at level 0
    prm = (np.array([1, 0]), np.array([49152, 65536]), z, z, z, z)
    x, y1, y2, lam = rng.mix_np(A, y, prm, "mixup")
    assert x.dtype == np.float32 and lam.dtype == np.float32
    assert np.array_equal(x[0].ravel(), [3.25, 6.5, 9.75, 13.0])
    assert np.array_equal(x[1], A[1])
    assert np.array_equal(lam, [0.75, 1.0])
    assert np.array_equal(y1, [7, 3]) and np.array_equal(y2, [3, 7])


def test_mixup_products_and_sum_are_single_fp32_operations():
    g = np.random.default_rng(0)
    A = g.standard_normal((2, 3, 3, 2)).astype(np.float32)
    lamq = np.array([65536 - 21845, 65536 - 7])
    prm = (np.array([1, 0]), lamq, *(np.zeros(2, np.int64),) * 4)
    x = rng.mix_np(A, np.zeros(2, np.int64), prm, "mixup")[0]
    for i, j in ((0, 1), (1, 0)):
        lam = np.float32(lamq[i]) * np.float32(2.0 ** -16)
        w = np.float32(65536 - lamq[i]) * np.float32(2.0 ** -16)
        want = (np.float32(lam) * A[i]).astype(np.float32) + (np.float32(w) * A[j]).astype(np.float32)
        assert np.array_equal(x[i], want)
        assert float(lam) + float(w) == 1.0  # both exact in fp32


def test_cutmix_box_at_a_corner_and_nowhere_else():
    A = np.stack([np.full((4, 4, 2), 1.0, np.float32), np.full((4, 4, 2), 5.0, np.float32)])
    y = np.array([2, 9])
    one = np.ones(2, np.int64)
    # row 0: a 2 x 3 box at the bottom right corner; row 1: no box
    prm = (np.array([1, 0]), np.array([65536 - 24576, 65536]), np.array([2, 0]), np.array([1, 0]),
           np.array([2, 0]), np.array([3, 0]))
    x, y1, y2, lam = rng.mix_np(A, y, prm, "cutmix")
    box = np.zeros((4, 4), bool)
    box[2:4, 1:4] = True
    assert (x[0][box] == 5.0).all() and (x[0][~box] == 1.0).all()
    assert np.array_equal(x[1], A[1])
    assert np.array_equal(lam, [0.625, 1.0]) and np.array_equal(y2, [9, 2]) and one.all()


@pytest.mark.parametrize("kind", ["mixup", "cutmix"])
def test_level_zero_returns_the_pass(kind):
    x, y = synthetic_rows("train", 0, 9)
    z = np.zeros(9, np.int64)
    prm = (rng.shuffle_perm(5, 9), np.full(9, 65536), z, z, z, z)
    out, y1, y2, lam = rng.mix_np(x, y, prm, kind)
    assert np.array_equal(out, x) and np.array_equal(y1, y) and (lam == 1.0).all()
    assert np.array_equal(y2, y[prm[0]])


# ----------------------------------------------------------------- oracles ----
@pytest.mark.parametrize("kind,M_", [("mixup", 50), ("mixup", 10), ("cutmix", 50), ("cutmix", 10)])
@pytest.mark.parametrize("shape", [(28, 28, 1), (5, 7, 3)])
def test_mix_torch_equals_mix_np(kind, M_, shape):
    n = 37
    g = np.random.default_rng(n)
    A = g.standard_normal((n,) + shape).astype(np.float32)
    y = g.integers(0, 10, n)
    prm = rng.mix_params(11, n, rng.mix_table(kind, M_, shape[0], shape[1]), shape[0], shape[1])
    want = rng.mix_np(A, y, prm, kind)
    got = rng.mix_torch(torch.from_numpy(A), torch.from_numpy(y), prm, kind)
    for a, b in zip(got, want):
        assert np.array_equal(a.numpy(), b)
    assert not np.array_equal(want[0], A)


def test_soft_targets():
    y1, y2 = np.array([0, 3, 3, 9]), np.array([1, 3, 0, 2])
    lam = np.array([0.75, 0.5, 1.0, 0.625], np.float32)
    for eps in (0.0, 0.1):
        t = rng.soft_targets(y1, y2, lam, eps, 10)
        assert t.dtype == np.float64 and t.shape == (4, 10)
        assert np.allclose(t.sum(1), 1.0, rtol=0, atol=1e-15)
    t = rng.soft_targets(y1, y2, lam, 0.1, 10)
    assert t[0, 0] == pytest.approx(0.9 * 0.75 + 0.01) and t[0, 1] == pytest.approx(0.9 * 0.25 + 0.01)
    assert t[1, 3] == pytest.approx(0.91) and t[0, 5] == pytest.approx(0.01)
    onehot = rng.soft_targets(y1, None, None, 0.0, 10)
    assert np.array_equal(onehot, np.eye(10)[y1])
    assert np.array_equal(rng.soft_targets(y1, y2, np.ones(4), 0.0, 10), np.eye(10)[y1])


def test_cross_entropy_routes():
    g = torch.Generator().manual_seed(0)
    z = torch.randn(6, 10, generator=g)
    y1, y2 = torch.randint(0, 10, (6,), generator=g), torch.randint(0, 10, (6,), generator=g)
    lam = torch.tensor([1.0, 0.5, 0.75, 0.625, 1.0, 0.5])
    assert torch.equal(Fn.cross_entropy(z, y1), torch.nn.functional.cross_entropy(z, y1))
    t = torch.from_numpy(rng.soft_targets(y1.numpy(), y2.numpy(), lam.numpy(), 0.1, 10)).float()
    want = -(t * torch.log_softmax(z, 1)).sum(1).mean()
    assert torch.equal(Fn.cross_entropy(z, y1, y2, lam, 0.1), want)
    # the hard label is the soft formula's eps = 0, lam = 1
    assert torch.allclose(Fn.cross_entropy(z, y1, y1, torch.ones(6), 0.0), Fn.cross_entropy(z, y1))
    with pytest.raises(ValueError, match="labels2"):
        Fn.cross_entropy(z, y1, None, lam)
    with pytest.raises(ValueError, match="labels2"):  # never silently ignored
        Fn.cross_entropy(z, y1, y2, None, 0.1)


# ---------------------------------------------------------- torch engines ----
N, B = 24, 8  # the EMA / augment CPU tests' shard: 16 rows a pass, 2 steps


def _cfg(**kw):
    kw.setdefault("batch_size", B)
    kw.setdefault("device", "cpu")
    kw.setdefault("backend", "torch")
    return C.TrainConfig(**kw).validate()


def _host_pass(x, y, p, cfg, rank=0):
    """(x, y1, y2, lam) of pass p as the definition gives them."""
    n = x.shape[0]
    rows = (rng.shuffle_perm(rng.shuffle_key(cfg.seed, rank, p), n) if cfg.shuffle
            else np.arange(n))
    hx, hy = x[rows], np.asarray(y)[rows]
    if cfg.augment is not None:
        s = C.parse_augment_spec(cfg.augment, cfg.model)
        hx = rng.augment_np(hx, *rng.augment_params(rng.augment_key(cfg.seed, rank, p), rows, s.K,
                                                    s.flip), s.fill)
    if cfg.mix is None:
        return hx, hy, hy, np.ones(n, np.float32)
    kind, M_ = C.parse_mix(cfg.mix)
    H, W = x.shape[1:3]
    prm = rng.mix_params(rng.mix_key(cfg.seed, rank, p), n, rng.mix_table(kind, M_, H, W), H, W)
    return rng.mix_np(hx, hy, prm, kind)


def _soft_loss(hy, hy2, hlam, eps, off, logits):
    z = slice(off, off + logits.shape[0])
    t = torch.from_numpy(rng.soft_targets(hy[z], hy2[z], hlam[z], eps, logits.shape[1]))
    return -(t.to(logits.dtype) * torch.log_softmax(logits, 1)).sum(1).mean()


FLAG_SETS = [dict(mix="mixup:50", label_smoothing=0.1), dict(mix="cutmix:50"),
             dict(label_smoothing=0.1),
             dict(mix="mixup:25", label_smoothing=0.05, shuffle=True, augment="shift:2")]
FLAG_IDS = ["mixup+ls", "cutmix", "ls", "mixup+shuffle+augment"]


@pytest.fixture(scope="module")
def shard24():
    return synthetic_rows("train", 0, N)


@pytest.mark.parametrize("flags", FLAG_SETS, ids=FLAG_IDS)
def test_torch_mnist_engine_equals_hand_loop(shard24, flags):
    """3 steps (passes 0, 0, 1) equal plain engines fed the host-mixed rows whose
    loss is the soft-target formula on float64 targets."""
    x, y = shard24
    cfg = _cfg(**flags)
    eng = TorchMnistEngine(cfg, x, y, CPU)
    assert (eng.shuffler is not None) == (cfg.mix is not None or cfg.shuffle)
    p0 = eng.params.clone()
    eng.train(3)
    hand = None
    for p, k in ((0, 2), (1, 1)):
        hx, hy, hy2, hlam = _host_pass(x, y, p, cfg)
        nxt = TorchMnistEngine(_cfg(), hx, hy, CPU)
        assert nxt.shuffler is None and not nxt.soft_targets
        nxt.soft_loss_torch = (lambda logits, yb, off, a=(hy, hy2, hlam):
                               _soft_loss(*a, cfg.label_smoothing, off, logits))
        if hand is not None:
            nxt.params.copy_(hand.params)
            nxt.mom.copy_(hand.mom)
            nxt.set_step(hand.step)
        hand = nxt
        hand.train(k)
    assert eng.step == hand.step == 3
    assert torch.equal(eng.params, hand.params) and torch.equal(eng.mom, hand.mom)
    assert not torch.equal(eng.params, p0)
    plain = TorchMnistEngine(_cfg(), x, y, CPU)
    plain.train(3)
    assert not torch.equal(plain.params, eng.params)


@pytest.mark.parametrize("flags", FLAG_SETS[:2], ids=FLAG_IDS[:2])
def test_lenet5_torch_path_equals_hand_loop(monkeypatch, flags):
    """The generic engine's PyTorch path (LeNet-5) the same way."""
    from mpi_tensorflow_amd.runtime.generic_engine import GenericEngine

    x, y = synthetic_rows("train", 0, N, shape=(32, 32, 3))
    cfg = _cfg(model="lenet5", **flags)
    eng = GenericEngine(cfg, x, y, CPU)
    assert eng.soft_targets and eng.y2b is None
    eng.train(3)
    hand = None
    for p, k in ((0, 2), (1, 1)):
        hx, hy, hy2, hlam = _host_pass(x, y, p, cfg)
        nxt = GenericEngine(_cfg(model="lenet5"), hx, hy, CPU)
        if hand is not None:
            with torch.no_grad():
                nxt.params.copy_(hand.params)
            nxt.mom.copy_(hand.mom)
            nxt.set_step(hand.step)
        hand = nxt
        monkeypatch.setattr(Fn, "cross_entropy", lambda logits, yb, *a, e=hand, h=(hy, hy2, hlam):
                            _soft_loss(*h, cfg.label_smoothing, batch_offset(e.step, N, B), logits))
        hand.train(k)
        monkeypatch.undo()
    assert eng.step == hand.step == 3
    assert torch.equal(eng.params.detach(), hand.params.detach()) and torch.equal(eng.mom, hand.mom)


def test_resnet18_torch_path_takes_the_flags():
    from mpi_tensorflow_amd.runtime.generic_engine import GenericEngine

    x, y = synthetic_rows("train", 0, 12, shape=(32, 32, 3))
    a = GenericEngine(_cfg(model="resnet18", batch_size=4, mix="mixup:50", label_smoothing=0.1), x, y,
                      CPU)
    b = GenericEngine(_cfg(model="resnet18", batch_size=4), x, y, CPU)
    a.train(1)
    b.train(1)
    assert torch.isfinite(a.params).all() and not torch.equal(a.params.detach(), b.params.detach())
    assert a.loss_value() != b.loss_value()


def test_shuffler_is_made_for_mix_alone_and_carries_the_pad_rows(shard24):
    x, y = shard24
    assert make_shuffler(_cfg(), 0, N, torch.from_numpy(x), torch.from_numpy(y)) is None
    assert make_shuffler(_cfg(label_smoothing=0.1), 0, N, torch.from_numpy(x),
                         torch.from_numpy(y)) is None
    wx = torch.cat([torch.from_numpy(x), torch.zeros(3, 28, 28, 1)])
    wy = torch.cat([torch.from_numpy(y), torch.zeros(3, dtype=torch.int64)])
    cfg = _cfg(mix="mixup:50")
    sh = make_shuffler(cfg, 0, N, wx, wy)
    assert sh is not None and not sh.shuffle and sh.augment is None and sh.mix[:2] == ("mixup", 50.0)
    sh.ensure(2)
    hx, hy, hy2, hlam = _host_pass(x, y, 1, cfg)
    assert np.array_equal(sh.work_x[:N].numpy(), hx) and np.array_equal(sh.work_y[:N].numpy(), hy)
    assert np.array_equal(sh.work_y2[:N].numpy(), hy2) and np.array_equal(sh.work_lam[:N].numpy(), hlam)
    assert sh.work_y2.shape[0] == sh.work_lam.shape[0] == N + 3
    assert int(sh.work_y2[N:].abs().sum()) == 0 and bool((sh.work_lam[N:] == 1).all())
    assert float(sh.work_x[N:].abs().sum()) == 0.0
    assert np.array_equal(sh.src_x.numpy(), x)  # the pristine copy is not written


# ------------------------------------------------------------------ resume ----
def _trainer(**kw):
    from mpi_tensorflow_amd.runtime.trainer import Trainer

    kw.setdefault("synthetic", True)
    kw.setdefault("quiet", True)
    return Trainer(_cfg(**kw))


def test_resume_in_mid_pass_continues_bit_identically(tmp_path):
    flags = dict(mix="mixup:50", label_smoothing=0.1, shuffle=True, augment="shift:2")
    ck = str(tmp_path / "c.npz")
    tr = _trainer(**flags)
    n = tr.shard.train_x.shape[0]
    k = (n - B) // B + 3  # three steps into pass 1
    assert pass_of(k, n, B) == 1 and pass_of(k - 1, n, B) == 1
    tr.engine.train(k)
    tr.save_checkpoint(ck)
    with np.load(ck, allow_pickle=False) as z:
        assert not [f for f in z.files if "mix" in f.lower() or "lam" in f.lower()]
    tr.engine.train(3)
    want = (tr.engine.params.clone(), tr.engine.mom.clone())
    tr.watchdog.stop()
    tr = _trainer(resume=ck, **flags)
    assert tr.engine.step == k
    tr.engine.train(3)
    tr.watchdog.stop()
    assert torch.equal(tr.engine.params, want[0]) and torch.equal(tr.engine.mom, want[1])


def test_train_prediction_sees_the_mixed_rows():
    flags = dict(mix="cutmix:50", shuffle=True, augment="shift:2")
    tr = _trainer(dropout_keep=1.0, **flags)
    eng = tr.engine
    eng.set_step(3)
    got = tr.train_prediction()
    eng.shuffler.ensure(3)
    n = tr.shard.train_x.shape[0]
    off = batch_offset(3, n, B)
    want = tr.eval_prediction(eng.train_x[off:off + B].numpy(), dropout=True)
    tr.watchdog.stop()
    assert torch.equal(torch.as_tensor(got), torch.as_tensor(want))


# ------------------------------------------------------------ command line ----
def _mpipy(*args, timeout=600):
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="",
               HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, "mpipy.py", "--synthetic", "--backend", "torch", "--device", "cpu", *args]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def _json_line(out, key):
    return json.loads([ln for ln in out.splitlines() if ln.startswith('{"%s"' % key)][-1])[key]


def test_cli_records_the_flags_only_when_set(tmp_path):
    mj, mj0 = str(tmp_path / "m.jsonl"), str(tmp_path / "m0.jsonl")
    common = ("--batch-size", "8", "--max-steps", "3", "--eval-every", "0")
    out = _mpipy(*common, "--mix", "mixup:50", "--label-smoothing", "0.1", "--metrics-jsonl", mj)
    summ = _json_line(out, "summary")
    assert summ["mix"] == "mixup:50" and summ["label_smoothing"] == 0.1
    with open(mj) as f:
        final = [json.loads(ln) for ln in f if ln.strip()][-1]
    assert final["final"] and final["mix"] == "mixup:50" and final["label_smoothing"] == 0.1
    out0 = _mpipy(*common, "--metrics-jsonl", mj0)
    summ0 = _json_line(out0, "summary")
    assert "mix" not in summ0 and "label_smoothing" not in summ0
    with open(mj0) as f:
        final0 = [json.loads(ln) for ln in f if ln.strip()][-1]
    assert "mix" not in final0 and "label_smoothing" not in final0
    assert summ0["final_loss"] != summ["final_loss"]


# ---------------------------------------------------------- two gloo ranks ----
def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker_mix(rank, world, port, out_dir, steps):
    torch.set_num_threads(2)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    for k in ("OMPI_COMM_WORLD_RANK", "PMI_RANK", "SLURM_PROCID"):
        os.environ.pop(k, None)
    from mpi_tensorflow_amd.parallel import dist as D
    from mpi_tensorflow_amd.parallel.comm import make_comm
    from mpi_tensorflow_amd.parallel.sync import replicas_identical

    di = D.init("cpu")
    comm = make_comm(di, CPU)
    x, y = synthetic_rows("train", rank * N, (rank + 1) * N)
    eng = TorchMnistEngine(_cfg(mix="mixup:50", label_smoothing=0.1), x, y, CPU, rank, world, comm)
    assert eng.grad_sync
    eng.train(steps)
    same = replicas_identical(eng.params) and replicas_identical(eng.mom)
    np.save(os.path.join(out_dir, f"p{rank}.npy"), eng.params.numpy())
    np.save(os.path.join(out_dir, f"lam{rank}.npy"), eng.shuffler.work_lam.numpy())
    np.save(os.path.join(out_dir, f"j{rank}.npy"), eng.shuffler.mix_params(0)[0])
    with open(os.path.join(out_dir, f"same{rank}"), "w") as f:
        f.write(str(same))
    D.shutdown()


def test_two_ranks_stay_identical_and_draw_different_partners(tmp_path):
    world, port = 2, _free_port()
    mp.spawn(_worker_mix, args=(world, port, str(tmp_path), 3), nprocs=world, join=True)
    assert np.array_equal(np.load(tmp_path / "p0.npy"), np.load(tmp_path / "p1.npy"))
    assert open(tmp_path / "same0").read() == "True" and open(tmp_path / "same1").read() == "True"
    assert not np.array_equal(np.load(tmp_path / "j0.npy"), np.load(tmp_path / "j1.npy"))
    assert not np.array_equal(np.load(tmp_path / "lam0.npy"), np.load(tmp_path / "lam1.npy"))
