"""Rotate / scale / cutout in --augment, host side: the spec
(config.parse_augment_spec, and parse_augment which keeps refusing them), the
tables, the draws and the transform (utils/rng.py affine_tables / affine_params
/ affine_np, the definition the device mirrors bit for bit), and the PyTorch
engines and the Trainer on the CPU.
"""

import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.runtime.mnist_engine import TorchMnistEngine
from mpi_tensorflow_amd.runtime.shuffle import PassShuffler, make_shuffler
from mpi_tensorflow_amd.utils import rng
from mpi_tensorflow_amd.utils.data import batch_offset, pass_of, synthetic_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, B = 200, 50  # 150 rows a pass: 3 steps
SPEC = "shift:2,rotate:10,scale:10"
IDENTITY = [65536, 0, 0, 65536]


# ---------------------------------------------------------------- the spec --
def test_spec_parsing():
    S = C.AugmentSpec
    assert C.parse_augment_spec("shift:2") == S(2, False, -0.5, 0.0, 0.0, 0)
    assert C.parse_augment_spec("rotate:10") == S(0, False, -0.5, 10.0, 0.0, 0)
    assert C.parse_augment_spec("scale:7.5", "lenet5") == S(0, False, 0.0, 0.0, 7.5, 0)
    assert C.parse_augment_spec("cutout:4,fill:1", "lenet5") == S(0, False, 1.0, 0.0, 0.0, 4)
    assert (C.parse_augment_spec(" cutout:8 , scale:50,flip,rotate:45 ,shift:3", "resnet18")
            == S(3, True, 0.0, 45.0, 50.0, 8))
    assert not C.parse_augment_spec("shift:2,flip").affine
    for s in ("rotate:1", "scale:1", "cutout:1"):
        assert C.parse_augment_spec(s).affine
    with pytest.raises(dataclasses.FrozenInstanceError):
        C.parse_augment_spec("flip").K = 3
    for bad in ("rotate:0", "rotate:46", "rotate:-5", "rotate:nan", "rotate", "rotate:x",
                "scale:0", "scale:51", "scale:-1", "scale:inf", "scale",
                "cutout:0", "cutout:-2", "cutout:2.5", "cutout",
                "rotate:5,rotate:5", "scale:5,scale:6", "cutout:2,cutout:2", "flip,flip",
                "fill:1", "", "shear:3", "shift:0", "shift:2,fill:nan"):
        with pytest.raises(ValueError):
            C.parse_augment_spec(bad)
        with pytest.raises(ValueError):
            C.TrainConfig(augment=bad).validate()
    cfg = C.config_from_args(["--augment", "shift:2,rotate:10,scale:10,cutout:4"])
    assert cfg.augment == "shift:2,rotate:10,scale:10,cutout:4"


def test_parse_augment_keeps_its_triples_and_refuses_the_new_items():
    assert C.parse_augment("shift:2") == (2, False, -0.5)
    assert C.parse_augment("shift:4,flip", "lenet5") == (4, True, 0.0)
    assert C.parse_augment("flip,fill:1", "resnet18") == (0, True, 1.0)
    for spec in ("rotate:5", "shift:2,scale:10", "flip,cutout:4"):
        with pytest.raises(ValueError, match="training-only"):
            C.parse_augment(spec)
    for bad in ("fill:1", "shift:0", "flip,flip", "crop", ""):
        with pytest.raises(ValueError):
            C.parse_augment(bad)


def test_predict_tta_rejects_the_new_items(tmp_path):
    ck = tmp_path / "ck.pt"
    ck.write_bytes(b"")
    with pytest.raises(ValueError, match="--predict-tta.*training-only"):
        C.TrainConfig(predict="test", resume=str(ck), predict_tta="rotate:5").validate()
    C.TrainConfig(predict="test", resume=str(ck), predict_tta="shift:1").validate()


# -------------------------------------------------------------- the tables --
def test_tables():
    T = rng.affine_tables(15.0, 15.0)
    assert T.dtype == np.int32 and T.shape == (3, 129)
    assert T[:, 64].tolist() == [65536, 0, 65536]
    assert np.array_equal(T[0], T[0][::-1]) and np.array_equal(T[1], -T[1][::-1])
    assert T[1][0] < 0 < T[1][128] and np.all(np.diff(T[1]) > 0)
    assert T[2][0] > 65536 > T[2][128] and np.all(np.diff(T[2]) < 0)
    # the ends written out
    assert T[0][128] == round(np.cos(np.radians(15.0)) * 65536)
    assert T[1][128] == round(np.sin(np.radians(15.0)) * 65536)
    assert T[2][0] == round(65536 / 0.85) and T[2][128] == round(65536 / 1.15)
    # rotate / scale absent: every level is the identity
    Z = rng.affine_tables(0.0, 0.0)
    assert (Z[0] == 65536).all() and (Z[1] == 0).all() and (Z[2] == 65536).all()
    # the widest spec keeps |m| <= 2^17
    assert np.abs(rng.affine_tables(45.0, 50.0)).max() == 131072


# --------------------------------------------------------------- the draws --
def test_affine_params_golden_values():
    """The draws written out with Python integers for a few rows."""
    def mix(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)

    H, W = 28, 30
    spec = C.parse_augment_spec("shift:2,flip,rotate:15,scale:20,cutout:5")
    T = rng.affine_tables(15.0, 20.0).tolist()
    key = rng.augment_key(1, 0, 1)
    rows = [0, 1, 54999, 0x7FFFFFFE]
    q = rng.affine_params(key, rows, spec, H, W)
    for j, s in enumerate(rows):
        h = [mix(key ^ s)]
        for _ in range(6):
            h.append(mix(h[-1] + rng.GOLDEN))
        assert (q.dy[j], q.dx[j], q.flipped[j]) == (h[0] % 5 - 2, h[1] % 5 - 2, bool(h[2] >> 31))
        ia, ib = h[3] % 129, h[4] % 129
        assert (q.ia[j], q.ib[j]) == (ia, ib)
        r = lambda v: (v + 32768) >> 16  # noqa: E731
        m = [r(T[0][ia] * T[2][ib]), r(T[1][ia] * T[2][ib]), r(-T[1][ia] * T[2][ib]),
             r(T[0][ia] * T[2][ib])]
        assert q.m[j].tolist() == m
        assert q.cutout[0] == 5
        assert (q.cutout[1][j], q.cutout[2][j]) == (h[5] % (H - 4), h[6] % (W - 4))


def test_affine_params_extend_the_shift_flip_draws():
    key, rows = rng.augment_key(1, 0, 0), np.arange(5000)
    spec = C.parse_augment_spec("shift:2,flip,rotate:10,scale:10,cutout:4")
    q = rng.affine_params(key, rows, spec, 28, 28)
    # the shift and flip of a row do not change when rotate / scale are added
    for got, want in zip((q.dy, q.dx, q.flipped), rng.augment_params(key, rows, 2, True)):
        assert np.array_equal(got, want)
    # pure in (key, row)
    order = np.random.default_rng(3).permutation(5000)
    q2 = rng.affine_params(key, rows[order], spec, 28, 28)
    assert np.array_equal(q2.m, q.m[order]) and np.array_equal(q2.cutout[1], q.cutout[1][order])
    # every level, and every cutout corner that fits
    assert set(q.ia.tolist()) == set(q.ib.tolist()) == set(range(129))
    assert set(q.cutout[1].tolist()) == set(q.cutout[2].tolist()) == set(range(25))
    # rotate / scale absent: identity matrices, the draw still taken; no cutout
    q0 = rng.affine_params(key, rows, C.parse_augment_spec("shift:2,cutout:4"), 28, 28)
    assert (q0.m == np.array(IDENTITY)).all() and np.array_equal(q0.ia, q.ia)
    assert np.array_equal(q0.cutout[2], q.cutout[2])
    assert rng.affine_params(key, rows, C.parse_augment_spec("rotate:10"), 28, 28).cutout is None
    # other passes and ranks draw differently
    for other in (rng.augment_key(1, 0, 1), rng.augment_key(1, 1, 0)):
        assert not np.array_equal(rng.affine_params(other, rows, spec, 28, 28).ia, q.ia)


# ----------------------------------------------------------- the transform --
SHAPES = [(28, 28, 1), (32, 32, 3), (5, 7, 3), (3, 5, 1), (224, 224, 3)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_identity_matrix_is_the_shift_flip_transform(shape):
    H, W, _ = shape
    n, K = 6, min(H, W) - 1
    x = np.random.default_rng(H * W).standard_normal((n,) + shape).astype(np.float32)
    dy, dx, fl = rng.augment_params(0xde56f3b3, np.arange(n), K, True)
    got = rng.affine_np(x, [IDENTITY] * n, dy, dx, fl, -0.5)
    assert got.dtype == np.float32 and np.array_equal(got, rng.augment_np(x, dy, dx, fl, -0.5))
    assert dy.any() and dx.any() and set(fl.tolist()) == {False, True}


def test_quarter_turn_is_rot90():
    img = np.random.default_rng(1).standard_normal((1, 6, 6, 2)).astype(np.float32)
    z = np.zeros(1, np.int64)
    got = rng.affine_np(img, [[0, 65536, -65536, 0]], z, z, [False], 9.0)
    assert np.array_equal(got[0], np.rot90(img[0], -1))  # clockwise as displayed (y down)
    # a positive angle level: the picture's top row moves towards the right edge
    T = rng.affine_tables(45.0, 0.0)
    m = [[T[0][128], T[1][128], -T[1][128], T[0][128]]]
    bar = np.zeros((1, 9, 9, 1), np.float32)
    bar[0, 0, 4] = 1.0  # a dot at the top centre
    out = rng.affine_np(bar, m, z, z, [False], 0.0)[0, :, :, 0]
    y, x = np.unravel_index(out.argmax(), out.shape)
    assert x > 4 and y < 4


def test_half_scale_by_hand():
    a = np.arange(16, dtype=np.float32).reshape(1, 4, 4, 1)
    z = np.zeros(1, np.int64)
    out = rng.affine_np(a, [[32768, 0, 0, 32768]], z, z, [False], 0.0)[0, :, :, 0]
    assert out[0].tolist() == [3.75, 4.25, 4.75, 5.25]
    assert out[3].tolist() == [9.75, 10.25, 10.75, 11.25]
    # zooming out by two: the corners sample half a pixel outside, the fill is blended in
    out = rng.affine_np(a, [[131072, 0, 0, 131072]], z, z, [False], -8.0)[0, :, :, 0]
    assert out[1, 1] == 0.25 * (0 + 1 + 4 + 5) and out[0, 0] == -8.0


def test_cutout_lands_at_its_corner_only():
    n, H, W = 40, 9, 11
    x = np.random.default_rng(2).standard_normal((n, H, W, 2)).astype(np.float32) + 10.0
    spec = C.parse_augment_spec("cutout:3,fill:-7")
    q = rng.affine_params(77, np.arange(n), spec, H, W)
    S, cy0, cx0 = q.cutout
    assert S == 3 and cy0.max() <= H - 3 and cx0.max() <= W - 3
    out = rng.affine_np(x, q.m, q.dy, q.dx, q.flipped, spec.fill, q.cutout)
    want = x.copy()
    for i in range(n):
        want[i, cy0[i]:cy0[i] + 3, cx0[i]:cx0[i] + 3] = -7.0
    assert np.array_equal(out, want) and (out == -7.0).sum() == n * 9 * 2
    assert len(set(zip(cy0.tolist(), cx0.tolist()))) > 20


@pytest.mark.parametrize("shape", SHAPES[:4], ids=lambda s: "x".join(map(str, s)))
def test_affine_torch_equals_affine_np(shape):
    H, W, _ = shape
    n = 50
    x = np.random.default_rng(H + W).standard_normal((n,) + shape).astype(np.float32)
    spec = C.parse_augment_spec(f"shift:{min(2, H - 1)},flip,rotate:30,scale:30,cutout:2")
    q = rng.affine_params(0xffffffff, np.arange(n), spec, H, W)
    keep = x.copy()
    want = rng.affine_np(x, q.m, q.dy, q.dx, q.flipped, 0.25, q.cutout)
    got = rng.affine_torch(torch.from_numpy(x), q.m, q.dy, q.dx, q.flipped, 0.25, q.cutout)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    assert np.array_equal(rng.affine_torch(torch.from_numpy(x), q.m, q.dy, q.dx, q.flipped,
                                           0.25).numpy(),
                          rng.affine_np(x, q.m, q.dy, q.dx, q.flipped, 0.25))
    assert np.array_equal(x, keep) and not np.array_equal(want, x)


# ------------------------------------------------------------- the engines --
@pytest.fixture(scope="module")
def data200():
    return synthetic_rows("train", 0, N)


def _cfg(**kw):
    return C.TrainConfig(batch_size=B, device="cpu", **kw).validate()


def _host_pass(x, y, p, shuffle, spec=SPEC, model="mnist_cnn", seed=1, rank=0):
    """Rows and labels of pass p as the definition gives them."""
    n, H, W, _ = x.shape
    rows = rng.shuffle_perm(rng.shuffle_key(seed, rank, p), n) if shuffle else np.arange(n)
    s = C.parse_augment_spec(spec, model)
    q = rng.affine_params(rng.augment_key(seed, rank, p), rows, s, H, W)
    return rng.affine_np(x[rows], q.m, q.dy, q.dx, q.flipped, s.fill, q.cutout), y[rows]


@pytest.mark.parametrize("shuffle", [False, True], ids=["file-order", "shuffle"])
def test_torch_engine_grads_equal_host_transformed_engine(data200, shuffle):
    x, y = data200
    eng = TorchMnistEngine(_cfg(augment=SPEC, shuffle=shuffle), x, y, torch.device("cpu"))
    assert eng.shuffler.affine is not None and eng.shuffler.augment is None
    seen = []
    for step in (0, 4):  # passes 0, 1
        eng.forward_backward(step)
        p = pass_of(step, N, B)
        hx, hy = _host_pass(x, y, p, shuffle)
        assert eng.shuffler.loaded == p
        assert np.array_equal(eng.train_x.numpy(), hx) and np.array_equal(eng.train_y.numpy(), hy)
        plain = TorchMnistEngine(_cfg(), hx, hy, torch.device("cpu"))
        plain.forward_backward(step)
        assert torch.equal(eng.grads, plain.grads)
        seen.append(hx)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], x)
    assert np.array_equal(eng.shuffler.src_x.numpy(), x)  # the pristine copy
    # rotate / scale do change the rows of the shift-only spec
    only_shift = TorchMnistEngine(_cfg(augment="shift:2", shuffle=shuffle), x, y,
                                  torch.device("cpu"))
    only_shift.forward_backward(4)
    assert not np.array_equal(only_shift.train_x.numpy(), seen[1])


def test_torch_engine_resume_is_bit_identical(data200):
    x, y = data200
    dev = torch.device("cpu")
    cfg = _cfg(augment=SPEC + ",cutout:4", shuffle=True)
    whole = TorchMnistEngine(cfg, x, y, dev)
    whole.train(4)
    at4 = (whole.params.clone(), whole.mom.clone())
    whole.train(3)
    tail = TorchMnistEngine(cfg, x, y, dev)  # resumed inside pass 1 from the step-4 state alone
    tail.params.copy_(at4[0])
    tail.mom.copy_(at4[1])
    tail.set_step(4)
    tail.train(3)
    assert tail.step == whole.step == 7
    assert torch.equal(tail.params, whole.params) and torch.equal(tail.mom, whole.mom)
    other = TorchMnistEngine(_cfg(augment=SPEC, shuffle=True), x, y, dev)
    other.train(7)
    assert not torch.equal(other.params, whole.params)  # the cutout matters


def test_make_shuffler_holds_the_spec_and_checks_the_shape(data200):
    x, y = data200
    tx, ty = torch.from_numpy(x), torch.from_numpy(y)
    old = make_shuffler(_cfg(augment="shift:2,flip"), 0, N, tx, ty, image_shape=(28, 28, 1))
    assert old.augment == (2, True, -0.5, (28, 28, 1)) and old.affine is None
    new = make_shuffler(_cfg(augment="rotate:10,cutout:27"), 0, N, tx, ty, image_shape=(28, 28, 1))
    assert new.augment is None and new.affine == (C.AugmentSpec(0, False, -0.5, 10.0, 0.0, 27),
                                                  (28, 28, 1))
    assert np.array_equal(new.tables, rng.affine_tables(10.0, 0.0))
    with pytest.raises(ValueError, match="cutout"):  # S >= min(H, W)
        make_shuffler(_cfg(augment="cutout:28"), 0, N, tx, ty, image_shape=(28, 28, 1))
    with pytest.raises(ValueError, match="shift"):
        TorchMnistEngine(_cfg(augment="shift:28,rotate:5"), x, y, torch.device("cpu"))
    with pytest.raises(ValueError):
        PassShuffler(1, 0, N, B, tx, ty, augment=(C.parse_augment_spec("rotate:5"), (28, 14, 2)))


def test_trainer_train_prediction_reads_the_transformed_rows():
    from mpi_tensorflow_amd.runtime.trainer import Trainer

    spec = SPEC + ",cutout:4"
    cfg = C.config_from_args(["--synthetic", "--device", "cpu", "--augment", spec, "--shuffle",
                              "--max-steps", "2", "--eval-every", "0", "--quiet"])
    tr = Trainer(cfg)
    tr.run()
    eng, sh = tr.engine, tr.shard
    n = sh.train_x.shape[0]
    hx, hy = _host_pass(sh.train_x, sh.train_y, 0, True, spec, seed=cfg.seed)
    assert eng.step == 2 and eng.shuffler.loaded == 0
    assert np.array_equal(eng.train_x.numpy(), hx) and np.array_equal(eng.train_y.numpy(), hy)
    off = batch_offset(2, n, cfg.batch_size)
    assert torch.equal(tr.train_prediction(),
                       tr.eval_prediction(hx[off:off + cfg.batch_size], dropout=True))


def test_mpipy_runs_the_full_spec_as_a_subprocess():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mpipy.py"), "--synthetic", "--device",
                        "cpu", "--augment", "shift:2,rotate:10,scale:10,cutout:4", "--max-steps",
                        "3", "--eval-every", "0"], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    torch.set_num_threads(2)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    for k in ("OMPI_COMM_WORLD_RANK", "PMI_RANK", "SLURM_PROCID"):
        os.environ.pop(k, None)
    from mpi_tensorflow_amd.parallel import dist as D
    from mpi_tensorflow_amd.parallel.comm import make_comm

    cpu = torch.device("cpu")
    di = D.init("cpu")
    comm = make_comm(di, cpu)
    x, y = synthetic_rows("train", 0, N)  # the same rows on both ranks: only the draws differ
    eng = TorchMnistEngine(_cfg(augment=SPEC), x, y, cpu, rank, world, comm)
    assert eng.grad_sync and eng.shuffler.rank == rank
    eng.train(4)  # into pass 1
    np.save(os.path.join(out_dir, f"x{rank}.npy"), eng.train_x.numpy())
    np.save(os.path.join(out_dir, f"p{rank}.npy"), eng.params.numpy())
    D.shutdown()


def test_two_gloo_ranks_draw_differently_and_reproducibly(tmp_path, data200):
    x, y = data200
    runs = []
    for name in ("a", "b"):
        out = tmp_path / name
        out.mkdir()
        mp.spawn(_worker, args=(2, _free_port(), str(out)), nprocs=2, join=True)
        runs.append([np.load(out / f"{k}{r}.npy") for r in (0, 1) for k in ("x", "p")])
    x0, p0, x1, p1 = runs[0]
    assert np.array_equal(x0, _host_pass(x, y, 1, False, rank=0)[0])
    assert np.array_equal(x1, _host_pass(x, y, 1, False, rank=1)[0])
    assert not np.array_equal(x0, x1)
    assert np.array_equal(p0, p1)  # per-step gradient all-reduce
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
