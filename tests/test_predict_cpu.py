"""Inference from a checkpoint, CPU side: the --predict flags, the TTA view
enumeration, the torch oracles of Fn.predict_prep / Fn.predict_head on
hand-worked rows, the Predictor against the torch engine's own evaluation
(every input format), mpipy.py --predict as a subprocess and the row split
over two gloo ranks."""

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
SEED_2RANKS = 1  # the 101 rows of the two-rank test: rows 0..100 of the synthetic test split


# ------------------------------------------------------------------ flags --
def test_flags_are_validated_with_messages_naming_the_flag(tmp_path):
    from mpi_tensorflow_amd import config as C

    ck = str(tmp_path / "c.npz")
    with pytest.raises(ValueError, match="--resume"):
        C.TrainConfig(predict="test").validate()
    with pytest.raises(ValueError, match="resnet18"):
        C.TrainConfig(predict="test", resume=ck, model="resnet18").validate()
    for k in (0, 11):
        with pytest.raises(ValueError, match="--predict-topk"):
            C.TrainConfig(predict="test", resume=ck, predict_topk=k).validate()
    with pytest.raises(ValueError, match="--predict-tta"):
        C.TrainConfig(predict="test", resume=ck, predict_tta="shift:4").validate()
    with pytest.raises(ValueError, match="--predict-tta"):
        C.TrainConfig(predict="test", resume=ck, predict_tta="rotate").validate()
    with pytest.raises(ValueError, match="--predict:"):
        C.TrainConfig(predict="train", resume=ck).validate()
    with pytest.raises(ValueError, match="--predict"):
        C.TrainConfig(predict_out="o.npz").validate()
    ok = C.config_from_args(["--resume", ck, "--predict", "val", "--predict-topk", "10",
                             "--predict-tta", "shift:3,flip", "--predict-probs"])
    assert (ok.predict, ok.predict_topk, ok.predict_tta, ok.predict_probs) == (
        "val", 10, "shift:3,flip", True)
    d = C.TrainConfig()  # everything off by default
    assert (d.predict, d.predict_labels, d.predict_out, d.predict_topk, d.predict_tta,
            d.predict_probs) == (None, None, None, 3, None, False)


def test_view_enumeration():
    from mpi_tensorflow_amd.runtime.predict import tta_views

    assert tta_views(None) == ([(0, 0, False)], 0.0)
    for spec, K, flip in (("shift:1", 1, False), ("shift:1,flip", 1, True), ("flip", 0, True),
                          ("shift:3,flip,fill:0.5", 3, True)):
        views, fill = tta_views(spec, "mnist_cnn")
        span = 2 * K + 1
        assert len(views) == span * span * (2 if flip else 1)
        for v, (dy, dx, f) in enumerate(views):
            assert v == (int(f) * span + dy + K) * span + dx + K
            assert -K <= dy <= K and -K <= dx <= K
        assert views.count((0, 0, False)) == 1
        assert fill == (0.5 if "fill" in spec else -0.5)
    assert [len(tta_views(s)[0]) for s in ("shift:1", "shift:1,flip", "flip")] == [9, 18, 2]
    assert tta_views("flip", "lenet5")[1] == 0.0
    with pytest.raises(ValueError, match="shift"):
        tta_views("shift:4")


# ------------------------------------------------------------ prep oracle --
def test_norm_table_is_extract_datas_expression_bit_for_bit():
    from mpi_tensorflow_amd.ops import functional as Fn

    want = (np.arange(256, dtype=np.uint8).astype(np.float32) - 127.5) / 255
    got = Fn.predict_norm_table()
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    x = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1)
    assert Fn.predict_prep(x).numpy().tobytes() == want.tobytes()


def test_prep_oracle_hand_worked_three_channels():
    from mpi_tensorflow_amd.ops import functional as Fn

    # x[0, y, x, c] = 30 y + 10 x + c: H = 2, W = 3, C = 3
    x = np.array([[[[30 * y + 10 * col + c for c in range(3)] for col in range(3)]
                   for y in range(2)]], np.uint8)
    got = Fn.predict_prep(torch.from_numpy(x), dy=1, dx=-1, flip=True, fill=0.25).numpy()
    nrm = lambda p: (np.float32(p) - np.float32(127.5)) / np.float32(255)  # noqa: E731
    F = np.float32(0.25)
    # dst[y, x, c] = src[y + 1, (2 - x) - 1, c]: line 0 reads line 1 mirrored
    # and shifted (columns 1, 0, then outside), line 1 reads line 2: outside
    want = np.array([[[[nrm(40), nrm(41), nrm(42)], [nrm(30), nrm(31), nrm(32)], [F, F, F]],
                      [[F, F, F], [F, F, F], [F, F, F]]]], np.float32)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    # float32 input: the identity instead of the table
    xf = x.astype(np.float32)
    gotf = Fn.predict_prep(torch.from_numpy(xf), dy=1, dx=-1, flip=True, fill=0.25).numpy()
    assert gotf[0, 0, 0].tolist() == [40.0, 41.0, 42.0] and gotf[0, 1, 2, 0] == F
    with pytest.raises(ValueError):
        Fn.predict_prep(torch.from_numpy(x), dy=2)


@pytest.mark.parametrize("shape", [(28, 28, 1), (32, 32, 3)])
def test_prep_oracle_equals_augment_np_of_the_normalised_rows(shape):
    from mpi_tensorflow_amd.ops import functional as Fn
    from mpi_tensorflow_amd.utils import rng

    g = np.random.default_rng(7)
    u8 = g.integers(0, 256, size=(5,) + shape, dtype=np.uint8)
    x = (u8.astype(np.float32) - 127.5) / 255  # extract_data
    for dy, dx, fl, fill in ((0, 0, False, 0.0), (2, -1, False, -0.5), (-3, 3, True, 0.25),
                             (0, 0, True, 0.0)):
        want = rng.augment_np(x, [dy] * 5, [dx] * 5, [fl] * 5, fill)
        for src in (u8, x):
            got = Fn.predict_prep(torch.from_numpy(src), dy, dx, fl, fill).numpy()
            assert got.tobytes() == want.tobytes(), (shape, dy, dx, fl, src.dtype)


# ------------------------------------------------------------ head oracle --
def test_head_oracle_hand_worked_rows():
    from mpi_tensorflow_amd.ops import functional as Fn

    tie = [0.0] * 10
    tie[4] = tie[7] = 5.0
    big = [80.0 if j % 2 == 0 else -80.0 for j in range(10)]
    x = torch.tensor([[1.5] * 10, tie, big], dtype=torch.float32)
    r = Fn.predict_head(x, k=3)
    assert r.topk_class.dtype == torch.int32 and r.topk_class.shape == (3, 3)
    assert r.topk_class[0].tolist() == [0, 1, 2]  # all equal: index order
    assert r.topk_class[1].tolist() == [4, 7, 0]  # the tie goes to the lower index
    assert r.topk_class[2].tolist() == [0, 2, 4]
    assert torch.equal(r.scores, x)  # one view: the logits themselves
    assert torch.isfinite(r.probs).all() and torch.isfinite(r.topk_prob).all()
    assert torch.allclose(r.probs.sum(1), torch.ones(3), atol=1e-6)
    assert torch.equal(r.topk_prob, r.probs.gather(1, r.topk_class.long()))
    assert r.probs[0].tolist() == pytest.approx([0.1] * 10, abs=1e-7)
    # the +-80 row through two views: log(max(p, FLT_MIN)) stays finite
    r2 = Fn.predict_head([x, x], k=10)  # the -80 classes: p = 0 in fp32
    assert torch.isfinite(r2.scores).all()
    assert r2.scores[2].min().item() == pytest.approx(np.log(np.finfo(np.float32).tiny), rel=1e-6)
    assert sorted(r2.topk_class[2].tolist()) == list(range(10))
    with pytest.raises(ValueError):
        Fn.predict_head(x, k=0)
    with pytest.raises(ValueError):
        Fn.predict_head(x, k=11)


def test_head_oracle_averages_probabilities_not_logits():
    from mpi_tensorflow_amd.ops import functional as Fn

    a = torch.tensor([[3.0, 0.0, 0.0]])
    b = torch.tensor([[-5.0, 0.0, 1.0]])
    assert int(((a + b) / 2).argmax(1)) == 2  # the mean logit's winner
    r = Fn.predict_head([a, b], k=3)
    pa = np.exp([3.0, 0, 0]) / np.exp([3.0, 0, 0]).sum()
    pb = np.exp([-5.0, 0, 1]) / np.exp([-5.0, 0, 1]).sum()
    want = (pa + pb) / 2  # [0.455, 0.157, 0.388]
    assert r.probs[0].tolist() == pytest.approx(want.tolist(), abs=1e-6)
    assert r.topk_class[0].tolist() == [0, 2, 1]  # the mean probability's order
    assert r.scores[0].tolist() == pytest.approx(np.log(want).tolist(), abs=1e-5)


# ---------------------------------------------------------------- Predictor --
def _to_u8(x):
    u8 = np.rint(x * 255 + 127.5).astype(np.uint8)
    back = (u8.astype(np.float32) - 127.5) / 255
    assert back.tobytes() == np.ascontiguousarray(x, np.float32).tobytes()  # the round trip is exact
    return u8


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """A TorchMnistEngine trained 3 steps, its checkpoint, 101 test rows."""
    from mpi_tensorflow_amd import config as C
    from mpi_tensorflow_amd.runtime.mnist_engine import TorchMnistEngine
    from mpi_tensorflow_amd.utils import checkpoint as ckpt_mod
    from mpi_tensorflow_amd.utils.data import synthetic_rows

    torch.set_num_threads(2)
    d = tmp_path_factory.mktemp("predict")
    cfg = C.TrainConfig(device="cpu", backend="torch", synthetic=True).validate()
    tx, ty = synthetic_rows("train", 0, 256)
    eng = TorchMnistEngine(cfg, tx, ty, torch.device("cpu"))
    eng.train(3)
    path = str(d / "c.npz")
    ckpt_mod.save(path, eng.layout, eng.params, eng.mom, eng.step,
                  meta={"model": "mnist_cnn", "world": 1})
    x, y = synthetic_rows("test", 0, 101, seed=SEED_2RANKS)
    return d, eng, path, x, y


def test_predictor_equals_the_engines_evaluation(trained):
    from mpi_tensorflow_amd.runtime.predict import Predictor

    d, eng, path, x, y = trained
    x, y = x[:50], y[:50]
    err, logits = eng.evaluate(x, y, return_logits=True)
    pr = Predictor.from_checkpoint(path, device="cpu")
    assert (pr.model, pr.dtype, pr.backend, pr.step) == ("mnist_cnn", "fp32", "torch", 3)
    assert not hasattr(pr, "grads") and not hasattr(pr, "mom")
    res = pr.predict(x, labels=y, return_probs=True)
    assert res.pred.dtype == torch.int32 and res.pred.shape == (50,)
    assert torch.equal(res.pred.long(), logits.argmax(1))
    assert res.metrics.wrong == round(err * 50 / 100.0) and res.metrics.n == 50
    assert (res.n, res.views) == (50, 1) and res.seconds > 0.0
    assert res.topk_class.shape == (50, 3) and res.topk_prob.shape == (50, 3)
    assert res.probs.shape == (50, 10)
    assert torch.equal(res.probs, torch.softmax(res.scores, 1))
    # [n, H, W] for the one-channel model, uint8 rows, a torch tensor
    u8 = _to_u8(x)
    for alt in (x[..., 0], u8, torch.from_numpy(u8[..., 0])):
        r2 = pr.predict(alt, labels=y, return_probs=True)
        assert torch.equal(r2.scores, res.scores) and torch.equal(r2.topk_class, res.topk_class)
    assert pr.predict(x).metrics is None and pr.predict(x).probs is None
    with pytest.raises(ValueError):
        pr.predict(x.astype(np.float64))
    with pytest.raises(ValueError):
        pr.predict(x[:, :27])
    with pytest.raises(ValueError):
        pr.predict(x, topk=11)
    # TTA: 18 views, the mean of the per-view softmax of the engine's own logits
    from mpi_tensorflow_amd.utils import rng
    from mpi_tensorflow_amd.runtime.predict import tta_views

    r3 = pr.predict(x[:7], tta="shift:1,flip", return_probs=True, chunk=4)
    acc = np.zeros((7, 10))
    for dy, dx, fl in tta_views("shift:1,flip")[0]:
        xv = rng.augment_np(x[:7], [dy] * 7, [dx] * 7, [fl] * 7, -0.5)
        acc += torch.softmax(eng.evaluate(xv, y[:7], return_logits=True)[1].double(), 1).numpy()
    assert r3.views == 18
    assert np.abs(r3.probs.numpy() - acc / 18).max() <= 1e-5
    # from_engine shares the buffer: an in-place change shows
    pe = Predictor.from_engine(eng)
    assert pe.params.data_ptr() == eng.params.data_ptr()
    assert torch.equal(pe.predict(x).scores, res.scores)
    off = eng.layout.offsets["fc2_bias"]
    old = float(eng.params[off + 3])
    eng.params[off + 3] += 100.0
    try:
        assert (pe.predict(x).pred == 3).all()
    finally:
        eng.params[off + 3] = old
    with pytest.raises(ValueError, match="resnet18"):
        Predictor.from_checkpoint(path, model="resnet18", device="cpu")
    with pytest.raises(ValueError, match="saved model"):
        Predictor.from_checkpoint(path, model="lenet5", device="cpu")


def test_every_input_format_gives_the_same_result(trained):
    from mpi_tensorflow_amd import config as C
    from mpi_tensorflow_amd.runtime.predict import Predictor, predict_main
    from mpi_tensorflow_amd.utils.idx import write_idx

    d, eng, path, x, y = trained
    x, y = x[:50], y[:50]
    u8 = _to_u8(x)
    write_idx(str(d / "x-idx3-ubyte"), u8[..., 0], gz=False)
    write_idx(str(d / "x-idx3-ubyte.gz"), u8[..., 0], gz=True)
    write_idx(str(d / "y-idx1-ubyte.gz"), y.astype(np.uint8), gz=True)
    np.save(str(d / "x_u8.npy"), u8)
    np.save(str(d / "x_f32.npy"), x)
    np.save(str(d / "y.npy"), y)
    want = Predictor.from_checkpoint(path, device="cpu").predict(x, labels=y)
    for src, lab in (("x-idx3-ubyte", "y-idx1-ubyte.gz"), ("x-idx3-ubyte.gz", "y.npy"),
                     ("x_u8.npy", "y-idx1-ubyte.gz"), ("x_f32.npy", "y.npy")):
        out = str(d / (src + ".out.npz"))
        cfg = C.TrainConfig(device="cpu", backend="torch", resume=path, predict=str(d / src),
                            predict_labels=str(d / lab), predict_out=out)
        rec = predict_main(cfg)["predict"]
        z = np.load(out, allow_pickle=False)
        assert np.array_equal(z["pred"], want.pred.numpy()), src
        assert np.array_equal(z["topk_class"], want.topk_class.numpy())
        assert z["topk_prob"].tobytes() == want.topk_prob.numpy().tobytes()
        assert rec["n"] == 50 and rec["error"] == want.metrics.error
        assert rec["loss"] == pytest.approx(want.metrics.loss, rel=1e-12)
        assert str(z["__meta__/source"]) == str(d / src)
    # without labels: no metrics keys
    cfg = C.TrainConfig(device="cpu", backend="torch", resume=path, predict=str(d / "x_u8.npy"))
    rec = predict_main(cfg)["predict"]
    assert not {"error", "loss", "top3_error", "confusion"} & set(rec)
    with pytest.raises(ValueError, match="--predict"):
        predict_main(C.TrainConfig(device="cpu", resume=path, predict=str(d / "missing.npy")))


# ---------------------------------------------------------------------- CLI --
def _mpipy(*args, timeout=600):
    env = dict(os.environ, OMP_NUM_THREADS="2", PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="",
               HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, "mpipy.py", "--synthetic", "--backend", "torch", "--device", "cpu", *args]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def _json_line(out, key):
    return json.loads([ln for ln in out.splitlines() if ln.startswith('{"%s"' % key)][-1])[key]


def test_cli_predicts_its_own_test_split(tmp_path):
    from mpi_tensorflow_amd.utils.data import synthetic_rows

    ck, o = str(tmp_path / "c.npz"), str(tmp_path / "o.npz")
    first = _mpipy("--max-steps", "3", "--eval-every", "0", "--ckpt", ck)
    summ = _json_line(first, "summary")
    out = _mpipy("--resume", ck, "--predict", "test", "--predict-out", o)
    assert '"summary"' not in out and "training session starts" not in out
    rec = _json_line(out, "predict")
    assert set(rec) == {"model", "dtype", "n", "views", "world", "checkpoint_step",
                        "images_per_sec", "out", "error", "loss", "top3_error", "confusion"}
    assert (rec["model"], rec["dtype"], rec["n"], rec["views"], rec["world"]) == (
        "mnist_cnn", "fp32", 10000, 1, 1)
    assert rec["checkpoint_step"] == 3 and rec["out"] == o and rec["images_per_sec"] > 0
    z = np.load(o, allow_pickle=False)
    assert set(z.files) == {"pred", "topk_class", "topk_prob", "__meta__/model", "__meta__/dtype",
                            "__meta__/step", "__meta__/tta", "__meta__/views", "__meta__/source"}
    assert z["pred"].shape == (10000,) and z["pred"].dtype == np.int32
    assert z["topk_class"].shape == (10000, 3) and z["topk_class"].dtype == np.int32
    assert z["topk_prob"].shape == (10000, 3) and z["topk_prob"].dtype == np.float32
    assert np.array_equal(z["pred"], z["topk_class"][:, 0])
    assert (str(z["__meta__/model"]), str(z["__meta__/step"]), str(z["__meta__/views"])) == (
        "mnist_cnn", "3", "1")
    _, labels = synthetic_rows("test", 0, 10000)
    assert rec["error"] == 100.0 * float(np.mean(z["pred"] != labels))
    assert rec["error"] == summ["final_test_error_local"]
    assert np.array(rec["confusion"]).sum() == 10000
    # a checkpoint written at another world size is accepted (training refuses it)
    ck2 = str(tmp_path / "c2.npz")
    with np.load(ck, allow_pickle=False) as zz:
        arrays = {k: zz[k] for k in zz.files}
    arrays["__meta__/world"] = np.array("2")
    np.savez(ck2, **arrays)
    out2 = _mpipy("--resume", ck2, "--predict", "val", "--predict-probs", "--predict-topk", "1",
                  "--predict-out", o)
    rec2 = _json_line(out2, "predict")
    assert rec2["n"] == 5000 and np.load(o)["probs"].shape == (5000, 10)
    assert np.load(o)["topk_class"].shape == (5000, 1)
    # the same command without --predict trains on and prints what it always did
    again = _mpipy("--resume", ck, "--max-steps", "4", "--eval-every", "0")
    assert '"predict"' not in again and "training session starts" in again
    summ2 = _json_line(again, "summary")
    assert set(summ2) == set(summ) and summ2["steps"] == 1


# -------------------------------------------------------------- gloo, world 2 --
def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker_predict(rank, world, port, ckpt, src, labels, out_dir):
    torch.set_num_threads(2)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    for k in ("OMPI_COMM_WORLD_RANK", "PMI_RANK", "SLURM_PROCID"):
        os.environ.pop(k, None)
    from mpi_tensorflow_amd import config as C
    from mpi_tensorflow_amd.parallel import dist as D
    from mpi_tensorflow_amd.runtime.predict import load_source, predict_main

    cfg = C.TrainConfig(device="cpu", backend="torch", resume=ckpt, predict=src,
                        predict_labels=labels, predict_probs=True,
                        predict_out=os.path.join(out_dir, "two.npz"), collective_timeout_s=120.0)
    rec = predict_main(cfg)["predict"]
    n, a, x, y, _ = load_source(cfg, rank, world)
    with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
        json.dump({"rec": rec, "n": n, "a": a, "rows": int(x.shape[0])}, f)
    D.barrier()
    D.shutdown()


def test_two_ranks_split_the_rows_and_rank_0_gets_them_all(trained):
    from mpi_tensorflow_amd.runtime.predict import Predictor

    d, eng, path, x, y = trained
    assert x.shape[0] == 101
    src, lab = str(d / "x101.npy"), str(d / "y101.npy")
    np.save(src, x)
    np.save(lab, y)
    one = Predictor.from_checkpoint(path, device="cpu").predict(x, labels=y, return_probs=True)
    world, port = 2, _free_port()
    mp.spawn(_worker_predict, args=(world, port, path, src, lab, str(d)), nprocs=world, join=True)
    r0, r1 = (json.load(open(d / f"r{r}.json")) for r in (0, 1))
    assert (r0["a"], r0["rows"], r1["a"], r1["rows"]) == (0, 50, 50, 51)
    assert r0["rec"]["n"] == 101 and r0["rec"]["world"] == 2
    assert r0["rec"]["confusion"] == r1["rec"]["confusion"]  # summed over the ranks
    assert np.array(r0["rec"]["confusion"]).sum() == 101
    z = np.load(d / "two.npz", allow_pickle=False)
    assert z["pred"].shape == (101,) and z["probs"].shape == (101, 10)
    assert z["pred"].dtype == np.int32 and z["probs"].dtype == np.float32
    # every row filled: probabilities sum to one in both halves
    assert np.abs(z["probs"].sum(1) - 1.0).max() <= 1e-5
    p1 = one.probs.numpy()
    print(f"two ranks vs one process: max |probs diff| {np.abs(z['probs'] - p1).max():.3e}")
    assert np.abs(z["probs"] - p1).max() <= 1e-5
    top2 = np.sort(p1, axis=1)[:, -2:]
    sure = (top2[:, 1] - top2[:, 0]) > 1e-3
    print(f"rows past the 1e-3 top-two gate: {int(sure.sum())} of 101")
    assert int(sure.sum()) >= 95
    assert np.array_equal(z["pred"][sure], one.pred.numpy()[sure])
    assert np.array_equal(z["topk_class"][:, 0], z["pred"])
