"""The inference kernels (csrc/kernels/predict.hip) and the Predictor on the
GPU: predict_prep bit for bit against its CPU oracle, predict_head against
fp64 torch (and its ordering rule exactly, on the device's own key), the
Predictor against the engines' own evaluation (the same forward launches on
the same operands: bit-identical logits), test-time augmentation end to end
and mpipy's --predict path in process.

Measured on an MI355X, in units of 1 + |ref| against the bound of 1e-5:
largest predict_head probability error 9.3e-8 with one view and 6.3e-8 with
three; largest error of the 18-view TTA probabilities against the fp64 mean
of the per-view softmax 3.7e-8 (docs/ACCURACY.md)."""

import dataclasses

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.ops import functional as Fn
from mpi_tensorflow_amd.utils import rng
from mpi_tensorflow_amd.utils.data import synthetic_rows

pytestmark = pytest.mark.gpu

# the project's fp32-kernel-against-fp64 tolerance: |dev - ref| <= TOL (1 + |ref|)
TOL = 1e-5
CASES = [(1, 10), (3, 10), (257, 10), (64, 3), (130, 64)]
VIEWS = [(0, 0, False), (2, -1, False), (-3, 3, True), (0, 0, True)]
SENTINEL = 7.5


# --------------------------------------------------------------------- prep --
@pytest.mark.parametrize("n", [1, 5, 33])
@pytest.mark.parametrize("shape", [(28, 28, 1), (32, 32, 3)])
def test_prep_kernel_is_bit_identical_to_the_oracle(cuda_dev, n, shape):
    """A row count that does not fill a block, odd shifts that break the
    4-byte alignment of the source, the channel order under a flip, both
    source types; rows of the output at n and above stay as they were."""
    g = np.random.default_rng(100 * n + shape[0])
    u8 = torch.from_numpy(g.integers(0, 256, size=(n,) + shape, dtype=np.uint8))
    f32 = torch.from_numpy(g.standard_normal((n,) + shape).astype(np.float32))
    row = shape[0] * shape[1] * shape[2]
    for src in (u8, f32):
        sd = src.to(cuda_dev)
        for dy, dx, fl in VIEWS:
            for fill in (-0.5, 0.25):
                want = Fn.predict_prep(src, dy, dx, fl, fill)  # CPU: the oracle
                buf = torch.full(((n + 2) * row,), SENTINEL, device=cuda_dev)
                got = Fn.predict_prep(sd, dy, dx, fl, fill, out=buf)
                assert got.shape == want.shape and got.data_ptr() == buf.data_ptr()
                assert torch.equal(got.cpu(), want), (src.dtype, dy, dx, fl, fill)
                assert (buf[n * row:] == SENTINEL).all()
    # without `out`, and the uint8 table over all 256 values
    assert torch.equal(Fn.predict_prep(sd, 1, 1, True, 0.0).cpu(),
                       Fn.predict_prep(src, 1, 1, True, 0.0))
    allv = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1)
    assert (Fn.predict_prep(allv.to(cuda_dev)).cpu().numpy().tobytes()
            == ((np.arange(256, dtype=np.uint8).astype(np.float32) - 127.5) / 255).tobytes())


def test_prep_takes_rows_that_are_no_multiple_of_four(cuda_dev):
    """5 x 5 x 1 rows: the scalar-store path."""
    g = np.random.default_rng(3)
    u8 = torch.from_numpy(g.integers(0, 256, size=(7, 5, 5, 1), dtype=np.uint8))
    for dy, dx, fl in ((0, 0, False), (1, -2, True)):
        assert torch.equal(Fn.predict_prep(u8.to(cuda_dev), dy, dx, fl, 0.5).cpu(),
                           Fn.predict_prep(u8, dy, dx, fl, 0.5))


# --------------------------------------------------------------------- head --
def _case(n, c):
    """The case table of test_eval_metrics_gpu.py: randn * 3 logits with row 0 =
    +-80 alternating, row 1 all equal, every third row from 2 on small
    integers (ties); random labels, two of the 257 rows outside [0, C)."""
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


def _views_of(x, V):
    """x, then fixed random perturbations of it"""
    g = torch.Generator().manual_seed(17)
    return [x] + [x + 0.5 * torch.randn(x.shape, generator=g) for _ in range(V - 1)]


def _order(key, k):
    """descending key, ties to the lower index"""
    return np.argsort(-key.astype(np.float64), axis=1, kind="stable")[:, :k]


@pytest.mark.parametrize("n,c", CASES)
def test_head_kernel_matches_fp64_and_its_ordering_rule(cuda_dev, n, c):
    x, y = _case(n, c)
    for V in (1, 3):
        views = _views_of(x, V)
        ref = sum(torch.softmax(v.double(), 1) for v in views) / V
        dviews = [v.to(cuda_dev) for v in views]
        for k in sorted({1, 3, c}):
            r = Fn.predict_head(dviews, k=k)
            probs = r.probs.cpu()
            err = ((probs.double() - ref).abs() / (1.0 + ref.abs())).max().item()
            print(f"predict_head n={n} C={c} V={V} k={k}: max probs error {err:.3e} "
                  f"in units of (1 + |ref|)")
            assert err <= TOL
            key = (x if V == 1 else probs).numpy()  # the device's own key
            cls = r.topk_class.cpu().numpy()
            assert cls.dtype == np.int32 and cls.shape == (n, k)
            assert np.array_equal(cls, _order(key, k)), (V, k)
            assert torch.equal(r.topk_prob.cpu(), probs.gather(1, r.topk_class.cpu().long()))
            scores = r.scores.cpu()
            assert torch.isfinite(scores).all()
            if V == 1:
                assert torch.equal(scores, x)
                a = Fn.eval_metrics(r.scores, y.to(cuda_dev))
                b = Fn.eval_metrics(x.to(cuda_dev), y.to(cuda_dev))
                assert np.array_equal(a.confusion, b.confusion)
                assert np.array_equal(cls[:, 0], _order(x.numpy(), 1)[:, 0])
            else:
                want = torch.log(probs.clamp_min(torch.finfo(torch.float32).tiny)).double()
                assert ((scores.double() - want).abs() <= TOL * (1.0 + want.abs())).all()
            again = Fn.predict_head(dviews, k=k)
            for f in dataclasses.fields(Fn.PredictHeadOut):
                assert torch.equal(getattr(again, f.name), getattr(r, f.name)), f.name
    assert ref.shape == (n, c)


def test_ops_in_oracle_mode_on_device_tensors(cuda_dev):
    x, _ = _case(64, 3)
    with Fn.oracle_mode():
        a = Fn.predict_head(x.to(cuda_dev), k=2)
    b = Fn.predict_head(x, k=2)
    assert a.probs.is_cuda and torch.equal(a.probs.cpu(), b.probs)
    assert torch.equal(a.topk_class.cpu(), b.topk_class)
    u8 = torch.arange(2 * 4 * 4 * 3, dtype=torch.uint8).reshape(2, 4, 4, 3)
    with Fn.oracle_mode():
        v = Fn.predict_prep(u8.to(cuda_dev), 1, 0, True, 0.0)
    assert v.is_cuda and torch.equal(v.cpu(), Fn.predict_prep(u8, 1, 0, True, 0.0))


# ---------------------------------------------------------------- Predictor --
def _engine(kind, dev):
    """as test_eval_metrics_gpu.py builds them: random-init weights"""
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


def _to_u8(x):
    u8 = np.rint(x * 255 + 127.5).astype(np.uint8)
    back = (u8.astype(np.float32) - 127.5) / 255
    assert back.tobytes() == np.ascontiguousarray(x, np.float32).tobytes()
    return u8


@pytest.mark.parametrize("kind", ["fp32", "bf16", "lenet5"])
def test_predictor_is_bit_identical_to_the_engines_evaluation(cuda_dev, kind, tmp_path):
    """100 rows in chunks of 32: four chunks, a tail of 4 (half a bf16 group of 8)."""
    from mpi_tensorflow_amd.runtime.predict import Predictor
    from mpi_tensorflow_amd.utils import checkpoint as ckpt_mod

    eng, (tx, ty) = _engine(kind, cuda_dev)
    model = "lenet5" if kind == "lenet5" else "mnist_cnn"
    dtype = "fp32" if kind == "lenet5" else kind
    err, logits = eng.evaluate(tx, ty, chunk=32, return_logits=True)
    path = str(tmp_path / "c.npz")
    ckpt_mod.save(path, eng.layout, eng.params, eng.mom, 0, meta={"model": model, "world": 8})
    pr = Predictor.from_checkpoint(path, dtype=dtype, device="cuda")
    assert (pr.model, pr.dtype, pr.backend) == (model, dtype, "native")
    assert not hasattr(pr, "grads") and not hasattr(pr, "mom")
    res = pr.predict(tx, labels=ty, chunk=32, return_probs=True)
    assert torch.equal(res.scores, logits)  # the same kernels on the same operands
    wrong = err * 100 / 100.0
    assert abs(wrong - round(wrong)) < 1e-9 and res.metrics.wrong == int(round(wrong))
    assert res.metrics.n == 100 and (res.n, res.views) == (100, 1) and res.seconds > 0
    assert torch.equal(res.pred, res.topk_class[:, 0]) and res.pred.dtype == torch.int32
    assert np.array_equal(res.pred.cpu().numpy(),
                          np.argsort(-logits.cpu().numpy().astype(np.float64), 1, kind="stable")[:, 0])
    ref = torch.softmax(logits.double(), 1)
    assert ((res.probs.double() - ref).abs() <= TOL * (1.0 + ref)).all()
    # uint8 rows, normalised on the device, and a resident device tensor
    r8 = pr.predict(_to_u8(tx), labels=ty, chunk=32)
    assert torch.equal(r8.scores, res.scores) and r8.metrics.wrong == res.metrics.wrong
    rd = pr.predict(torch.from_numpy(tx).to(cuda_dev), chunk=32)
    assert torch.equal(rd.scores, res.scores) and rd.metrics is None and rd.probs is None
    # from_engine: zero copy, follows an in-place change of the weights (for
    # bf16 also of a weight that is read through its shadow)
    pe = Predictor.from_engine(eng)
    assert pe.params.data_ptr() == eng.params.data_ptr() and pe.dtype == dtype
    assert torch.equal(pe.predict(tx, chunk=32).scores, logits)
    off = eng.layout.offsets
    eng.params[off["f3_b" if kind == "lenet5" else "fc2_bias"] + 3] += 1.0e4
    if kind != "lenet5":
        eng.params[off["conv2_weight"]:off["conv2_weight"] + 4000] *= 0.5
    _, changed = eng.evaluate(tx, ty, chunk=32, return_logits=True)
    r2 = pe.predict(tx, chunk=32)
    assert not torch.equal(changed, logits)
    assert torch.equal(r2.scores, changed) and (r2.pred == 3).all()


def test_predictor_on_the_torch_backend_agrees_with_the_kernels(cuda_dev):
    from mpi_tensorflow_amd.runtime.predict import Predictor

    eng, (tx, ty) = _engine("fp32", cuda_dev)
    nat = Predictor.from_engine(eng).predict(tx[:20], return_probs=True)
    ora = Predictor("mnist_cnn", eng.params, backend="torch").predict(tx[:20], return_probs=True)
    assert (nat.probs - ora.probs).abs().max().item() <= 1e-4
    with pytest.raises(NotImplementedError):
        Predictor("mnist_cnn", eng.params, dtype="bf16", backend="torch")


def test_tta_end_to_end(cuda_dev):
    """fp32 MNIST, shift:1,flip: 18 views of 9 rows in chunks of 4, 4, 1."""
    from mpi_tensorflow_amd.runtime.predict import Predictor, tta_views

    eng, (tx, ty) = _engine("fp32", cuda_dev)
    x, y = tx[:9], ty[:9]
    pr = Predictor.from_engine(eng)
    res = pr.predict(x, tta="shift:1,flip", chunk=4, return_probs=True, labels=y)
    views, fill = tta_views("shift:1,flip", "mnist_cnn")
    assert res.views == 18 == len(views) and fill == -0.5
    ref = torch.zeros(9, 10, dtype=torch.float64)
    for dy, dx, fl in views:
        xv = rng.augment_np(x, [dy] * 9, [dx] * 9, [fl] * 9, fill)
        _, lg = eng.evaluate(xv, y, return_logits=True)
        ref += torch.softmax(lg.double().cpu(), 1)
    ref /= 18
    probs = res.probs.cpu()
    err = ((probs.double() - ref).abs() / (1.0 + ref)).max().item()
    print(f"TTA 18 views: max probs error {err:.3e} in units of (1 + |ref|)")
    assert err <= TOL
    assert np.array_equal(res.topk_class.cpu().numpy(),
                          np.argsort(-probs.numpy().astype(np.float64), 1, kind="stable")[:, :3])
    assert res.metrics.n == 9 and np.isfinite(res.metrics.loss)
    # the same views of the uint8 rows: the same bits
    r8 = pr.predict(_to_u8(x), tta="shift:1,flip", chunk=4, return_probs=True)
    assert torch.equal(r8.probs, res.probs)


def test_predict_main_equals_the_runs_own_final_evaluation(cuda_dev, tmp_path):
    from mpi_tensorflow_amd.runtime.predict import Predictor, predict_main
    from mpi_tensorflow_amd.runtime.trainer import Trainer

    ck, out = str(tmp_path / "c.npz"), str(tmp_path / "o.npz")
    cfg = C.TrainConfig(model="mnist_cnn", synthetic=True, max_steps=4, eval_every=0, quiet=True,
                        ckpt=ck).validate()
    summ = Trainer(cfg).run()
    pcfg = dataclasses.replace(cfg, ckpt=None, resume=ck, predict="test", predict_out=out)
    rec = predict_main(pcfg)["predict"]
    assert rec["error"] == summ.final_test_error_local  # world 1: exactly
    assert (rec["n"], rec["views"], rec["world"], rec["checkpoint_step"]) == (10000, 1, 1, 4)
    z = np.load(out, allow_pickle=False)
    _, labels = synthetic_rows("test", 0, 10000)
    assert rec["error"] == 100.0 * float(np.mean(z["pred"] != labels))
    assert z["topk_prob"].dtype == np.float32 and z["topk_class"].shape == (10000, 3)
    pr = Predictor.from_checkpoint(ck, device="cuda")
    assert not hasattr(pr, "grads") and not hasattr(pr, "mom") and not hasattr(pr, "comm")
    assert pr.step == 4
