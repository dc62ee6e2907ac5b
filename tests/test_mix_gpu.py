"""--mix and --label-smoothing on the device: the mix_rows load
(csrc/kernels/augment.hip) against the host definition (utils/rng.py mix_params /
mix_np) bit for bit, the soft-target loss sites (MNIST head, xent_mean_soft)
against fp64, and the native engines under the flags against the PyTorch engine
with the same flags.

Bounds: the head's are test_mnist_fc_chain_gpu.py::test_head_matches_fp64's
(1e-5 of the largest reference magnitude); xent_mean_soft's are
test_generic_ops_gpu.py::test_avgpool_and_xent's (loss 1e-4, dlogits 1e-5 by
norm); the engines' are the per-step ones of test_mnist_any_batch_gpu.py (fp32:
loss 1e-4, gradients 2e-4 of the largest, with the conv gradients under the
near-tie model of test_native_mnist_gpu.py::test_per_step_grads_along_native_trajectory;
bf16: loss 2e-2, gradients 6e-2 by norm), test_lenet_native_gpu.py (loss 1e-5,
gradients 2e-5) and
test_generic_ops_gpu.py::test_model_grads_native_vs_oracle (loss 1e-4, gradients
1e-3 by norm); the two-rank ones are tests/helpers/native_sync_ranks.py's.
"""

import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.models import mnist_cnn as M
from mpi_tensorflow_amd.ops import functional as Fn
from mpi_tensorflow_amd.ops import native, ptr, stream_handle
from mpi_tensorflow_amd.runtime.generic_engine import GenericEngine
from mpi_tensorflow_amd.runtime.lenet_engine import NativeLenetEngine
from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine, TorchMnistEngine
from mpi_tensorflow_amd.utils import rng
from mpi_tensorflow_amd.utils.data import batch_offset, pass_of, synthetic_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCLS = 10
SENTINELS = 3

# n, (H, W, C), unaligned base
CASES = {
    "one-row": (1, (28, 28, 1), False),
    "5x7x3": (37, (5, 7, 3), True),       # U = 1: 105 floats a row, base one float off
    "mnist": (37, (28, 28, 1), False),    # U = 4, one piece
    "lenet": (16, (32, 32, 3), False),    # U = 4, 3 pieces, ragged last
}
COVERED = ("5x7x3", "mnist")  # the n = 37 cases


# -------------------------------------------------------------- mix_rows ----
def _rows(dev, n, shape, unaligned):
    g = torch.Generator().manual_seed(n * 7919 + int(np.prod(shape)))
    x = torch.randn((n,) + shape, generator=g)
    y = torch.randint(0, 1000, (n,), generator=g, dtype=torch.int32)
    row = int(np.prod(shape))
    buf = torch.zeros(n * row + 5, device=dev)
    src = buf[1:1 + n * row] if unaligned else buf[:n * row]
    src = src.view((n,) + shape)
    src.copy_(x)
    return x.numpy(), y.numpy(), src, y.to(dev)


def _dst(dev, n, shape, unaligned):
    row = int(np.prod(shape))
    m = n + SENTINELS
    buf = torch.full((m * row + 5,), float("nan"), device=dev)
    dst = (buf[1:1 + m * row] if unaligned else buf[:m * row]).view((m,) + shape)
    return (dst, torch.full((m,), -9, dtype=torch.int32, device=dev),
            torch.full((m,), -9, dtype=torch.int32, device=dev),
            torch.full((m,), float("nan"), device=dev))


def _oracle_key(kind, M_, n, shape):
    """The first key under which the definition itself mixes >= 80 % of the rows."""
    H, W, _ = shape
    tab = rng.mix_table(kind, M_, H, W)
    for key in range(1, 64):
        j, lamq = rng.mix_params(key, n, tab, H, W)[:2]
        if np.mean((lamq < 65536) & (j != np.arange(n))) >= 0.8:
            return key
    raise AssertionError("no key mixes 80 % of the rows")


def _launch(src_x, src_y, dst, n, shape, kind, key, tab):
    H, W, Cc = shape
    native().ops.mix_rows(ptr(src_x), ptr(src_y), ptr(dst[0]), ptr(dst[1]), ptr(dst[2]), ptr(dst[3]),
                          n, H, W, Cc, kind == "cutmix", key, ptr(tab), stream_handle())


def _check(dst, n, want):
    wx, wy, wy2, wlam = want
    assert np.array_equal(dst[0][:n].cpu().numpy(), wx)
    assert np.array_equal(dst[1][:n].cpu().numpy(), wy)
    assert np.array_equal(dst[2][:n].cpu().numpy(), wy2)
    assert np.array_equal(dst[3][:n].cpu().numpy(), wlam)
    # rows at n and above keep their poison
    assert bool(torch.isnan(dst[0][n:]).all()) and bool(torch.isnan(dst[3][n:]).all())
    assert bool((dst[1][n:] == -9).all()) and bool((dst[2][n:] == -9).all())


@pytest.mark.parametrize("M_", [50.0, 10.0])
@pytest.mark.parametrize("kind", ["mixup", "cutmix"])
@pytest.mark.parametrize("case", list(CASES))
def test_mix_rows_equals_definition(cuda_dev, case, kind, M_):
    n, shape, unaligned = CASES[case]
    H, W, _ = shape
    hx, hy, src_x, src_y = _rows(cuda_dev, n, shape, unaligned)
    tab = rng.mix_table(kind, M_, H, W)
    key = _oracle_key(kind, M_, n, shape) if case in COVERED else 0xde56f3b3
    prm = rng.mix_params(key, n, tab, H, W)
    if case in COVERED:
        mixed = np.mean((prm[1] < 65536) & (prm[0] != np.arange(n)))
        print(case, kind, M_, f"key {key}: {100 * mixed:.0f} % of the rows mixed")
        assert mixed >= 0.8
    want = rng.mix_np(hx, hy, prm, kind)
    if case in COVERED:
        assert not np.array_equal(want[0], hx)
    dst = _dst(cuda_dev, n, shape, unaligned)
    keep = src_x.clone()
    _launch(src_x, src_y, dst, n, shape, kind, key, torch.from_numpy(tab).to(cuda_dev))
    torch.cuda.synchronize()
    _check(dst, n, want)
    assert torch.equal(src_x, keep)


@pytest.mark.parametrize("kind", ["mixup", "cutmix"])
def test_mix_rows_in_a_captured_graph(cuda_dev, kind):
    n, shape, _ = CASES["lenet"]
    hx, hy, src_x, src_y = _rows(cuda_dev, n, shape, False)
    tab = rng.mix_table(kind, 50.0, shape[0], shape[1])
    d_tab = torch.from_numpy(tab).to(cuda_dev)
    dst = _dst(cuda_dev, n, shape, False)
    eager = _dst(cuda_dev, n, shape, False)
    _launch(src_x, src_y, eager, n, shape, kind, 77, d_tab)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _launch(src_x, src_y, dst, n, shape, kind, 77, d_tab)
    want = rng.mix_np(hx, hy, rng.mix_params(77, n, tab, shape[0], shape[1]), kind)
    for _ in range(2):
        for t in dst:
            t[:n].zero_()
        g.replay()
        torch.cuda.synchronize()
        _check(dst, n, want)
        for a, b in zip(dst, eager):
            assert torch.equal(a[:n], b[:n])


def test_mix_rows_argument_checks(cuda_dev):
    """Each raises before anything is launched: dst keeps its poison."""
    n, shape, _ = CASES["mnist"]
    _, _, src_x, src_y = _rows(cuda_dev, n, shape, False)
    dst = _dst(cuda_dev, n, shape, False)
    tab = torch.from_numpy(rng.mix_table("mixup", 50.0, 28, 28)).to(cuda_dev)
    ops, st = native().ops, stream_handle()
    good = [ptr(src_x), ptr(src_y), ptr(dst[0]), ptr(dst[1]), ptr(dst[2]), ptr(dst[3]), n, 28, 28, 1,
            False, 5, ptr(tab), st]
    for i in (0, 1, 2, 3, 4, 5, 12):  # a null buffer, the table included
        bad = list(good)
        bad[i] = 0
        with pytest.raises(RuntimeError, match="null"):
            ops.mix_rows(*bad)
    bad = list(good)
    bad[2] = ptr(src_x) + 4 * 784  # dst inside src
    with pytest.raises(RuntimeError, match="overlap"):
        ops.mix_rows(*bad)
    bad = list(good)
    bad[3] = ptr(src_y)
    with pytest.raises(RuntimeError, match="overlap"):
        ops.mix_rows(*bad)
    for i, other in ((5, 4), (5, 3), (5, 1), (4, 1), (4, 3), (5, 2), (4, 0)):  # dst_lam, dst_y2
        bad = list(good)
        bad[i] = good[other]
        with pytest.raises(RuntimeError, match="overlap"):
            ops.mix_rows(*bad)
    for bad_n in (-1, 2 ** 31):
        bad = list(good)
        bad[6] = bad_n
        with pytest.raises(RuntimeError, match="n out of range"):
            ops.mix_rows(*bad)
    bad = list(good)
    bad[6:10] = [1, 1025, 2, 1]
    with pytest.raises(RuntimeError, match="1024"):
        ops.mix_rows(*bad)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst[0]).all()) and bool((dst[1] == -9).all())


# ------------------------------------------------------- soft MNIST head ----
def _rel(a, b):
    """max |a - b| relative to the largest reference magnitude"""
    return (a.double().cpu() - b).abs().max().item() / max(1e-30, b.abs().max().item())


def _head_inputs(batch, ns, seed):
    """As test_mnist_fc_chain_gpu.py: slabs whose sum (+ bias) stays 0.05 away from
    zero, so the fp32 and the fp64 ReLU gates agree on every unit."""
    g = torch.Generator().manual_seed(seed)
    b3 = torch.randn(M.FC1_OUT, generator=g) * 0.1
    zt = torch.randn(batch, M.FC1_OUT, generator=g, dtype=torch.float64)
    zt = zt + 0.05 * torch.sign(zt)
    part = torch.randn(ns, batch, M.FC1_OUT, generator=g)
    part[ns - 1] = (zt - b3.double() - part[:ns - 1].double().sum(0)).float()
    w4 = torch.randn(M.FC1_OUT, NCLS, generator=g) * 0.1
    b4 = torch.randn(NCLS, generator=g) * 0.1
    return part, b3, w4, b4


@pytest.fixture
def chain(cuda_dev):
    k = native().mnist
    yield k
    k.set_fc_chain(-1)


def _head_out(dev, batch):
    return dict(hd=torch.full((batch, M.FC1_OUT), float("nan"), device=dev),
                dh=torch.full((batch, M.FC1_OUT), float("nan"), device=dev),
                dlog=torch.full((batch, NCLS), float("nan"), device=dev),
                loss=torch.full((batch,), float("nan"), device=dev),
                lr=torch.full((1,), float("nan"), device=dev),
                correct=torch.zeros(1, dtype=torch.int32, device=dev),
                dh16=torch.zeros(M.FC1_OUT // 16, batch, 16, dtype=torch.bfloat16, device=dev),
                dht16=torch.zeros(batch // 16, M.FC1_OUT, 16, dtype=torch.bfloat16, device=dev))


@pytest.mark.parametrize("keep", [0.5, 1.0])
@pytest.mark.parametrize("splits", ["feature-major", "staged"])
@pytest.mark.parametrize("lb,batch", [(32, 32), (40, 64)])
def test_soft_head_matches_fp64(cuda_dev, chain, lb, batch, splits, keep):
    """EPS in {0, 0.1}, with and without labels2 / lam (rows with y1 == y2
    included): hd, dh, dlog, loss rows against fp64 of the definition within 1e-5
    of the largest reference magnitude; `correct` exact (argmax against y1); pad
    rows exactly +0; dh16 / dht16 = dh rounded; at EPS = 0 without lam the outputs
    of `fc_head_train_full` bit for bit under BOTH masks of set_fc_chain, i.e. of
    both hard kernels.  The soft head is one kernel and ignores the mask, so the
    last comparison (mask 0 against -1) only shows that the mask does not reach
    it."""
    k = chain
    ns = k.fc1_train_t_splits() if splits == "feature-major" else k.fc1_train_splits()
    n_local, base_lr, decay = 1000, 0.01, 0.95
    part, b3, w4, b4 = _head_inputs(batch, ns, 7 * batch + ns)
    g = torch.Generator().manual_seed(3)
    labels = torch.randint(0, NCLS, (n_local,), generator=g, dtype=torch.int32)
    labels2 = torch.randint(0, NCLS, (n_local,), generator=g, dtype=torch.int32)
    labels2[::3] = labels[::3]  # y1 == y2 on a third of the rows
    lam = (torch.randint(32768, 65537, (n_local,), generator=g).float() / 65536.0)
    dev = cuda_dev
    d_part, d_b3, d_w4, d_b4, d_lab, d_lab2, d_lam = (
        t.to(dev) for t in (part, b3, w4, b4, labels, labels2, lam))
    z = part.double().sum(0) + b3.double()
    h = z.clamp_min(0)
    bf16 = splits == "staged"
    step = (n_local - 1) // lb + 1
    d_step = torch.tensor([step], dtype=torch.int64, device=dev)
    off = (step * lb) % (n_local - lb)
    valid = (torch.arange(batch) < lb)
    s = stream_handle()

    def args(o):
        return (ptr(d_part), ptr(d_b3), ptr(d_w4), ptr(d_b4), ptr(d_lab), n_local, ptr(d_step),
                batch, keep, 11, 0, base_lr, decay, ptr(o["hd"]), ptr(o["dh"]), ptr(o["dlog"]),
                ptr(o["loss"]), ptr(o["lr"]), ptr(o["correct"]), s, ptr(o["dh16"]) if bf16 else 0,
                ptr(o["dht16"]) if bf16 else 0, ns, lb if lb != batch else 0)

    for eps in (0.0, 0.1):
        for mixed in (False, True):
            per_mask = []
            for mask in (0, -1):
                k.set_fc_chain(mask)
                o = _head_out(dev, batch)
                k.fc_head_train_soft(*args(o), ptr(d_lab2) if mixed else 0,
                                     ptr(d_lam) if mixed else 0, eps)
                torch.cuda.synchronize()
                per_mask.append(o)
                tag = (eps, mixed, mask)
                y1 = labels[off:off + batch].long()
                kp = (o["hd"].cpu() != 0) if keep < 1 else torch.ones(batch, M.FC1_OUT,
                                                                      dtype=torch.bool)
                hd_ref = torch.where(kp, h / keep, torch.zeros_like(h))
                logits = hd_ref @ w4.double() + b4.double()
                t = torch.from_numpy(rng.soft_targets(
                    y1.numpy(), labels2[off:off + batch].numpy() if mixed else None,
                    lam[off:off + batch].numpy() if mixed else None, eps, NCLS))
                assert torch.allclose(t.sum(1), torch.ones(batch, dtype=torch.float64))
                p = torch.softmax(logits, 1)
                dlog_ref = (p - t) / lb * valid[:, None]
                gate = kp & (z > 0)
                dh_ref = (dlog_ref @ w4.double().t()) * gate / keep
                loss_ref = (torch.logsumexp(logits, 1) - (t * logits).sum(1)) * valid
                corr_ref = int(((logits.argmax(1) == y1) & valid).sum())
                errs = {"hd": _rel(o["hd"], hd_ref), "dh": _rel(o["dh"], dh_ref),
                        "dlog": _rel(o["dlog"], dlog_ref), "loss": _rel(o["loss"], loss_ref)}
                print(tag, {n: f"{v:.1e}" for n, v in errs.items()}, int(o["correct"].item()),
                      corr_ref)
                assert max(errs.values()) < 1e-5, (tag, errs)
                assert int(o["correct"].item()) == corr_ref, tag
                if lb < batch:
                    pad = slice(lb, batch)
                    zero = torch.zeros(1, device=dev)
                    for name in ("dlog", "dh", "loss"):
                        assert torch.equal(o[name][pad], zero.expand_as(o[name][pad])), (tag, name)
                    assert not torch.signbit(o["dh"][pad]).any(), tag
                    assert not torch.signbit(o["dlog"][pad]).any(), tag
                if bf16:
                    want = o["dh"].to(torch.bfloat16)
                    assert torch.equal(o["dh16"].permute(1, 0, 2).reshape(batch, M.FC1_OUT), want)
                    assert torch.equal(o["dht16"].permute(0, 2, 1).reshape(batch, M.FC1_OUT), want)
                if eps == 0.0 and not mixed:  # the hard head's bits
                    hard = _head_out(dev, batch)
                    k.fc_head_train_full(*args(hard))
                    torch.cuda.synchronize()
                    for name in ("hd", "dh", "dlog", "loss", "lr", "correct"):
                        assert torch.equal(o[name], hard[name]), (tag, name)
            for name in ("hd", "dh", "dlog", "loss", "lr", "correct"):
                assert torch.equal(per_mask[0][name], per_mask[1][name]), (eps, mixed, name)


# --------------------------------------------------------- xent_mean_soft ----
@pytest.mark.parametrize("K", [10, 1000])
@pytest.mark.parametrize("B", [1, 8, 33])
def test_xent_mean_soft_matches_fp64(cuda_dev, B, K):
    g = torch.Generator().manual_seed(100 * B + K)
    logits = torch.randn(B, K, generator=g) * 3
    y1 = torch.randint(0, K, (B,), generator=g)
    y2 = torch.randint(0, K, (B,), generator=g)
    y2[::3] = y1[::3]
    lam = torch.randint(32768, 65537, (B,), generator=g).float() / 65536.0
    d = cuda_dev
    for eps in (0.0, 0.1):
        for mixed in (False, True):
            t = torch.from_numpy(rng.soft_targets(y1.numpy(), y2.numpy() if mixed else None,
                                                  lam.numpy() if mixed else None, eps, K))
            z = logits.double()
            loss_ref = (torch.logsumexp(z, 1) - (t * z).sum(1)).mean().item()
            dlog_ref = (torch.softmax(z, 1) - t) / B
            lg = logits.to(d).requires_grad_(True)
            loss = Fn.cross_entropy(lg, y1.to(d).int(), y2.to(d).int() if mixed else None,
                                    lam.to(d) if mixed else None, eps)
            if eps == 0.0 and not mixed:  # (that call took the hard route: ask for the soft one)
                loss = Fn._XentSoftFn.apply(lg, y1.to(d).int(), None, None, 0.0)
            loss.backward()
            err = ((lg.grad.cpu().double() - dlog_ref).norm() / dlog_ref.norm()).item()
            print(B, K, eps, mixed, f"loss {abs(loss.item() - loss_ref):.1e} dlog {err:.1e}")
            assert abs(loss.item() - loss_ref) < 1e-4
            assert err < 1e-5
            # the binding itself, with its hit counter: argmax (lowest index) against y1
            ops = native().ops
            lz = logits.to(d)
            rows, dl = torch.empty(B, device=d), torch.empty(B, K, device=d)
            mean = torch.empty((), device=d)
            hits = torch.zeros(1, dtype=torch.int32, device=d)
            l1, l2, lm = y1.to(d).int(), y2.to(d).int(), lam.to(d)
            for _ in range(2):  # it accumulates
                ops.xent_mean_soft(ptr(lz), ptr(l1), ptr(l2) if mixed else 0, ptr(lm) if mixed else 0,
                                   eps, B, K, ptr(rows), ptr(dl), ptr(mean), ptr(hits),
                                   stream_handle())
            torch.cuda.synchronize()
            assert int(hits.item()) == 2 * int((logits.argmax(1) == y1).sum())
            assert torch.equal(dl, lg.grad) and torch.equal(mean, loss.detach())
            assert abs(rows.double().mean().item() - loss_ref) < 1e-4
            if eps == 0.0 and not mixed:  # xent_mean's bits
                lh = logits.to(d).requires_grad_(True)
                hard = Fn.cross_entropy(lh, y1.to(d).int())
                hard.backward()
                assert torch.equal(hard, loss) and torch.equal(lh.grad, lg.grad)


# ----------------------------------------------------------------- engines ----
N, B_ = 200, 50  # test_augment_affine_gpu.py's: 150 rows a pass, 3 steps; Bp = 64
FLAGS = [dict(mix="mixup:50", label_smoothing=0.1), dict(mix="cutmix:50", label_smoothing=0.1)]
IDS = ["mixup", "cutmix"]
STEPS = (0, 4, 6)  # passes 0, 1, 2


@pytest.fixture(scope="module")
def mnist200():
    """Uniform random images: on the clipped `synthetic_rows` the Winograd pool-2
    argmax need not be the oracle's first-of-equals
    (test_shuffle_gpu.py::test_native_mnist_per_step_grads_match_shuffled_oracle)."""
    g = np.random.default_rng(20240)
    return (g.random((N, 28, 28, 1), dtype=np.float32) - np.float32(0.5),
            g.integers(0, 10, N).astype(np.int64))


@pytest.fixture(scope="module")
def lenet200():
    return synthetic_rows("train", 0, N, shape=(32, 32, 3))


def _cfg(**kw):
    return C.TrainConfig(batch_size=kw.pop("batch_size", B_), graph=kw.pop("graph", False),
                         **kw).validate()


def _host_pass(x, y, p, kind, M_, seed=1, rank=0):
    H, W = x.shape[1:3]
    prm = rng.mix_params(rng.mix_key(seed, rank, p), x.shape[0], rng.mix_table(kind, M_, H, W), H, W)
    return rng.mix_np(x, y, prm, kind)


def _check_working_copy(eng, x, y, p, flags):
    kind, M_ = C.parse_mix(flags["mix"])
    hx, hy, hy2, hlam = _host_pass(x, y, p, kind, M_)
    n = x.shape[0]
    assert eng.shuffler.loaded == p
    assert np.array_equal(eng.train_x[:n].cpu().numpy(), hx)
    assert np.array_equal(eng.train_y[:n].cpu().numpy(), hy.astype(np.int32))
    y2, lam = eng.mix_rows()
    assert np.array_equal(y2[:n].cpu().numpy(), hy2.astype(np.int32))
    assert np.array_equal(lam[:n].cpu().numpy(), hlam)
    # the any-batch-size pad rows: zero images, label 0, share 1
    assert float(eng.train_x[n:].abs().sum()) == 0.0 and int(eng.train_y[n:].abs().sum()) == 0
    assert int(y2[n:].abs().sum()) == 0 and bool((lam[n:] == 1).all())


# test_native_mnist_gpu.py::test_per_step_grads_along_native_trajectory's per-step model: a
# max-pool near-tie (fp32 summation order; the Winograd conv2 rounds ~1.4e-6 away from the
# oracle's direct sum) can re-route single elements of dY2 / dA1, which shifts the conv grads -
# never the FC grads or the loss - by up to TIE_ERR of their norm; everything else agrees to
# fp32 rounding.  That test allows 4 (winograd) / 2 (direct) such steps in 12 steps of 64 rows;
# pro rata for the 3 steps of at most 64 rows here that is 1 / 0.5, rounded up: 1.
TIE_ERR = {"winograd": 1e-2, "direct": 5e-3}
MAX_TIE_STEPS = 1


@pytest.mark.parametrize("flags", FLAGS, ids=IDS)
@pytest.mark.parametrize("kw", [dict(conv_algo="winograd"), dict(conv_algo="direct"),
                                dict(conv_algo="winograd", batch_size=64)],
                         ids=["winograd", "direct", "winograd-b64"])
def test_native_mnist_fp32_steps_match_torch_engine(cuda_dev, mnist200, kw, flags):
    """Three steps in three passes, each at the initial parameters: the loss
    within 1e-4 and the FC gradients - what the soft target changes - within 2e-4
    of the largest (test_mnist_any_batch_gpu.py's bounds) and 1e-4 by norm.  The
    2e-4 bound is NOT applied to the conv gradients: they are held only to the
    near-tie model above (measured: one step in three of winograd-mixup and of one
    other case moved conv2_weight by 3.6e-3 of the largest, 7e-4 by norm; every
    other step agrees to 2e-6), and MAX_TIE_STEPS is this file's own figure, not an
    existing one.  The images are uniform random, not the affine tests' shard:
    see the fixture."""
    x, y = mnist200
    nat = NativeMnistEngine(_cfg(**kw, **flags), x, y, cuda_dev)
    ref = TorchMnistEngine(_cfg(**{k: v for k, v in kw.items() if k != "conv_algo"}, **flags), x, y,
                           cuda_dev)
    assert nat.ptrs.train_y2 != 0 and nat.ptrs.train_lam != 0
    assert abs(nat.ptrs.label_smoothing - 0.1) < 1e-7
    ties = 0
    for step in STEPS:
        nat.set_step(step)
        ref.set_step(step)
        nat.forward_backward_only()
        ref.forward_backward(step)
        torch.cuda.synchronize()
        loss = nat.bufs["loss_rows"][:nat.B].sum().item() / nat.B
        nv, rv = nat.layout.views(nat.grads), ref.layout.views(ref.grads)
        mx = {s.name: (nv[s.name] - rv[s.name]).abs().max().item()
              / max(1e-6, rv[s.name].abs().max().item()) for s in nat.layout.specs}
        nrm = {s.name: ((nv[s.name] - rv[s.name]).norm() / rv[s.name].norm()).item()
               for s in nat.layout.specs}
        print(f"step={step} loss={loss:.6f} ref={ref.last_loss:.6f} max-rel",
              {k: f"{v:.1e}" for k, v in mx.items()}, "norm-rel",
              {k: f"{v:.1e}" for k, v in nrm.items()})
        assert abs(loss - ref.last_loss) < 1e-4
        for name in mx:
            if name.startswith("fc"):
                assert mx[name] < 2e-4 and nrm[name] < 1e-4, (step, name, mx[name], nrm[name])
        assert max(nrm.values()) < TIE_ERR[kw["conv_algo"]], (step, nrm)
        if max(nrm.values()) > 1e-4:
            ties += 1
        assert torch.equal(nat.train_x[:N], ref.train_x)
        _check_working_copy(nat, x.astype(np.float32), y, pass_of(step, N, nat.B), flags)
        if nat.Bp > nat.B:
            assert float(nat.bufs["dlog"].view(nat.Bp, 10)[nat.B:].abs().sum()) == 0.0
            assert float(nat.bufs["dh"].view(nat.Bp, -1)[nat.B:].abs().sum()) == 0.0
    assert ties <= MAX_TIE_STEPS, ties


@pytest.mark.parametrize("flags", FLAGS, ids=IDS)
@pytest.mark.parametrize("batch", [50, 64])
def test_native_mnist_bf16_steps_match_torch_engine(cuda_dev, batch, flags):
    """The bounds of test_mnist_bf16_gpu.py::test_bf16_grads_match_fp32_oracle and
    test_mnist_any_batch_gpu.py::test_bf16_grads_match_oracle_b50 (mask flips under
    bf16 rounding: loss 2e-2, gradients 6e-2 by norm, far above what a pooling tie
    moves) on the shard of test_augment_affine_gpu.py's engine tests, rows 0..199
    of `synthetic_rows`, at its batch 50 (Bp = 64: live pad rows) and at 64.

    Measured on an MI355X (the same figures on two boxes), the largest error of
    each case - conv1_weight, the gradient farthest from the head, every time:
    B = 50 mixup 5.61e-2, cutmix 5.97e-2 (step 6: it passes by little); B = 64
    mixup 5.41e-2, cutmix 5.14e-2.  The FC gradients, which the soft target feeds
    through dh16 / dht16, stay below 2.5e-2 and fc2 below 4e-3.  The narrow
    margin is this shard's at B = 50, not the flags': at step 6 the hard-label
    bf16 engine gives conv1_weight 5.79e-2 on the unmixed rows (6.30e-2 at step
    9, which no test uses) and 5.92e-2 / 5.97e-2 on the host-cutmixed /
    host-mixed-up rows, against 5.97e-2 / 5.61e-2 with the soft target."""
    x, y = synthetic_rows("train", 0, N)
    nat = NativeMnistEngine(_cfg(dtype="bf16", batch_size=batch, **flags), x, y, cuda_dev)
    ref = TorchMnistEngine(_cfg(batch_size=batch, **flags), x, y, cuda_dev)
    assert [pass_of(s, N, batch) for s in STEPS] == [0, 1, 2]
    for step in STEPS:
        nat.set_step(step)
        ref.set_step(step)
        nat.forward_backward_only()
        ref.forward_backward(step)
        torch.cuda.synchronize()
        loss = nat.bufs["loss_rows"][:nat.B].sum().item() / nat.B
        nv, rv = nat.layout.views(nat.grads), ref.layout.views(ref.grads)
        errs = {s.name: ((nv[s.name].float() - rv[s.name].float()).norm()
                         / max(1e-12, rv[s.name].float().norm())).item()
                for s in nat.layout.specs}
        print(f"bf16 B={batch} step={step} loss={loss:.5f} ref={ref.last_loss:.5f}",
              {k: f"{v:.3e}" for k, v in errs.items()})
        assert abs(loss - ref.last_loss) < 2e-2 * max(1, ref.last_loss)
        for name, e in errs.items():
            assert e < 6e-2, (step, name, e)
        _check_working_copy(nat, x.astype(np.float32), y, pass_of(step, N, nat.B), flags)
        if nat.Bp > nat.B:  # the pad rows' seed and its bf16 operand copies are exactly zero
            assert float(nat.bufs["dlog"].view(nat.Bp, 10)[nat.B:].abs().sum()) == 0.0
            assert float(nat.bufs["dh"].view(nat.Bp, -1)[nat.B:].abs().sum()) == 0.0
            assert float(nat.bufs["dh16"].float().view(-1, nat.Bp, 16)[:, nat.B:].abs().sum()) == 0.0
            d16 = nat.bufs["dht16"].float().view(nat.Bp // 16, -1, 16)
            assert float(d16[nat.B // 16, :, nat.B % 16:].abs().sum()) == 0.0


def test_label_smoothing_alone_needs_no_shuffler(cuda_dev, mnist200):
    """One step, so no tie count: loss and FC gradients at the strict bounds, the
    conv gradients only under TIE_ERR (not the 2e-4 bound)."""
    x, y = mnist200
    nat = NativeMnistEngine(_cfg(label_smoothing=0.1), x, y, cuda_dev)
    ref = TorchMnistEngine(_cfg(label_smoothing=0.1), x, y, cuda_dev)
    hard = NativeMnistEngine(_cfg(), x, y, cuda_dev)
    assert nat.shuffler is None and nat.ptrs.train_y2 == 0 and nat.ptrs.train_lam == 0
    assert hard.ptrs.label_smoothing == 0.0 and hard.ptrs.train_lam == 0
    for e in (nat, hard):
        e.set_step(2)
        e.forward_backward_only()
    ref.set_step(2)
    ref.forward_backward(2)
    torch.cuda.synchronize()
    loss = nat.bufs["loss_rows"][:nat.B].sum().item() / nat.B
    assert abs(loss - ref.last_loss) < 1e-4
    nv, rv = nat.layout.views(nat.grads), ref.layout.views(ref.grads)
    for s in nat.layout.specs:
        err = (nv[s.name] - rv[s.name]).abs().max().item() / max(1e-6, rv[s.name].abs().max().item())
        nrm = ((nv[s.name] - rv[s.name]).norm() / rv[s.name].norm()).item()
        print(s.name, f"{err:.1e} {nrm:.1e}")
        if s.name.startswith("fc"):
            assert err < 2e-4 and nrm < 1e-4, (s.name, err, nrm)
        assert nrm < TIE_ERR["winograd"], (s.name, nrm)  # (a near-tie: the model above)
    assert not torch.equal(nat.grads, hard.grads)


@pytest.mark.parametrize("flags", FLAGS, ids=IDS)
@pytest.mark.parametrize("kw", [dict(), dict(dtype="bf16"), dict(shuffle=True, augment="shift:2")],
                         ids=["fp32", "bf16", "shuffle-augment"])
def test_native_mnist_graph_equals_eager(cuda_dev, mnist200, kw, flags):
    """7 steps cross two pass boundaries: graph replay (2-step graphs + 1-step
    remainders) equals eager launches bit for bit."""
    x, y = mnist200
    eager = NativeMnistEngine(_cfg(**kw, **flags), x, y, cuda_dev)
    graphed = NativeMnistEngine(_cfg(graph=True, graph_steps=2, **kw, **flags), x, y, cuda_dev)
    p0 = eager.params.clone()
    eager.train(7)
    graphed.train(7)
    torch.cuda.synchronize()
    assert eager.step == graphed.step == int(graphed.step_dev.item()) == 7
    assert torch.equal(eager.params, graphed.params) and torch.equal(eager.mom, graphed.mom)
    assert torch.isfinite(eager.params).all() and not torch.equal(eager.params, p0)
    assert eager.shuffler.loaded == graphed.shuffler.loaded == 2
    for name in ("work_x", "work_y", "work_y2", "work_lam"):
        assert torch.equal(getattr(eager.shuffler, name), getattr(graphed.shuffler, name)), name
    if not kw.get("shuffle"):
        _check_working_copy(eager, x.astype(np.float32), y, 2, flags)


def test_schedule_tune_and_prewarm_leave_the_mixed_pass(cuda_dev, mnist200):
    """The sync-schedule tune (emulated 8-rank ring) and the pre-warm started at
    step 4: params, momentum, step and the working copy (pass 1, mixed, with its
    partner labels and shares) are afterwards those of step 4."""
    from mpi_tensorflow_amd.parallel.comm import EmulatedDeviceComm

    x, y = mnist200
    flags = FLAGS[0]
    comm = EmulatedDeviceComm(8, lat_us=10.0, busbw_gbps=150.0, blocks=32)
    eng = NativeMnistEngine(_cfg(graph=True, graph_steps=2, **flags), x, y, cuda_dev, comm=comm,
                            force_sync=True)
    eng.set_step(4)
    p0, m0 = eng.params.clone(), eng.mom.clone()
    assert eng.tune_schedule() > 0
    torch.cuda.synchronize()
    assert eng.step == int(eng.step_dev.item()) == 4
    assert torch.equal(eng.params, p0) and torch.equal(eng.mom, m0)
    _check_working_copy(eng, x.astype(np.float32), y, 1, flags)
    assert eng.prewarm_train(1.0) > 0
    torch.cuda.synchronize()
    assert eng.step == int(eng.step_dev.item()) == 4
    assert torch.equal(eng.params, p0) and torch.equal(eng.mom, m0)
    _check_working_copy(eng, x.astype(np.float32), y, 1, flags)
    eng.train(3)  # steps 4, 5 | 6
    torch.cuda.synchronize()
    assert eng.step == int(eng.step_dev.item()) == 7
    _check_working_copy(eng, x.astype(np.float32), y, 2, flags)
    assert torch.isfinite(eng.params).all() and not torch.equal(eng.params, p0)


def _lcfg(**kw):
    return C.TrainConfig(model="lenet5", batch_size=B_, graph=kw.pop("graph", False),
                         **kw).validate()


def _lenet_oracle(params, eng, x, y, step, flags):
    """fp64 gradients of the soft-target loss on the host-mixed batch of `step`
    (test_lenet_native_gpu.py's oracle with the definition's loss)."""
    from mpi_tensorflow_amd.models.generic import make_model

    kind, M_ = C.parse_mix(flags["mix"])
    hx, hy, hy2, hlam = _host_pass(x, y, pass_of(step, N, B_), kind, M_)
    m = make_model("lenet5")
    lay = m.layout
    p = params.detach().cpu().double().clone().requires_grad_(True)
    g = torch.zeros_like(p)
    pv, gv = lay.views(p), lay.views(g)
    P = {s.name: Fn.Param(pv[s.name], gv[s.name]) for s in lay.specs}
    off = batch_offset(step, N, B_)
    z = slice(off, off + B_)
    logits = m.forward(P, {}, torch.from_numpy(hx[z]).double(), True)
    t = torch.from_numpy(rng.soft_targets(hy[z], hy2[z], hlam[z], flags["label_smoothing"], 10))
    loss = -(t * torch.log_softmax(logits, 1)).sum(1).mean()
    (grad,) = torch.autograd.grad(loss, [p])
    return grad.float(), float(loss.detach())


@pytest.mark.parametrize("flags", FLAGS, ids=IDS)
def test_native_lenet_steps_and_graph(cuda_dev, lenet200, flags):
    x, y = lenet200
    eng = NativeLenetEngine(_lcfg(**flags), x, y, cuda_dev)
    ref = GenericEngine(_lcfg(device="cpu", **flags), x, y, torch.device("cpu"))
    lay = eng.layout
    for step in STEPS:
        eng.set_step(step)
        eng.forward_backward_only()
        torch.cuda.synchronize()
        want, want_loss = _lenet_oracle(eng.params, eng, x, y, step, flags)
        assert abs(eng.loss_rows.mean().item() - want_loss) < 1e-5 * max(1.0, want_loss)
        gv, rv = lay.views(eng.grads.cpu()), lay.views(want)
        errs = {s.name: float((gv[s.name] - rv[s.name]).abs().max()
                              / max(rv[s.name].abs().max(), 1e-12)) for s in lay.specs}
        print(step, {k: f"{v:.1e}" for k, v in errs.items()})
        for k, e in errs.items():
            assert e < 2e-5, (step, k, e)
        _check_working_copy(eng, x, y, pass_of(step, N, B_), flags)
    # the torch engine with the same flags, three steps (test_training_trajectory_matches_oracle)
    nat = NativeLenetEngine(_lcfg(**flags), x, y, cuda_dev)
    ref.params.data.copy_(nat.params.cpu())
    nat.train(3)
    ref.train(3)
    torch.cuda.synchronize()
    d = (nat.params.cpu() - ref.params.detach()).abs().max().item()
    assert d < 1e-4 * ref.params.detach().abs().max().item(), d
    # graph replay against eager launches across the boundaries
    a = NativeLenetEngine(_lcfg(graph=True, graph_steps=2, **flags), x, y, cuda_dev)
    b = NativeLenetEngine(_lcfg(**flags), x, y, cuda_dev)
    a.train(7)
    b.train(7)
    torch.cuda.synchronize()
    assert a.step == b.step == int(a.step_dev.item()) == 7
    assert torch.equal(a.params, b.params) and torch.equal(a.mom, b.mom)
    _check_working_copy(a, x, y, 2, flags)


@pytest.mark.parametrize("flags", FLAGS, ids=IDS)
def test_generic_engine_steps_and_graph(cuda_dev, lenet200, flags):
    x, y = lenet200
    gpu = GenericEngine(_lcfg(**flags), x, y, cuda_dev)
    cpu = GenericEngine(_lcfg(device="cpu", **flags), x, y, torch.device("cpu"))
    assert gpu.on_gpu and gpu.y2b is not None
    for step in STEPS:
        cpu.params.data.copy_(gpu.params.detach().cpu())
        gpu.set_step(step)
        cpu.set_step(step)
        gpu.forward_backward_gpu()
        cpu._step_cpu()  # (its update is overwritten by the copy above)
        torch.cuda.synchronize()
        assert abs(gpu.loss_value() - cpu.loss_value()) < 1e-4 * max(1.0, cpu.loss_value())
        gv, cv = gpu.layout.views(gpu.grads), cpu.layout.views(cpu.grads)
        for s in gpu.layout.specs:
            e = ((gv[s.name].cpu() - cv[s.name]).norm() / max(1e-12, cv[s.name].norm())).item()
            assert e < 1e-3, (step, s.name, e)
        p = pass_of(step, N, B_)
        _check_working_copy(gpu, x, y, p, flags)
        off = batch_offset(step, N, B_)
        y2, lam = gpu.mix_rows()
        assert torch.equal(gpu.y2b, y2[off:off + B_]) and torch.equal(gpu.lamb, lam[off:off + B_])
        assert torch.equal(cpu.train_x, gpu.train_x.cpu())
    a = GenericEngine(_lcfg(graph=True, graph_steps=2, **flags), x, y, cuda_dev)
    b = GenericEngine(_lcfg(**flags), x, y, cuda_dev)
    a.train(7)
    b.train(7)
    torch.cuda.synchronize()
    assert a.step == b.step == int(a.step_dev.item()) == 7
    assert torch.equal(a.params, b.params) and torch.equal(a.mom, b.mom)
    _check_working_copy(a, x, y, 2, flags)


def test_generic_bucket_tune_leaves_the_mixed_pass(cuda_dev, lenet200):
    """The generic engine's start-up tune (world-1 RCCL communicator, as
    test_generic_ops_gpu.py::test_generic_bucket_plan_autotune) started at step 3:
    params, momentum, step and the working copy (pass 1, mixed) are afterwards
    those of before, and training goes on as an untuned engine's.  (The native
    LeNet-5 engine tunes only over an xGMI communicator of several ranks, which
    one GPU does not have: its tune is not exercised here.)"""
    from mpi_tensorflow_amd.parallel.comm import RcclDeviceComm
    from mpi_tensorflow_amd.parallel.dist import DistInfo

    x, y = lenet200
    flags = FLAGS[0]
    comm = RcclDeviceComm(DistInfo())
    eng = GenericEngine(_lcfg(graph=True, graph_steps=2, **flags), x, y, cuda_dev, comm=comm,
                        force_sync=True)
    plain = GenericEngine(_lcfg(**flags), x, y, cuda_dev)
    for e in (eng, plain):
        e.set_step(3)
    assert pass_of(3, N, B_) == pass_of(5, N, B_) == 1  # (the tune's eager warm-up: steps 3..5)
    p0, m0 = eng.params.detach().clone(), eng.mom.clone()
    assert eng.tune_schedule() > 0
    torch.cuda.synchronize()
    assert eng.step == int(eng.step_dev.item()) == 3
    assert torch.equal(eng.params.detach(), p0) and torch.equal(eng.mom, m0)
    _check_working_copy(eng, x, y, 1, flags)
    eng.train(4)  # steps 3, 4, 5 | 6
    plain.train(4)
    torch.cuda.synchronize()
    assert eng.step == int(eng.step_dev.item()) == 7
    assert torch.equal(eng.params.detach(), plain.params.detach())
    assert torch.equal(eng.mom, plain.mom)
    _check_working_copy(eng, x, y, 2, flags)


# ------------------------------------------------------ two ranks, one GPU ----
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_buckets_and_factors_match_serial():
    """tests/helpers/mix_sync_ranks.py: 2 ranks on one GPU under
    --mix mixup:50 --label-smoothing 0.1, schedules buckets and factors."""
    port = str(_free_port())
    procs = []
    for r in range(2):
        env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", RANK=str(r), WORLD_SIZE="2",
                   LOCAL_RANK="0", LOCAL_WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "tests", "helpers", "mix_sync_ranks.py"), "4"],
            cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r}:\n{out[-4000:]}"
    assert "MIX_SYNC_OK world=2 steps=4" in outs[0]
