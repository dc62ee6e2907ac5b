"""Per-pass shuffled training batches (--shuffle) on the device: the HIP
permutation and row gather (csrc/kernels/shuffle.hip) against the host
permutation (utils/rng.py), and the native engines with shuffle on against
shuffle-off engines built on host-permuted data, bit for bit.
"""

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.ops import native, ptr, stream_handle
from mpi_tensorflow_amd.runtime.generic_engine import GenericEngine
from mpi_tensorflow_amd.runtime.lenet_engine import NativeLenetEngine
from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine, TorchMnistEngine
from mpi_tensorflow_amd.utils import rng
from mpi_tensorflow_amd.utils.data import pass_of, synthetic_rows
from test_mnist_any_batch_gpu import _check_grads_fp32

pytestmark = pytest.mark.gpu

KEYS = (0xde56f3b3, 1, 0xffffffff)
N, B = 200, 50  # 150 rows a pass: 3 steps; Bp = 64, so the pad rows are live


# ------------------------------------------------------------- the kernels --
@pytest.mark.parametrize("n", [2, 3, 33, 64, 65, 97, 1000, 8192, 55000])
def test_device_perm_equals_host(cuda_dev, n):
    """65 and 97 are the long walks (the Feistel domain is almost 4 n)."""
    ops = native().ops
    for key in KEYS:
        out = torch.full((n + 3,), -7, dtype=torch.int32, device=cuda_dev)
        ops.shuffle_perm(ptr(out), n, key, stream_handle())
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], rng.shuffle_perm(key, n)), (n, key)
        assert (got[n:] == -7).all()


def _rows_case(dev, n, row_elems, key, sentinels=3):
    g = torch.Generator(device="cpu").manual_seed(n * 7919 + row_elems)
    src_x = torch.randn(n, row_elems, generator=g).to(dev)
    src_y = torch.randint(0, 1000, (n,), generator=g, dtype=torch.int32).to(dev)
    dst_x = torch.full((n + sentinels, row_elems), -3.25, device=dev)
    dst_y = torch.full((n + sentinels,), -9, dtype=torch.int32, device=dev)
    return src_x, src_y, dst_x, dst_y


@pytest.mark.parametrize("row_elems", [1, 3, 4, 5, 784, 3072])
def test_shuffle_rows_equals_indexing(cuda_dev, row_elems):
    """float4 path (4, 784, 3072) and scalar path (1, 3, 5); 3072 floats is
    three vectors a thread, 784 leaves lanes idle."""
    n, key = 97, KEYS[0]
    src_x, src_y, dst_x, dst_y = _rows_case(cuda_dev, n, row_elems, key)
    keep_x, keep_y = src_x.clone(), src_y.clone()
    native().ops.shuffle_rows(ptr(src_x), ptr(src_y), ptr(dst_x), ptr(dst_y), n, row_elems, key,
                              stream_handle())
    torch.cuda.synchronize()
    perm = torch.from_numpy(rng.shuffle_perm(key, n)).to(cuda_dev)
    assert torch.equal(dst_x[:n], keep_x[perm])
    assert torch.equal(dst_y[:n], keep_y[perm])
    assert bool((dst_x[n:] == -3.25).all()) and bool((dst_y[n:] == -9).all())  # sentinel rows
    assert torch.equal(src_x, keep_x) and torch.equal(src_y, keep_y)


def test_shuffle_rows_long_rows_and_unaligned_base(cuda_dev):
    """A row of several 16 KB pieces with a ragged last one (the ResNet-shaped
    path: blockIdx.y picks the piece), more rows than workgroups of one piece
    column, and a base that is not 16-byte aligned (scalar path)."""
    ops = native().ops
    for n, row_elems, shift in ((5, 150528, 0), (1500, 4 * 1030, 0), (97, 784, 1)):
        key = KEYS[1]
        buf = torch.randn(n * row_elems + 4, device=cuda_dev)
        src_x = buf[shift:shift + n * row_elems].view(n, row_elems)
        src_y = torch.arange(n, dtype=torch.int32, device=cuda_dev)
        dst_x = torch.zeros(n, row_elems, device=cuda_dev)
        dst_y = torch.zeros(n, dtype=torch.int32, device=cuda_dev)
        ops.shuffle_rows(ptr(src_x), ptr(src_y), ptr(dst_x), ptr(dst_y), n, row_elems, key,
                         stream_handle())
        torch.cuda.synchronize()
        perm = torch.from_numpy(rng.shuffle_perm(key, n)).to(cuda_dev)
        assert torch.equal(dst_x, src_x[perm]), (n, row_elems, shift)
        assert torch.equal(dst_y, perm.to(torch.int32))


def test_shuffle_rows_element_offsets_past_2_31(cuda_dev):
    """33 rows of 2^26 + 4 floats: 2.2e9 elements, so the row offsets of the
    last rows do not fit 32 bits (and a row is 16385 pieces)."""
    n, row_elems, key = 33, (1 << 26) + 4, KEYS[2]
    assert n * row_elems > 2 ** 31
    base = torch.arange(row_elems, dtype=torch.float32, device=cuda_dev)
    src_x = torch.empty(n, row_elems, device=cuda_dev)
    for i in range(n):
        torch.mul(base, float(i + 1), out=src_x[i])
    del base
    dst_x = torch.zeros(n, row_elems, device=cuda_dev)
    native().ops.shuffle_rows(ptr(src_x), 0, ptr(dst_x), 0, n, row_elems, key, stream_handle())
    torch.cuda.synchronize()
    perm = rng.shuffle_perm(key, n)
    for i in range(n):
        assert torch.equal(dst_x[i], src_x[int(perm[i])]), i


def test_shuffle_rows_in_a_captured_graph(cuda_dev):
    n, row_elems, key = 97, 784, KEYS[0]
    src_x, src_y, dst_x, dst_y = _rows_case(cuda_dev, n, row_elems, key)
    ops = native().ops
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.shuffle_rows(ptr(src_x), ptr(src_y), ptr(dst_x), ptr(dst_y), n, row_elems, key,
                         stream_handle())
    perm = torch.from_numpy(rng.shuffle_perm(key, n)).to(cuda_dev)
    for _ in range(2):
        dst_x[:n].zero_()
        dst_y[:n].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(dst_x[:n], src_x[perm]) and torch.equal(dst_y[:n], src_y[perm])
        assert bool((dst_x[n:] == -3.25).all()) and bool((dst_y[n:] == -9).all())


# ------------------------------------------------------------ native MNIST --
@pytest.fixture(scope="module")
def mnist200():
    return synthetic_rows("train", 0, N)


def _cfg(**kw):
    return C.TrainConfig(batch_size=B, graph=kw.pop("graph", False), **kw).validate()


def _permuted(x, y, p, seed=1, rank=0):
    perm = rng.shuffle_perm(rng.shuffle_key(seed, rank, p), x.shape[0])
    return x[perm], y[perm]


@pytest.mark.parametrize("kw", [dict(conv_algo="winograd"), dict(conv_algo="direct"),
                                dict(dtype="bf16")], ids=["winograd", "direct", "bf16"])
def test_native_mnist_grads_equal_permuted_engine(cuda_dev, mnist200, kw):
    x, y = mnist200
    step = 4
    assert pass_of(step, N, B) == 1
    shuf = NativeMnistEngine(_cfg(shuffle=True, **kw), x, y, cuda_dev)
    plain = NativeMnistEngine(_cfg(**kw), *_permuted(x, y, 1), cuda_dev)
    assert plain.shuffler is None and shuf.Bp == 64
    for e in (shuf, plain):
        e.set_step(step)
        e.forward_backward_only()
    torch.cuda.synchronize()
    assert float(shuf.grads.abs().max()) > 0
    assert torch.equal(shuf.grads, plain.grads)
    assert torch.equal(shuf.train_x, plain.train_x) and torch.equal(shuf.train_y, plain.train_y)
    # the pad rows of the any-batch-size step are still zero
    assert shuf.train_x.shape[0] == N + 14
    assert float(shuf.train_x[N:].abs().sum()) == 0.0 and int(shuf.train_y[N:].abs().sum()) == 0
    # a step of another pass reloads the working copy
    file_order = NativeMnistEngine(_cfg(**kw), x, y, cuda_dev)
    assert not torch.equal(shuf.train_x, file_order.train_x)
    shuf.set_step(0)
    shuf.forward_backward_only()
    torch.cuda.synchronize()
    px, _ = _permuted(x, y, 0)
    assert np.array_equal(shuf.train_x[:N].cpu().numpy(), px)


def test_native_mnist_train_graph_equals_eager_equals_hand_loop(cuda_dev, mnist200):
    """7 steps cross two boundaries (3 steps a pass).  Graph replay (2-step
    graphs + 1-step remainders) equals eager launches, and both equal the run
    spelled out with shuffle-off engines on host-permuted data, bit for bit."""
    x, y = mnist200
    eager = NativeMnistEngine(_cfg(shuffle=True), x, y, cuda_dev)
    graphed = NativeMnistEngine(_cfg(shuffle=True, graph=True, graph_steps=2), x, y, cuda_dev)
    split = NativeMnistEngine(_cfg(shuffle=True, graph=True, graph_steps=2), x, y, cuda_dev)
    eager.train(7)
    graphed.train(7)
    for k in (2, 2, 3):  # the caller's cuts fall elsewhere
        split.train(k)
    hand = None
    for p, k in ((0, 3), (1, 3), (2, 1)):
        nxt = NativeMnistEngine(_cfg(), *_permuted(x, y, p), cuda_dev)
        if hand is not None:
            nxt.params.copy_(hand.params)
            nxt.mom.copy_(hand.mom)
            nxt.set_step(hand.step)
        hand = nxt
        hand.train(k)
    torch.cuda.synchronize()
    assert eager.step == graphed.step == split.step == hand.step == 7
    assert int(graphed.step_dev.item()) == 7
    for e in (graphed, split, hand):
        assert torch.equal(eager.params, e.params)
        assert torch.equal(eager.mom, e.mom)
    assert eager.shuffler.loaded == 2
    assert set(n for _, n in graphed._graphs) <= {1, 2}


@pytest.mark.parametrize("algo", ["winograd", "direct"])
def test_native_mnist_per_step_grads_match_shuffled_oracle(cuda_dev, algo):
    """Steps 0..6 (passes 0, 1, 2) against the shuffled PyTorch oracle with
    `_check_grads_fp32` and its bounds (loss 1e-4, gradients 2e-4 of the
    largest).  Those are the bounds of one forward + backward at the initial
    parameters; along a trained trajectory pooling ties exceed them with
    shuffle off too (test_per_step_grads_along_native_trajectory_b50), so each
    step is checked at the initial parameters, as that helper's other users do.

    The rows are uniform random images, not `synthetic_rows`: those are
    clipped to [-0.5, 0.5], and over their saturated flat regions the conv
    outputs of a pooling window are equal in exact arithmetic.  The Winograd
    conv2 rounds them apart and its pool-2 argmax then need not be the
    oracle's first-of-equals, a second valid subgradient.  Measured on rows
    0..199 of `synthetic_rows`: the batches of steps 2 and 4 differ from the
    oracle by 1.59e-2 of the largest conv2_weight gradient (conv2_bias, the FC
    gradients and the loss agree to 1e-6), with shuffle on and, by the same
    1.59e-2, for shuffle-off engines built on the host-permuted rows; `direct`
    stays at 7e-7.  With continuous pixels no two outputs tie and the oracle's
    gradient is unique."""
    g = np.random.default_rng(20240)
    x = g.random((N, 28, 28, 1), dtype=np.float32) - np.float32(0.5)
    y = g.integers(0, 10, N).astype(np.int64)
    nat = NativeMnistEngine(_cfg(shuffle=True, conv_algo=algo), x, y, cuda_dev)
    ref = TorchMnistEngine(_cfg(shuffle=True), x, y, cuda_dev)
    for step in range(7):
        _check_grads_fp32(nat, ref, step)
        assert nat.shuffler.loaded == ref.shuffler.loaded == pass_of(step, N, B)
        assert torch.equal(nat.train_x[:N], ref.train_x)


def test_schedule_tune_leaves_the_pass_of_the_step(cuda_dev, mnist200):
    """The sync-schedule tune (emulated 8-rank ring, as
    test_sync_schedule_autotune_with_emulated_ring) started at step 4: its
    trial steps are discarded, and afterwards the device step, the parameters
    and the working copy are those of step 4 (pass 1); training then goes on
    across the next boundary."""
    from mpi_tensorflow_amd.parallel.comm import EmulatedDeviceComm

    x, y = mnist200
    comm = EmulatedDeviceComm(8, lat_us=10.0, busbw_gbps=150.0, blocks=32)
    eng = NativeMnistEngine(_cfg(shuffle=True, graph=True, graph_steps=2), x, y, cuda_dev, comm=comm,
                            force_sync=True)
    eng.set_step(4)
    p0 = eng.params.clone()
    assert eng.tune_schedule() > 0
    torch.cuda.synchronize()
    assert eng.step == int(eng.step_dev.item()) == 4 and torch.equal(eng.params, p0)
    assert eng.shuffler.loaded == 1
    assert np.array_equal(eng.train_x[:N].cpu().numpy(), _permuted(x, y, 1)[0])
    eng.train(3)  # steps 4, 5 | 6
    torch.cuda.synchronize()
    assert eng.step == int(eng.step_dev.item()) == 7 and eng.shuffler.loaded == 2
    assert np.array_equal(eng.train_x[:N].cpu().numpy(), _permuted(x, y, 2)[0])
    assert np.array_equal(eng.train_y[:N].cpu().numpy(), _permuted(x, y, 2)[1].astype(np.int32))
    assert float(eng.train_x[N:].abs().sum()) == 0.0
    assert torch.isfinite(eng.params).all() and not torch.equal(eng.params, p0)


# ------------------------------------------------------ LeNet-5 / generic --
@pytest.fixture(scope="module")
def lenet200():
    return synthetic_rows("train", 0, N, shape=(32, 32, 3))


def _lcfg(**kw):
    return C.TrainConfig(model="lenet5", batch_size=B, graph=kw.pop("graph", False),
                         **kw).validate()


def test_native_lenet_grads_and_train_equal_permuted_engine(cuda_dev, lenet200):
    x, y = lenet200
    shuf = NativeLenetEngine(_lcfg(shuffle=True), x, y, cuda_dev)
    plain = NativeLenetEngine(_lcfg(), *_permuted(x, y, 1), cuda_dev)
    for e in (shuf, plain):
        e.set_step(4)
        e.forward_backward_only()
    torch.cuda.synchronize()
    assert float(shuf.grads.abs().max()) > 0
    assert torch.equal(shuf.grads, plain.grads)
    # train across the boundaries, graph replay against eager launches
    a = NativeLenetEngine(_lcfg(shuffle=True, graph=True, graph_steps=2), x, y, cuda_dev)
    b = NativeLenetEngine(_lcfg(shuffle=True), x, y, cuda_dev)
    a.train(7)
    b.train(7)
    torch.cuda.synchronize()
    assert a.step == b.step == int(a.step_dev.item()) == 7
    assert torch.equal(a.params, b.params) and torch.equal(a.mom, b.mom)
    assert np.array_equal(a.train_x.cpu().numpy(), _permuted(x, y, 2)[0])


def test_generic_engine_grads_and_train_equal_permuted_engine(cuda_dev, lenet200):
    x, y = lenet200
    shuf = GenericEngine(_lcfg(shuffle=True), x, y, cuda_dev)
    plain = GenericEngine(_lcfg(), *_permuted(x, y, 1), cuda_dev)
    assert shuf.on_gpu and plain.shuffler is None
    for e in (shuf, plain):
        e.set_step(4)
        e.forward_backward_gpu()
    torch.cuda.synchronize()
    assert float(shuf.grads.abs().max()) > 0
    assert torch.equal(shuf.grads, plain.grads)
    assert torch.equal(shuf.xb, plain.xb) and torch.equal(shuf.yb, plain.yb)
    # the PyTorch path of the same engine on the GPU indexes with the host permutation
    orc = GenericEngine(_lcfg(shuffle=True), x, y, cuda_dev, oracle=True)
    orc.set_step(4)
    orc.train(1)
    assert torch.equal(orc.train_x, shuf.train_x) and torch.equal(orc.train_y, shuf.train_y)
    # eager training across the boundaries ends on the order of pass 2
    t = GenericEngine(_lcfg(shuffle=True), x, y, cuda_dev)
    t.train(7)
    torch.cuda.synchronize()
    assert t.step == int(t.step_dev.item()) == 7
    assert np.array_equal(t.train_x.cpu().numpy(), _permuted(x, y, 2)[0])
