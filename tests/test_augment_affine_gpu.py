"""Rotate / scale / cutout in --augment on the device: the fused HIP load
(csrc/kernels/augment.hip affine_rows) against the host definition (utils/rng.py
affine_params / affine_np) bit for bit, and the native engines under
shift:2,rotate:10,scale:10 against plain engines built on host-transformed data.
The shapes and n are those of tests/test_augment_gpu.py with rotate:15,scale:15
added to each and a cutout on two of them.
"""

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.ops import native, ptr, stream_handle
from mpi_tensorflow_amd.runtime.generic_engine import GenericEngine
from mpi_tensorflow_amd.runtime.lenet_engine import NativeLenetEngine
from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine
from mpi_tensorflow_amd.utils import rng
from mpi_tensorflow_amd.utils.data import pass_of, synthetic_rows

pytestmark = pytest.mark.gpu

KEYS = (0xde56f3b3, 1, 0xffffffff)
N, B = 200, 50  # 150 rows a pass: 3 steps; Bp = 64, so the pad rows are live
SENTINELS = 3
S = C.AugmentSpec

# n, (H, W, C), spec
CASES = {
    "mnist-k2": (97, (28, 28, 1), S(2, False, -0.5, 15.0, 15.0, 0)),           # vector path
    "lenet-k4-flip": (97, (32, 32, 3), S(4, True, 0.0, 15.0, 15.0, 8)),        # 3-float pixels
    "5x7x3-k4": (5, (5, 7, 3), S(4, False, -0.5, 15.0, 15.0, 2)),              # scalar path, mostly fill
    "3x5x1-flip": (3, (3, 5, 1), S(0, True, 0.0, 15.0, 15.0, 0)),              # odd W
    "resnet-k16-flip": (3, (224, 224, 3), S(16, True, 0.25, 15.0, 15.0, 0)),   # 37 pieces, ragged last
    "one-row": (1, (28, 28, 1), S(2, True, -0.5, 15.0, 15.0, 0)),
}
# The cases the coverage conditions are asserted on: the 97-row 28x28x1 and 32x32x3 ones, where
# the definition itself gives 82-87 % interpolated pixels per key and levels from 0 to 128.  (The
# single 28x28x1 row of "one-row" is three draws in all: 75-90 % and no spread of levels to ask for.)
COVERED = ("mnist-k2", "lenet-k4-flip")


# -------------------------------------------------------------- the kernel --
def _case(dev, n, shape):
    g = torch.Generator(device="cpu").manual_seed(n * 7919 + int(np.prod(shape)))
    src_x = torch.randn((n,) + shape, generator=g)
    src_y = torch.randint(0, 1000, (n,), generator=g, dtype=torch.int32)
    return src_x.numpy(), src_y.numpy(), src_x.to(dev), src_y.to(dev)


def _dst(dev, n, shape):
    return (torch.full((n + SENTINELS,) + shape, -3.25, device=dev),
            torch.full((n + SENTINELS,), -9, dtype=torch.int32, device=dev))


def _tables(dev, spec):
    return torch.from_numpy(rng.affine_tables(spec.rotate, spec.scale)).to(dev)


def _host(x, y, use_perm, perm_key, aug_key, spec):
    """The definition's rows and labels, and its draws."""
    n, H, W, _ = x.shape
    rows = rng.shuffle_perm(perm_key, n) if use_perm else np.arange(n)
    q = rng.affine_params(aug_key, rows, spec, H, W)
    return rng.affine_np(x[rows], q.m, q.dy, q.dx, q.flipped, spec.fill, q.cutout), y[rows], q


def _interpolated_share(q, H, W):
    """Share of output pixels whose four taps lie inside the image and whose
    sample blends them (a non-zero fx or fy), by the definition's own coordinates."""
    SX, SY = rng.affine_coords(np, q.m, q.dy, q.dx, q.flipped, H, W)
    ix, iy = SX >> 17, SY >> 17
    inside = (ix >= 0) & (ix + 1 < W) & (iy >= 0) & (iy + 1 < H)
    return float((inside & (((SX & 0x1FFFF) != 0) | ((SY & 0x1FFFF) != 0))).mean())


def _launch(src_x, src_y, dst_x, dst_y, n, shape, use_perm, perm_key, aug_key, spec, tables):
    native().ops.affine_rows(ptr(src_x), ptr(src_y), ptr(dst_x), ptr(dst_y), n, *shape, use_perm,
                             perm_key, aug_key, spec.K, spec.flip, spec.fill, ptr(tables),
                             spec.cutout, stream_handle())


@pytest.mark.parametrize("use_perm", [False, True], ids=["file-order", "perm"])
@pytest.mark.parametrize("case", list(CASES))
def test_affine_rows_equals_host(cuda_dev, case, use_perm):
    n, shape, spec = CASES[case]
    H, W, _ = shape
    hx, hy, src_x, src_y = _case(cuda_dev, n, shape)
    tables = _tables(cuda_dev, spec)
    flips, ias, ibs = set(), [], []
    for j, aug_key in enumerate(KEYS):
        perm_key = KEYS[(j + 1) % 3]
        dst_x, dst_y = _dst(cuda_dev, n, shape)
        _launch(src_x, src_y, dst_x, dst_y, n, shape, use_perm, perm_key, aug_key, spec, tables)
        torch.cuda.synchronize()
        want_x, want_y, q = _host(hx, hy, use_perm, perm_key, aug_key, spec)
        flips |= set(q.flipped.tolist())
        ias += q.ia.tolist()
        ibs += q.ib.tolist()
        assert np.array_equal(dst_x[:n].cpu().numpy(), want_x), (case, hex(aug_key))
        assert np.array_equal(dst_y[:n].cpu().numpy(), want_y)
        assert bool((dst_x[n:] == -3.25).all()) and bool((dst_y[n:] == -9).all())  # sentinel rows
        assert np.array_equal(src_x.cpu().numpy(), hx) and np.array_equal(src_y.cpu().numpy(), hy)
        if case in COVERED:  # the comparison is not one of fill against fill
            share = _interpolated_share(q, H, W)
            print(f"{case} {hex(aug_key)}: interpolated share {share:.3f}")
            assert share >= 0.80
        if spec.cutout:
            assert (want_x == np.float32(spec.fill)).all(axis=-1).sum() >= n * spec.cutout ** 2
    if case in COVERED:  # both signs of both levels
        assert min(ias) < 64 < max(ias) and min(ibs) < 64 < max(ibs)
    if spec.flip and n > 1:
        assert flips == {False, True}  # both kinds of row were run


def test_affine_rows_unaligned_bases(cuda_dev):
    """A src_x (and a dst_x) base one float off 16-byte alignment takes the
    scalar path: the same result as the aligned call."""
    n, shape, spec = CASES["mnist-k2"]
    spec = S(spec.K, True, spec.fill, spec.rotate, spec.scale, 5)
    hx, hy, src_x, src_y = _case(cuda_dev, n, shape)
    tables = _tables(cuda_dev, spec)
    want_x, want_y, _ = _host(hx, hy, True, KEYS[1], KEYS[0], spec)
    row = int(np.prod(shape))
    buf = torch.zeros(n * row + 4, device=cuda_dev)
    off_src = buf[1:1 + n * row].view((n,) + shape)
    off_src.copy_(src_x)
    assert ptr(off_src) % 16 == 4
    dst_x, dst_y = _dst(cuda_dev, n, shape)
    _launch(off_src, src_y, dst_x, dst_y, n, shape, True, KEYS[1], KEYS[0], spec, tables)
    torch.cuda.synchronize()
    assert np.array_equal(dst_x[:n].cpu().numpy(), want_x)
    assert np.array_equal(dst_y[:n].cpu().numpy(), want_y)
    assert bool((dst_x[n:] == -3.25).all())
    out = torch.full((n * row + 8,), -3.25, device=cuda_dev)
    off_dst = out[1:1 + n * row].view((n,) + shape)
    _launch(src_x, src_y, off_dst, dst_y, n, shape, True, KEYS[1], KEYS[0], spec, tables)
    torch.cuda.synchronize()
    assert np.array_equal(off_dst.cpu().numpy(), want_x)
    assert float(out[0]) == -3.25 and bool((out[1 + n * row:] == -3.25).all())


def test_affine_rows_in_a_captured_graph(cuda_dev):
    n, shape, spec = CASES["lenet-k4-flip"]
    hx, hy, src_x, src_y = _case(cuda_dev, n, shape)
    tables = _tables(cuda_dev, spec)
    dst_x, dst_y = _dst(cuda_dev, n, shape)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _launch(src_x, src_y, dst_x, dst_y, n, shape, True, KEYS[0], KEYS[2], spec, tables)
    want_x, want_y, _ = _host(hx, hy, True, KEYS[0], KEYS[2], spec)
    for _ in range(2):
        dst_x[:n].zero_()
        dst_y[:n].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(dst_x[:n].cpu().numpy(), want_x)
        assert np.array_equal(dst_y[:n].cpu().numpy(), want_y)
        assert bool((dst_x[n:] == -3.25).all()) and bool((dst_y[n:] == -9).all())


def test_affine_rows_argument_checks(cuda_dev):
    """Each raises before anything is launched: dst keeps its sentinels."""
    n, shape, spec = CASES["mnist-k2"]
    _, _, src_x, src_y = _case(cuda_dev, n, shape)
    dst_x, dst_y = _dst(cuda_dev, n, shape)
    tab = ptr(_tables(cuda_dev, spec))
    keep = src_x.clone()
    ops, st = native().ops, stream_handle()
    args = (n, *shape, True, KEYS[0], KEYS[1])
    K, tail = spec.K, (spec.flip, spec.fill, tab, 0, st)
    with pytest.raises(RuntimeError, match="overlap"):  # src == dst
        ops.affine_rows(ptr(src_x), ptr(src_y), ptr(src_x), ptr(dst_y), *args, K, *tail)
    with pytest.raises(RuntimeError, match="overlap"):  # dst starts inside src
        ops.affine_rows(ptr(src_x), ptr(src_y), ptr(src_x[n - 1]), ptr(dst_y), *args, K, *tail)
    with pytest.raises(RuntimeError, match="overlap"):  # the labels
        ops.affine_rows(ptr(src_x), ptr(src_y), ptr(dst_x), ptr(src_y), *args, K, *tail)
    for bad_k in (28, 29, -1):  # K >= min(H, W)
        with pytest.raises(RuntimeError, match="shift"):
            ops.affine_rows(ptr(src_x), ptr(src_y), ptr(dst_x), ptr(dst_y), *args, bad_k, *tail)
    for bad_s in (28, 29, -1):  # S >= min(H, W)
        with pytest.raises(RuntimeError, match="cutout"):
            ops.affine_rows(ptr(src_x), ptr(src_y), ptr(dst_x), ptr(dst_y), *args, K, spec.flip,
                            spec.fill, tab, bad_s, st)
    with pytest.raises(RuntimeError, match="null table"):
        ops.affine_rows(ptr(src_x), ptr(src_y), ptr(dst_x), ptr(dst_y), *args, K, spec.flip,
                        spec.fill, 0, 0, st)
    with pytest.raises(RuntimeError, match="null"):  # a null dst_x
        ops.affine_rows(ptr(src_x), ptr(src_y), 0, ptr(dst_y), *args, K, *tail)
    with pytest.raises(RuntimeError, match="null"):
        ops.affine_rows(ptr(src_x), ptr(src_y), ptr(dst_x), 0, *args, K, *tail)
    with pytest.raises(RuntimeError, match="n out of range"):
        ops.affine_rows(ptr(src_x), ptr(src_y), ptr(dst_x), ptr(dst_y), -1, *args[1:], K, *tail)
    with pytest.raises(RuntimeError, match="1024"):  # 32-bit source coordinates
        ops.affine_rows(ptr(src_x), ptr(src_y), ptr(dst_x), ptr(dst_y), 1, 1025, 2, 1, False, 0,
                        KEYS[1], 0, *tail)
    torch.cuda.synchronize()
    assert bool((dst_x == -3.25).all()) and bool((dst_y == -9).all())
    assert torch.equal(src_x, keep)


# ------------------------------------------------------------ native MNIST --
SPEC = "shift:2,rotate:10,scale:10"


@pytest.fixture(scope="module")
def mnist200():
    return synthetic_rows("train", 0, N)


def _cfg(**kw):
    return C.TrainConfig(batch_size=B, graph=kw.pop("graph", False), **kw).validate()


def _host_pass(x, y, p, shuffle, model="mnist_cnn", seed=1, rank=0):
    """Rows and labels of pass p as the definition gives them."""
    hx, hy, _ = _host(x, y, shuffle, rng.shuffle_key(seed, rank, p), rng.augment_key(seed, rank, p),
                      C.parse_augment_spec(SPEC, model))
    return hx, hy


@pytest.fixture(scope="module")
def mnist_passes(mnist200):
    """(shuffle, pass) -> host-transformed rows, computed once."""
    x, y = mnist200
    return {(sh, p): _host_pass(x, y, p, sh) for sh in (False, True) for p in (0, 1, 2)}


@pytest.mark.parametrize("shuffle", [False, True], ids=["file-order", "shuffle"])
@pytest.mark.parametrize("kw", [dict(conv_algo="winograd"), dict(conv_algo="direct"),
                                dict(dtype="bf16")], ids=["winograd", "direct", "bf16"])
def test_native_mnist_grads_equal_host_transformed_engine(cuda_dev, mnist200, mnist_passes, kw,
                                                          shuffle):
    x, y = mnist200
    step = 4
    assert pass_of(step, N, B) == 1
    aug = NativeMnistEngine(_cfg(augment=SPEC, shuffle=shuffle, **kw), x, y, cuda_dev)
    assert aug.shuffler.affine is not None and aug.shuffler.tables.device.type == "cuda"
    hx, hy = mnist_passes[shuffle, 1]
    plain = NativeMnistEngine(_cfg(**kw), hx, hy, cuda_dev)
    assert plain.shuffler is None and aug.Bp == 64
    for e in (aug, plain):
        e.set_step(step)
        e.forward_backward_only()
    torch.cuda.synchronize()
    assert float(aug.grads.abs().max()) > 0
    assert torch.equal(aug.grads, plain.grads)
    assert np.array_equal(aug.train_x[:N].cpu().numpy(), hx)
    assert np.array_equal(aug.train_y[:N].cpu().numpy(), hy.astype(np.int32))
    # the pad rows of the any-batch-size step are still zero
    assert float(aug.train_x[N:].abs().sum()) == 0.0 and int(aug.train_y[N:].abs().sum()) == 0
    # a step of another pass reloads the working copy; pass 0 is augmented too
    aug.set_step(0)
    aug.forward_backward_only()
    torch.cuda.synchronize()
    h0, _ = mnist_passes[shuffle, 0]
    assert np.array_equal(aug.train_x[:N].cpu().numpy(), h0)
    assert not np.array_equal(h0, hx) and not np.array_equal(h0, x)


@pytest.mark.parametrize("shuffle", [False, True], ids=["file-order", "shuffle"])
def test_native_mnist_train_graph_equals_eager_equals_hand_loop(cuda_dev, mnist200, mnist_passes,
                                                                shuffle):
    """7 steps cross two boundaries (3 steps a pass).  Graph replay (2-step
    graphs + 1-step remainders) equals eager launches, and both equal the run
    spelled out with plain engines on host-transformed data, bit for bit."""
    x, y = mnist200
    kw = dict(augment=SPEC, shuffle=shuffle)
    eager = NativeMnistEngine(_cfg(**kw), x, y, cuda_dev)
    graphed = NativeMnistEngine(_cfg(graph=True, graph_steps=2, **kw), x, y, cuda_dev)
    eager.train(7)
    graphed.train(7)
    hand = None
    for p, k in ((0, 3), (1, 3), (2, 1)):
        nxt = NativeMnistEngine(_cfg(), *mnist_passes[shuffle, p], cuda_dev)
        if hand is not None:
            nxt.params.copy_(hand.params)
            nxt.mom.copy_(hand.mom)
            nxt.set_step(hand.step)
        hand = nxt
        hand.train(k)
    torch.cuda.synchronize()
    assert eager.step == graphed.step == hand.step == 7
    assert int(graphed.step_dev.item()) == 7
    for e in (graphed, hand):
        assert torch.equal(eager.params, e.params)
        assert torch.equal(eager.mom, e.mom)
    assert eager.shuffler.loaded == 2


def test_schedule_tune_leaves_the_augmented_pass_of_the_step(cuda_dev, mnist200, mnist_passes):
    """The sync-schedule tune (emulated 8-rank ring) started at step 4: its
    trial steps are discarded, and afterwards the device step, the parameters
    and the working copy are those of step 4 (pass 1, augmented); training
    then goes on across the next boundary."""
    from mpi_tensorflow_amd.parallel.comm import EmulatedDeviceComm

    x, y = mnist200
    comm = EmulatedDeviceComm(8, lat_us=10.0, busbw_gbps=150.0, blocks=32)
    eng = NativeMnistEngine(_cfg(augment=SPEC, shuffle=True, graph=True, graph_steps=2), x, y,
                            cuda_dev, comm=comm, force_sync=True)
    eng.set_step(4)
    p0 = eng.params.clone()
    assert eng.tune_schedule() > 0
    torch.cuda.synchronize()
    assert eng.step == int(eng.step_dev.item()) == 4 and torch.equal(eng.params, p0)
    assert eng.shuffler.loaded == 1
    assert np.array_equal(eng.train_x[:N].cpu().numpy(), mnist_passes[True, 1][0])
    eng.train(3)  # steps 4, 5 | 6
    torch.cuda.synchronize()
    assert eng.step == int(eng.step_dev.item()) == 7 and eng.shuffler.loaded == 2
    h2x, h2y = mnist_passes[True, 2]
    assert np.array_equal(eng.train_x[:N].cpu().numpy(), h2x)
    assert np.array_equal(eng.train_y[:N].cpu().numpy(), h2y.astype(np.int32))
    assert float(eng.train_x[N:].abs().sum()) == 0.0
    assert torch.isfinite(eng.params).all() and not torch.equal(eng.params, p0)


# ------------------------------------------------------ LeNet-5 / generic --
@pytest.fixture(scope="module")
def lenet200():
    return synthetic_rows("train", 0, N, shape=(32, 32, 3))


@pytest.fixture(scope="module")
def lenet_passes(lenet200):
    x, y = lenet200
    return {(sh, p): _host_pass(x, y, p, sh, "lenet5") for sh in (False, True) for p in (1, 2)}


def _lcfg(**kw):
    return C.TrainConfig(model="lenet5", batch_size=B, graph=kw.pop("graph", False),
                         **kw).validate()


@pytest.mark.parametrize("shuffle", [False, True], ids=["file-order", "shuffle"])
def test_native_lenet_grads_and_train_equal_host_transformed_engine(cuda_dev, lenet200,
                                                                    lenet_passes, shuffle):
    x, y = lenet200
    kw = dict(augment=SPEC, shuffle=shuffle)
    aug = NativeLenetEngine(_lcfg(**kw), x, y, cuda_dev)
    plain = NativeLenetEngine(_lcfg(), *lenet_passes[shuffle, 1], cuda_dev)
    for e in (aug, plain):
        e.set_step(4)
        e.forward_backward_only()
    torch.cuda.synchronize()
    assert float(aug.grads.abs().max()) > 0
    assert torch.equal(aug.grads, plain.grads)
    assert torch.equal(aug.train_x, plain.train_x) and torch.equal(aug.train_y, plain.train_y)
    # train across the boundaries, graph replay against eager launches
    a = NativeLenetEngine(_lcfg(graph=True, graph_steps=2, **kw), x, y, cuda_dev)
    b = NativeLenetEngine(_lcfg(**kw), x, y, cuda_dev)
    a.train(7)
    b.train(7)
    torch.cuda.synchronize()
    assert a.step == b.step == int(a.step_dev.item()) == 7
    assert torch.equal(a.params, b.params) and torch.equal(a.mom, b.mom)
    assert np.array_equal(a.train_x.cpu().numpy(), lenet_passes[shuffle, 2][0])
    assert np.array_equal(b.train_x.cpu().numpy(), lenet_passes[shuffle, 2][0])


@pytest.mark.parametrize("shuffle", [False, True], ids=["file-order", "shuffle"])
def test_generic_engine_grads_and_train_equal_host_transformed_engine(cuda_dev, lenet200,
                                                                      lenet_passes, shuffle):
    x, y = lenet200
    kw = dict(augment=SPEC, shuffle=shuffle)
    aug = GenericEngine(_lcfg(**kw), x, y, cuda_dev)
    h1x, h1y = lenet_passes[shuffle, 1]
    plain = GenericEngine(_lcfg(), h1x, h1y, cuda_dev)
    assert aug.on_gpu and plain.shuffler is None
    for e in (aug, plain):
        e.set_step(4)
        e.forward_backward_gpu()
    torch.cuda.synchronize()
    assert float(aug.grads.abs().max()) > 0
    assert torch.equal(aug.grads, plain.grads)
    assert torch.equal(aug.xb, plain.xb) and torch.equal(aug.yb, plain.yb)
    assert np.array_equal(aug.train_x.cpu().numpy(), h1x)
    # the PyTorch path of the same engine on the GPU: host permutation + the torch transform
    orc = GenericEngine(_lcfg(**kw), x, y, cuda_dev, oracle=True)
    orc.set_step(4)
    orc.train(1)
    assert torch.equal(orc.train_x, aug.train_x) and torch.equal(orc.train_y, aug.train_y)
    # training across the boundaries, graph replay against eager launches
    a = GenericEngine(_lcfg(graph=True, graph_steps=2, **kw), x, y, cuda_dev)
    b = GenericEngine(_lcfg(**kw), x, y, cuda_dev)
    a.train(7)
    b.train(7)
    torch.cuda.synchronize()
    assert a.step == b.step == int(a.step_dev.item()) == 7
    assert torch.equal(a.params, b.params) and torch.equal(a.mom, b.mom)
    h2x, h2y = lenet_passes[shuffle, 2]
    for e in (a, b):
        assert np.array_equal(e.train_x.cpu().numpy(), h2x)
        assert np.array_equal(e.train_y.cpu().numpy(), h2y.astype(np.int32))
