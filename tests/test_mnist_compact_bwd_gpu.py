"""Compact backward of the fp32 Winograd MNIST step (csrc/kernels/mnist.hip):
dY2 travels from fc1 backward to the conv2 backward as the pooled gradient
dp2 [B][7][7][64] + the pool2 argmax codes idx2 instead of the dense NHWC
image (one value and three structural zeros per 2x2 window), a1 is kept only
in its zero-bordered form a1pf, and the masked dA1 is not stored.  Every
surviving value and every summation order is the dense path's, so all
comparisons here are bitwise (torch.equal), no element exempt.

B = 32 is the engine's minimum: 16 filter groups (the XCD group mapping,
ngroups % 8 == 0) and 128 bwd-data blocks, the single-tile-row blocks pg = 3
included; B = 64 is the benchmark's batch."""
import pytest
import torch

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.models import mnist_cnn as M
from mpi_tensorflow_amd.ops import native, ptr, stream_handle
from mpi_tensorflow_amd.utils.data import synthetic_rows

pytestmark = pytest.mark.gpu

N_LOCAL = 512


def _expand(dp2, idx2):
    """dense NHWC dY2 of (pooled gradient, argmax code 2 dy + dx)"""
    B = dp2.shape[0]
    dy2 = torch.zeros(B, 14, 14, 64, dtype=dp2.dtype, device=dp2.device)
    zero = torch.zeros((), dtype=dp2.dtype, device=dp2.device)
    for k in range(4):
        dy2[:, k >> 1::2, k & 1::2, :] = torch.where(idx2 == k, dp2, zero)
    return dy2


def _pooled_grad(B, g):
    """seeded (dp2, idx2): uniform codes, about half the gradients zero (ReLU2
    masked), the rest of both signs"""
    idx2 = torch.randint(0, 4, (B, 7, 7, 64), generator=g).to(torch.uint8)
    dp2 = torch.randn(B, 7, 7, 64, generator=g)
    dp2 = torch.where(torch.rand(B, 7, 7, 64, generator=g) < 0.5, torch.zeros(()), dp2)
    for k in range(4):
        assert (idx2 == k).any()
    assert (dp2 == 0).any() and (dp2 > 0).any() and (dp2 < 0).any()
    return dp2, idx2


@pytest.fixture(scope="module", params=[32, 64])
def operands(request, cuda_dev):
    """one set of conv2 backward operands per batch size, shared and left
    unchanged by the tests"""
    B = request.param
    Cn = native()
    g = torch.Generator().manual_seed(1000 + B)
    dp2, idx2 = _pooled_grad(B, g)
    a1 = torch.relu(torch.randn(B, 14, 14, 32, generator=g))
    a1pf = torch.zeros(B, 18, 18, 32)
    a1pf[:, 2:16, 2:16] = a1
    idx1 = torch.randint(0, 4, (B, 14, 14, 32), generator=g).to(torch.uint8)
    w2 = torch.randn(5, 5, 32, 64, generator=g) * 0.05
    x, _ = synthetic_rows("train", 0, N_LOCAL)
    o = dict(B=B, dp2=dp2, idx2=idx2, a1=a1, a1pf=a1pf, idx1=idx1, w2=w2,
             x=torch.from_numpy(x), step=torch.tensor([3], dtype=torch.int64))
    o = {k: (v.to(cuda_dev) if torch.is_tensor(v) else v) for k, v in o.items()}
    o["dy2"] = _expand(o["dp2"], o["idx2"])
    assert int((o["dy2"] != 0).sum()) == int((o["dp2"] != 0).sum())
    o["Ud"] = torch.empty(36 * 64 * 32, device=cuda_dev)
    U = torch.empty(36 * 32 * 64, device=cuda_dev)
    Cn.mnist.conv2_wino_weights(ptr(o["w2"]), ptr(U), ptr(o["Ud"]), stream_handle())
    torch.cuda.synchronize()
    return o


def _outputs(o, da1m=True):
    k = native().mnist
    dev = o["dp2"].device
    B = o["B"]
    return dict(
        part2=torch.full((k.part2_floats_wino(B),), float("nan"), device=dev),
        part1=torch.full((B * 4 * 832,), float("nan"), device=dev),
        da1m=torch.full((B, 14, 14, 32), float("nan"), device=dev) if da1m else None)


def _merged(o, out, compact, a1=True):
    """both conv2 backward roles in one launch, as the executor runs them"""
    native().mnist.conv2_bwd_wino(
        ptr(o["Ud"]), ptr(o["a1"]) if a1 else 0, ptr(o["a1pf"]), 0 if compact else ptr(o["dy2"]),
        ptr(o["dp2"]) if compact else 0, ptr(o["idx2"]) if compact else 0, o["B"],
        ptr(out["da1m"]), ptr(out["part2"]), ptr(o["x"]), ptr(o["step"]), N_LOCAL, ptr(o["idx1"]),
        ptr(out["part1"]), stream_handle())
    torch.cuda.synchronize()


def _diff(name, a, b):
    """'' if a and b are equal bit for bit (NaN - a cell the kernel did not
    write - never is), else where they first differ"""
    if torch.equal(a, b):
        return ""
    bad = (a != b).flatten().nonzero().flatten()
    i = int(bad[0])
    return (f"{name}: {bad.numel()} of {a.numel()} differ, first at {i}: "
            f"{a.flatten()[i].item()!r} vs {b.flatten()[i].item()!r}; ")


def _same(a, b):
    msg = "".join(_diff(n, a[n], b[n]) for n in ("part2", "part1", "da1m")
                  if a[n] is not None and b[n] is not None)
    assert not msg, msg
    return True


def test_merged_backward_compact_equals_dense(operands):
    """part2 (all tap slabs and the db2 rows), part1 and da1m of the merged
    launch: compact (dp2, idx2) input vs its dense host expansion"""
    o = operands
    dense, comp = _outputs(o), _outputs(o)
    _merged(o, dense, compact=False)
    _merged(o, comp, compact=True)
    assert torch.isfinite(dense["part2"]).all() and torch.isfinite(dense["part1"]).all()
    assert torch.isfinite(dense["da1m"]).all()
    assert dense["part2"].abs().max() > 0 and dense["part1"].abs().max() > 0
    assert _same(dense, comp)


def test_backward_roles_compact_equal_dense(operands):
    """the two roles as launches of their own (the schedule with the FC SGD in
    the bwd-data launch): bwd-data + conv1 filter-gradient epilogue, and the
    filter gradient"""
    o = operands
    k = native().mnist
    s = stream_handle()
    B = o["B"]
    dense, comp = _outputs(o), _outputs(o)
    for out, compact in ((dense, False), (comp, True)):
        k.conv2_bwd_data_wino_c1(0 if compact else ptr(o["dy2"]), ptr(o["dp2"]) if compact else 0,
                                 ptr(o["idx2"]) if compact else 0, ptr(o["Ud"]), ptr(o["a1"]),
                                 ptr(o["a1pf"]), B, ptr(out["da1m"]), ptr(o["x"]), ptr(o["step"]),
                                 N_LOCAL, ptr(o["idx1"]), ptr(out["part1"]), s)
    k.conv2_bwd_filter_wino(ptr(o["a1pf"]), ptr(o["dy2"]), B, ptr(dense["part2"]), s)
    k.conv2_bwd_filter_wino_dp2(ptr(o["a1pf"]), ptr(o["dp2"]), ptr(o["idx2"]), B,
                                ptr(comp["part2"]), s)
    torch.cuda.synchronize()
    assert torch.isfinite(dense["part2"]).all() and torch.isfinite(dense["da1m"]).all()
    assert _same(dense, comp)
    # and the merged launch forms the same sums as the two launches
    merged = _outputs(o)
    _merged(o, merged, compact=True)
    assert _same(dense, merged)


def test_backward_without_a1_and_da1m(operands):
    """da1m = nullptr and the ReLU1 mask read from a1pf: same part1 / part2 as
    with both buffers, for either dY2 form"""
    o = operands
    full = _outputs(o)
    _merged(o, full, compact=False)
    for compact in (False, True):
        lean = _outputs(o, da1m=False)
        _merged(o, lean, compact=compact, a1=False)
        assert torch.isfinite(lean["part2"]).all() and torch.isfinite(lean["part1"]).all()
        assert _same(full, lean)
    # the mask from a1pf also fills da1m as before where a buffer is passed
    keep = _outputs(o)
    _merged(o, keep, compact=True, a1=False)
    assert _same(full, keep)


@pytest.mark.parametrize("B", [32, 64])
def test_fc1_backward_dp2_equals_dense(cuda_dev, B):
    """fc1 backward: the dense-mode dy2 is the host expansion of the
    compact-mode dp2 (seeded idx2; a2 with ReLU-inactive entries), and the
    other roles' gradients do not depend on the form"""
    k = native().mnist
    g = torch.Generator().manual_seed(77 + B)
    a2 = torch.relu(torch.randn(B, M.FC1_IN, generator=g)).to(cuda_dev)
    idx2 = torch.randint(0, 4, (B, M.FC1_IN), generator=g).to(torch.uint8).to(cuda_dev)
    dh = torch.randn(B, M.FC1_OUT, generator=g).to(cuda_dev)
    hd = torch.relu(torch.randn(B, M.FC1_OUT, generator=g)).to(cuda_dev)
    dlog = torch.randn(B, 10, generator=g).to(cuda_dev)
    w1 = (torch.randn(M.FC1_IN, M.FC1_OUT, generator=g) * 0.05).to(cuda_dev)
    assert (a2 == 0).any() and (a2 > 0).any()
    for c in range(4):
        assert (idx2 == c).any()
    s = stream_handle()

    def grads():
        return [torch.full((n,), float("nan"), device=cuda_dev)
                for n in (M.FC1_IN * M.FC1_OUT, M.FC1_OUT, M.FC1_OUT * 10, 10)]

    gd, gc = grads(), grads()
    dy2 = torch.full((B, 14, 14, 64), float("nan"), device=cuda_dev)
    dp2 = torch.full((B, 7, 7, 64), float("nan"), device=cuda_dev)
    k.fc1_bwd(ptr(a2), ptr(idx2), ptr(dh), ptr(hd), ptr(dlog), ptr(w1), B, *[ptr(t) for t in gd],
              ptr(dy2), 0, s)
    k.fc1_bwd_dp2(ptr(a2), ptr(idx2), ptr(dh), ptr(hd), ptr(dlog), ptr(w1), B,
                  *[ptr(t) for t in gc], ptr(dp2), s)
    torch.cuda.synchronize()
    assert torch.isfinite(dp2).all() and torch.isfinite(dy2).all()
    assert (dp2 == 0).any() and (dp2 > 0).any() and (dp2 < 0).any()
    assert float(dp2.view(B, -1)[a2 <= 0].abs().sum()) == 0.0
    assert torch.equal(dy2, _expand(dp2, idx2.view(B, 7, 7, 64)))
    for a, b in zip(gd, gc):
        assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("B", [32, 64])
def test_fused_forward_without_a1(cuda_dev, B):
    """the fused Winograd forward with a1 = nullptr leaves a1pf / idx1 / a2 /
    idx2 equal to the two-buffer call"""
    k = native().mnist
    g = torch.Generator().manual_seed(31)
    x, _ = synthetic_rows("train", 0, N_LOCAL)
    xd = torch.from_numpy(x).to(cuda_dev)
    w1 = (torch.randn(5, 5, 1, 32, generator=g) * 0.2).to(cuda_dev)
    b1 = (torch.randn(32, generator=g) * 0.1).to(cuda_dev)
    w2 = (torch.randn(5, 5, 32, 64, generator=g) * 0.05).to(cuda_dev)
    b2 = (torch.randn(64, generator=g) * 0.1).to(cuda_dev)
    st = torch.tensor([2], dtype=torch.int64, device=cuda_dev)
    U = torch.empty(36 * 32 * 64, device=cuda_dev)
    s = stream_handle()
    k.conv2_wino_weights(ptr(w2), ptr(U), 0, s)
    runs = []
    for with_a1 in (True, False):
        o = dict(a1=torch.full((B, 14, 14, 32), float("nan"), device=cuda_dev),
                 a1pf=torch.zeros(B, 18, 18, 32, device=cuda_dev),
                 idx1=torch.full((B, 14, 14, 32), 255, dtype=torch.uint8, device=cuda_dev),
                 a2=torch.full((B, 7, 7, 64), float("nan"), device=cuda_dev),
                 idx2=torch.full((B, 7, 7, 64), 255, dtype=torch.uint8, device=cuda_dev))
        k.conv12_fwd_wino(ptr(xd), ptr(st), N_LOCAL, B, ptr(w1), ptr(b1),
                          ptr(o["a1"]) if with_a1 else 0, ptr(o["a1pf"]), ptr(o["idx1"]), ptr(w2),
                          ptr(U), ptr(b2), ptr(o["a2"]), ptr(o["idx2"]), 0, s)
        runs.append(o)
    torch.cuda.synchronize()
    full, lean = runs
    assert torch.isfinite(full["a2"]).all() and int(full["idx1"].max()) < 4
    assert torch.equal(full["a1pf"][:, 2:16, 2:16], full["a1"])
    assert torch.isnan(lean["a1"]).all()  # not written
    for name in ("a1pf", "idx1", "a2", "idx2"):
        assert torch.equal(full[name], lean[name]), name


def _train_pair(cuda_dev, steps, **kw):
    from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine

    x, y = synthetic_rows("train", 0, 1024)
    out = []
    for compact in (True, False):
        cfg = C.TrainConfig(graph=True, batch_size=32, **kw.get("cfg", {})).validate()
        e = NativeMnistEngine(cfg, x, y, cuda_dev, compact_bwd=compact, **kw.get("eng", {}))
        assert e.wino and e.compact_bwd == compact and ("dp2" in e.bufs) == compact
        e.train(steps)
        out.append(e)
    torch.cuda.synchronize()
    return out


def _assert_same_state(a, b):
    assert torch.isfinite(a.params).all()
    assert torch.equal(a.params, b.params)
    assert torch.equal(a.mom, b.mom)
    assert torch.equal(a.bufs["loss_rows"], b.bufs["loss_rows"])


def test_engine_compact_bwd_bit_identical(cuda_dev):
    """30 captured steps at B = 32 with compact_bwd on and off: parameters,
    momenta and the loss are equal bit for bit"""
    a, b = _train_pair(cuda_dev, 30)
    assert a.bufs["a1"].numel() == 0 and a.bufs["dy2"].numel() == 0
    assert a.bufs["da1m"].numel() == 0 and b.bufs["dy2"].numel() > 0
    _assert_same_state(a, b)


def test_engine_compact_bwd_serial_schedule(cuda_dev):
    """the same through the multi-rank code (serial schedule on a world-1
    forced-sync communicator): the flat-gradient path runs the same bodies"""
    from mpi_tensorflow_amd.parallel.comm import RcclDeviceComm
    from mpi_tensorflow_amd.parallel.dist import DistInfo

    comm = RcclDeviceComm(DistInfo())
    a, b = _train_pair(cuda_dev, 30, cfg=dict(sync_schedule="serial"),
                       eng=dict(comm=comm, force_sync=True))
    assert a.sync_schedule == "serial" and b.sync_schedule == "serial"
    _assert_same_state(a, b)
