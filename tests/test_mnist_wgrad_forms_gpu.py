"""The forms of the Winograd conv2 filter gradient (csrc/kernels/mnist.hip
bwd_filter_wino_block, native().mnist.set_wgrad_form): the older form (mask
0), each shorter form alone and the default, on one build.  A form changes
which thread does a piece of work and how addresses are formed, never a float
expression or the order of a sum, so every comparison is torch.equal over the
whole buffer - the db2 rows included - pre-filled with NaN.  The values
themselves are guarded by the fp64 checks of test_wino_gpu.py.

Batches: 1 (one group, its second image masked), 2 (one full group), 3 (a
partial last group), 16 (8 groups: the XCD-aware block mapping), 18 (9 groups:
the plain mapping)."""
import pytest
import torch

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.ops import native, ptr, stream_handle
from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine
from mpi_tensorflow_amd.utils.data import synthetic_rows

pytestmark = pytest.mark.gpu

N_LOCAL = 512
BATCHES = (1, 2, 3, 16, 18)


@pytest.fixture
def forms(cuda_dev):
    k = native().mnist
    yield k
    k.set_wgrad_form(-1)


def _masks(k):
    """the older form, each kept form alone, the default"""
    bits = [1 << i for i in range(8) if k.WGRAD_DEFAULT >> i & 1]
    return [0] + bits + [-1]


@pytest.fixture(scope="module")
def operands(cuda_dev):
    """per batch size: ReLU'd a1 in its zero-bordered form, a pool-scattered
    dY2 (one value per 2x2 window, as in
    test_wino_conv2_bwd_filter_matches_oracle) with its compact form dp2 / idx2,
    and what the merged launch's other role reads; shared, left unchanged"""
    Cn = native()
    out = {}
    x, _ = synthetic_rows("train", 0, N_LOCAL)
    for B in BATCHES:
        g = torch.Generator().manual_seed(13 + B)
        a1 = torch.relu(torch.randn(B, 14, 14, 32, generator=g))
        dp2 = torch.randn(B, 7, 7, 64, generator=g)
        idx2 = torch.randint(0, 4, (B, 7, 7, 64), generator=g).to(torch.uint8)
        dy2 = torch.zeros(B, 14, 14, 64)
        for q in range(4):
            dy2[:, q >> 1::2, q & 1::2, :] = torch.where(idx2 == q, dp2, torch.zeros(()))
        a1pf = torch.zeros(B, 18, 18, 32)
        a1pf[:, 2:16, 2:16] = a1
        idx1 = torch.randint(0, 4, (B, 14, 14, 32), generator=g).to(torch.uint8)
        w2 = torch.randn(5, 5, 32, 64, generator=g) * 0.05
        o = dict(a1pf=a1pf, dy2=dy2, dp2=dp2, idx2=idx2, idx1=idx1, w2=w2, x=torch.from_numpy(x),
                 step=torch.tensor([3], dtype=torch.int64))
        o = {n: v.to(cuda_dev) for n, v in o.items()}
        o["B"] = B
        o["Ud"] = torch.empty(36 * 64 * 32, device=cuda_dev)
        U = torch.empty(36 * 32 * 64, device=cuda_dev)
        Cn.mnist.conv2_wino_weights(ptr(o["w2"]), ptr(U), ptr(o["Ud"]), stream_handle())
        out[B] = o
    torch.cuda.synchronize()
    return out


def _nan(n, dev):
    return torch.full((n,), float("nan"), device=dev)


def _diff(name, a, b):
    if torch.equal(a, b):
        return ""
    bad = (a != b).flatten().nonzero().flatten()
    i = int(bad[0])
    return (f"{name}: {bad.numel()} of {a.numel()} differ, first at {i}: "
            f"{a.flatten()[i].item()!r} vs {b.flatten()[i].item()!r}; ")


@pytest.mark.parametrize("compact", [False, True], ids=["dy2", "dp2"])
@pytest.mark.parametrize("B", BATCHES)
def test_standalone_forms_write_equal_part2(operands, forms, B, compact):
    """conv2_bwd_filter_wino (dense dy2) / conv2_bwd_filter_wino_dp2 (compact):
    the whole part2 buffer under every mask equals the older form's"""
    k, o = forms, operands[B]
    dev = o["dy2"].device
    got = {}
    for mask in _masks(k):
        k.set_wgrad_form(mask)
        part2 = _nan(k.part2_floats_wino(B), dev)
        if compact:
            k.conv2_bwd_filter_wino_dp2(ptr(o["a1pf"]), ptr(o["dp2"]), ptr(o["idx2"]), B,
                                        ptr(part2), stream_handle())
        else:
            k.conv2_bwd_filter_wino(ptr(o["a1pf"]), ptr(o["dy2"]), B, ptr(part2), stream_handle())
        torch.cuda.synchronize()
        got[mask] = part2
    G = k.conv2_wino_filter_groups(B)
    old = got[0]
    assert torch.isfinite(old).all() and old[:G * 51200].abs().max() > 0
    assert old[G * 51200:].abs().max() > 0  # the db2 rows
    msg = "".join(_diff(f"mask {m}", old, p) for m, p in got.items() if m != 0)
    assert not msg, msg


@pytest.mark.parametrize("B", [2, 18])
def test_merged_launch_forms_write_equal_outputs(operands, forms, B):
    """conv2_bwd_wino (compact form), both roles in one launch: part2 under
    every mask equals the older form's, and so do part1 and da1m - the bwd-data
    role shares the kernel with the filter-gradient role and must not move"""
    k, o = forms, operands[B]
    dev = o["dp2"].device
    got = {}
    for mask in _masks(k):
        k.set_wgrad_form(mask)
        out = dict(part2=_nan(k.part2_floats_wino(B), dev), part1=_nan(B * 4 * 832, dev),
                   da1m=_nan(B * 14 * 14 * 32, dev))
        k.conv2_bwd_wino(ptr(o["Ud"]), 0, ptr(o["a1pf"]), 0, ptr(o["dp2"]), ptr(o["idx2"]), B,
                         ptr(out["da1m"]), ptr(out["part2"]), ptr(o["x"]), ptr(o["step"]), N_LOCAL,
                         ptr(o["idx1"]), ptr(out["part1"]), stream_handle())
        torch.cuda.synchronize()
        got[mask] = out
    old = got[0]
    for n in ("part2", "part1", "da1m"):
        assert torch.isfinite(old[n]).all() and old[n].abs().max() > 0, n
    msg = "".join(_diff(f"mask {m} {n}", old[n], out[n])
                  for m, out in got.items() if m != 0 for n in ("part2", "part1", "da1m"))
    assert not msg, msg
    # and the merged launch forms the sums of the launch of its own
    k.set_wgrad_form(-1)
    alone = _nan(k.part2_floats_wino(B), dev)
    k.conv2_bwd_filter_wino_dp2(ptr(o["a1pf"]), ptr(o["dp2"]), ptr(o["idx2"]), B, ptr(alone),
                                stream_handle())
    torch.cuda.synchronize()
    assert not _diff("merged vs alone", got[-1]["part2"], alone)


def test_engine_steps_older_form_against_default(cuda_dev, forms):
    """30 captured steps at B = 32 with the older form and with the default:
    parameters and momentum equal bit for bit (the mask is set before the
    capture: a graph keeps the kernels it recorded)"""
    x, y = synthetic_rows("train", 0, 1024)
    runs = []
    for mask in (0, -1):
        forms.set_wgrad_form(mask)
        e = NativeMnistEngine(C.TrainConfig(graph=True, batch_size=32).validate(), x, y, cuda_dev)
        if not runs:
            p0 = e.params.clone()
        e.train(30)
        torch.cuda.synchronize()
        runs.append(e)
    old, new = runs
    assert int(new.step_dev.item()) == 30
    assert torch.isfinite(new.params).all() and not torch.equal(old.params, p0)
    assert torch.equal(new.params, old.params)
    assert torch.equal(new.mom, old.mom)
