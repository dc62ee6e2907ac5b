"""The two launch tails of the fp32 Winograd MNIST step (csrc/kernels/mnist.hip):

* the conv1 filter-gradient epilogue of the conv2 bwd-data block
  (bwd_data_wino_block): every part1 row (image n, band pg of four a1 rows)
  against a float64 correlation of the zero-padded input with the pre-pool
  gradient scattered from the kernel's own da1m through idx1;
* the conv roles of the SGD launch (sgd_finalize_kernel): the slab form
  against grad_finalize + the flat form and the flat optimizer, bit for bit,
  and U / Ud against a fresh transform of the updated weights."""
import pytest
import torch

from mpi_tensorflow_amd.ops import native, ptr, stream_handle
from mpi_tensorflow_amd.utils.data import batch_offset, synthetic_rows

pytestmark = pytest.mark.gpu

B = 3
N_LOCAL = 64
STEP = 5


def _rel(a, b):
    return (a - b).abs().max().item() / max(1e-6, b.abs().max().item())


def _expand(dp2, idx2):
    dy2 = torch.zeros(dp2.shape[0], 14, 14, 64, dtype=dp2.dtype, device=dp2.device)
    zero = torch.zeros((), dtype=dp2.dtype, device=dp2.device)
    for k in range(4):
        dy2[:, k >> 1::2, k & 1::2, :] = torch.where(idx2 == k, dp2, zero)
    return dy2


@pytest.fixture(scope="module")
def operands(cuda_dev):
    """conv2 bwd-data operands at B = 3 (12 blocks), built as
    test_mnist_compact_bwd_gpu.py builds them; shared and left unchanged"""
    g = torch.Generator().manual_seed(2024)
    idx2 = torch.randint(0, 4, (B, 7, 7, 64), generator=g).to(torch.uint8)
    dp2 = torch.randn(B, 7, 7, 64, generator=g)
    dp2 = torch.where(torch.rand(B, 7, 7, 64, generator=g) < 0.5, torch.zeros(()), dp2)
    a1 = torch.relu(torch.randn(B, 14, 14, 32, generator=g))
    a1pf = torch.zeros(B, 18, 18, 32)
    a1pf[:, 2:16, 2:16] = a1
    idx1 = torch.randint(0, 4, (B, 14, 14, 32), generator=g).to(torch.uint8)
    for k in range(4):
        assert (idx1 == k).any() and (idx2 == k).any()
    assert (a1 == 0).any() and (a1 > 0).any()
    w2 = torch.randn(5, 5, 32, 64, generator=g) * 0.05
    x, _ = synthetic_rows("train", 0, N_LOCAL)
    off = batch_offset(STEP, N_LOCAL, B)
    assert off > 0
    o = dict(dp2=dp2, idx2=idx2, a1=a1, a1pf=a1pf, idx1=idx1, w2=w2, x=torch.from_numpy(x),
             step=torch.tensor([STEP], dtype=torch.int64))
    o = {k: v.to(cuda_dev) for k, v in o.items()}
    o["dy2"] = _expand(o["dp2"], o["idx2"])
    o["Ud"] = torch.empty(36 * 64 * 32, device=cuda_dev)
    U = torch.empty(36 * 32 * 64, device=cuda_dev)
    native().mnist.conv2_wino_weights(ptr(o["w2"]), ptr(U), ptr(o["Ud"]), stream_handle())
    torch.cuda.synchronize()
    o["off"] = off
    return o


def _run(o, compact, lean):
    """the standalone data kernel with the conv1 epilogue; lean: a1 = da1m =
    nullptr (mask from a1pf, dA1 not stored).  Returns (part1 [B * 4][832],
    da1m or None)."""
    dev = o["dp2"].device
    part1 = torch.full((B * 4, 832), float("nan"), device=dev)
    da1m = None if lean else torch.full((B, 14, 14, 32), float("nan"), device=dev)
    native().mnist.conv2_bwd_data_wino_c1(
        0 if compact else ptr(o["dy2"]), ptr(o["dp2"]) if compact else 0,
        ptr(o["idx2"]) if compact else 0, ptr(o["Ud"]), 0 if lean else ptr(o["a1"]),
        ptr(o["a1pf"]), B, 0 if lean else ptr(da1m), ptr(o["x"]), ptr(o["step"]), N_LOCAL,
        ptr(o["idx1"]), ptr(part1), stream_handle())
    torch.cuda.synchronize()
    return part1, da1m


@pytest.fixture(scope="module")
def reference(operands):
    """float64 part1 rows on the host from the kernel's own da1m (dense input,
    a1 and da1m given): [B][4][832], computed once"""
    o = operands
    _, da1m = _run(o, compact=False, lean=False)
    assert torch.isfinite(da1m).all()
    a1 = o["a1"].cpu()
    da1m = da1m.cpu()
    assert float(da1m[a1 <= 0].abs().sum()) == 0.0 and (a1 <= 0).any()  # masked entries
    assert (da1m != 0).any()
    idx1 = o["idx1"].cpu()
    dz = torch.zeros(B, 28, 28, 32, dtype=torch.float64)  # pre-pool gradient
    for k in range(4):
        dz[:, k >> 1::2, k & 1::2, :] = torch.where(idx1 == k, da1m.double(),
                                                    torch.zeros((), dtype=torch.float64))
    x = o["x"].cpu().double()[o["off"]:o["off"] + B].view(B, 28, 28)
    xp = torch.zeros(B, 32, 32, dtype=torch.float64)
    xp[:, 2:30, 2:30] = x
    win = xp.unfold(1, 5, 1).unfold(2, 5, 1).reshape(B, 28, 28, 25)  # [n][y][x][kh * 5 + kw]
    ref = torch.zeros(B, 4, 832, dtype=torch.float64)
    for pg in range(4):
        r0, r1 = 8 * pg, min(8 * pg + 8, 28)  # pre-pool rows of a1 rows 4 pg .. 4 pg + 3
        ref[:, pg, :800] = torch.einsum("nyxt,nyxc->ntc", win[:, r0:r1], dz[:, r0:r1]).reshape(B, 800)
        ref[:, pg, 800:] = dz[:, r0:r1].sum((1, 2))
    return ref


@pytest.mark.parametrize("compact,lean", [(False, False), (True, False), (False, True), (True, True)])
def test_part1_rows_match_float64(operands, reference, compact, lean):
    """every one of the B x 4 part1 rows on its own at the fp32 kernel
    tolerance 1e-5 (the sum over rows would hide a wrong band edge); the top
    border block pg = 0 and the two-row block pg = 3 are named checks"""
    part1, _ = _run(operands, compact, lean)
    assert torch.isfinite(part1).all()
    got = part1.cpu().double().view(B, 4, 832)
    err = {(n, pg): _rel(got[n, pg], reference[n, pg]) for n in range(B) for pg in range(4)}
    print("part1 row errors:", {k: f"{v:.2e}" for k, v in err.items()})
    for n in range(B):
        assert reference[n, 0].abs().max() > 0 and reference[n, 3].abs().max() > 0
        assert err[(n, 0)] <= 1e-5, f"top band of image {n}: {err[(n, 0)]:.3e}"
        assert err[(n, 3)] <= 1e-5, f"two-row band of image {n}: {err[(n, 3)]:.3e}"
    for key, e in err.items():
        assert e <= 1e-5, f"part1 row (n, pg) = {key}: {e:.3e}"


# ------------------------------------------------------------- SGD roles ----

SB = 4  # two image groups


@pytest.mark.parametrize("shift", [0, 2])
def test_sgd_conv_roles_slab_equals_flat(cuda_dev, shift):
    """one sgd_step of the conv parameters in slab mode at B = 4 vs the same
    update from grad_finalize + (a) the launch's flat form, (b) the flat
    optimizer: weights, biases and momenta torch.equal; U / Ud torch.equal to
    conv2_wino_weights of the updated weights.  shift = 2: the conv1 weights
    and biases off a 16-byte boundary (the role's scalar loads)."""
    Cn = native()
    k = Cn.mnist
    s = stream_handle()
    g = torch.Generator().manual_seed(99 + shift)
    off_w2 = 8
    off_b2 = off_w2 + 51200
    off_w1 = off_b2 + 64 + shift
    off_b1 = off_w1 + 800
    total = off_b1 + 32 + 2
    groups = k.conv2_wino_filter_groups(SB)
    assert groups == 2
    nblk1 = k.conv1_filter_blocks(SB, 4)
    part2 = torch.randn(k.part2_floats_wino(SB), generator=g).to(cuda_dev)
    part1 = torch.randn(nblk1 * 832, generator=g).to(cuda_dev)
    w0 = (torch.randn(total, generator=g) * 0.1).to(cuda_dev)
    m0 = (torch.randn(total, generator=g) * 0.01).to(cuda_dev)
    lr = torch.tensor([0.05], device=cuda_dev)
    mu, gs = 0.9, 1.0

    def state():
        return dict(w=w0.clone(), m=m0.clone(), U=torch.full((36 * 32 * 64,), float("nan"), device=cuda_dev),
                    Ud=torch.full((36 * 64 * 32,), float("nan"), device=cuda_dev))

    def step(st, grads, slabs):
        k.sgd_step_conv(ptr(st["w"]), ptr(grads) if grads is not None else 0, ptr(st["m"]), off_w2,
                        off_b2, off_w1, off_b1, mu, gs, ptr(lr), ptr(part2) if slabs else 0, groups,
                        ptr(part1) if slabs else 0, nblk1, ptr(st["U"]), ptr(st["Ud"]), s)

    slab = state()
    step(slab, None, True)
    # the flat gradient of the same slabs (finalize needs aligned outputs)
    gw2 = torch.empty(51200, device=cuda_dev)
    gb2 = torch.empty(64, device=cuda_dev)
    gw1 = torch.empty(800, device=cuda_dev)
    gb1 = torch.empty(32, device=cuda_dev)
    k.grad_finalize(ptr(part2), groups, ptr(part1), nblk1, ptr(gw2), ptr(gb2), ptr(gw1), ptr(gb1), s)
    grads = torch.zeros(total, device=cuda_dev)
    grads[off_w2:off_w2 + 51200] = gw2
    grads[off_b2:off_b2 + 64] = gb2
    grads[off_w1:off_w1 + 800] = gw1
    grads[off_b1:off_b1 + 32] = gb1
    flat = state()
    step(flat, grads, False)
    segs = dict(w2=(off_w2, 51200), b2=(off_b2, 64), w1=(off_w1, 800), b1=(off_b1, 32))
    opt = {}  # the flat optimizer on aligned copies of each segment (float4 kernel)
    for name, (lo, n) in segs.items():
        ws, ms, gg = (t[lo:lo + n].clone() for t in (w0, m0, grads))
        Cn.optim.sgd_momentum(ptr(ws), ptr(gg), ptr(ms), n, 0, 0.0, mu, gs, ptr(lr), 0.0, 0, s)
        opt[name] = (ws, ms)
    torch.cuda.synchronize()
    assert torch.isfinite(slab["w"]).all() and torch.isfinite(slab["m"]).all()
    for name, (lo, n) in segs.items():
        assert not torch.equal(slab["w"][lo:lo + n], w0[lo:lo + n]), f"{name} was not updated"
        assert torch.equal(slab["w"][lo:lo + n], opt[name][0]), f"{name} vs the flat optimizer"
        assert torch.equal(slab["m"][lo:lo + n], opt[name][1]), f"{name} momentum vs the flat optimizer"
    assert torch.equal(slab["w"], flat["w"]), "parameters vs the flat launch"
    assert torch.equal(slab["m"], flat["m"]), "momenta vs the flat launch"
    # nothing outside the four segments moved
    keep = torch.ones(total, dtype=torch.bool, device=cuda_dev)
    for lo, n in segs.values():
        keep[lo:lo + n] = False
    assert torch.equal(slab["w"][keep], w0[keep]) and torch.equal(slab["m"][keep], m0[keep])
    U = torch.empty(36 * 32 * 64, device=cuda_dev)
    Ud = torch.empty(36 * 64 * 32, device=cuda_dev)
    w2 = slab["w"][off_w2:off_w2 + 51200].clone()
    k.conv2_wino_weights(ptr(w2), ptr(U), ptr(Ud), s)
    torch.cuda.synchronize()
    for st in (slab, flat):
        assert torch.equal(st["U"], U) and torch.equal(st["Ud"], Ud)
