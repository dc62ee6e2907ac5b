"""The FC chain of the fp32 MNIST step - fc1 forward (feature-major), train
head, fc1 backward dX - kernel by kernel against fp64 references built here,
for the older and the shorter form of each (native().mnist.set_fc_chain), and
the whole step, older forms against shorter ones, on one build."""
import numpy as np
import pytest
import torch

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.models import mnist_cnn as M
from mpi_tensorflow_amd.ops import native, ptr, stream_handle
from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine
from mpi_tensorflow_amd.utils.data import synthetic_rows

pytestmark = pytest.mark.gpu

NCLS = 10
T_LD = 20  # row length of the channel-major dY2 image (common.h MNIST32_T_LD)


def _rel(a, b):
    """max |a - b| relative to the largest reference magnitude"""
    return (a.double().cpu() - b).abs().max().item() / max(1e-30, b.abs().max().item())


@pytest.fixture
def chain(cuda_dev):
    k = native().mnist
    yield k
    k.set_fc_chain(-1)


def _chains(k):
    return (0, -1)


# ------------------------------------------------------------------- head ----
def _head_inputs(batch, ns, seed):
    """Slabs whose sum (+ bias) stays at least 0.05 away from zero, so the fp32
    and the fp64 ReLU gates agree on every unit."""
    g = torch.Generator().manual_seed(seed)
    b3 = torch.randn(M.FC1_OUT, generator=g) * 0.1
    zt = torch.randn(batch, M.FC1_OUT, generator=g, dtype=torch.float64)
    zt = zt + 0.05 * torch.sign(zt)
    part = torch.randn(ns, batch, M.FC1_OUT, generator=g)
    part[ns - 1] = (zt - b3.double() - part[:ns - 1].double().sum(0)).float()
    w4 = torch.randn(M.FC1_OUT, NCLS, generator=g) * 0.1
    b4 = torch.randn(NCLS, generator=g) * 0.1
    return part, b3, w4, b4


@pytest.mark.parametrize("keep", [0.5, 1.0])
@pytest.mark.parametrize("splits", ["feature-major", "staged"])
@pytest.mark.parametrize("lb,batch", [(32, 32), (40, 64)])
def test_head_matches_fp64(cuda_dev, chain, lb, batch, splits, keep):
    """hd, dh, dlog, loss rows and lr against fp64 from the same slabs, labels
    and dropout mask (the kernel's own hd != 0 at keep < 1) within 1e-5 of the
    largest reference magnitude; `correct` exact; pad rows (>= lb): dlogits
    and dh exactly +0, loss 0; the bf16 operand copies of dh (the bf16
    engine's slab count) are dh rounded; the shorter kernel's outputs equal the
    older kernel's bit for bit.  The step runs on both sides of an epoch
    boundary and above 2^31 / B (64-bit step * B)."""
    k = chain
    ns = k.fc1_train_t_splits() if splits == "feature-major" else k.fc1_train_splits()
    n_local, base_lr = 1000, 0.01
    part, b3, w4, b4 = _head_inputs(batch, ns, 7 * batch + ns)
    g = torch.Generator().manual_seed(3)
    labels = torch.randint(0, NCLS, (n_local,), generator=g, dtype=torch.int32)
    dev = cuda_dev
    d_part, d_b3, d_w4, d_b4, d_lab = (t.to(dev) for t in (part, b3, w4, b4, labels))
    z = part.double().sum(0) + b3.double()
    h = z.clamp_min(0)
    s_lo = (n_local - 1) // lb
    steps = [(s_lo, 0.95), (s_lo + 1, 0.95), (2 ** 31 // lb + 5, float(np.float32(0.999999)))]
    bf16 = splits == "staged"
    older = {}  # step -> the older kernel's outputs: the shorter form must give the same bits
    for mask in _chains(k):
        k.set_fc_chain(mask)
        for step, decay in steps:
            d_step = torch.tensor([step], dtype=torch.int64, device=dev)
            hd = torch.full((batch, M.FC1_OUT), float("nan"), device=dev)
            dh = torch.full_like(hd, float("nan"))
            dlog = torch.full((batch, NCLS), float("nan"), device=dev)
            loss = torch.full((batch,), float("nan"), device=dev)
            lr = torch.full((1,), float("nan"), device=dev)
            correct = torch.zeros(1, dtype=torch.int32, device=dev)
            dh16 = torch.zeros(M.FC1_OUT // 16, batch, 16, dtype=torch.bfloat16, device=dev)
            dht16 = torch.zeros(batch // 16, M.FC1_OUT, 16, dtype=torch.bfloat16, device=dev)
            k.fc_head_train_full(ptr(d_part), ptr(d_b3), ptr(d_w4), ptr(d_b4), ptr(d_lab), n_local,
                                 ptr(d_step), batch, keep, 11, 0, base_lr, decay, ptr(hd), ptr(dh),
                                 ptr(dlog), ptr(loss), ptr(lr), ptr(correct), stream_handle(),
                                 ptr(dh16) if bf16 else 0, ptr(dht16) if bf16 else 0, ns,
                                 lb if lb != batch else 0)
            torch.cuda.synchronize()
            tag = (mask, step)
            off = (step * lb) % (n_local - lb)
            lab = labels[off:off + batch].long()
            valid = (torch.arange(batch) < lb)
            kp = (hd.cpu() != 0) if keep < 1 else torch.ones(batch, M.FC1_OUT, dtype=torch.bool)
            if keep < 1:  # about half of the active units kept
                frac = kp[h > 0].double().mean().item()
                assert 0.4 < frac < 0.6, (tag, frac)
            hd_ref = torch.where(kp, h / keep, torch.zeros_like(h))
            logits = hd_ref @ w4.double() + b4.double()
            p = torch.softmax(logits, 1)
            onehot = torch.nn.functional.one_hot(lab, NCLS).double()
            dlog_ref = (p - onehot) / lb * valid[:, None]
            gate = kp & (z > 0)
            dh_ref = (dlog_ref @ w4.double().t()) * gate / keep
            loss_ref = (torch.logsumexp(logits, 1) - logits.gather(1, lab[:, None])[:, 0]) * valid
            lr_ref = base_lr * float(np.float32(decay)) ** ((step * lb) // n_local)
            corr_ref = int(((logits.argmax(1) == lab) & valid).sum())
            errs = {"hd": _rel(hd, hd_ref), "dh": _rel(dh, dh_ref), "dlog": _rel(dlog, dlog_ref),
                    "loss": _rel(loss, loss_ref),
                    "lr": abs(lr.item() - lr_ref) / lr_ref}
            print(tag, {n: f"{v:.1e}" for n, v in errs.items()}, int(correct.item()), corr_ref)
            assert max(errs.values()) < 1e-5, (tag, errs)
            assert int(correct.item()) == corr_ref, tag
            if lb < batch:
                pad = slice(lb, batch)
                zero = torch.zeros(1, device=dev)
                for name, t in (("dlog", dlog[pad]), ("dh", dh[pad]), ("loss", loss[pad])):
                    assert torch.equal(t, zero.expand_as(t)), (tag, name)
                assert not torch.signbit(dh[pad]).any(), tag  # d == +0.f
            got = (hd, dh, dlog, loss, lr, correct)
            if mask == 0:
                older[step] = got
            else:
                for name, a, b in zip(("hd", "dh", "dlog", "loss", "lr", "correct"), got,
                                      older[step]):
                    assert torch.equal(a, b), (tag, name)
            if bf16:
                want = dh.to(torch.bfloat16)
                assert torch.equal(dh16.permute(1, 0, 2).reshape(batch, M.FC1_OUT), want), tag
                assert torch.equal(dht16.permute(0, 2, 1).reshape(batch, M.FC1_OUT), want), tag


# ---------------------------------------------------------- fc1 backward dX ----
@pytest.fixture(scope="module")
def dx_case():
    """One set of operands and fp64 references per batch, shared by the tests."""
    out = {}
    for batch in (32, 64):
        g = torch.Generator().manual_seed(100 + batch)
        dh = torch.randn(batch, M.FC1_OUT, generator=g)
        dh = dh * (torch.rand(batch, M.FC1_OUT, generator=g) < 0.5)
        w1 = torch.randn(M.FC1_IN, M.FC1_OUT, generator=g) * 0.05
        a2 = torch.randn(batch, M.FC1_IN, generator=g).clamp_min(0)  # about half ReLU-inactive
        idx2 = torch.randint(0, 4, (batch, M.FC1_IN), generator=g, dtype=torch.uint8)
        gref = dh.double() @ w1.double().t()
        gref = gref * (a2 > 0)
        out[batch] = (dh, w1, a2, idx2, gref)
    return out


def _run_dx(k, dev, case, batch, dense):
    dh, w1, a2, idx2, _ = case
    d = [t.to(dev) for t in (a2, idx2, dh, w1)]
    dummy = torch.zeros(16, device=dev)  # roles == 1: the weight-gradient operands are not read
    s = stream_handle()
    if dense:
        dy2 = torch.full((batch, 14, 14, 64), float("nan"), device=dev)
        dy2t = torch.full((batch, 64, 18, T_LD), -7.0, device=dev)
        k.fc1_bwd(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(dummy), ptr(dummy), ptr(d[3]), batch,
                  ptr(dummy), ptr(dummy), ptr(dummy), ptr(dummy), ptr(dy2), ptr(dy2t), s, 1)
        torch.cuda.synchronize()
        return dy2, dy2t
    dp2 = torch.full((batch, M.FC1_IN), float("nan"), device=dev)
    k.fc1_bwd_dp2(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(dummy), ptr(dummy), ptr(d[3]), batch,
                  ptr(dummy), ptr(dummy), ptr(dummy), ptr(dummy), ptr(dp2), s, 1)
    torch.cuda.synchronize()
    return dp2


@pytest.mark.parametrize("batch", [32, 64])
def test_fc1_bwd_dx_compact_matches_fp64(cuda_dev, chain, dx_case, batch):
    """dp2 = (dh W1^T) masked by a2 > 0 at a2's flat index."""
    gref = dx_case[batch][4]
    for mask in _chains(chain):
        chain.set_fc_chain(mask)
        dp2 = _run_dx(chain, cuda_dev, dx_case[batch], batch, dense=False)
        err = _rel(dp2, gref)
        print(mask, f"{err:.1e}")
        assert err < 1e-5, (mask, err)
        assert (dp2.cpu()[dx_case[batch][2] <= 0] == 0).all(), mask  # ReLU-inactive: exact zeros


@pytest.mark.parametrize("batch", [32, 64])
def test_fc1_bwd_dx_dense_matches_fp64(cuda_dev, chain, dx_case, batch):
    """dy2 (NHWC) / dy2t (channel-major, zero-bordered): the pooled gradient
    at its argmax position, exact zeros at the three others and everywhere a
    ReLU-inactive unit; dy2t's border keeps its sentinel."""
    _, _, a2, idx2, gref = dx_case[batch]
    gq = gref.view(batch, 7, 7, 64)
    q = idx2.view(batch, 7, 7, 64).long()
    ref = torch.zeros(batch, 14, 14, 64, dtype=torch.float64)
    for dy in range(2):
        for dx in range(2):
            ref[:, dy::2, dx::2, :] = gq * (q == 2 * dy + dx)
    for mask in _chains(chain):
        chain.set_fc_chain(mask)
        dy2, dy2t = _run_dx(chain, cuda_dev, dx_case[batch], batch, dense=True)
        err = _rel(dy2, ref)
        print(mask, f"{err:.1e}")
        assert err < 1e-5, (mask, err)
        assert (dy2.cpu()[ref == 0] == 0).all(), mask  # inactive / non-argmax: exact zeros
        t = dy2t.cpu()
        inner = t[:, :, 2:16, 2:16]
        assert torch.equal(inner, dy2.cpu().permute(0, 3, 1, 2)), mask
        border = torch.ones(18, T_LD, dtype=torch.bool)
        border[2:16, 2:16] = False
        assert (t[:, :, border] == -7.0).all(), mask


# ------------------------------------------------------------ fc1 forward ----
@pytest.mark.parametrize("batch", [32, 64])
def test_fc1_forward_slabs_match_fp64(cuda_dev, chain, batch):
    k = chain
    g = torch.Generator().manual_seed(50 + batch)
    a2 = torch.relu(torch.randn(batch, M.FC1_IN, generator=g)) * torch.rand(M.FC1_IN, generator=g)
    w = torch.randn(M.FC1_IN, M.FC1_OUT, generator=g) * 0.05 + 0.01
    a2t, wd = a2.t().contiguous().to(cuda_dev), w.to(cuda_dev)
    ref = a2.double() @ w.double()
    ns = k.fc1_train_t_splits()
    masks = (0, k.FC_CHAIN_FWD, k.FC_CHAIN_FWD_LOADS, k.FC_CHAIN_FWD | k.FC_CHAIN_FWD_LOADS, -1)
    for mask in masks:
        k.set_fc_chain(mask)
        part = torch.full((k.fc1_part_floats(batch),), float("nan"), device=cuda_dev)
        k.fc1_fwd_train_t(ptr(a2t), ptr(wd), batch, ptr(part), stream_handle())
        torch.cuda.synchronize()
        got = part[:ns * batch * M.FC1_OUT].view(ns, batch, M.FC1_OUT).double().sum(0)
        err = _rel(got, ref)
        print(mask, f"{err:.1e}")
        assert torch.isfinite(got).all() and err < 1e-5, (mask, err)


# -------------------------------------------------------------- whole step ----
def test_whole_step_older_forms_against_shorter(cuda_dev, chain):
    """30 captured steps at B = 64, single rank, older forms against the
    shorter ones on one build.  The shorter forms keep every sum's association
    and every quotient's form, so parameters and momentum must be equal bit for
    bit (which is inside the per-step gradient tolerance 2e-4 of the update,
    the measure of test_training_trajectory_matches_oracle, asserted too)."""
    x, y = synthetic_rows("train", 0, 1024)
    runs = []
    for mask in (0, -1):
        chain.set_fc_chain(mask)  # before the capture: a graph keeps what it recorded
        e = NativeMnistEngine(C.TrainConfig(batch_size=64, graph=True, graph_steps=5).validate(),
                              x, y, cuda_dev)
        if not runs:
            p0 = e.params.clone()
        e.train(30)
        torch.cuda.synchronize()
        runs.append(e)
    old, new = runs
    assert int(new.step_dev.item()) == 30
    d = (new.params - old.params).double().norm().item()
    upd = (old.params - p0).double().norm().item()
    print(f"whole step: |new - old| / |update| = {d / upd:.3e}")
    assert torch.isfinite(new.params).all()
    assert d / upd < 2e-4, d / upd
    assert torch.equal(new.params, old.params) and torch.equal(new.mom, old.mom)
    assert abs(new.device_lr() - old.device_lr()) <= 1e-5 * old.device_lr()
