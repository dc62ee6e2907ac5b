"""The bf16 MNIST step, stage by stage against float64 on its own operands.

After `forward_backward_only()` (or a training step) every intermediate of
the step sits in `engine.bufs`.  Each test reads one stage's inputs from the device exactly as
the kernels left them (bf16 values, argmax bytes, bf16 weight shadows),
computes that stage in float64 on the CPU (tests/helpers/mnist_bf16_ref.py)
and compares the stage's output: the reference sees the kernel's rounded
operands and masks, so what is left is fp32 accumulation order plus one bf16
rounding, and the bound is the derived one (`tol()` there: n 2^-23 S, plus
2^-8 relative for a bf16 output; structural zeros exact), not a tuned one.
tests/test_mnist_bf16_ref_cpu.py shows on the CPU that a dropped K-step, a
missing image, a shifted row, a truncating store, a stale shadow, a transposed
argmax and a misplaced ReLU mask each fail these checks.

Inputs: the project's synthetic rows and init (the CPU test
`test_argmax_caps_on_the_projects_rows_and_init` found the argmax checks well
under their caps on them).  One engine step per case; every test of a case
reads the same CPU snapshot.

MTA_STAGE_REPORT=<path>: the per-stage worst err / tol and the argmax shares
of the run are also written there as JSON (docs/ACCURACY.md holds a run's)."""

import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine
from mpi_tensorflow_amd.utils import rng
from mpi_tensorflow_amd.utils.data import batch_offset, synthetic_rows

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("mnist_bf16_ref",
                                               os.path.join(_HERE, "helpers", "mnist_bf16_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

# case -> (batch, steps trained before the step under test, the step under
# test is a training step).  The first three run forward_backward_only() (the
# shadows re-derived by the conv1 launch, conv2 forward in a launch of its own,
# the gradients finished by the finalize launch); the last reads what the
# fourth step of train(4) left: the fused conv1 + conv2 forward on the shadows
# the SGD wrote, the FC SGD riding in the conv2 backward, and the conv
# gradients still as the slabs (part2, part1) the SGD launch sums.
CASES = {"b32_step0": (32, 0, False), "b32_step3": (32, 3, False), "b50_step2": (50, 2, False),
         "b32_train_step3": (32, 3, True)}
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    rows = {}
    for case, res in REPORT.items():
        for k, e in res.items():
            rows.setdefault(k, {})[case] = e[1] if e[0] != "argmax" else e[3]
    for k, by_case in rows.items():
        print(f"[bf16 stages] {k}: " + ", ".join(f"{c} {v:.3g}" for c, v in by_case.items()))
    path = os.environ.get("MTA_STAGE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(rows, f, indent=1, sort_keys=True)


def _f(t):
    return t.float()


def _engine(cuda_dev, B):
    x, y = synthetic_rows("train", 0, 2048)
    cfg = C.TrainConfig(dtype="bf16", graph=False, batch_size=B).validate()
    return NativeMnistEngine(cfg, x, y, cuda_dev)


@pytest.fixture(scope="module", params=list(CASES))
def snap(request, cuda_dev):
    """One step on the GPU; every buffer, the parameters and the batch rows
    on the CPU in logical form (the snapshot of mnist_bf16_ref.py)."""
    B, k, train_step = CASES[request.param]
    eng = _engine(cuda_dev, B)
    if k:
        eng.train(k)
    torch.cuda.synchronize()
    Bp, step = eng.Bp, eng.step
    assert int(eng.step_dev.item()) == step == k
    pre = {n: eng.bufs[n].detach().cpu().clone() for n in ("w1b", "w1t", "w2tb", "w2b")}
    p = {n: v.detach().cpu().clone() for n, v in eng.param_views().items()}
    if train_step:
        eng.train(1)
    else:
        eng.forward_backward_only()
    torch.cuda.synchronize()
    raw = {n: v.detach().cpu().clone() for n, v in eng.bufs.items()}
    g = {n: v.detach().cpu().clone() for n, v in eng.layout.views(eng.grads).items()}
    p_after = {n: v.detach().cpu().clone() for n, v in eng.param_views().items()}
    if train_step:
        # no finalize launch: the conv gradients are the sums of the slabs
        assert all(not torch.equal(p_after[n], p[n]) for n in p)
        G, rows = Bp // 8, Bp * 196 // 64
        part2, part1 = raw["part2"].double(), raw["part1"][:rows * 832].double().reshape(rows, 832).sum(0)
        g["conv2_weight"] = part2[:G * 51200].reshape(G, 5, 5, 32, 64).sum(0)
        g["conv2_bias"] = part2[G * 51200:G * 51456].reshape(4 * G, 64).sum(0)
        g["conv1_weight"], g["conv1_bias"] = part1[:800].reshape(5, 5, 1, 32), part1[800:]
    else:
        assert all(torch.equal(p_after[n], p[n]) for n in p)  # the step moved no parameter
    off = batch_offset(step, eng.n_local, B)
    assert (off != 0) == (k != 0)
    s = dict(case=request.param, Bp=Bp, lb=B, keep=eng.cfg.dropout_keep, step=step, raw=raw, pre=pre, p=p,
             trained=k, train_step=train_step, p_after=p_after, lr_dev=float(eng.lr_dev.item()),
             lr=eng.lr(step),
             x=eng.train_x[off:off + Bp].cpu().reshape(Bp, 28, 28),
             labels=eng.train_y[off:off + Bp].cpu().to(torch.int64),
             mask=rng.keep_mask_torch(rng.dropout_key(eng.cfg.seed, eng.drop_rank, step, 0), (Bp, 512),
                                      eng.cfg.dropout_keep),
             g=g)
    sh = pre if train_step else raw  # the shadows the step under test read
    s.update(
        w1t=_f(R.unpack_w1t(sh["w1t"])), w1b=_f(R.unpack_w1b(sh["w1b"])),
        w2t=_f(R.unpack_w2t(sh["w2tb"])), w2b=_f(R.unpack_w2b(sh["w2b"])),
        a1=_f(R.interior(R.unpack_a1p(raw["a1p"], Bp))), a1f=_f(R.unpack_a1t(raw["a1t"], Bp)[:, :, :18]),
        idx1=raw["idx1"].reshape(Bp, 14, 14, 32),
        a2=_f(R.unpack_a2p(raw["a2h"], Bp)), a2t=_f(R.unpack_a2t(raw["a2t"], Bp)),
        idx2=raw["idx2"].reshape(Bp, 3136),
        hd=raw["hd"].reshape(Bp, 512), dh=raw["dh"].reshape(Bp, 512), dlog=raw["dlog"].reshape(Bp, 10),
        loss=raw["loss_rows"].reshape(Bp),
        dh16=_f(R.unpack_dh16(raw["dh16"], Bp)), dht=_f(R.unpack_dht(raw["dht16"], Bp)),
        dy2=_f(R.interior(R.unpack_dy2p(raw["dy2p"], Bp))),
        dy2f=_f(R.unpack_dy2t(raw["dy2t"], Bp)[:, :, :14]),
        da1m=raw["da1m"].reshape(Bp, 14, 14, 32))
    del eng
    return s


def _settle(s, res):
    """Prints and records a stage's figures, then asserts its checks."""
    for k, e in res.items():
        print(f"[{s['case']}] {k}: {e}")
    REPORT.setdefault(s["case"], {}).update(res)
    bad = R.failures(res)
    assert not bad, (s["case"], bad)


def _same(a, b):
    return ("bits", int((R.as_bits(a.contiguous()) != R.as_bits(b.contiguous())).sum()))


def _zero(t):
    return ("bits", int((R.as_bits(t.contiguous()) != 0).sum()))


def test_shadows(snap):
    """w1b / w1t / w2tb / w2b = pack(RNE(master weights)) bit for bit: as the
    step's first launch re-derives them and, after train(k), as the fused SGD
    launches of the steps before left them."""
    s = snap

    def packed(p):
        w1 = R.bf16_bits(p["fc1_weight"].reshape(3136, 512))
        w2 = R.bf16_bits(p["conv2_weight"].reshape(25, 32, 64))
        return dict(w1b=R.pack_w1b(w1), w1t=R.pack_w1t(w1), w2tb=R.pack_w2t(w2), w2b=R.pack_w2b(w2))

    want = packed(s["p"])
    # after the step: re-derived by its first launch, or (training step)
    # written by its SGD launches for the parameters it moved
    after = packed(s["p_after"])
    res = {n: _same(s["raw"][n], after[n]) for n in after}
    if s["trained"]:
        res.update({n + " (written by the SGD)": _same(s["pre"][n], want[n]) for n in want})
    res.update({"stage_" + n: e for n, e in R.stage_shadows(s).items()})
    _settle(s, res)


def test_conv1_forward(snap):
    s, Bp = snap, snap["Bp"]
    res = R.stage_conv1(s)
    a1p, a1t = R.unpack_a1p(s["raw"]["a1p"], Bp), R.unpack_a1t(s["raw"]["a1t"], Bp)
    res["a1p border"] = _zero(a1p[:, R.border_mask()])
    res["a1t == a1p"] = _same(a1t[:, :, :18], a1p)
    res["a1t padding"] = _zero(a1t[:, :, 18:])
    _settle(s, res)


def test_conv2_forward(snap):
    s = snap
    res = R.stage_conv2(s)
    res["a2t == a2h"] = _same(R.unpack_a2t(s["raw"]["a2t"], s["Bp"]), R.unpack_a2p(s["raw"]["a2h"], s["Bp"]))
    _settle(s, res)


def test_fc1_forward_and_head(snap):
    s = snap
    res = R.stage_fc1(s)
    res.update(R.stage_head(s))
    _settle(s, res)
    # the schedule's LR at this step (fp32 base rate, powf of a whole epoch count)
    assert abs(s["lr_dev"] - s["lr"]) <= 2.0 ** -21 * s["lr"], (s["lr_dev"], s["lr"])


def test_fc1_backward(snap):
    s, Bp = snap, snap["Bp"]
    res = R.stage_fc1_bwd(s)
    dy2p, dy2t = R.unpack_dy2p(s["raw"]["dy2p"], Bp), R.unpack_dy2t(s["raw"]["dy2t"], Bp)
    res["dy2p border"] = _zero(dy2p[:, R.border_mask()])
    res["dy2t == dy2p"] = _same(dy2t[:, :, :14], R.interior(dy2p))
    res["dy2t columns 14 / 15"] = _zero(dy2t[:, :, 14:])
    _settle(s, res)


def test_conv2_backward_data(snap):
    _settle(snap, R.stage_conv2_bwd_data(snap))


def test_conv2_backward_filter(snap):
    """The finished conv2 gradients and the per-group slabs (8 images each)
    they are summed from."""
    s, Bp = snap, snap["Bp"]
    res = R.stage_conv2_bwd_filter(s)
    G = Bp // 8
    slabs = s["raw"]["part2"][:G * 51200].reshape(G, 25, 32, 64)
    res.update(R.stage_conv2_bwd_filter(s, [(8 * g, 8 * g + 8, slabs[g]) for g in range(G)]))
    _settle(s, res)


def test_conv1_backward_filter(snap):
    _settle(snap, R.stage_conv1_bwd_filter(snap))


def test_pad_rows_are_exactly_zero(snap):
    """Rows B .. Bp - 1 seed nothing (B = 50: rows 50..63); the gradients were
    compared with references over the real rows only in the stage tests."""
    s, lb = snap, snap["lb"]
    res = {}
    for name in ("dlog", "dh", "dh16", "dy2", "da1m", "loss"):
        res[f"{name} pad rows"] = ("bits", int((s[name][lb:] != 0).sum()))
    res["dy2t pad rows"] = ("bits", int((s["dy2f"][lb:] != 0).sum()))
    _settle(s, res)
    if s["case"] == "b50_step2":
        assert s["Bp"] == 64 and s["dlog"][lb:].numel() == 14 * 10


# -------------------------------------------------------------------- eval ----
def _eval_chain(eng, x, lg, M, case):
    """Chain check of the last chunk evaluate() ran (M rows, padded to Mp):
    a1 -> a2 -> h -> logits through the eval workspace."""
    Mp = (M + 7) // 8 * 8
    _, a1w, a2w, hw = eng._eval_ws
    p = {n: v.detach().cpu() for n, v in eng.param_views().items()}
    a1p = R.unpack_a1p(a1w[:2 * Mp * 18 * 18 * 16].cpu(), Mp)
    a1 = _f(R.interior(a1p))[:M]
    a2 = _f(R.unpack_a2p(a2w[:Mp * 3136].cpu(), Mp))[:M]
    h = hw[:M * 512].cpu().reshape(M, 512)
    xs = torch.from_numpy(np.ascontiguousarray(x, np.float32)).reshape(M, 28, 28)
    res = {}
    ref, S, _, _ = R.conv1_pool(xs, p["conv1_weight"], p["conv1_bias"])
    res["eval a1"] = ("tol",) + R.check(a1, ref, S, R.N_CONV1, bf16_out=True)
    res["eval a1 border"] = _zero(a1p[:M][:, R.border_mask()])
    ref, S, _, _ = R.conv2_pool(a1, _f(R.unpack_w2t(eng.bufs["w2tb"].cpu())), p["conv2_bias"])
    res["eval a2"] = ("tol",) + R.check(a2, ref, S, R.N_CONV2, bf16_out=True)
    ref, S = R.fc1_fwd(a2, _f(R.unpack_w1t(eng.bufs["w1t"].cpu())), p["fc1_bias"], None, 1.0)
    res["eval h"] = ("tol",) + R.check(h, ref, S, R.N_FC1)
    hl = R.head_loss(h, p["fc2_weight"], p["fc2_bias"], torch.zeros(M, dtype=torch.int64), M)
    res["eval logits"] = ("tol",) + R.check(lg.cpu(), hl["logits"], hl["S_logits"], R.N_FC2)
    _settle(dict(case=case), res)


def test_eval_chain_and_pad_row_independence(cuda_dev):
    eng = _engine(cuda_dev, 32)
    eng.train(2)
    tx, ty = synthetic_rows("test", 0, 300)
    # 13 rows are padded to 16: the logits must not depend on what the
    # workspace rows 13..15 held before
    _, lg0 = eng.evaluate(tx[:13], ty[:13], chunk=13, return_logits=True)
    torch.cuda.synchronize()
    _, a1w, a2w, _ = eng._eval_ws
    big = 3.0e38  # finite in bf16
    a1w.view(2, 16, 18, 18, 16)[:, 13:, 2:16, 2:16, :] = big  # interiors only: the borders stay zero
    a2w.view(196, 16, 16)[:, 13:, :] = big
    err, lg1 = eng.evaluate(tx[:13], ty[:13], chunk=13, return_logits=True)
    torch.cuda.synchronize()
    assert torch.isfinite(lg1).all()
    assert torch.equal(lg0, lg1)
    assert err == 100.0 * int((lg1.argmax(1).cpu().numpy() != ty[:13]).sum()) / 13
    _eval_chain(eng, tx[:13], lg1, 13, "eval_13")
    # 300 rows in chunks of 128: the last chunk has 44 rows (padded to 48)
    err, lg = eng.evaluate(tx, ty, chunk=128, return_logits=True)
    torch.cuda.synchronize()
    assert lg.shape == (300, 10) and torch.isfinite(lg).all()
    assert err == pytest.approx(100.0 * int((lg.argmax(1).cpu().numpy() != ty).sum()) / 300)
    _eval_chain(eng, tx[256:], lg[256:], 44, "eval_300_last_chunk")
