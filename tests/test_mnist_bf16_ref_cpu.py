"""The fp64 stage checker of the bf16 MNIST step (tests/helpers/mnist_bf16_ref.py)
checked without a GPU: the layout codecs against index loops written from the
table in csrc/kernels/mnist_bf16.h, the integer RNE against torch's cast, and
the derived bounds against a torch emulation of every stage (fp32 arithmetic
on bf16-rounded operands, bf16-rounded outputs): the emulation passes every
stage check, and each of a set of subtly wrong emulations fails the check of
its stage at the shapes tests/test_mnist_bf16_stages_gpu.py uses."""

import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mpi_tensorflow_amd import config as C
from mpi_tensorflow_amd.models import mnist_cnn as M
from mpi_tensorflow_amd.utils import rng
from mpi_tensorflow_amd.utils.data import synthetic_rows

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, "helpers", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("mnist_bf16_ref")
F32 = torch.float32


# ------------------------------------------------------------------ codecs ----
# (name, unpack, pack, logical shape for B, flat index of logical index tuple)
# The index functions restate the header's table: [K/16][rows][16] K-packing.
def _codecs(B):
    def a1p(n, Y, X, ci):  # [2][B][18][18][16], ci = 16 s + c
        return ((((ci // 16) * B + n) * 18 + Y) * 18 + X) * 16 + ci % 16

    def a1t(n, Y, X, ci):  # [B][18][32][24] = [n][Y][ci][X]
        return ((n * 18 + Y) * 32 + ci) * 24 + X

    def a2p(n, i):  # [196][B][16], i = 16 k + c
        return ((i // 16) * B + n) * 16 + i % 16

    def a2t(n, i):  # [B/16][3136][16]
        return ((n // 16) * 3136 + i) * 16 + n % 16

    def dh16(n, j):  # [32][B][16], j = 16 k + c
        return ((j // 16) * B + n) * 16 + j % 16

    def dht(n, j):  # [B/16][512][16]
        return ((n // 16) * 512 + j) * 16 + n % 16

    def dy2p(n, Y, X, co):  # [4][B][18][18][16], co = 16 k + c
        return ((((co // 16) * B + n) * 18 + Y) * 18 + X) * 16 + co % 16

    def dy2t(n, y, x, co):  # [B][14][64][16] = [n][y][co][x]
        return ((n * 14 + y) * 64 + co) * 16 + x

    def w2t(t, ci, co):  # [25][2][64][16]: B[k = ci][n = co] per tap
        return ((t * 2 + ci // 16) * 64 + co) * 16 + ci % 16

    def w2b(t, ci, co):  # [25][4][32][16]: B[k = co][n = ci] per tap
        return ((t * 4 + co // 16) * 32 + ci) * 16 + co % 16

    def w1t(i, j):  # [196][512][16]: B[k = i][n = j]
        return ((i // 16) * 512 + j) * 16 + i % 16

    def w1b(i, j):  # [32][3136][16]: B[k = j][n = i]
        return ((j // 16) * 3136 + i) * 16 + j % 16

    ub = lambda f: (lambda buf: f(buf, B))  # noqa: E731
    return [
        ("a1p", ub(R.unpack_a1p), R.pack_a1p, (B, 18, 18, 32), a1p),
        ("a1t", ub(R.unpack_a1t), R.pack_a1t, (B, 18, 24, 32), a1t),
        ("a2p", ub(R.unpack_a2p), R.pack_a2p, (B, 3136), a2p),
        ("a2t", ub(R.unpack_a2t), R.pack_a2t, (B, 3136), a2t),
        ("dh16", ub(R.unpack_dh16), R.pack_dh16, (B, 512), dh16),
        ("dht", ub(R.unpack_dht), R.pack_dht, (B, 512), dht),
        ("dy2p", ub(R.unpack_dy2p), R.pack_dy2p, (B, 18, 18, 64), dy2p),
        ("dy2t", ub(R.unpack_dy2t), R.pack_dy2t, (B, 14, 16, 64), dy2t),
        ("w2t", R.unpack_w2t, R.pack_w2t, (25, 32, 64), w2t),
        ("w2b", R.unpack_w2b, R.pack_w2b, (25, 32, 64), w2b),
        ("w1t", R.unpack_w1t, R.pack_w1t, (3136, 512), w1t),
        ("w1b", R.unpack_w1b, R.pack_w1b, (3136, 512), w1b),
    ]


@pytest.mark.parametrize("name", [c[0] for c in _codecs(16)])
def test_codec_round_trip_and_index_loop(name):
    B = 16  # the smallest batch a2t / dht exist at
    _, unpack, pack, shape, index = next(c for c in _codecs(B) if c[0] == name)
    n = int(np.prod(shape))
    flat = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(torch.int32)
    x = unpack(flat)
    assert tuple(x.shape) == shape
    assert torch.equal(pack(x), flat)                                # pack(unpack(buf)) == buf
    y = torch.arange(n, dtype=torch.int32).reshape(shape)
    assert torch.equal(unpack(pack(y)).reshape(shape), y)            # unpack(pack(x)) == x
    # index by index, from the header table: every element of the small
    # buffers, the corners and 20,000 seeded elements of the large ones
    if n <= 60000:
        picks = range(n)
    else:
        r = np.random.RandomState(2)
        picks = list(r.randint(0, n, 20000)) + [0, n - 1]
    xl, fl = x.reshape(-1).tolist(), flat.tolist()
    seen = set()
    for e in picks:
        li = np.unravel_index(int(e), shape)
        f = index(*[int(v) for v in li])
        assert 0 <= f < n
        assert xl[int(e)] == fl[f], (name, li)
        seen.add(f)
    if n <= 60000:
        assert len(seen) == n  # the table's formula is a bijection


# --------------------------------------------------------------------- RNE ----
def test_bf16_rne_equals_torch_cast():
    g = torch.Generator().manual_seed(3)
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (1_000_000,), generator=g, dtype=torch.int64).to(torch.int32)
    x = bits.view(torch.float32)
    x = x[~torch.isnan(x)]  # every exponent, subnormals and infinities among them
    scaled = torch.randn(200_000, generator=g) * 0.1
    special = torch.tensor([0.0, -0.0, 1.0, -1.0, float("inf"), -float("inf"), 3.3895314e38, -3.3895314e38,
                            1e-45, -1e-45, 1.1754942e-38, 9.1835e-41, 5.8774718e-39])
    # exact ties (low half = 0x8000) on even and odd upper halves, and their neighbours
    hi = torch.randint(0, 0x7F7F, (4096,), generator=g, dtype=torch.int64)
    ties = []
    for low in (0x8000, 0x7FFF, 0x8001):
        for sign in (0, 1 << 31):
            v = ((hi << 16) | low | sign).numpy().astype(np.uint32)
            ties.append(torch.from_numpy(v.view(np.float32).copy()))
    for t in [x, scaled, special] + ties:
        want = t.bfloat16()
        assert torch.equal(R.bf16_bits(t), want.view(torch.int16)), "bit patterns"
        assert torch.equal(R.bf16_rne(t).view(torch.int32), want.float().view(torch.int32))
    assert torch.isnan(R.bf16_rne(torch.tensor([float("nan")]))).all()
    # truncation is what RNE is not
    assert not torch.equal(R.bf16_trunc(scaled), R.bf16_rne(scaled))


# --------------------------------------------------------------- emulation ----
def _inputs(kind, Bp, seed=0):
    """x [Bp, 28, 28], labels [Bp] and a flat parameter vector.  synthetic:
    the project's rows and init; random: uniform images in [-0.5, 0.5] and
    seeded normal parameters."""
    lay = M.layout()
    flat = torch.zeros(lay.total)
    g = torch.Generator().manual_seed(100 + seed)
    if kind == "synthetic":
        x, y = synthetic_rows("train", 0, Bp)
        x, y = torch.from_numpy(np.ascontiguousarray(x, np.float32)).reshape(Bp, 28, 28), torch.from_numpy(
            np.asarray(y).astype(np.int64))
        M.init_params(flat, lay, seed=C.SEED)
    else:
        x = torch.rand(Bp, 28, 28, generator=g) - 0.5
        y = torch.randint(0, 10, (Bp,), generator=g)
        v = lay.views(flat)
        for s in lay.specs:
            std = 0.2 if s.name == "conv1_weight" else 0.05 if s.name.endswith("weight") else 0.1
            v[s.name].copy_(torch.randn(s.shape, generator=g) * std)
    return x, y, flat


def _transpose_q(q):
    return (q & 1) * 2 + (q >> 1)


def emulate(x, labels, flat, lb, mut="", shadow_flat=None, step=0):
    """One bf16 step in torch: fp32 arithmetic on bf16-rounded operands,
    bf16-rounded outputs, the kernels' stage boundaries.  mut: one defect."""
    lay = M.layout()
    p = {k: v.clone() for k, v in lay.views(flat).items()}
    ps = p if shadow_flat is None else lay.views(shadow_flat)
    Bp, keep = x.shape[0], C.DROPOUT_KEEP
    rnd = lambda name: R.bf16_trunc if mut == "trunc_" + name else R.bf16_rne  # noqa: E731
    mask = rng.keep_mask_torch(rng.dropout_key(C.SEED, 0, step, 0), (Bp, 512), keep)
    w1s = R.bf16_rne(ps["fc1_weight"].reshape(3136, 512))
    w2s = R.bf16_rne(ps["conv2_weight"].reshape(25, 32, 64))
    s = dict(Bp=Bp, lb=lb, keep=keep, x=x, labels=labels, mask=mask, p=p, w1t=w1s, w1b=w1s, w2t=w2s,
             w2b=w2s)
    # conv1 (fp32 operands)
    ref, _, zq, _ = R.conv1_pool(x, p["conv1_weight"], p["conv1_bias"], dt=F32)
    s["a1"] = rnd("a1")(ref)
    q1 = zq.argmax(-1)
    s["idx1"] = _transpose_q(q1) if mut == "idx_transposed" else q1
    # conv2
    w = w2s.clone()
    if mut == "conv2_kstep":
        w[7, 16:32, :] = 0  # one 16-channel half of one tap
    ref, _, zq, _ = R.conv2_pool(s["a1"], w, p["conv2_bias"], dt=F32)
    s["a2"] = s["a2t"] = rnd("a2")(ref)
    q2 = zq.argmax(-1)
    s["idx2"] = _transpose_q(q2) if mut == "idx_transposed" else q2
    # fc1 + head
    a2 = s["a2"].clone()
    if mut == "fc1_kstep":
        a2[:, 160:176] = 0  # one K-step of 16 of 196
    s["hd"], _ = R.fc1_fwd(a2, w1s, p["fc1_bias"], mask, keep, dt=F32)
    h = R.head_loss(s["hd"], p["fc2_weight"], p["fc2_bias"], labels, lb, dt=F32)
    s["dlog"], s["loss"] = h["dlog"], h["loss"]
    s["dh"], _ = R.head_dh(s["dlog"], p["fc2_weight"], s["hd"], keep, dt=F32)
    s["dh16"] = s["dht"] = rnd("dh16")(s["dh"])
    # fc1 backward
    d16, dht = s["dh16"].clone(), s["dht"].clone()
    if mut == "dx_kstep":
        d16[:, 32:48] = 0
    if mut == "dw1_image":
        dht[5] = 0
    iq = _transpose_q(s["idx2"]) if mut == "scatter_transposed" else s["idx2"]
    r = R.fc1_bwd(d16, w1s, iq, s["a2"], s["a2t"], dht, s["hd"], s["dh"], s["dlog"], dt=F32)
    s["dy2"] = s["dy2f"] = rnd("dy2")(r["dy2"])
    g = dict(fc1_weight=r["dW1"], fc1_bias=r["db3"], fc2_weight=r["dW4"], fc2_bias=r["db4"])
    # conv2 backward
    w = w2s.clone()
    if mut == "bwd_data_kstep":
        w[12, :, 16:32] = 0  # one 16-channel chunk of one tap
    a1m = torch.ones_like(s["a1"]) if mut == "da1_unmasked" else s["a1"]
    s["da1m"], _, _ = R.conv2_bwd_data(s["dy2"], w, a1m, dt=F32)
    s["a1f"] = F.pad(s["a1"], (0, 0, 2, 2, 2, 2))
    dy = s["dy2f"].clone()
    if mut == "dw2_image":
        dy[5] = 0
    if mut == "dw2_rowshift":  # one image row read one column off
        dy[3, 6, 1:] = s["dy2f"][3, 6, :-1]
        dy[3, 6, 0] = 0
    g["conv2_weight"], _, g["conv2_bias"], _ = R.conv2_bwd_filter(s["a1f"], dy, dt=F32)
    i1 = _transpose_q(s["idx1"]) if mut == "scatter_transposed" else s["idx1"]
    g["conv1_weight"], _, g["conv1_bias"], _ = R.conv1_bwd_filter(s["da1m"], i1, x, dt=F32)
    s["g"] = g
    return s


def _all_failures(s):
    return {name: R.failures(fn(s)) for name, fn in R.STAGES.items()}


@pytest.fixture(scope="module")
def base32():
    x, y, flat = _inputs("synthetic", 32)
    return x, y, flat


@pytest.mark.parametrize("kind,Bp,lb", [("synthetic", 32, 32), ("synthetic", 64, 50), ("random", 32, 32)])
def test_emulation_passes_every_stage(kind, Bp, lb):
    x, y, flat = _inputs(kind, Bp)
    s = emulate(x, y, flat, lb)
    for name, fn in R.STAGES.items():
        res = fn(s)
        print(name, {k: tuple(round(v, 4) if isinstance(v, float) else v for v in e[1:]) for k, e in res.items()})
        assert not R.failures(res), (name, R.failures(res))
    if lb < Bp:  # pad rows seed nothing
        for k in ("dlog", "dh", "dh16", "dy2", "da1m"):
            assert not s[k][lb:].any(), k


def test_argmax_caps_on_the_projects_rows_and_init():
    """The reference alone on the synthetic rows and the project's init: the
    share of active windows whose fp64 lead is within 2 acc stays under the
    caps (0.5 % pool1, 2 % pool2), so the GPU tests use these inputs."""
    x, y, flat = _inputs("synthetic", 64)
    s = emulate(x, y, flat, 64)
    e1, e2 = R.stage_conv1(s)["idx1"], R.stage_conv2(s)["idx2"]
    print("left out: pool1 %.4f %%, pool2 %.4f %%" % (100 * e1[3], 100 * e2[3]))
    assert e1[3] <= R.ARGMAX_CAP["idx1"] and e2[3] <= R.ARGMAX_CAP["idx2"]
    assert e1[1] == 0 and e2[1] == 0


# defect -> the stage whose check must catch it
MUTANTS = [
    ("fc1_kstep", "fc1"), ("dx_kstep", "fc1_bwd"), ("conv2_kstep", "conv2"),
    ("bwd_data_kstep", "conv2_bwd_data"),
    ("dw1_image", "fc1_bwd"), ("dw2_image", "conv2_bwd_filter"), ("dw2_rowshift", "conv2_bwd_filter"),
    ("trunc_a1", "conv1"), ("trunc_a2", "conv2"), ("trunc_dh16", "head"), ("trunc_dy2", "fc1_bwd"),
    ("idx_transposed", "conv1"), ("idx_transposed", "conv2"),
    ("scatter_transposed", "fc1_bwd"), ("scatter_transposed", "conv1_bwd_filter"),
    ("da1_unmasked", "conv2_bwd_data"),
]


@pytest.mark.parametrize("mut,stage", MUTANTS)
def test_defect_fails_its_stage(base32, mut, stage):
    x, y, flat = base32
    s = emulate(x, y, flat, 32, mut=mut)
    bad = R.failures(R.STAGES[stage](s))
    print(mut, stage, bad)
    assert bad, f"{mut} passed the {stage} check: the bound is too loose for this stage"


def test_stale_shadow_fails_the_shadow_check(base32):
    """Shadows taken from the parameters one SGD step earlier."""
    x, y, flat = base32
    s0 = emulate(x, y, flat, 32)
    lay = M.layout()
    new = flat.clone()
    nv, ov = lay.views(new), lay.views(flat)
    for name, g in s0["g"].items():
        l2 = C.L2_COEF if name.startswith("fc") else 0.0
        nv[name].sub_(C.BASE_LR * (g.reshape(ov[name].shape) + l2 * ov[name]))
    s = emulate(x, y, new, 32, shadow_flat=flat, step=1)
    bad = R.failures(R.stage_shadows(s))
    assert len(bad) == 4, bad  # each of the four shadows is caught
    assert not R.failures(R.stage_shadows(emulate(x, y, new, 32, step=1)))


def test_fc1_head_chains_its_pieces(base32):
    """fc1_head with the device's hd / dlog as the downstream inputs equals
    the three pieces the stage checks call."""
    x, y, flat = base32
    s, p = emulate(x, y, flat, 32), M.layout().views(flat)
    out = R.fc1_head(s["a2"], s["w1t"], p["fc1_bias"], p["fc2_weight"], p["fc2_bias"], y, s["mask"], s["keep"],
                     32, hd_dev=s["hd"], dlog_dev=s["dlog"])
    hd, S = R.fc1_fwd(s["a2"], s["w1t"], p["fc1_bias"], s["mask"], s["keep"])
    h = R.head_loss(s["hd"], p["fc2_weight"], p["fc2_bias"], y, 32)
    dh, S_dh = R.head_dh(s["dlog"], p["fc2_weight"], s["hd"], s["keep"])
    for got, want in ((out["hd"], hd), (out["S_hd"], S), (out["logits"], h["logits"]), (out["dlog"], h["dlog"]),
                      (out["loss"], h["loss"]), (out["dh"], dh), (out["S_dh"], S_dh)):
        assert torch.equal(got, want)
    # chained on its own values it is the fp64 model of the whole head
    own = R.fc1_head(s["a2"], s["w1t"], p["fc1_bias"], p["fc2_weight"], p["fc2_bias"], y, s["mask"], s["keep"], 32)
    assert (own["dh"] - s["dh"].double()).abs().max() < 1e-6


def test_dw2_group_slabs_check(base32):
    """The conv2 filter gradient per group of 8 images (the kernel's part2
    slabs): K shrinks from Bp 224 to 8 x 224."""
    x, y, flat = base32
    s = emulate(x, y, flat, 32)
    groups = []
    for n0 in range(0, 32, 8):
        dW, _, _, _ = R.conv2_bwd_filter(s["a1f"][n0:n0 + 8], s["dy2f"][n0:n0 + 8], dt=F32)
        groups.append((n0, n0 + 8, dW))
    assert not R.failures(R.stage_conv2_bwd_filter(s, groups))
    dy = s["dy2f"].clone()
    dy[11, 6, 1:] = s["dy2f"][11, 6, :-1]
    dy[11, 6, 0] = 0
    dW, _, _, _ = R.conv2_bwd_filter(s["a1f"][8:16], dy[8:16], dt=F32)
    groups[1] = (8, 16, dW)
    bad = R.failures(R.stage_conv2_bwd_filter(s, groups))
    assert len(bad) == 1 and "part2[8:16]" in bad[0], bad
