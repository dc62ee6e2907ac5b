"""tests/helpers/step_ref.py on a CPU-only machine: the references that
tests/test_step_kernels_gpu.py holds the optimizer, FC, loss and staging
kernels to are themselves right (a hand-computed SGD case, torch autograd in
float64, the stem layouts as inverses of each other), their input generators
meet the conditions the GPU cases are named for, and outputs a subtly wrong
kernel would write fail the same comparisons."""

import importlib.util
import os

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("step_ref", os.path.join(_HERE, "helpers", "step_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)
F32, F64 = torch.float32, torch.float64


# -------------------------------------------------------------- optimizer ----
def test_sgd_ref_hand_computed():
    """8 elements, L2 on the first 4: l2 = 0.5, momentum = 0.5, gscale = 0.5,
    lr = 0.25, every figure worked out by hand."""
    w = torch.tensor([4.0, -8.0, 2.0, 0.0, 4.0, -8.0, 2.0, 0.0])
    g = torch.tensor([2.0, 4.0, -6.0, 8.0, 2.0, 4.0, -6.0, 8.0])
    m = torch.tensor([8.0, -4.0, 2.0, 6.0, 8.0, -4.0, 2.0, 6.0])
    w2, m2 = R.sgd_ref(w, g, m, 4, 0.5, 0.5, 0.5, 0.25)
    # g' = g / 2 (+ w / 2):  [3, -2, -2, 4 | 1, 2, -3, 4];  m' = m / 2 + g'
    assert m2.tolist() == [7.0, -4.0, -1.0, 7.0, 5.0, 0.0, -2.0, 7.0]
    # w' = w - m' / 4
    assert w2.tolist() == [2.25, -7.0, 2.25, -1.75, 2.75, -8.0, 2.5, -1.75]
    assert w2.dtype == F64 and m2.dtype == F64
    tw, tm = R.sgd_tol(w, g, m, 4, 0.5, 0.5, 0.5, 0.25)
    assert tm.tolist() == [4 * R.EPS * v for v in (7.0, 8.0, 5.0, 7.0, 5.0, 4.0, 4.0, 7.0)]
    assert float(tw[0]) == R.EPS * 2.25 + 0.25 * float(tm[0]) + 2 * R.EPS * 0.25 * 7.0


def test_sgd_exact_operands_stay_exact():
    """Integers in +-64 with the dyadic constants: fp32 evaluation in any
    contraction equals float64."""
    g = torch.Generator().manual_seed(0)
    w, gr, m = (torch.randint(-64, 65, (4096,), generator=g).to(F32) for _ in range(3))
    w2, m2 = R.sgd_ref(w, gr, m, 2048, 0.5, 0.5, 0.5, 0.25)
    assert torch.equal(w2.to(F32).to(F64), w2) and torch.equal(m2.to(F32).to(F64), m2)
    lc = torch.zeros(4096)
    lc[:2048] = 0.5
    m32 = 0.5 * m + (gr * 0.5 + lc * w)
    assert torch.equal(m32.to(F64), m2) and torch.equal((w - 0.25 * m32).to(F64), w2)


def test_sgd_mutants_fail():
    """A dropped tail float4, L2 one float4 short, gscale left out."""
    n, l2_end = 1020, 508
    g = torch.Generator().manual_seed(1)
    w, gr, m = (torch.randn(n, generator=g) for _ in range(3))
    c = dict(l2=R.f32(5e-4), momentum=R.f32(0.9), gscale=R.f32(0.5), lr=R.f32(0.05))
    w2, m2 = R.sgd_ref(w, gr, m, l2_end, **c)
    tw, tm = R.sgd_tol(w, gr, m, l2_end, **c)

    def ok(a, b):
        return bool(((a - w2).abs() <= tw).all() and ((b - m2).abs() <= tm).all())
    assert ok(w2.to(F32).to(F64), m2.to(F32).to(F64))
    a, b = w2.clone(), m2.clone()
    a[-4:], b[-4:] = w[-4:].to(F64), m[-4:].to(F64)
    assert not ok(a, b)
    c2 = dict(c, l2=R.f32(0.1))  # (5e-4 x one float4 of w is below the bound: the exact mode's job)
    w3, m3 = R.sgd_ref(w, gr, m, l2_end, **c2)
    tw3, tm3 = R.sgd_tol(w, gr, m, l2_end, **c2)
    a, b = R.sgd_ref(w, gr, m, l2_end - 4, **c2)
    assert bool(((b - m3).abs() > tm3).any())
    assert not ok(*R.sgd_ref(w, gr, m, l2_end, **dict(c, gscale=1.0)))
    # exact mode sees the short L2 prefix at the real constant too
    wi, gi, mi = (torch.randint(-64, 65, (n,), generator=g).to(F32) for _ in range(3))
    wi[l2_end - 4:l2_end] = 3.0
    assert not torch.equal(R.sgd_ref(wi, gi, mi, l2_end, 0.5, 0.5, 0.5, 0.25)[0],
                           R.sgd_ref(wi, gi, mi, l2_end - 4, 0.5, 0.5, 0.5, 0.25)[0])


def test_l2_ends_are_float4_aligned():
    for n in (4, 1020, 4096, R.SGD_CAP_FLOATS + 1200):
        ends = R.l2_ends(n)
        assert all(e % 4 == 0 and 0 <= e <= n for e in ends) and 0 in ends and n in ends
    assert (R.SGD_CAP_FLOATS + 1200) % 4 == 0 and 1200 // 4 % 256 != 0  # second pass, ragged


# -------------------------------------------------------- fully connected ----
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,K,N", [(1, 1, 1), (5, 3, 1), (6, 130, 65), (130, 33, 10)])
def test_linear_ref_equals_autograd(M, K, N, relu):
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g, dtype=F64).requires_grad_(True)
    w = torch.randn(K, N, generator=g, dtype=F64).requires_grad_(True)
    b = torch.randn(N, generator=g, dtype=F64).requires_grad_(True)
    dy = torch.randn(M, N, generator=g, dtype=F64)
    y = x @ w + b
    if relu:
        y = y.relu()
    y.backward(dy)
    yr, S, n = R.linear_ref(x.detach(), w.detach(), b.detach(), relu)
    assert torch.allclose(yr, y.detach(), rtol=1e-13, atol=1e-13)
    assert n == K + R.lin_groups(N) + 1 and bool((S >= yr.abs() - 1e-12).all())
    r = R.linear_bwd_ref(x.detach(), w.detach(), yr, dy, relu)
    for k, t in (("dw", w.grad), ("db", b.grad), ("dx", x.grad)):
        assert torch.allclose(r[k][0], t, rtol=1e-12, atol=1e-12), k
    assert (r["dw"][2], r["db"][2], r["dx"][2]) == (M, M, N)


def test_linear_groups_follow_the_tile():
    assert [R.lin_groups(N) for N in (1, 2, 10, 64, 65, 120)] == [256, 128, 16, 4, 4, 4]


def test_linear_mask_is_zero_at_zero():
    """y == 0 passes no gradient (the kernel tests y <= 0), -0 included."""
    x, w = torch.ones(1, 1), torch.ones(1, 3)
    y = torch.tensor([[0.0, -0.0, 1.0]])
    r = R.linear_bwd_ref(x, w, y, torch.full((1, 3), 5.0), True)
    assert r["db"][0].tolist() == [0.0, 0.0, 5.0]


def test_linear_mutants_fail():
    """Column 64 skipped, the last K group dropped: both leave the bound."""
    M, K, N = 6, 130, 65
    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) * K ** -0.5, torch.randn(N, generator=g)
    y, S, n = R.linear_ref(x, w, b)
    t = R.lin_tol(S, n)
    assert bool(((y.to(F32).to(F64) - y).abs() <= t).all())
    bad = y.clone()
    bad[:, 64] = float("nan")
    assert not bool(((bad - y).abs() <= t).all())
    kg = R.lin_groups(N)
    keep = torch.arange(K) % kg != kg - 1
    short = R.linear_ref(x[:, keep], w[keep], b)[0]
    assert bool(((short - y).abs() > t).any())


# ------------------------------------------------------------------- loss ----
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("B,C", [(1, 1), (3, 10), (4, 64), (5, 65), (257, 1000)])
def test_xent_ref_equals_torch(B, C, shifted):
    z, lab = R.xent_inputs(B, C, seed=B + C, shifted=shifted)
    loss, dl, p, hits = R.xent_ref(z, lab)
    zt = z.to(F64).requires_grad_(True)
    lt = torch.nn.functional.cross_entropy(zt, lab.to(torch.int64), reduction="none")
    lt.mean().backward()
    assert torch.allclose(loss, lt.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(dl, zt.grad, rtol=1e-12, atol=1e-15)
    assert torch.allclose(p, torch.softmax(z.to(F64), 1), rtol=1e-12, atol=1e-300)
    assert bool(torch.isfinite(loss).all() and torch.isfinite(dl).all())
    # the fp32 yardstick stays finite as well
    l32, d32, p32, _ = R.xent_ref(z, lab, dt=F32)
    assert l32.dtype == F32 and bool(torch.isfinite(l32).all() and torch.isfinite(d32).all())
    if shifted and C >= 2:
        assert float(z[0].max()) == 88.0 and float(z[0].min()) == -88.0
        assert float(p32[0, C - 1]) == 0.0 and float(p[0, C - 1]) > 0.0  # e^-176: fp32 underflows, finite
    if shifted and C == 1000:  # without the max subtraction a +80 row overflows
        assert not bool(torch.isfinite(torch.exp(z).sum(1)).all())


@pytest.mark.parametrize("C", [4, 10, 64, 65, 1000])
def test_tie_rows_count_the_lowest_index(C):
    z, lab, hits = R.tie_rows(C)
    assert sum(hits) == 5 and z.shape == (11, C)
    on_later = 0
    for r in range(11):
        top = (z[r] == z[r].max()).nonzero().reshape(-1).tolist()
        assert len(top) in (2, 3)
        assert (int(lab[r]) == top[0]) == bool(hits[r])
        on_later += int(lab[r]) in top[1:]
        assert R.xent_ref(z[r:r + 1], lab[r:r + 1])[3] == hits[r]
    assert on_later == 3 and hits.count(0) == 6  # label on a later maximum, and on none
    assert R.xent_ref(z, lab)[3] == 5
    # the highest-index rule counts another total
    last = C - 1 - np.argmax(z.numpy()[:, ::-1], axis=1)
    assert int((torch.from_numpy(last.copy()) == lab).sum()) == 3


# ---------------------------------------------------------------- staging ----
def test_lr_ref():
    assert R.lr_ref(0, 100, 7, 0.01, 0.95) == R.f32(0.01)
    assert R.lr_ref(14, 100, 7, 0.01, 0.95) == R.f32(0.01)                      # 98 // 100
    assert R.lr_ref(15, 100, 7, 0.01, 0.95) == R.f32(0.01) * R.f32(0.95)        # 105 // 100
    assert abs(R.lr_ref(300, 100, 7, 0.01, 0.95) / (R.f32(0.01) * R.f32(0.95) ** 21) - 1) < 1e-15
    assert R.lr_ref(2 ** 33, 100, 256, 0.01, 0.95) == 0.0
    assert abs(R.lr_f32(300, 100, 7, 0.01, 0.95) / R.lr_ref(300, 100, 7, 0.01, 0.95) - 1) < 4 * 2.0 ** -24


@pytest.mark.parametrize("n_local,batch", [(100, 1), (100, 7), (100, 64), (101, 64), (301, 256)])
def test_gather_steps_reach_the_edges(n_local, batch):
    steps = R.gather_steps(n_local, batch)
    mod = n_local - batch
    offs = [R.batch_offset(s, n_local, batch) for s in steps]
    assert all(0 <= o < mod for o in offs) and 0 in steps and 1 in steps and 2 ** 33 in steps
    w = [s for s in steps if 0 < s < 2 ** 33 and R.batch_offset(s, n_local, batch) < R.batch_offset(s - 1, n_local, batch)]
    assert w or batch == 1 and mod in steps or mod == 1
    if np.gcd(batch, mod) == 1:
        assert mod - 1 in offs
    # a modulus of n_local would read other rows at the wrapped step
    assert any((s * batch) % n_local != o for s, o in zip(steps, offs))


# ----------------------------------------------------------- stem layouts ----
def test_im2col_layouts():
    assert R.im2col_layout(7, 7, 3) == (21, 24, 192)
    assert R.im2col_layout(3, 3, 7) == (21, 24, 128)


@pytest.mark.parametrize("R_,S,C,K", [(7, 7, 3, 8), (3, 3, 7, 8), (3, 3, 7, 64)])
def test_stem_layouts_are_inverses(R_, S, C, K):
    sc, seg, kp = R.im2col_layout(R_, S, C)
    w = torch.arange(1, R_ * sc * K + 1, dtype=F32).reshape(R_, S, C, K)
    wt = R.stem_wt_ref(w, R_, sc, seg, kp, K)
    pad = R.stem_pad_mask(R_, sc, seg, kp)
    assert int((~pad).sum()) == R_ * sc and bool((wt[:, pad] == 0).all()) and bool((wt[:, ~pad] != 0).all())
    # k = kh seg + kw C + ci
    assert float(wt[K - 1, 2 * seg + 1 * C + 2]) == float(w[2, 1, 2, K - 1])
    gpad = wt.t().clone()
    gpad[pad] = 1e30
    assert torch.equal(R.stem_wgrad_ref(gpad, R_, sc, seg, K).reshape(w.shape), w)


@pytest.mark.parametrize("K", [8, 64])
def test_s2d_wgrad_ref_inverts_the_weight_layout(K):
    w = torch.arange(1, 147 * K + 1, dtype=F32).reshape(7, 7, 3, K)
    wt8 = R.s2d_weight_ref(w, K)
    real = R.s2d_real_mask()
    assert int(real.sum()) == 147 and bool((wt8[:, ~real] == 0).all()) and bool((wt8[:, real] != 0).all())
    assert sorted(wt8[:, real].reshape(-1).tolist()) == list(range(1, 147 * K + 1))  # each tap once
    # spot values of the comment: k = (a 4 + b) 16 + (p 2 + q) 3 + ci <- w[2a + p - 1][2b + q - 1][ci]
    assert float(wt8[3, (1 * 4 + 2) * 16 + (1 * 2 + 0) * 3 + 2]) == float(w[2, 3, 2, 3])
    assert float(wt8[0, 3]) == 0.0 and float(wt8[0, 9]) == float(w[0, 0, 0, 0])  # (a, b) = 0: only p = q = 1
    assert bool((wt8[:, 12::16] == 0).all()) and not bool(real[12::16].any())
    dw8 = wt8.t().clone()
    dw8[~real] = 1e30
    assert torch.equal(R.s2d_wgrad_ref(dw8, K), w)
