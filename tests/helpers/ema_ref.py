"""The --ema definition in float64, and the bound the tests hold the fp32
implementations to (tests/test_ema_cpu.py, tests/test_ema_gpu.py, the rank
helper ema_sync_ranks.py).

Definition (docs/ACCURACY.md): t = optimizer steps applied; t % K != 0: nothing;
else u = t / K - 1, d = min(DECAY, (1 + u) / (10 + u)), ema += (1 - d) (w - ema).
DECAY enters as the float32 the implementations receive; everything else here
is float64.

Bound, derived (u = 2^-24, M = max(|w|, |ema|) of the element): one fp32
update differs from the float64 one by less than 8 u M = 2^-21 M -
fl(w - ema) errs by at most 2 u M, the one fma rounding by at most u M, and
an omd that is one ulp of the fp32 division and of the subtraction off adds at
most 4 u M.  An earlier error is carried on scaled by d < 1, so k updates stay
within k 2^-21 M, M taken over every value the element took.
"""
import numpy as np
import torch

ONE_UPDATE = 2.0 ** -21


def decay64(t: int, decay: float, K: int = 1):
    """d of the update after step t in float64, None when t % K != 0."""
    if t % K:
        return None
    u = t // K - 1
    return min(float(np.float32(decay)), (1.0 + u) / (10.0 + u))


def update64(ema64: torch.Tensor, w: torch.Tensor, t: int, decay: float, K: int = 1) -> torch.Tensor:
    d = decay64(t, decay, K)
    if d is None:
        return ema64
    return ema64 + (1.0 - d) * (w.double() - ema64)


def recurrence(ema0: torch.Tensor, params, decay: float, K: int = 1, t0: int = 0):
    """params[i]: the fp32 parameters after optimizer step t0 + i + 1.
    -> (ema in float64, the per-element bound k 2^-21 M)."""
    ema = ema0.detach().double().cpu()
    M = ema.abs()
    k = 0
    for i, w in enumerate(params):
        w = w.detach().cpu()
        t = t0 + i + 1
        if decay64(t, decay, K) is None:
            continue
        ema = update64(ema, w, t, decay, K)
        M = torch.maximum(M, torch.maximum(w.double().abs(), ema.abs()))
        k += 1
    return ema, k * ONE_UPDATE * M


def assert_within(got: torch.Tensor, want64: torch.Tensor, bound: torch.Tensor, what: str) -> None:
    err = (got.detach().double().cpu() - want64).abs()
    over = err > bound
    worst = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert not bool(over.any()), (f"{what}: {int(over.sum())} elements past the bound, worst "
                                  f"err / bound {worst:.3f}")
