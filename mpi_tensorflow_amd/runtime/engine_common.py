"""What the training engines share (runtime/mnist_engine.py, lenet_engine.py,
generic_engine.py).

* `EngineBase`: the state and the contract of every engine - flat fp32
  param / grad / momentum buffers in the parallel/flat.py layout (allocated by
  the engine: `params`, `grads`, `mom`, `layout`), the host step counter, the
  reference's LR schedule and batch offset (step * B) % (N_local - B), DP by
  per-step gradient all-reduce (`grad_sync`); under cfg.ema one more flat
  buffer `ema`, the moving average of `params` (`init_ema`, `ema_step`).
* `GraphStepDriver`: `train` / `capture` / `_run_steps` of the engines whose
  step is a fixed launch sequence replayed from captured G-step graphs; the
  engine supplies `_launch_one()` and `_graph(n)`.
* the pieces of a side-effect-free sync tune: `StateSnapshot`,
  `timed_replays`, `all_ranks_ok`, and the acceptance checks of an xGMI
  peer-to-peer communicator (`xgmi_healthy`, `xgmi_step_matches`), which
  decide whether it may train at all.
"""

from __future__ import annotations

import math
from typing import Dict, Iterator, List, Optional

import torch

from .. import config as C
from ..ops import functional as Fn
from ..parallel import dist as D
from ..parallel.comm import DeviceComm
from ..parallel.sync import replicas_identical
from ..utils.schedule import learning_rate

TUNE_REPLAYS = 2  # timed graph replays per tune candidate (after one untimed)
# xgmi_step_matches: max |update(xGMI) - update(baseline)| / max |update(baseline)|
XGMI_STEP_RTOL = 1e-4


class EngineBase:
    def __init__(self, cfg: C.TrainConfig, n_local: int, device: torch.device, rank: int = 0,
                 world: int = 1, comm: Optional[DeviceComm] = None, force_sync: bool = False):
        self.cfg, self.device, self.rank, self.world, self.comm = cfg, device, rank, world, comm
        self.B = cfg.batch_size
        self.n_local = int(n_local)
        if self.n_local <= self.B:
            raise ValueError(f"local shard of {self.n_local} rows must exceed batch {self.B}")
        self.step = 0  # host mirror of the global step (TF iter_)
        self.step_dev = None  # the device step counter, for engines whose kernels read one
        # rank of the dropout, shuffle and augment streams (quirk Q14)
        self.drop_rank = 0 if cfg.same_seed_all_ranks else rank
        # force_sync: exercise the collective path at world 1
        self.grad_sync = comm is not None and (force_sync or (cfg.sync == "grad" and world > 1))
        # cfg.shuffle / cfg.augment / cfg.mix: the per-pass rows (runtime/shuffle.py)
        self.shuffler = None
        # cfg.label_smoothing: the EPS of the soft training target (0: the hard label)
        self.label_smoothing = float(getattr(cfg, "label_smoothing", 0.0) or 0.0)
        # cfg.ema: the moving average of `params` (same layout; init_ema), else None
        self.ema: Optional[torch.Tensor] = None
        self.ema_decay, self.ema_every = C.parse_ema(cfg.ema) if cfg.ema is not None else (0.0, 1)

    def init_ema(self) -> None:
        """cfg.ema: allocates `ema` next to the (initialised) params and sets
        it to them - TF's shadow-variable initial value.  Without the flag
        nothing is allocated."""
        if self.cfg.ema is None:
            return
        if self.layout.total % 4:
            raise ValueError(f"--ema needs a flat buffer of 4k floats, got {self.layout.total}")
        self.ema = self.params.detach().clone()

    def ema_step(self, step=None) -> None:
        """One moving-average update on the current stream, after a step's
        SGD: `step` = the optimizer steps applied (default: the device
        counter, which the SGD has incremented; no host read)."""
        Fn.ema_update(self.ema, self.params, self.step_dev if step is None else step,
                      self.ema_decay, self.ema_every)

    @property
    def soft_targets(self) -> bool:
        """The training loss takes a soft target (--label-smoothing, --mix)."""
        return self.label_smoothing > 0.0 or self.mix_rows() is not None

    def mix_rows(self):
        """(work_y2, work_lam) of the shuffler under cfg.mix, else None."""
        sh = self.shuffler
        return (sh.work_y2, sh.work_lam) if sh is not None and sh.mix is not None else None

    def soft_loss_torch(self, logits: torch.Tensor, y: torch.Tensor, off: int) -> torch.Tensor:
        """The PyTorch paths' mean loss of the batch at row `off` of the working
        copy: the soft-target formula under the flags, else the hard-label one."""
        if not self.soft_targets:
            return torch.nn.functional.cross_entropy(logits, y.long())
        from ..utils.rng import soft_xent_torch
        m = self.mix_rows()
        y2, lam = (t[off:off + y.shape[0]] for t in m) if m is not None else (None, None)
        return soft_xent_torch(logits, y, y2, lam, self.label_smoothing)

    def param_views(self) -> Dict[str, torch.Tensor]:
        return self.layout.views(self.params)

    def lr(self, step: Optional[int] = None) -> float:
        s = self.step if step is None else step
        return learning_rate(s, self.n_local, self.B, self.cfg.base_lr, self.cfg.lr_decay)

    def sync_optimizer_state(self) -> None:
        """Makes `mom` whole on every rank (a sharded optimizer keeps only
        its own shard current); no-op for replicated optimizers."""

    def extra_state(self):
        """Non-trained state saved with checkpoints (none by default)."""
        return {}

    def set_step(self, step: int) -> None:
        self.step = int(step)
        if self.step_dev is not None:
            self.step_dev.fill_(int(step))

    def synchronize(self) -> None:
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)


def graph_sizes(k: int, G: int) -> List[int]:
    """Lengths of the graphs k steps replay: the G-step graph, the remainder."""
    return ([G] if k >= G else []) + ([k % G] if k % G else [])


def pass_pieces(shuffler, step: int, k: int, before_load=None) -> Iterator[int]:
    """Cuts the k steps from `step` at the pass boundaries of `shuffler`
    (whatever the caller asked for; the pieces reuse the per-length graph
    cache) and loads each pass before yielding its step count."""
    if shuffler is None:
        yield k
        return
    for p, m in shuffler.segments(step, k):
        if before_load is not None:
            before_load()
        shuffler.load(p)
        yield m


class GraphStepDriver:
    """Mixin: the engine has `use_graph`, `graph_steps`, `_tuned`, `step`,
    `shuffler`, and supplies `tune_schedule()`, `_launch_one()` (one eager
    step) and `_graph(n)` (the captured n-step graph, or None after a failed
    capture, which may also clear `use_graph`)."""

    _before_steps = _before_pass_load = _after_steps = None  # hooks of train()

    def train(self, k: int) -> None:
        if k <= 0:
            return
        if not self._tuned:  # side-effect free: restores the state it trained
            self.tune_schedule()
        if self._before_steps is not None:
            self._before_steps()
        for m in pass_pieces(self.shuffler, self.step, k, self._before_pass_load):
            self._run_steps(m)
        if self._after_steps is not None:
            self._after_steps()
        self.step += k

    def _run_steps(self, k: int) -> None:
        """k steps on the shard as it stands: graph replays, else eager launches."""
        done = 0
        if self.use_graph:
            G = self.graph_steps
            full, rem = divmod(k, G)
            g = self._graph(G) if full else None
            if g is not None:
                for _ in range(full):
                    g.replay()
                done = full * G
            if rem and self.use_graph:
                g = self._graph(rem)
                if g is not None:
                    g.replay()
                    done += rem
        for _ in range(k - done):  # eager (no graphs, or capture unavailable)
            self._launch_one()

    def capture(self, k: int) -> None:
        """Pre-captures the graphs `train(k)` will replay (outside timing)."""
        if self.use_graph and k > 0:
            for n in graph_sizes(k, self.graph_steps):
                self._graph(n)


class StateSnapshot:
    """Copies of the tensors a tune's trial steps change (params first, then
    momentum, the device step, ...).  `restore()` writes them back in place:
    the executors and the captured graphs hold the tensors' raw pointers."""

    def __init__(self, *tensors: torch.Tensor):
        self.tensors = tensors
        self.saved = [t.detach().clone() for t in tensors]

    def restore(self, sync: bool = False) -> None:
        with torch.no_grad():  # (the generic engine's params require grad)
            for t, s in zip(self.tensors, self.saved):
                t.copy_(s)
        if sync and self.tensors[0].is_cuda:
            torch.cuda.synchronize(self.tensors[0].device)


def all_ranks_ok(ok: bool) -> bool:
    """Collective vote: True only if `ok` on every rank (a tune candidate or a
    capture that failed on any rank is dropped on all of them)."""
    return D.allreduce_max_host(0.0 if ok else 1.0) == 0.0


def timed_replays(graph, replays: int, G: int, device: torch.device) -> float:
    """Max-over-ranks us per step of `replays` replays of the G-step `graph`."""
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(replays):
        graph.replay()
    t1.record()
    torch.cuda.synchronize(device)
    return D.allreduce_max_host(1000.0 * t0.elapsed_time(t1) / (replays * G))


def xgmi_healthy(eng) -> Optional[str]:
    """Collective: None when no rank's xGMI barrier timed out (the device
    kernels never hang: a missing peer sets a sticky error bit instead)
    and the replicas agree bit for bit after the trial steps, else why."""
    bad = eng.xcomm.error() if eng.xcomm is not None else 0
    if D.allreduce_max_host(float(bad)) != 0.0:
        return "a peer barrier timed out"
    if eng.xcomm is None or eng.xcomm.emulated_comm:
        return None
    # replicas must agree bit for bit after the trial steps (a lost or torn
    # peer read would show here): gather the sharded momentum and compare
    eng.sync_optimizer_state()
    torch.cuda.synchronize(eng.device)
    if not (replicas_identical(eng.params) and replicas_identical(eng.mom)):
        return "the replicas differ after the trial steps"
    return None


def xgmi_step_matches(eng, name: str, start: torch.Tensor, got: torch.Tensor, want: torch.Tensor,
                      baseline: str) -> Optional[str]:
    """Collective: `got` / `want` are the params after one eager step of the
    xGMI candidate `name` / of the baseline sync over the other communicator,
    both from the params `start`.  Identical replicas cannot reveal a
    wrong-but-consistent reduction (every rank gathers the same wrong
    segments), this can: the two parameter updates must agree to
    XGMI_STEP_RTOL of the largest update (rank-order vs RCCL summation is
    ~1e-7; a rank left out of the sum is ~1/N).  None = match (the measured
    difference goes to `eng.xgmi_step_check`), else why."""
    dx, ds = got - start, want - start
    ref = float(ds.abs().max())
    err = float((dx - ds).abs().max())
    bad = not (err <= XGMI_STEP_RTOL * ref) or not math.isfinite(err)
    worst = D.allreduce_max_host(err / max(ref, 1e-30))
    if not all_ranks_ok(not bad):
        return (f"one trial step differs from {baseline} by {worst:.2e} of the "
                f"largest update (bound {XGMI_STEP_RTOL:g})")
    eng.xgmi_step_check[name] = worst
    return None
