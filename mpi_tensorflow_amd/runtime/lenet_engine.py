"""Native LeNet-5 engine (BASELINE config 4) on the fused kernels of
`csrc/kernels/lenet.hip` through the C++ `LenetExecutor`.

State and step contract of `engine_common.EngineBase` (flat fp32 param /
grad / momentum buffers in the parallel/flat.py layout, device step counter,
reference LR schedule + momentum SGD of /root/reference/mpipy.py:59-66,
batch offset (step * B) % (N - B) of :80, per-step gradient all-reduce for
DP), but a training step is two kernel launches (one workgroup per image for
the whole forward + backward, then the batch-level weight gradients + SGD)
instead of the ~37 of the generic op-by-op path, and G steps are captured
into one hipGraph (`engine_common.GraphStepDriver`).  The numerics oracle is the generic engine's CPU path
(models/generic.py LeNet5 on plain PyTorch ops).
"""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from .. import config as C
from ..models.generic import make_model
from ..ops import native, ptr, stream_handle
from ..parallel.comm import DeviceComm, XgmiDeviceComm
from ..utils.devcache import DeviceArrayCache
from .engine_common import (TUNE_REPLAYS, EngineBase, GraphStepDriver, StateSnapshot,
                            all_ranks_ok, timed_replays, xgmi_healthy, xgmi_step_matches)
from .shuffle import make_shuffler

# the executor's xGMI sync modes (csrc/lenet_executor.h XGMI_*)
XGMI_MODES = C.XGMI_MODES
XGMI_MODE_IDS = {m: i for i, m in enumerate(XGMI_MODES)}

_OFFSETS = (("c1w", "c1_w"), ("c1b", "c1_b"), ("c2w", "c2_w"), ("c2b", "c2_b"), ("f1w", "f1_w"),
            ("f1b", "f1_b"), ("f2w", "f2_w"), ("f2b", "f2_b"), ("f3w", "f3_w"), ("f3b", "f3_b"))


class NativeLenetEngine(GraphStepDriver, EngineBase):
    kind = "native-lenet5"

    def __init__(self, cfg: C.TrainConfig, train_x: np.ndarray, train_y: np.ndarray,
                 device: torch.device, rank: int = 0, world: int = 1,
                 comm: Optional[DeviceComm] = None, force_sync: bool = False,
                 xcomm: Optional[XgmiDeviceComm] = None):
        """xcomm: an exactness-gated xGMI communicator (parallel/setup.py) next
        to an RCCL `comm`: tune_schedule() times both syncs and keeps the
        faster (the xGMI one only after one trial step matched RCCL's)."""
        if device.type != "cuda":
            raise RuntimeError("NativeLenetEngine needs a GPU")
        if cfg.model != "lenet5":
            raise ValueError("NativeLenetEngine trains lenet5 only")
        if cfg.dtype != "fp32":
            raise NotImplementedError("the fused LeNet-5 kernels are fp32 (VALU convs over 3 / 6 "
                                      "channels); use the generic engine for bf16")
        super().__init__(cfg, train_x.shape[0], device, rank, world, comm, force_sync)
        self.model = make_model("lenet5")
        self.layout = self.model.layout
        if tuple(train_x.shape[1:]) != (32, 32, 3):
            raise ValueError(f"LeNet-5 input must be 32x32x3 NHWC, got {train_x.shape[1:]}")
        host = torch.zeros(self.layout.total)
        self.model.init_params(host, cfg.seed)
        dev = device
        self.params = host.to(dev)
        self.init_ema()
        self.grads = torch.zeros(self.layout.total, device=dev)
        self.mom = torch.zeros(self.layout.total, device=dev)
        self.bn: Dict = {}
        self._eval_x = DeviceArrayCache()
        self.train_x = torch.from_numpy(np.ascontiguousarray(train_x, np.float32)).to(dev)
        self.train_y = torch.from_numpy(np.asarray(train_y).astype(np.int32)).to(dev)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self.lr_dev = torch.zeros(1, device=dev)
        self.correct_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        C_ = native()
        self._C = C_
        # cfg.shuffle / cfg.augment: the per-pass row order and shift / flip of the
        # working copy above (runtime/shuffle.py; keyed by the rank of the dropout
        # stream, Q14)
        self.shuffler = make_shuffler(cfg, self.drop_rank, self.n_local, self.train_x, self.train_y,
                                      native=C_, image_shape=(32, 32, 3))
        na, nd, nc = C_.lenet_buffer_floats(self.B)
        self.acts = torch.zeros(na, device=dev)
        self.deltas = torch.zeros(nd, device=dev)
        self.convp = torch.zeros(nc, device=dev)
        self.loss_rows = torch.zeros(self.B, device=dev)
        p = C_.LenetPtrs()
        p.train_x, p.train_y = ptr(self.train_x), ptr(self.train_y)
        p.n_local, p.batch = self.n_local, self.B
        if self.mix_rows() is not None:  # cfg.mix / cfg.label_smoothing: the soft xent wave
            p.train_y2, p.train_lam = (ptr(t) for t in self.mix_rows())
        p.label_smoothing = self.label_smoothing
        p.params, p.grads, p.mom = ptr(self.params), ptr(self.grads), ptr(self.mom)
        p.total = self.layout.total
        off = C_.LenetOffsets()
        for attr, name in _OFFSETS:
            setattr(off, attr, self.layout.offsets[name])
        p.off = off
        p.step, p.lr, p.correct = ptr(self.step_dev), ptr(self.lr_dev), ptr(self.correct_dev)
        p.acts, p.deltas, p.convp = ptr(self.acts), ptr(self.deltas), ptr(self.convp)
        p.loss_rows = ptr(self.loss_rows)
        p.base_lr, p.lr_decay, p.momentum = cfg.base_lr, cfg.lr_decay, cfg.momentum
        self.gb16 = None  # bf16 gradient wire staging (--grad-comm-dtype bf16)
        if cfg.grad_comm_dtype == "bf16" and self.grad_sync:
            if self.layout.total % 4:
                raise RuntimeError("bf16 gradient wire needs a flat buffer of 4k floats")
            self.gb16 = torch.zeros(self.layout.total, dtype=torch.bfloat16, device=dev)
            p.grad_bf16, p.gb16 = 1, ptr(self.gb16)
        self._native_comm = None
        self.xcomm = None
        self._sync = None  # the communicator the step syncs over (native handle)
        if self.grad_sync:
            self._native_comm = comm.native_handle
            if self._native_comm is None:
                raise RuntimeError("GPU grad sync needs the native RCCL communicator")
            if getattr(comm, "kind", "") == "host-staged":  # test comm: eager only
                comm.bases = [self.grads] + ([self.gb16] if self.gb16 is not None else [])
            self.xcomm = comm if isinstance(comm, XgmiDeviceComm) else xcomm
            if self.xcomm is not None:  # xGMI peer to peer: peers read the grads and
                # params, and (to make it whole) the sharded momentum
                if self.gb16 is not None:
                    raise ValueError("the xGMI communicator reduces fp32 grads only")
                self.xcomm.register(self.grads, self.params, self.mom)
                # receive slots [2 parities][N ranks][total] of the push sync
                # fused into the update launch (lenet.h PushArgs, replicated
                # momentum); the two-phase launch is the other xGMI form
                self.xrecv = torch.zeros(2 * self.xcomm.size * self.layout.total, device=dev)
                self.xcomm.register(self.xrecv)
                p.xrecv = ptr(self.xrecv)
                # the one-shot (pull) sync: double-buffered gradient slots
                # [2][total] read by every peer, and its completion counter
                self.xgrads2 = torch.zeros(2 * self.layout.total, device=dev)
                self.xcomm.register(self.xgrads2)
                self.xdone = torch.zeros(16, dtype=torch.int32, device=dev)
                p.xgrads2, p.xdone = ptr(self.xgrads2), ptr(self.xdone)
            self._sync = self._native_comm
            # connection setup of the collective, outside any capture (the
            # executor copies the pointer struct: made after xrecv is set)
            self.ptrs = p
            self.exe = C_.LenetExecutor(p)
            if self.xcomm is not None:
                self.exe.set_xgmi_mode(XGMI_MODE_IDS[cfg.xgmi_mode])
            self._native_comm.all_reduce(ptr(self.grads), ptr(self.grads), self.layout.total, 7, 0,
                                         stream_handle())
            torch.cuda.synchronize(dev)
        if not self.grad_sync:
            self.ptrs = p
            self.exe = C_.LenetExecutor(p)
        self.tune_log: Dict[str, Optional[float]] = {}
        self.tune_reject: Dict[str, str] = {}
        self.xgmi_step_check: Dict[str, float] = {}
        self._tuned = not (self.grad_sync and xcomm is not None and self.xcomm is xcomm
                           and cfg.graph and cfg.sync_schedule == "auto")
        self.use_graph = cfg.graph and getattr(comm, "kind", "") != "host-staged"
        self.graph_steps = max(1, cfg.graph_steps)
        self._graphs: Dict[int, torch.cuda.CUDAGraph] = {}

    # ------------------------------------------------------------------ util
    def sync_optimizer_state(self) -> None:
        """Replicated optimizer state: nothing to gather, except over the xGMI
        communicator's two-phase sync, whose fused all-reduce + SGD keeps each
        rank's momentum segment only (csrc/xgmi_comm.h all_reduce_sgd); the
        push and pull syncs keep the momentum replicated."""
        if self._syncs_over_xgmi() and self.xgmi_mode == "two-phase":
            self._sync.gather_segments(ptr(self.mom), self.layout.total, stream_handle())
            torch.cuda.synchronize(self.device)

    def _syncs_over_xgmi(self) -> bool:
        return self.xcomm is not None and self._sync is self.xcomm.native_handle

    @property
    def xgmi_mode(self) -> str:
        """The sync over the xGMI communicator: two-phase | push | pull."""
        m = self.exe.xgmi_mode if getattr(self, "exe", None) is not None else 0
        return XGMI_MODES[m]

    @property
    def sync_schedule(self) -> str:
        if not self.grad_sync:
            return "none"
        if self._syncs_over_xgmi():
            return {"two-phase": "xgmi", "push": "xgmi-push", "pull": "xgmi-pull"}[self.xgmi_mode]
        return "all-reduce"

    def loss_value(self) -> float:
        return float(self.loss_rows.mean().item())

    # ------------------------------------------------------------------ step
    def _launch_one(self) -> None:
        self.exe.train_step(stream_handle(), self._sync)
        if self.ema is not None:  # (one stream: the step's parameter writes are in order)
            self.ema_step()

    def _set_sync(self, c, mode: Optional[str] = None) -> None:
        mode = self.xgmi_mode if mode is None else mode
        if c is self._sync and mode == self.xgmi_mode:
            return
        self.sync_optimizer_state()  # (two-phase xGMI: the sharded momentum made whole)
        self._sync = c
        self.exe.set_xgmi_mode(XGMI_MODE_IDS[mode])

    def _graph(self, n: int):
        key = (id(self._sync), self.xgmi_mode, n)
        g = self._graphs.get(key)
        if g is None:
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g):
                    for _ in range(n):
                        self._launch_one()
            except RuntimeError as e:  # keep training eagerly rather than fail the run
                print(f"[rank {self.rank}] hipGraph capture failed ({e}); using eager launches",
                      flush=True)
                self.use_graph = False
                torch.cuda.synchronize(self.device)
                return None
            self._graphs[key] = g
        return g

    def tune_schedule(self) -> int:
        """With an xGMI candidate next to RCCL (setup_comms): times TUNE
        replays of each sync's captured G-step graph and keeps the faster.
        The xGMI sync must first pass the health vote (no barrier timed out,
        identical replicas) and one trial step equal to RCCL's within
        XGMI_STEP_RTOL of the update (identical replicas cannot show a
        wrong-but-consistent sum).  Side-effect free (params, momentum and the
        device step are restored); collective (max-over-ranks times, voted
        checks).  Returns the trial steps run."""
        if self._tuned:
            return 0
        G = self.graph_steps
        if self.shuffler is not None:  # the (discarded) trial steps read the current pass
            self.shuffler.ensure(self.step)
        snap = StateSnapshot(self.params, self.mom, self.step_dev,
                             *([self.ema] if self.ema is not None else []))
        xh = self.xcomm.native_handle
        base = (self._native_comm, "two-phase")
        cands = [("all-reduce",) + base, ("xgmi", xh, "two-phase"),
                 ("xgmi-push", xh, "push"), ("xgmi-pull", xh, "pull")]
        best, steps = None, 0
        for name, c, mode in cands:
            if c is not self._native_comm and self.xcomm is None:
                self.tune_log[name] = None  # (the xGMI communicator timed out before)
                continue
            self._set_sync(c, mode)
            snap.restore(sync=True)
            g = self._graph(G)
            if not all_ranks_ok(g is not None):
                self.tune_log[name] = None
                continue
            g.replay()
            torch.cuda.synchronize(self.device)
            steps += G
            if c is not self._native_comm:
                why = xgmi_healthy(self)
                if why is None and not self.xcomm.emulated_comm:  # one eager step each
                    outs = []
                    for cc, pp in ((c, mode), base):
                        self._set_sync(cc, pp)
                        snap.restore(sync=True)
                        self._launch_one()
                        torch.cuda.synchronize(self.device)
                        outs.append(self.params.clone())
                    self._set_sync(c, mode)
                    why = xgmi_step_matches(self, name, snap.saved[0], outs[0], outs[1],
                                            "the all-reduce's")
                if why is not None:
                    self.tune_log[name] = None
                    self.tune_reject[name] = why
                    if self.rank == 0:
                        print(f"[rank 0] sync {name} rejected: {why}", flush=True)
                    if "timed out" in why:
                        self.xcomm = None  # never used again (its barriers stop waiting)
                    continue
                snap.restore(sync=True)
            us = timed_replays(g, TUNE_REPLAYS, G, self.device)
            steps += TUNE_REPLAYS * G
            self.tune_log[name] = round(us, 2)
            if best is None or us < best[0]:
                best = (us, c, mode)
        if best is None:
            best = (0.0,) + base
        self._set_sync(best[1], best[2])
        snap.restore(sync=True)
        self._tuned = True
        return steps

    def forward_backward_only(self) -> None:
        """Forward + backward, weight grads into the flat grad buffer (no
        sync, no SGD, no step increment): numerics tests."""
        if self.shuffler is not None:
            self.shuffler.ensure(self.step)
        self.exe.forward_backward(stream_handle())

    # ------------------------------------------------------------------ eval
    @torch.no_grad()
    def evaluate(self, x: np.ndarray, y: np.ndarray, chunk: int = 4096, dropout: bool = False,
                 return_logits: bool = False):
        n = int(x.shape[0])
        xd = self._eval_x.get(x, self.device)
        yd = torch.from_numpy(np.asarray(y).astype(np.int32)).to(self.device)
        errors = torch.zeros(1, dtype=torch.int32, device=self.device)
        logits = torch.empty(n, 10, device=self.device) if return_logits else None
        s = stream_handle()
        for a in range(0, n, chunk):
            m = min(chunk, n - a)
            lg = ptr(logits) + 4 * 10 * a if logits is not None else 0
            self._C.LenetExecutor.eval_chunk(self.ptrs, ptr(xd) + 4 * 3072 * a, ptr(yd) + 4 * a, m,
                                             lg, ptr(errors), s)
        err = 100.0 * float(errors.item()) / max(1, n)
        return (err, logits) if return_logits else err
