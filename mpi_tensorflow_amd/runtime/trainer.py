"""The training driver: the reference's `main()` + `Cnn` re-built around the
engines (`/root/reference/mpipy.py:201-244` main, `:24-93` Cnn).

Flow (reference line refs in brackets):
  1. acquisition on rank 0 only, then a barrier            [:203-206; fixes Q3]
  2. rank/world from the launcher, GPU bound to local rank  [:208-210; fixes Q13]
  3. each rank loads/generates only its shard               [:211-241 Scatter x6]
  4. engine = fused HIP kernels (GPU) or PyTorch oracle (CPU)
  5. "Process ID: r  training session starts!"              [:77]
  6. steps = epochs * N_local // B                          [:79]
     - train segments run as replays of captured step graphs
     - every `eval_every` steps: local test error + reference log line [:86-90]
     - every `sync_every` steps in param_avg mode: weight averaging    [:91]
  7. final evaluation, throughput summary, optional checkpoint.

Training throughput excludes evaluation (the reference spends ~98 % of its
wall time evaluating every step); eval time is reported apart.
"""

from __future__ import annotations

import dataclasses
import time
import warnings
from typing import Dict, Optional

import numpy as np
import torch

from .. import config as C
from ..parallel import dist as D
from ..parallel.setup import check_health, comm_capacity_bytes, setup_comms  # noqa: F401
from ..parallel.watchdog import make_watchdog, run_in_chunks
from ..parallel.sync import average_params, average_params_root_only, replicas_identical
from ..utils import checkpoint as ckpt_mod
from ..utils.data import (data_exist_here, load_mnist_shard, local_train_rows, mnist_files_present,
                          steps_per_run, synthetic_image_shard)
from ..utils.logging import MetricsWriter, emit, progress_line, start_line
from ..ops import functional as Fn
from ..utils import rng
from ..utils.data import batch_offset, pass_of
from ..utils.devcache import DeviceArrayCache
from ..utils.metrics import EvalMetrics
from ..utils.faults import maybe_fail
from ..utils.profiling import SegmentTimer
from .shuffle import batch_rows


@dataclasses.dataclass
class RunSummary:
    model: str
    world: int
    steps: int
    batch: int
    images: int
    train_seconds: float
    eval_seconds: float
    images_per_sec_local: float
    images_per_sec_global: float
    final_test_error_local: float
    final_test_error_global: float
    final_loss: float
    final_lr: float
    device_step_ms: float
    engine: str
    comm: str
    synthetic: bool
    sync_schedule: str = "n/a"
    xgmi_gate: str = "n/a"
    # --eval-metrics only (global, summed over the ranks); left out of
    # as_dict() while unset, so a run without the flag reports what it always did
    final_test_loss: Optional[float] = None
    final_val_error: Optional[float] = None
    final_val_loss: Optional[float] = None
    # --ema only: the final test error of the averaged weights
    final_ema_test_error_local: Optional[float] = None
    final_ema_test_error_global: Optional[float] = None

    # --label-smoothing / --mix only: the run's soft-target flags as given
    label_smoothing: Optional[float] = None
    mix: Optional[str] = None

    _OPTIONAL = ("final_test_loss", "final_val_error", "final_val_loss",
                 "final_ema_test_error_local", "final_ema_test_error_global",
                 "label_smoothing", "mix")

    def as_dict(self) -> Dict:
        d = dataclasses.asdict(self)
        for k in self._OPTIONAL:
            if d[k] is None:
                del d[k]
        return d


class Trainer:
    def __init__(self, cfg: C.TrainConfig, di: Optional[D.DistInfo] = None):
        self.cfg = cfg.validate()
        self.device = D.resolve_device(cfg.device)
        self.di = di or D.init(str(self.device), timeout_s=cfg.collective_timeout_s)
        self.rank, self.world = self.di.rank, self.di.world
        maybe_fail("after_init", self.rank)
        # the watchdog exists before any communicator: a peer that dies during
        # start-up (communicator init, the engines' connection-setup
        # collectives) ends every rank within the deadline instead of hanging
        self.watchdog = make_watchdog([], cfg.collective_timeout_s, self.rank, self.world)
        self._chunk_state: Dict = {}
        with self.watchdog.guard("start-up (data, communicator, engine)"):
            self._prepare_data()
            maybe_fail("before_comm", self.rank)
            # the same communicator set-up as bench.py (parallel/setup.py): the
            # device comm, plus on one node the exactness-gated xGMI candidate
            self.comms = setup_comms(self.di, self.device, cfg, no_xgmi=cfg.no_xgmi)
            self.comm = self.comms.comm
            self.watchdog.add(self.comm)
            maybe_fail("after_comm", self.rank)
            self.engine = self._make_engine()
            self.watchdog.add(getattr(self.engine, "comm2", None))
            self._sync()
        if cfg.resume:
            step, _ = ckpt_mod.load(cfg.resume, self.engine.layout, self.engine.params,
                                    self.engine.mom, extra=self.engine.extra_state(),
                                    expect={"model": cfg.model, "world": self.world})
            self.engine.set_step(step)
            if self.engine.ema is not None:
                self._resume_ema(cfg.resume)
        self._ema_predictor: Dict = {}  # --ema: split -> the Predictor on engine.ema (kept)
        self.metrics = MetricsWriter(cfg.metrics_jsonl, self.rank)
        # the native MNIST engine evaluates device arrays: the test and the
        # validation split are uploaded at their first evaluation and stay
        # resident (the other GPU engines keep their own copy, utils/devcache.py)
        self._resident = cfg.model == "mnist_cnn" and getattr(self.engine, "kind", "") == "native"
        self.eval_cache = {"test": DeviceArrayCache(), "val": DeviceArrayCache()}
        self._eval_y: Dict = {}
        # --eval-metrics: the last event's global metrics per split; --ckpt-best
        self.last_metrics: Dict[str, EvalMetrics] = {}
        self.best_val_error = float("inf")
        self.best_step: Optional[int] = None

    # ------------------------------------------------------------------ data
    def _prepare_data(self):
        cfg = self.cfg
        if cfg.model == "mnist_cnn":
            if self.rank == 0 and cfg.download and not mnist_files_present(cfg.data_dir):
                for f in C.MNIST_FILES.values():
                    data_exist_here(f, cfg.data_dir, download=True)
            D.barrier()
            self.shard = load_mnist_shard(self.rank, self.world, cfg.data_dir, cfg.synthetic,
                                          pad=cfg.pad_train_shard, seed=cfg.seed)
        else:
            from ..models.generic import model_input_shape
            from ..utils.data import Shard, SplitSizes, synthetic_images_torch

            shape = model_input_shape(cfg.model)
            if cfg.model == "lenet5":
                rows = 8192
                self.shard = synthetic_image_shard(self.rank, self.world, rows, rows // 4, shape,
                                                   seed=cfg.seed)
            else:  # 224x224x3: generated with torch (numpy path is too heavy)
                rows, trows = 512, 256
                tx, ty = synthetic_images_torch(rows, shape, seed=cfg.seed, start=self.rank * rows)
                sx, sy = synthetic_images_torch(trows, shape, seed=cfg.seed, split="test",
                                                start=self.rank * trows)
                self.shard = Shard(tx.numpy(), ty.numpy(), sx.numpy(), sy.numpy(),
                                   sx.numpy()[:0], sy.numpy()[:0], True,
                                   SplitSizes(self.world, rows * self.world, trows * self.world, 0))
        if self.shard.test_x.shape[0] < 1:
            raise ValueError("empty local test shard")
        if cfg.ckpt_best and self.shard.val_x.shape[0] < 1:
            raise ValueError("--ckpt-best: this rank's shard has no validation rows")

    def _make_engine(self):
        cfg = self.cfg
        sh = self.shard
        if cfg.model == "mnist_cnn":
            from .mnist_engine import make_engine

            return make_engine(cfg, sh.train_x, sh.train_y, self.device, self.rank, self.world,
                               self.comm, xcomm=self.comms.xcomm)
        from .generic_engine import make_image_engine

        return make_image_engine(cfg, sh.train_x, sh.train_y, self.device, self.rank, self.world,
                                 self.comm, xcomm=self.comms.xcomm)

    # ------------------------------------------------------------------- run
    def total_steps(self) -> int:
        if self.cfg.max_steps is not None:
            return int(self.cfg.max_steps)
        return steps_per_run(self.engine.n_local, self.cfg.epochs, self.cfg.batch_size)

    def _event(self, s: int) -> bool:
        cfg = self.cfg
        if s <= 0:
            return False
        ev = cfg.effective_eval_every()
        if ev and s % ev == 0:
            return True
        if cfg.sync == "param_avg" and self.world > 1 and s % cfg.sync_every == 0:
            return True
        if cfg.ckpt and cfg.ckpt_every and s % cfg.ckpt_every == 0:
            return True
        return False

    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def _split(self, split: str):
        if split == "test":
            return self.shard.test_x, self.shard.test_y
        if split == "val":
            return self.shard.val_x, self.shard.val_y
        raise ValueError(f"unknown split {split!r}; choose 'test' or 'val'")

    def _labels_dev(self, split: str, y: np.ndarray) -> torch.Tensor:
        """int32 device copy of a split's labels, uploaded once per array object"""
        held = self._eval_y.get(split)
        if held is None or held[0] is not y:
            held = (y, torch.from_numpy(np.ascontiguousarray(y).astype(np.int32)).to(self.device))
            self._eval_y[split] = held
        return held[1]

    def _engine_evaluate(self, split: str, dropout: Optional[bool], return_logits: bool = False):
        x, y = self._split(split)
        d = self.cfg.eval_dropout if dropout is None else dropout
        if self._resident:
            x_dev = self.eval_cache[split].get(x, self.device)
            return self.engine.evaluate(x, y, dropout=d, x_dev=x_dev,
                                        y_dev=self._labels_dev(split, y),
                                        return_logits=return_logits)
        return self.engine.evaluate(x, y, dropout=d, return_logits=return_logits)

    def evaluate(self, dropout: Optional[bool] = None) -> float:
        return self._engine_evaluate("test", dropout)

    def _split_metrics(self, split: str, dropout: Optional[bool] = None):
        x, y = self._split(split)
        if x.shape[0] < 1:
            raise ValueError(f"this rank's {split} split is empty")
        err, logits = self._engine_evaluate(split, dropout, return_logits=True)
        labels = self._labels_dev(split, y) if self._resident else torch.from_numpy(
            np.ascontiguousarray(y).astype(np.int64))
        return err, Fn.eval_metrics(logits, labels)

    def evaluate_metrics(self, split: str = "test", dropout: Optional[bool] = None) -> EvalMetrics:
        """Metrics of this rank's rows of a split (utils/metrics.py): the
        engine's evaluation logits through Fn.eval_metrics, so it holds for
        every engine.  Global metrics are the sum over the ranks."""
        return self._split_metrics(split, dropout)[1]

    def _metrics_event(self, step: int, final: bool = False):
        """--eval-metrics at an eval event: this rank's test error (the log
        line's), the keys the event adds to its metrics record - the metrics
        of the test and validation splits summed over the ranks - and rank 0's
        extra log line.
        --ckpt-best: the checkpoint is written here when the global validation
        error improved (the same value, so the same branch, on every rank)."""
        cfg = self.cfg
        err, test = self._split_metrics("test")
        parts = {"test": test}
        if self.shard.val_x.shape[0] > 0:  # the same on every rank (5000 // world)
            parts["val"] = self._split_metrics("val")[1]
        packed = [m.pack() for m in parts.values()]
        ints = np.concatenate([p[0] for p in packed])
        sums = np.concatenate([p[1] for p in packed])
        if self.world > 1:
            with self.watchdog.guard(f"evaluation metrics all-reduce at step {step}"):
                ints, sums = D.allreduce_sum_host_array(ints), D.allreduce_sum_host_array(sums)
        k, per = test.classes, test.classes * (test.classes + 1) + 2
        for i, name in enumerate(parts):
            parts[name] = EvalMetrics.unpack(ints[i * per:(i + 1) * per], sums[i:i + 1], k)
        self.last_metrics = parts
        test, val = parts["test"], parts.get("val")
        rec = {"test_loss": test.loss, "test_error_global": test.error,
               "test_top3_error": test.topk_error(3)}
        line = (f"[metrics] step {step}: test loss {test.loss:.4f}, error {test.error:.2f}%, "
                f"top-3 error {test.topk_error(3):.2f}%")
        if val is not None:
            rec.update(val_error=val.error, val_loss=val.loss)
            line += f"; validation loss {val.loss:.4f}, error {val.error:.2f}%"
        if final:
            rec.update(test_confusion=test.confusion.tolist(), test_rank_hist=test.rank_hist.tolist(),
                       test_per_class_recall=test.to_json()["per_class_recall"])
            if val is not None:
                rec["val_confusion"] = val.confusion.tolist()
        if cfg.ckpt_best:  # val is there: checked at start-up
            if val.error < self.best_val_error:  # ties keep the earlier checkpoint
                self.best_val_error, self.best_step = val.error, step
                self.save_checkpoint(cfg.ckpt_best)
            rec.update(best_val_error=self.best_val_error, best_step=self.best_step)
            line += f" (best {self.best_val_error:.2f}% at step {self.best_step})"
        return err, rec, line

    def _resume_ema(self, path: str) -> None:
        """--ema on resume: the checkpoint's average, or - from a checkpoint
        written without --ema - the loaded parameters, with a warning; a saved
        spec other than this run's continues the saved average under the new one."""
        eng = self.engine
        found, spec = ckpt_mod.load_ema(path, eng.layout, eng.ema)
        if not found:
            with torch.no_grad():
                eng.ema.copy_(eng.params.detach())
            warnings.warn(f"{path} holds no moving average (written without --ema): the average "
                          f"starts from the loaded parameters")
        elif spec is not None and C.parse_ema(spec) != C.parse_ema(self.cfg.ema):
            warnings.warn(f"{path}: saved ema={spec} but this run has ema={self.cfg.ema}; the saved "
                          f"average continues under the new spec")

    def _ema_event(self, step: int, with_metrics: bool):
        """--ema at a logged eval event: the averaged weights on this rank's
        test split, through a Predictor that shares `engine.ema` (zero copy; the
        engines' static eval forward, so nothing of training is touched) and is
        kept with its workspaces for the later events -> (the keys the event
        adds to its metrics record, rank 0's extra log line).  with_metrics
        (--eval-metrics): also the test loss and the validation split, summed
        over the ranks as _metrics_event sums them."""
        from .predict import Predictor

        splits = ["test"]
        if with_metrics and self.shard.val_x.shape[0] > 0:  # the same on every rank
            splits.append("val")
        parts = {}
        on_dev = self.device.type == "cuda"
        for split in splits:
            # (a Predictor a split: each keeps the result buffers of its row count)
            if split not in self._ema_predictor:
                self._ema_predictor[split] = Predictor.from_engine(self.engine, weights="ema")
            x, y = self._split(split)
            xd = self.eval_cache[split].get(x, self.device) if on_dev else x
            parts[split] = self._ema_predictor[split].evaluate(
                xd, self._labels_dev(split, y) if on_dev else y)
        err = parts["test"].error
        rec = {"ema_test_error": err}
        line = f"[ema] step {step}: test error {err:.2f}%"
        if with_metrics:
            packed = [m.pack() for m in parts.values()]
            ints = np.concatenate([p[0] for p in packed])
            sums = np.concatenate([p[1] for p in packed])
            if self.world > 1:
                with self.watchdog.guard(f"ema evaluation metrics all-reduce at step {step}"):
                    ints, sums = D.allreduce_sum_host_array(ints), D.allreduce_sum_host_array(sums)
            k = parts["test"].classes
            per = k * (k + 1) + 2
            for i, name in enumerate(parts):
                parts[name] = EvalMetrics.unpack(ints[i * per:(i + 1) * per], sums[i:i + 1], k)
            test, val = parts["test"], parts.get("val")
            rec.update(ema_test_loss=test.loss, ema_test_error_global=test.error)
            if val is not None:
                rec.update(ema_val_error=val.error, ema_val_loss=val.loss)
        return rec, line

    def eval_prediction(self, x: np.ndarray, dropout: Optional[bool] = None) -> torch.Tensor:
        """`eval_prediction = softmax(model(eval_data))` of the reference
        (/root/reference/mpipy.py:68): class probabilities [n, 10] (dropout
        per --eval-dropout, as the reference's shared graph applies it)."""
        d = self.cfg.eval_dropout if dropout is None else dropout
        n = int(x.shape[0])
        _, logits = self.engine.evaluate(x, np.zeros(n, np.int64), dropout=d, return_logits=True)
        return Fn.softmax(logits)

    def train_prediction(self) -> torch.Tensor:
        """`train_prediction = softmax(logits)` of the reference's training graph
        (/root/reference/mpipy.py:67): probabilities for the current training
        batch (rows at the step's batch offset, dropout on as in training)."""
        sh, cfg, step = self.shard, self.cfg, self.engine.step
        n, B = sh.train_x.shape[0], cfg.batch_size
        rank = 0 if cfg.same_seed_all_ranks else self.rank
        if cfg.shuffle:  # the rows the step reads: this pass's order of the shard
            rows = batch_rows(cfg.seed, rank, step, n, B)
        else:
            off = batch_offset(step, n, B)
            rows = np.arange(off, off + B)
        p = pass_of(step, n, B)

        def loaded(rows):  # the shard rows `rows` as the pass's loader shows them
            x = sh.train_x[rows]
            if cfg.augment is not None:  # ... with this pass's draws for each of them
                spec = C.parse_augment_spec(cfg.augment, cfg.model)
                key = rng.augment_key(cfg.seed, rank, p)
                if spec.affine:
                    q = rng.affine_params(key, rows, spec, *x.shape[1:3])
                    return rng.affine_np(x, q.m, q.dy, q.dx, q.flipped, spec.fill, q.cutout)
                return rng.augment_np(x, *rng.augment_params(key, rows, spec.K, spec.flip),
                                      spec.fill)
            return x

        x = loaded(rows)
        if cfg.mix is not None:  # ... blended with their partner rows of the pass
            kind, M = C.parse_mix(cfg.mix)
            H, W = x.shape[1:3]
            order = (rng.shuffle_perm(rng.shuffle_key(cfg.seed, rank, p), n) if cfg.shuffle
                     else np.arange(n))
            off = batch_offset(step, n, B)
            q = [v[off:off + B] for v in rng.mix_params(rng.mix_key(cfg.seed, rank, p), n,
                                                        rng.mix_table(kind, M, H, W), H, W)]
            # the batch's rows, then their partners (which mix with nothing)
            both = np.concatenate([x, loaded(order[q[0]])])
            ident = [np.arange(B, 2 * B), np.full(B, 65536)] + [np.zeros(B, np.int64)] * 4
            q[0] = np.arange(B, 2 * B)
            prm = [np.concatenate([a, b]) for a, b in zip(q, ident)]
            x = rng.mix_np(both, np.zeros(2 * B, np.int64), prm, kind)[0][:B]
        return self.eval_prediction(x, dropout=True)

    def check_replicas(self, step: int, averaged: bool = False) -> None:
        """All ranks must hold bit-identical weights under per-step gradient
        all-reduce, and right after an all-ranks parameter average
        (`averaged`); a mismatch means a lost / corrupted collective."""
        if self.world <= 1 or (self.cfg.sync != "grad" and not averaged):
            return
        if not replicas_identical(self.engine.params):
            raise RuntimeError(f"replicas diverged at step {step}: the bitwise weight "
                               f"fingerprints differ between ranks")
        # the average follows the weights every step: identical only under grad sync
        if self.engine.ema is not None and self.cfg.sync == "grad" and not averaged:
            if not replicas_identical(self.engine.ema):
                raise RuntimeError(f"replicas diverged at step {step}: the bitwise fingerprints of "
                                   f"the averaged weights (--ema) differ between ranks")

    def sync_schedule(self) -> str:
        return getattr(self.engine, "sync_schedule", "n/a")

    def run(self) -> RunSummary:
        try:
            return self._run()
        finally:
            self.watchdog.stop()

    def _run(self) -> RunSummary:
        cfg, eng = self.cfg, self.engine
        emit(start_line(self.rank), cfg.quiet)
        # the gradient-sync schedule is chosen once, before training, exactly as
        # bench.py does (the trial steps are discarded: params, momentum and
        # step are restored), so mpipy and bench train with the same schedule
        if hasattr(eng, "tune_schedule"):
            with self.watchdog.guard("sync-schedule autotune"):
                eng.tune_schedule()
                self._sync()
        self._health("after the sync-schedule autotune")
        maybe_fail("before_train", self.rank)
        steps = self.total_steps()
        s = eng.step
        train_t = 0.0
        eval_t = 0.0
        trained = 0
        timer = SegmentTimer(self.device)
        while s < steps:
            nxt = s
            while nxt < steps - 1 and not self._event(nxt):
                nxt += 1
            k = nxt - s + 1
            self._sync()
            t0 = time.perf_counter()
            timer.start()
            run_in_chunks(self.watchdog, eng.train, self._sync, k, "train steps", first_step=s,
                          granule=getattr(eng, "graph_steps", 1), state=self._chunk_state)
            timer.stop(k)
            timer.collect()
            train_t += time.perf_counter() - t0
            trained += k
            s += k
            last = s - 1
            if not self._event(last):
                continue
            self._health(f"step {last}")
            ev = cfg.effective_eval_every()
            if ev and last % ev == 0:
                t1 = time.perf_counter()
                logged = last % (cfg.sync_every if cfg.reference_quirks else ev) == 0
                extra: Dict = {}
                if cfg.eval_metrics and logged:
                    err, extra, mline = self._metrics_event(last)
                else:
                    err = self.evaluate()
                if eng.ema is not None and logged:
                    erec, eline = self._ema_event(last, cfg.eval_metrics)
                eval_t += time.perf_counter() - t1
                if logged:
                    emit(progress_line(self.rank, last, err), cfg.quiet)
                    if extra and self.rank == 0:
                        emit(mline, cfg.quiet)
                    if eng.ema is not None:
                        extra = {**extra, **erec}
                        if self.rank == 0:
                            emit(eline, cfg.quiet)
                    self.metrics.write(step=last, test_error=err, loss=eng.loss_value(), **extra,
                                       sync_schedule=self.sync_schedule(),
                                       lr=eng.lr(last), train_seconds=train_t,
                                       device_step_ms=timer.step_ms(),
                                       images_per_sec=trained * cfg.batch_size / max(train_t, 1e-9))
                if cfg.check_replicas:
                    self.check_replicas(last)
            if cfg.sync == "param_avg" and self.world > 1 and last % cfg.sync_every == 0:
                t2 = time.perf_counter()
                with self.watchdog.guard(f"parameter averaging at step {last}"):
                    if cfg.root_only_average:
                        average_params_root_only(self.comm, eng.layout, eng.params)
                    else:
                        average_params(self.comm, eng.params)
                    self._sync()
                train_t += time.perf_counter() - t2
                if cfg.check_replicas and not cfg.root_only_average:
                    self.check_replicas(last, averaged=True)
            if cfg.ckpt and cfg.ckpt_every and last % cfg.ckpt_every == 0:
                self.save_checkpoint(cfg.ckpt)
        self._health(f"end of training (step {s - 1})")
        if cfg.check_replicas:
            self.check_replicas(s - 1)
        t1 = time.perf_counter()
        extra: Dict = {}
        if cfg.eval_metrics:
            final_err, extra, mline = self._metrics_event(s - 1, final=True)
            if self.rank == 0:
                emit(mline, cfg.quiet)
        else:
            final_err = self.evaluate()
        ema_err = None
        if eng.ema is not None:
            erec, eline = self._ema_event(s - 1, cfg.eval_metrics)
            extra = {**extra, **erec}
            ema_err = erec["ema_test_error"]
            if self.rank == 0:
                emit(eline, cfg.quiet)
        eval_t += time.perf_counter() - t1
        n_test = self.shard.test_x.shape[0]
        wrong_g = D.allreduce_sum_host(final_err * n_test / 100.0)
        n_g = D.allreduce_sum_host(float(n_test))
        ema_err_g = None
        if ema_err is not None:
            ema_err_g = 100.0 * D.allreduce_sum_host(ema_err * n_test / 100.0) / max(n_g, 1)
        train_t_max = D.allreduce_max_host(train_t)
        images = trained * cfg.batch_size
        summary = RunSummary(
            model=cfg.model, world=self.world, steps=trained, batch=cfg.batch_size, images=images,
            train_seconds=train_t, eval_seconds=eval_t,
            images_per_sec_local=images / max(train_t, 1e-9),
            images_per_sec_global=images * self.world / max(train_t_max, 1e-9),
            final_test_error_local=final_err, final_test_error_global=100.0 * wrong_g / max(n_g, 1),
            final_loss=eng.loss_value(), final_lr=eng.lr(max(0, s - 1)),
            device_step_ms=timer.step_ms(), engine=eng.kind,
            comm=getattr(self.comm, "kind", "none"), synthetic=self.shard.synthetic,
            sync_schedule=self.sync_schedule(), xgmi_gate=self.comms.xgmi_status,
            final_test_loss=extra.get("test_loss"), final_val_error=extra.get("val_error"),
            final_val_loss=extra.get("val_loss"),
            final_ema_test_error_local=ema_err, final_ema_test_error_global=ema_err_g,
            label_smoothing=cfg.label_smoothing if cfg.label_smoothing > 0 else None, mix=cfg.mix)
        self.metrics.write(final=True, **summary.as_dict(), **extra)
        if cfg.ckpt:
            self.save_checkpoint(cfg.ckpt)
        self.metrics.close()
        return summary

    def _health(self, where: str) -> None:
        """Every rank stops when any rank's xGMI barrier timed out (the later
        barriers of that communicator stop waiting: training on would read the
        peers' buffers unsynchronised); a vote, so all ranks raise together."""
        if self.world > 1:
            check_health(where, self.comm, self.engine)

    def save_checkpoint(self, path: str) -> None:
        self._health("before a checkpoint")
        self.engine.sync_optimizer_state()  # sharded FC momentum -> whole buffer
        if self.rank == 0:
            eng = self.engine
            meta = {"model": self.cfg.model, "world": self.world,
                    "sync_schedule": self.sync_schedule()}
            extra = dict(eng.extra_state())
            if eng.ema is not None:  # <tf_name>/ExponentialMovingAverage + the spec
                extra.update(ckpt_mod.ema_arrays(eng.layout, eng.ema))
                meta[ckpt_mod.EMA_META] = self.cfg.ema
            ckpt_mod.save(path, eng.layout, eng.params, eng.mom, eng.step, meta=meta, extra=extra)
        D.barrier()
