"""Global configuration: the reference's hard-coded constants plus CLI overrides.

The reference keeps every knob as a module global or an inline literal
(`/root/reference/mpipy.py:14-21` globals, `:57` L2 coefficient, `:60-64`
learning-rate schedule, `:65` momentum, `:87` sync period, `:166` dropout).
This module mirrors those defaults exactly and exposes them through one
dataclass (`TrainConfig`) plus an argparse builder, so the one-script API
(`mpipy.py`) keeps the reference defaults while every value is overridable.

`--reference-quirks` re-enables the reference's behavioural oddities that
the framework fixes by default:
  * Q5  - train shard padded with zero rows (tr_size//P rows, 5000/P zeros)
  * Q8  - dropout stays active at evaluation time
  * Q9  - full local test-set evaluation after every training step
  * Q11 - "bcast" = gather weights (not biases/momentum) to rank 0 and
          average there only; other ranks never receive the average
  * Q14 - identical dropout seeds on every rank
"""

from __future__ import annotations

import argparse
import dataclasses
import os
from typing import List, Optional

# --- reference constants (mpipy.py:14-21) -------------------------------
# mpipy.py:14 sets TF_CPP_MIN_LOG_LEVEL=2 and :15 MPI_OPTIMAL_PATH=1; the
# equivalents here are log verbosity knobs, not environment variables.
DATA_URL = "https://storage.googleapis.com/cvdf-datasets/mnist/"  # mpipy.py:17
ITERATION = 2  # epochs over the local shard, mpipy.py:18
IMAGE_SIZE = 28  # mpipy.py:19
BATCH_SIZE = 64  # per-rank batch, mpipy.py:20
NUM_CHANNEL = 10  # number of classes (named "channel" in mpipy.py:21)
NUM_CLASSES = NUM_CHANNEL
PIXEL_DEPTH = 255.0  # tutorial extract_data scaling: (x - 127.5) / 255

# --- optimisation constants (mpipy.py:57-66) ------------------------------
BASE_LR = 0.01  # mpipy.py:60
LR_DECAY = 0.95  # mpipy.py:63
MOMENTUM = 0.9  # mpipy.py:65
L2_COEF = 5e-4  # mpipy.py:57
DROPOUT_KEEP = 0.5  # mpipy.py:166
SEED = 1  # op seed of every truncated_normal and the dropout, mpipy.py:40,166
INIT_STDDEV = 0.1  # mpipy.py:39

# --- distributed constants ----------------------------------------------------
SYNC_EVERY = 50  # mpipy.py:87 (step>0 and step%50==0)
TRAIN_ROWS = 55000  # mpipy.py:211 (tr_size before rounding)
TEST_ROWS = 10000  # mpipy.py:212
VAL_ROWS = 5000  # mpipy.py:213
TRAIN_FILE_ROWS = 60000  # mpipy.py:216 (extract 60000 train images)

MNIST_FILES = {
    "train_images": "train-images-idx3-ubyte.gz",  # mpipy.py:203
    "train_labels": "train-labels-idx1-ubyte.gz",  # mpipy.py:204
    "test_images": "t10k-images-idx3-ubyte.gz",  # mpipy.py:205
    "test_labels": "t10k-labels-idx1-ubyte.gz",  # mpipy.py:206
}

MODELS = ("mnist_cnn", "lenet5", "resnet18")
SYNC_MODES = ("grad", "param_avg", "none")
# gradient-sync schedules of the native MNIST executor (grad sync, world > 1):
# "buckets" = all-reduce FC bucket then conv bucket; "sharded" = reduce-scatter
# FC grads + 1/N-shard SGD + all-gather overlapped with the next forward
# "split" = FC all-reduce + SGD on the comm stream, conv all-reduce on the
# compute stream over a second communicator
# "xgmi" = the peer-to-peer xGMI communicator's fused sync + SGD launch (MNIST,
# csrc/xgmi_comm.h; one node)
SYNC_SCHEDULES = ("auto", "buckets", "sharded", "split", "factors", "serial", "defer", "xgmi",
                  "xgmi-step", "xgmi-fac")
# device communicator (world > 1): "auto" = native RCCL when every rank has a
# GPU of its own, the shared-memory host-staged communicator when ranks share
# GPUs (the reference's layout: every rank on /GPU:0, quirk Q13); "rccl",
# "shm" and "torch" (torch.distributed) force one
# "xgmi": collectives as compute-stream kernels reading the peers' memory
# over the xGMI mesh (IPC-mapped; one node)
COMMS = ("auto", "rccl", "shm", "xgmi", "torch")
# LeNet-5's sync over the xGMI communicator (TrainConfig.xgmi_mode)
XGMI_MODES = ("two-phase", "push", "pull")
DTYPES = ("fp32", "bf16")
# --augment: what is shifted in from outside the image unless the spec says
# fill:V.  MNIST: the normalised raw 0 pixel, (0 - 127.5) / 255; the others:
# zero-padding of a centred image
AUGMENT_FILL = {"mnist_cnn": -0.5, "lenet5": 0.0, "resnet18": 0.0}
# --predict SRC: the words that name this configuration's own splits (anything
# else is a file), and the largest test-time-augmentation shift (shift:3 with
# flip is already 98 forwards per row)
PREDICT_SPLITS = ("test", "val")
MAX_TTA_SHIFT = 3
# --predict-weights: the trained weights, or their moving average (--ema)
PREDICT_WEIGHTS = ("raw", "ema")


MAX_ROTATE, MAX_SCALE = 45.0, 50.0  # degrees, percent: the largest rotate:D and scale:P


@dataclasses.dataclass(frozen=True)
class AugmentSpec:
    """A parsed --augment spec; rotate / scale / cutout are 0 when absent."""
    K: int
    flip: bool
    fill: float
    rotate: float = 0.0  # degrees either way
    scale: float = 0.0   # percent either way
    cutout: int = 0      # side of the erased square

    @property
    def affine(self) -> bool:
        """Needs the affine load (rotate, scale or cutout), not only shift / flip."""
        return self.rotate > 0 or self.scale > 0 or self.cutout > 0


def parse_augment_spec(spec: str, model: str = "mnist_cnn") -> AugmentSpec:
    """`shift:K` (K >= 1), `flip`, `rotate:D` (0 < D <= 45 degrees), `scale:P`
    (0 < P <= 50 percent), `cutout:S` (S >= 1) and optionally `fill:V`, comma
    separated, in any order, each at most once, at least one of the first five."""
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError("empty augment spec; expected e.g. 'shift:2', 'shift:4,flip', 'flip', "
                         "'shift:2,rotate:10,scale:10'")
    seen = {}
    for item in spec.split(","):
        name, sep, val = item.strip().partition(":")
        if name in seen:
            raise ValueError(f"augment spec {spec!r} names {name!r} twice")
        try:
            if name in ("shift", "cutout") and sep:
                seen[name] = int(val)
            elif name in ("fill", "rotate", "scale") and sep:
                seen[name] = float(val)
                if seen[name] != seen[name] or abs(seen[name]) == float("inf"):
                    raise ValueError
            elif name == "flip" and not sep:
                seen[name] = True
            else:
                raise ValueError
        except ValueError:
            raise ValueError(f"bad item {item!r} in augment spec {spec!r}; expected shift:K, "
                             f"flip, rotate:D, scale:P, cutout:S or fill:V") from None
    K = seen.get("shift", 0)
    if "shift" in seen and K < 1:
        raise ValueError(f"augment shift must be at least 1, got {K}")
    if "rotate" in seen and not 0.0 < seen["rotate"] <= MAX_ROTATE:
        raise ValueError(f"augment rotate must be in (0, {MAX_ROTATE:g}] degrees, got "
                         f"{seen['rotate']:g}")
    if "scale" in seen and not 0.0 < seen["scale"] <= MAX_SCALE:
        raise ValueError(f"augment scale must be in (0, {MAX_SCALE:g}] percent, got "
                         f"{seen['scale']:g}")
    if "cutout" in seen and seen["cutout"] < 1:
        raise ValueError(f"augment cutout must be at least 1, got {seen['cutout']}")
    if not any(k in seen for k in ("shift", "flip", "rotate", "scale", "cutout")):
        raise ValueError(f"augment spec {spec!r} asks for none of shift, flip, rotate, scale, "
                         f"cutout")
    return AugmentSpec(K, "flip" in seen, float(seen.get("fill", AUGMENT_FILL.get(model, 0.0))),
                       seen.get("rotate", 0.0), seen.get("scale", 0.0), seen.get("cutout", 0))


def parse_augment(spec: str, model: str = "mnist_cnn"):
    """The shift / flip subset of `parse_augment_spec` (test-time augmentation
    takes no other item) -> (K, flip, fill); K = 0 without a shift."""
    s = parse_augment_spec(spec, model)
    if s.affine:
        raise ValueError(f"augment spec {spec!r}: rotate, scale and cutout are training-only "
                         f"(--augment); here only shift:K, flip and fill:V apply")
    return s.K, s.flip, s.fill


def parse_ema(spec: str):
    """`DECAY` (a float, 0 < DECAY < 1) and optionally `every:K` (K >= 1), comma
    separated, in any order, each at most once -> (decay, K); K = 1 without
    an `every` (the definition: docs/ACCURACY.md)."""
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError("empty ema spec; expected e.g. '0.999', '0.99,every:4'")
    seen = {}
    for item in spec.split(","):
        name, sep, val = item.strip().partition(":")
        key = "every" if sep else "decay"
        try:
            if sep and name == "every":
                v = int(val)
            elif not sep:
                v = float(name)
            else:
                raise ValueError
        except ValueError:
            raise ValueError(f"bad item {item!r} in ema spec {spec!r}; expected DECAY or "
                             f"every:K") from None
        if key in seen:
            raise ValueError(f"ema spec {spec!r} names {key!r} twice")
        seen[key] = v
    if "decay" not in seen:
        raise ValueError(f"ema spec {spec!r} names no decay")
    decay, K = seen["decay"], seen.get("every", 1)
    if not 0.0 < decay < 1.0:  # (false for nan)
        raise ValueError(f"ema decay must be in (0, 1), got {decay}")
    if K < 1:
        raise ValueError(f"ema every must be at least 1, got {K}")
    return float(decay), int(K)


MAX_MIX = 50.0  # percent: the largest share --mix gives the partner row
MIX_KINDS = ("mixup", "cutmix")


def parse_mix(spec: str):
    """`mixup:M` or `cutmix:M` (exactly one; M a float in percent, 0 < M <= 50:
    the largest share of the partner row) -> (kind, M); the definition:
    docs/ACCURACY.md."""
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError("empty mix spec; expected e.g. 'mixup:50', 'cutmix:25'")
    seen = {}
    for item in spec.split(","):
        name, sep, val = item.strip().partition(":")
        try:
            if name not in MIX_KINDS or not sep:
                raise ValueError
            v = float(val)
            if v != v or abs(v) == float("inf"):
                raise ValueError
        except ValueError:
            raise ValueError(f"bad item {item!r} in mix spec {spec!r}; expected mixup:M or "
                             f"cutmix:M") from None
        if name in seen:
            raise ValueError(f"mix spec {spec!r} names {name!r} twice")
        seen[name] = v
    if len(seen) != 1:
        raise ValueError(f"mix spec {spec!r} names both mixup and cutmix; a run mixes one way")
    (kind, M), = seen.items()
    if not 0.0 < M <= MAX_MIX:
        raise ValueError(f"mix {kind} must be in (0, {MAX_MIX:g}] percent, got {M:g}")
    return kind, float(M)


def check_label_smoothing(eps) -> float:
    """--label-smoothing EPS: a float with 0 <= EPS < 1."""
    try:
        v = float(eps)
    except (TypeError, ValueError):
        raise ValueError(f"label smoothing must be a float, got {eps!r}") from None
    if not 0.0 <= v < 1.0:  # (false for nan)
        raise ValueError(f"label smoothing must be in [0, 1), got {v:g}")
    return v


@dataclasses.dataclass
class TrainConfig:
    """Every knob of a training run.  Defaults = the reference's behaviour
    with its bugs fixed (see module docstring for the quirk switch)."""

    model: str = "mnist_cnn"
    epochs: int = ITERATION
    batch_size: int = BATCH_SIZE
    dtype: str = "fp32"
    # gradient all-reduce every step (default, arXiv:1603.02339 intent) or the
    # reference's periodic weight averaging (mpipy.py:87-91)
    sync: str = "grad"
    sync_every: int = SYNC_EVERY
    sync_schedule: str = "auto"
    # "defer" schedule: fraction of the FC bucket all-reduced under the conv
    # backward (the rest overlaps the next step's conv forward)
    defer_split: float = 0.5
    # dtype of the gradient collectives: fp32 (the reference's MPI Gather of
    # fp32 tensors) or bf16 (half the bytes over xGMI; the sum is rounded to
    # bf16 on the wire, the update stays fp32)
    grad_comm_dtype: str = "fp32"
    # generic models (ResNet-18): how the flat gradients are cut into
    # all-reduce buckets (parallel/overlap.py plan_layout); "auto" times the
    # BUCKET_PLANS candidates on the real communicator at startup
    bucket_plan: str = "auto"
    comm: str = "auto"
    # comm auto, one node: do not set up the xGMI peer-to-peer communicator as
    # an extra sync-schedule candidate (parallel/setup.py setup_comms)
    no_xgmi: bool = False
    # LeNet-5 over the xGMI communicator (--comm xgmi): "two-phase" (this
    # rank's segment summed + SGD, then the others gathered; sharded momentum),
    # "push" (the gradient pushed into the peers' receive slots from the update
    # launch, one barrier, kernels/lenet.h PushArgs) or "pull" (double-buffered
    # gradient slots, one launch reads every rank's whole gradient, one
    # barrier, replicated SGD; kernels/xgmi.h OneShotArgs); with --comm auto
    # all three are tuned next to RCCL.  Default pull: emulated 8 ranks at
    # 1 us / 150 GB/s 34.97 us a step against 42.31 two-phase, 44.1 push
    xgmi_mode: str = "pull"
    # fp32 MNIST conv2 algorithm on the native engine: "winograd" (F(2x2,5x5),
    # kernels/wino.h; 2.8x fewer MFMAs, fp32 arithmetic throughout, ~1e-6
    # relative error) or "direct" (25-tap implicit GEMM)
    conv_algo: str = "winograd"
    # restrict sync_schedule="auto" to the schedules whose updates are bit
    # identical to the bucketed all-reduce (the factor schedule sums the FC
    # gradients in another order, so an auto run that picked it is only
    # reproducible by naming it; the chosen schedule is logged either way)
    deterministic: bool = False
    # evaluate (and print the reference log line) every N steps; the
    # reference evaluates every step (Q9) but prints every 50
    eval_every: int = SYNC_EVERY
    # data
    data_dir: str = "data"
    synthetic: Optional[bool] = None  # None = use real files if present
    download: bool = False
    # a new row order for every pass over the local shard (runtime/shuffle.py);
    # off = the reference's file order (mpipy.py:80), the same batches every pass
    shuffle: bool = False
    # per-pass random shift / horizontal flip / rotation / zoom / cutout of the
    # training images, redrawn for every row and pass on the device
    # (parse_augment_spec, runtime/shuffle.py);
    # None = every pass shows the same pixels
    augment: Optional[str] = None
    # exponential moving average of the weights, updated on the device after
    # every K-th step (parse_ema: DECAY[,every:K]), evaluated at every logged
    # eval event, saved with the checkpoints; None = no average is kept
    ema: Optional[str] = None
    # soft training targets (docs/ACCURACY.md): label smoothing EPS, the target
    # (1 - EPS) onehot + EPS / classes; 0 = the hard label, nothing extra runs
    label_smoothing: float = 0.0
    # mixup:M / cutmix:M (parse_mix): every training row blended with, or given
    # a box of, a partner row of its pass, redrawn each pass on the device; the
    # target is the same blend of the two labels; None = rows stay apart
    mix: Optional[str] = None
    # learning rate / optimiser
    base_lr: float = BASE_LR
    lr_decay: float = LR_DECAY
    momentum: float = MOMENTUM
    l2: float = L2_COEF
    dropout_keep: float = DROPOUT_KEEP
    seed: int = SEED
    # execution
    backend: str = "auto"  # auto | native (HIP kernels) | torch (oracle path)
    device: str = "auto"  # auto | cpu | cuda
    graph: bool = True  # capture the step into a HIP graph (native backend)
    graph_steps: int = 10  # training steps per captured graph replay
    max_steps: Optional[int] = None  # cap on steps (None = epochs-derived)
    # checkpoint / metrics
    ckpt: Optional[str] = None
    ckpt_every: int = 0
    resume: Optional[str] = None
    metrics_jsonl: Optional[str] = None
    # at every logged eval event and at the end: held-out loss, top-3 error,
    # confusion matrix of the test split and the validation split's error /
    # loss, summed over the ranks (utils/metrics.py, Trainer.evaluate_metrics)
    eval_metrics: bool = False
    # checkpoint written whenever the global validation error improves
    # (strictly); implies eval_metrics
    ckpt_best: Optional[str] = None
    # inference instead of training (runtime/predict.py): classify SRC - an
    # IDX ubyte image file (raw or gzip), a .npy of uint8 / float32 rows, or
    # "test" / "val" for this configuration's own split - with the checkpoint
    # --resume; no Trainer is built
    predict: Optional[str] = None
    predict_labels: Optional[str] = None  # IDX / .npy labels of a file SRC: adds the metrics
    predict_out: Optional[str] = None  # .npz of pred / topk_class / topk_prob [/ probs]
    predict_topk: int = 3
    predict_tta: Optional[str] = None  # test-time augmentation views, parse_augment syntax
    predict_probs: bool = False
    # raw | ema: the checkpoint's trained weights or their moving average (--ema);
    # None = raw, not named (the JSON record then has no "weights" entry)
    predict_weights: Optional[str] = None
    quiet: bool = False
    # robustness: process-group / collective timeout (a dead rank turns into
    # an error instead of a hang) and a cross-replica consistency probe at
    # every eval event in grad-sync mode (replicas must stay identical)
    collective_timeout_s: float = 600.0
    check_replicas: bool = False
    # compat
    reference_quirks: bool = False

    def validate(self) -> "TrainConfig":
        if self.model not in MODELS:
            raise ValueError(f"unknown model {self.model!r}; choose from {MODELS}")
        if self.sync not in SYNC_MODES:
            raise ValueError(f"unknown sync {self.sync!r}; choose from {SYNC_MODES}")
        if self.xgmi_mode not in XGMI_MODES:
            raise ValueError(f"unknown xgmi mode {self.xgmi_mode!r}; choose from {XGMI_MODES}")
        if self.sync_schedule not in SYNC_SCHEDULES:
            raise ValueError(f"unknown sync schedule {self.sync_schedule!r}; "
                             f"choose from {SYNC_SCHEDULES}")
        if not 0.0 < self.defer_split < 1.0:
            raise ValueError(f"defer_split must be in (0, 1), got {self.defer_split}")
        if self.grad_comm_dtype not in ("fp32", "bf16"):
            raise ValueError(f"unknown grad comm dtype {self.grad_comm_dtype!r}")
        if self.bucket_plan != "auto":
            from .parallel.overlap import check_plan
            check_plan(self.bucket_plan)
        if self.conv_algo not in ("winograd", "direct"):
            raise ValueError(f"unknown conv algo {self.conv_algo!r}")
        if self.comm not in COMMS:
            raise ValueError(f"unknown comm {self.comm!r}; choose from {COMMS}")
        if self.dtype not in DTYPES:
            raise ValueError(f"unknown dtype {self.dtype!r}; choose from {DTYPES}")
        if self.backend not in ("auto", "native", "torch"):
            raise ValueError(f"unknown backend {self.backend!r}")
        if self.batch_size <= 0 or self.epochs <= 0:
            raise ValueError("batch_size and epochs must be positive")
        if self.sync_every <= 0 or self.eval_every < 0:
            raise ValueError("sync_every must be > 0 and eval_every >= 0")
        if not 0.0 < self.dropout_keep <= 1.0:
            raise ValueError("dropout_keep must be in (0, 1]")
        if self.augment is not None:
            parse_augment_spec(self.augment, self.model)
        if self.ema is not None:
            parse_ema(self.ema)
            if self.model == "resnet18":
                raise ValueError("--ema does not support --model resnet18 (its forward lives in "
                                 "the autograd engine, and its BatchNorm statistics would need "
                                 "averaging too); use mnist_cnn or lenet5")
        self.label_smoothing = check_label_smoothing(self.label_smoothing)
        if self.mix is not None:
            parse_mix(self.mix)
        if self.predict_weights is not None and self.predict_weights not in PREDICT_WEIGHTS:
            raise ValueError(f"unknown predict weights {self.predict_weights!r}; choose from "
                             f"{PREDICT_WEIGHTS}")
        if self.ckpt_best:
            if self.model != "mnist_cnn":
                raise ValueError(f"--ckpt-best selects on the validation split, and the "
                                 f"{self.model} shards have no validation rows")
            if self.effective_eval_every() == 0:
                raise ValueError("--ckpt-best needs periodic evaluation (--eval-every > 0)")
            self.eval_metrics = True
        if self.predict is not None:
            self._validate_predict()
        elif (self.predict_labels or self.predict_out or self.predict_tta or self.predict_probs):
            raise ValueError("--predict-labels / --predict-out / --predict-tta / --predict-probs "
                             "need --predict SRC")
        elif self.predict_weights is not None:
            raise ValueError("--predict-weights needs --predict SRC")
        return self

    def _validate_predict(self) -> None:
        if self.mix is not None or self.label_smoothing > 0.0:
            raise ValueError("--predict: mix and label smoothing are training-only (--mix, "
                             "--label-smoothing); a prediction has no target to soften")
        if not self.resume:
            raise ValueError("--predict needs the checkpoint to predict with: --resume PATH")
        if self.model == "resnet18":
            raise ValueError("--predict does not support --model resnet18 (its forward lives in "
                             "the autograd engine); use mnist_cnn or lenet5")
        if not 1 <= self.predict_topk <= NUM_CLASSES:
            raise ValueError(f"--predict-topk must be in [1, {NUM_CLASSES}], got "
                             f"{self.predict_topk}")
        if self.predict_tta is not None:
            try:
                K = parse_augment(self.predict_tta, self.model)[0]
            except ValueError as e:
                raise ValueError(f"--predict-tta: {e}") from None
            if K > MAX_TTA_SHIFT:
                raise ValueError(f"--predict-tta: shift:{K} is too many views; the largest "
                                 f"shift is {MAX_TTA_SHIFT}")
        src = self.predict
        if src not in PREDICT_SPLITS and not src.endswith(".npy") and not os.path.isfile(src):
            raise ValueError(f"--predict: {src!r} is neither a file (IDX ubyte or .npy) nor one "
                             f"of the splits {PREDICT_SPLITS}")
        if self.predict_labels and src in PREDICT_SPLITS:
            raise ValueError(f"--predict-labels: --predict {src} brings its own labels")

    # quirk accessors ------------------------------------------------------
    @property
    def pad_train_shard(self) -> bool:  # Q5
        return self.reference_quirks

    @property
    def eval_dropout(self) -> bool:  # Q8
        return self.reference_quirks

    @property
    def root_only_average(self) -> bool:  # Q11
        return self.reference_quirks

    @property
    def same_seed_all_ranks(self) -> bool:  # Q14
        return self.reference_quirks

    def effective_eval_every(self) -> int:  # Q9
        return 1 if self.reference_quirks else self.eval_every


def build_arg_parser(prog: str = "mpipy.py") -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        prog=prog,
        description="MI355X-native data-parallel CNN trainer (reference-compatible "
        "one-script API of mpi-Tensorflow's mpipy.py).",
    )
    d = TrainConfig()
    p.add_argument("--model", default=d.model, choices=MODELS)
    p.add_argument("--epochs", type=int, default=d.epochs, help="local epochs (mpipy.py:18)")
    p.add_argument("--batch-size", type=int, default=d.batch_size,
                   help="rows per step and rank (mpipy.py:20), any positive size; the native "
                        "MNIST engine computes ceil(B / 32) * 32 rows a step, the rows past B "
                        "adding nothing to the gradients")
    p.add_argument("--dtype", default=d.dtype, choices=DTYPES)
    p.add_argument("--sync", default=d.sync, choices=SYNC_MODES)
    p.add_argument("--sync-every", type=int, default=d.sync_every)
    p.add_argument("--sync-schedule", default=d.sync_schedule, choices=SYNC_SCHEDULES,
                   help="native MNIST grad-sync schedule (auto / buckets / sharded FC update / "
                        "factors: all-gather the FC gradient factors, fp32 / defer: FC part B "
                        "overlaps the next conv forward, fp32)")
    p.add_argument("--defer-split", type=float, default=d.defer_split,
                   help="defer schedule: fraction of the FC bucket reduced under the conv backward")
    p.add_argument("--grad-comm-dtype", default=d.grad_comm_dtype, choices=("fp32", "bf16"),
                   help="wire dtype of the gradient all-reduce (bf16 halves the xGMI bytes)")
    p.add_argument("--bucket-plan", default=d.bucket_plan,
                   help="generic models: gradient all-reduce buckets (auto / layout / one / "
                        "bytes:MiB / geo:RATIO)")
    p.add_argument("--comm", default=d.comm, choices=COMMS,
                   help="device communicator: RCCL over xGMI (one GPU per rank), shm (host-"
                        "staged shared memory, ranks may share a GPU), xgmi (peer-to-peer "
                        "kernels on the compute stream, one node) or torch.distributed")
    p.add_argument("--no-xgmi", action="store_true",
                   help="comm auto: do not set up the xGMI peer-to-peer communicator "
                        "(otherwise gated by an exactness check, then tuned next to RCCL)")
    p.add_argument("--conv-algo", default=d.conv_algo, choices=("winograd", "direct"),
                   help="fp32 MNIST conv2 algorithm of the native engine")
    p.add_argument("--deterministic", action="store_true",
                   help="sync-schedule auto-tune picks only bit-identical schedules")
    p.add_argument("--eval-every", type=int, default=d.eval_every,
                   help="0 disables periodic eval")
    p.add_argument("--data-dir", default=d.data_dir)
    g = p.add_mutually_exclusive_group()
    g.add_argument("--synthetic", dest="synthetic", action="store_true", default=None)
    g.add_argument("--real-data", dest="synthetic", action="store_false")
    p.add_argument("--download", action="store_true", help="try DATA_URL if files missing")
    p.add_argument("--shuffle", action="store_true",
                   help="permute each rank's shard anew for every pass (on the device, a pure "
                        "function of seed, rank and pass; the reference reads in file order)")
    p.add_argument("--augment", default=d.augment, metavar="SPEC",
                   help="random shift, horizontal flip, rotation, zoom and erased square of every "
                        "training image, redrawn each pass on the device: any of shift:K, flip, "
                        "rotate:D (degrees either way, at most 45), scale:P (percent either way, "
                        "at most 50), cutout:S (an S x S square), and fill:V (the value shifted, "
                        "turned or cut in, default -0.5 for mnist_cnn, 0 otherwise)")
    p.add_argument("--ema", default=d.ema, metavar="SPEC",
                   help="keep an exponential moving average of the weights on the device: "
                        "DECAY[,every:K] (0 < DECAY < 1, updated after every K-th step with TF's "
                        "num_updates warm-up); evaluated at every logged eval event, saved with "
                        "the checkpoints (mnist_cnn, lenet5)")
    p.add_argument("--label-smoothing", type=float, default=d.label_smoothing, metavar="EPS",
                   help="train against (1 - EPS) onehot + EPS / classes, 0 <= EPS < 1 (0: the "
                        "hard label, the default); evaluation is untouched")
    p.add_argument("--mix", default=d.mix, metavar="SPEC",
                   help="mixup:M or cutmix:M (0 < M <= 50 percent, the largest share of the "
                        "partner row): every training row is blended with (mixup), or gets a box "
                        "of (cutmix), another row of its pass, redrawn each pass on the device; "
                        "the target blends the two labels alike (mixup:50 is the usual mixup)")
    p.add_argument("--base-lr", type=float, default=d.base_lr)
    p.add_argument("--lr-decay", type=float, default=d.lr_decay)
    p.add_argument("--momentum", type=float, default=d.momentum)
    p.add_argument("--l2", type=float, default=d.l2)
    p.add_argument("--dropout-keep", type=float, default=d.dropout_keep)
    p.add_argument("--seed", type=int, default=d.seed)
    p.add_argument("--backend", default=d.backend, choices=("auto", "native", "torch"))
    p.add_argument("--device", default=d.device)
    p.add_argument("--no-graph", dest="graph", action="store_false", default=True)
    p.add_argument("--graph-steps", type=int, default=d.graph_steps)
    p.add_argument("--max-steps", type=int, default=None)
    p.add_argument("--ckpt", default=None, help="checkpoint path written at the end")
    p.add_argument("--ckpt-every", type=int, default=0)
    p.add_argument("--resume", default=None)
    p.add_argument("--metrics-jsonl", default=None)
    p.add_argument("--eval-metrics", action="store_true",
                   help="at every logged eval event and at the end: test loss, top-3 error and "
                        "confusion matrix, validation error and loss, summed over the ranks "
                        "(one extra log line on rank 0, extra keys in --metrics-jsonl)")
    p.add_argument("--ckpt-best", default=None, metavar="PATH",
                   help="write the checkpoint there whenever the global validation error "
                        "improves (implies --eval-metrics; mnist_cnn, --eval-every > 0); "
                        "with --ema the selection stays on the raw weights")
    p.add_argument("--predict", default=None, metavar="SRC",
                   help="no training: classify SRC with the checkpoint --resume. SRC: an IDX "
                        "ubyte image file (raw or gzip), a .npy of uint8 or float32 rows, or "
                        "'test' / 'val' = this configuration's own split with its labels")
    p.add_argument("--predict-labels", default=None, metavar="PATH",
                   help="labels of a file SRC (IDX ubyte or .npy): adds error, loss, top-3 error "
                        "and the confusion matrix")
    p.add_argument("--predict-out", default=None, metavar="PATH.npz",
                   help="write pred, topk_class and topk_prob there (rank 0)")
    p.add_argument("--predict-topk", type=int, default=d.predict_topk, metavar="K")
    p.add_argument("--predict-tta", default=None, metavar="SPEC",
                   help="test-time augmentation: average the softmax over every view of "
                        "shift:K[,flip][,fill:V] (K <= 3; (2K+1)^2 views, twice with flip)")
    p.add_argument("--predict-probs", action="store_true",
                   help="--predict-out also holds the class probabilities [n, 10]")
    p.add_argument("--predict-weights", default=d.predict_weights, choices=PREDICT_WEIGHTS,
                   help="predict with the checkpoint's trained weights (raw, the default) or with "
                        "their moving average (ema: a checkpoint of an --ema run); when given, "
                        "the JSON record names it under \"weights\"")
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--collective-timeout-s", type=float, default=d.collective_timeout_s,
                   help="process-group / collective timeout (seconds)")
    p.add_argument("--check-replicas", action="store_true",
                   help="verify at every eval that all ranks hold identical weights (grad sync)")
    p.add_argument("--reference-quirks", action="store_true",
                   help="reproduce mpipy.py quirks Q5/Q8/Q9/Q11/Q14")
    return p


def config_from_args(argv: Optional[List[str]] = None, prog: str = "mpipy.py") -> TrainConfig:
    ns = build_arg_parser(prog).parse_args(argv)
    kw = {f.name: getattr(ns, f.name) for f in dataclasses.fields(TrainConfig) if hasattr(ns, f.name)}
    return TrainConfig(**kw).validate()


def env_flag(name: str, default: bool = False) -> bool:
    v = os.environ.get(name)
    if v is None:
        return default
    return v.strip().lower() not in ("", "0", "false", "no", "off")
