"""Inference from a checkpoint: `Predictor`, and `predict_main` behind
`mpipy.py --predict`.

A `Predictor` holds the flat parameter buffer of a trained model and nothing
of training: no shard, no communicator, no gradient / momentum / backward
buffers, no graphs, no extra streams.  On the GPU a chunk of rows goes through

    predict_prep  (uint8 -> fp32 normalisation and / or one test-time-
                   augmentation view; csrc/kernels/predict.hip)
    eval_chunk    the engines' own static forward (MnistExecutor /
                   LenetExecutor): the same launches on the same operands as
                   `engine.evaluate`, so the logits are bit-identical to it
    predict_head  softmax, the mean over the views, scores and top-k

once per view, one head launch per view and chunk.  On the CPU (and with
backend="torch") the models' torch forward and the torch oracles of the two
ops compute the same definitions: the oracle and the CPU user path.

Test-time augmentation takes the `--augment` syntax (config.parse_augment):
`shift:K[,flip][,fill:V]` enumerates every (flip, dy, dx) with dy, dx in
[-K, K] in the fixed order v = (f (2K+1) + dy + K) (2K+1) + dx + K, so the
mean over the views is reproducible; the identity view is there exactly once.
"""

from __future__ import annotations

import dataclasses
import os
import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import config as C
from ..ops import functional as Fn
from ..ops import native, ptr, stream_handle
from ..parallel import dist as D
from ..utils import checkpoint as ckpt_mod
from ..utils.metrics import EvalMetrics

PREDICT_MODELS = ("mnist_cnn", "lenet5")


def tta_views(spec: Optional[str], model: str = "mnist_cnn") -> Tuple[List[Tuple[int, int, bool]], float]:
    """([(dy, dx, flip)] in view order, fill) of a TTA spec; None = the identity."""
    if spec is None:
        return [(0, 0, False)], 0.0
    K, flip, fill = C.parse_augment(spec, model)
    if K > C.MAX_TTA_SHIFT:
        raise ValueError(f"TTA shift:{K} is {(2 * K + 1) ** 2 * (2 if flip else 1)} forwards per "
                         f"row; the largest shift is {C.MAX_TTA_SHIFT}")
    span = range(-K, K + 1)
    return [(dy, dx, bool(f)) for f in range(2 if flip else 1) for dy in span for dx in span], fill


def input_shape(model: str) -> Tuple[int, int, int]:
    if model == "mnist_cnn":
        return (C.IMAGE_SIZE, C.IMAGE_SIZE, 1)
    from ..models.generic import model_input_shape

    return model_input_shape(model)


def _check_model(model: str) -> None:
    if model == "resnet18":
        raise ValueError("Predictor does not support resnet18: its forward lives in the autograd "
                         f"engine; supported models: {PREDICT_MODELS}")
    if model not in PREDICT_MODELS:
        raise ValueError(f"unknown model {model!r}; Predictor supports {PREDICT_MODELS}")


def _layout_of(model: str):
    if model == "mnist_cnn":
        from ..models import mnist_cnn as M

        return M.layout(), None
    from ..models.generic import make_model

    m = make_model(model)
    return m.layout, m


@dataclasses.dataclass
class PredictResult:
    """Tensors on the predictor's device.  `scores` is what Fn.eval_metrics
    reads as logits: the logits themselves with one view, else log(probs)."""

    pred: torch.Tensor  # int32 [n] = topk_class[:, 0]
    topk_class: torch.Tensor  # int32 [n, k]
    topk_prob: torch.Tensor  # fp32 [n, k]
    scores: torch.Tensor  # fp32 [n, C]
    n: int
    views: int
    seconds: float  # the device work between two synchronisations (no file reads)
    probs: Optional[torch.Tensor] = None  # fp32 [n, C] (return_probs)
    metrics: Optional[EvalMetrics] = None  # with labels

    def numpy(self) -> Dict[str, np.ndarray]:
        out = {"pred": self.pred, "topk_class": self.topk_class, "topk_prob": self.topk_prob}
        if self.probs is not None:
            out["probs"] = self.probs
        return {k: v.detach().cpu().numpy() for k, v in out.items()}


class Predictor:
    def __init__(self, model: str, params: torch.Tensor, dtype: str = "fp32",
                 backend: str = "auto", step: int = 0, meta: Optional[Dict[str, str]] = None,
                 weights: str = "raw"):
        """`params`: the flat fp32 parameter buffer in the model's layout, on
        the device the predictions run on (used in place).  `weights` names
        what it holds: the trained weights ("raw") or their moving average
        ("ema", --ema); the forward is the same."""
        if weights not in C.PREDICT_WEIGHTS:
            raise ValueError(f"unknown weights {weights!r}; choose from {C.PREDICT_WEIGHTS}")
        self.weights = weights
        _check_model(model)
        if dtype not in C.DTYPES:
            raise ValueError(f"unknown dtype {dtype!r}; choose from {C.DTYPES}")
        if backend not in ("auto", "native", "torch"):
            raise ValueError(f"unknown backend {backend!r}")
        self.model, self.dtype = model, dtype
        self.layout, self._generic = _layout_of(model)
        self.device = params.device
        if backend == "auto":
            backend = "native" if self.device.type == "cuda" else "torch"
        if backend == "native" and self.device.type != "cuda":
            raise RuntimeError("the native Predictor needs a GPU")
        if dtype != "fp32" and (backend != "native" or model != "mnist_cnn"):
            raise NotImplementedError(f"dtype {dtype} needs the native (GPU) MNIST forward")
        self.backend = backend
        if params.dtype != torch.float32 or params.dim() != 1 or params.numel() != self.layout.total:
            raise ValueError(f"params must be the flat fp32 buffer of {self.layout.total} floats")
        self.params = params.detach()
        self.step, self.meta = int(step), dict(meta or {})
        self.shape = input_shape(model)
        self.classes = C.NUM_CLASSES
        self.bf16 = dtype == "bf16"
        self._ws: Optional[tuple] = None
        self._eval_out: Optional[tuple] = None
        self._shadows = None
        if backend == "native":
            self._C = native()
            self.ptrs = self._make_ptrs()

    # ---------------------------------------------------------- construction
    @classmethod
    def from_checkpoint(cls, path: str, model: Optional[str] = None, dtype: str = "fp32",
                        device: str = "auto", backend: str = "auto",
                        weights: str = "raw") -> "Predictor":
        """A checkpoint of utils/checkpoint.py, written at any world size (the
        LR schedule and the shards its `world` entry guards do not apply
        here); momentum slots are not read.  weights="ema": the moving
        average an --ema run saved (`<name>/ExponentialMovingAverage`)
        instead of the trained weights."""
        if weights not in C.PREDICT_WEIGHTS:
            raise ValueError(f"unknown weights {weights!r}; choose from {C.PREDICT_WEIGHTS}")
        suffix = ckpt_mod.EMA_SUFFIX if weights == "ema" else ""
        dev = D.resolve_device(device) if not isinstance(device, torch.device) else device
        with np.load(path, allow_pickle=False) as z:
            meta = {k[len(ckpt_mod.META_PREFIX):]: str(z[k]) for k in z.files
                    if k.startswith(ckpt_mod.META_PREFIX) and k != ckpt_mod.STEP_META}
            saved = meta.get("model")
            if model is not None:
                _check_model(model)
            if model is None:
                model = saved or "mnist_cnn"
            elif saved is not None and saved != model:
                raise ValueError(f"{path}: saved model={saved} but model={model} was asked for")
            _check_model(model)
            layout, _ = _layout_of(model)
            host = torch.zeros(layout.total, dtype=torch.float32)
            views = layout.views(host)
            for s in layout.specs:
                key = s.tf_name + suffix
                if key not in z.files:
                    raise ValueError(f"{path}: missing {key} ({s.name})" + (
                        "; the checkpoint was written without --ema" if suffix else ""))
                w = z[key]
                if tuple(w.shape) != tuple(s.shape):
                    raise ValueError(f"{path}: {key} ({s.name}) has shape {w.shape}, "
                                     f"expected {s.shape}")
                views[s.name].copy_(torch.from_numpy(np.ascontiguousarray(w, np.float32)))
            if ckpt_mod.STEP_META in z.files:
                step = int(z[ckpt_mod.STEP_META])
            else:
                step = int(float(z[ckpt_mod.STEP_NAME])) if ckpt_mod.STEP_NAME in z.files else 0
        return cls(model, host.to(dev), dtype, backend, step, meta, weights)

    @classmethod
    def from_engine(cls, engine, weights: str = "raw") -> "Predictor":
        """Shares the engine's parameter buffer (zero copy): later training
        steps and in-place writes show in the next predict().  weights="ema":
        the engine's moving average (cfg.ema) instead, shared the same way."""
        cfg = engine.cfg
        buf = engine.params
        if weights == "ema":
            buf = getattr(engine, "ema", None)
            if buf is None:
                raise ValueError("the engine keeps no moving average (it was built without --ema)")
        native_kind = str(getattr(engine, "kind", "")).startswith("native")
        dtype = "bf16" if getattr(engine, "bf16", False) and cfg.model == "mnist_cnn" else "fp32"
        return cls(cfg.model, buf, dtype, "native" if native_kind else "torch",
                   step=getattr(engine, "step", 0), meta={"model": cfg.model}, weights=weights)

    def _make_ptrs(self):
        C_, off = self._C, self.layout.offsets
        if self.model == "lenet5":
            from .lenet_engine import _OFFSETS

            p = C_.LenetPtrs()
            o = C_.LenetOffsets()
            for attr, name in _OFFSETS:
                setattr(o, attr, off[name])
            p.params, p.total, p.off = ptr(self.params), self.layout.total, o
            return p
        from ..models import mnist_cnn as M

        p = C_.MnistPtrs()
        p.params, p.total = ptr(self.params), self.layout.total
        for attr, name in (("off_w4", "fc2_weight"), ("off_b4", "fc2_bias"), ("off_w3", "fc1_weight"),
                           ("off_b3", "fc1_bias"), ("off_w2", "conv2_weight"), ("off_b2", "conv2_bias"),
                           ("off_w1", "conv1_weight"), ("off_b1", "conv1_bias")):
            setattr(p, attr, off[name])
        p.bf16 = 1 if self.bf16 else 0
        if self.bf16:  # the four weight shadows (layouts in csrc/kernels/mnist_bf16.h)
            b16 = dict(dtype=torch.bfloat16, device=self.device)
            self._shadows = dict(w1b=torch.zeros(M.FC1_IN * M.FC1_OUT, **b16),
                                 w1t=torch.zeros(M.FC1_OUT * M.FC1_IN, **b16),
                                 w2tb=torch.zeros(25 * 64 * 32, **b16),
                                 w2b=torch.zeros(25 * 32 * 64, **b16))
            for name, t in self._shadows.items():
                setattr(p, name, ptr(t))
        return p

    # ---------------------------------------------------------------- inputs
    def _rows(self, x) -> torch.Tensor:
        t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
        if not isinstance(t, torch.Tensor):
            raise TypeError("predict takes a numpy array or a torch tensor")
        H, W, Cc = self.shape
        if t.dim() == 3 and Cc == 1:
            t = t.unsqueeze(-1)
        if t.dim() != 4 or tuple(t.shape[1:]) != (H, W, Cc):
            raise ValueError(f"{self.model} takes [n, {H}, {W}, {Cc}] rows"
                             + (f" (or [n, {H}, {W}])" if Cc == 1 else "")
                             + f", got {tuple(t.shape)}")
        if t.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"predict takes uint8 or float32 rows, got {t.dtype}")
        return t.to(self.device).contiguous()  # (a device tensor is used in place)

    def _labels(self, labels, n: int) -> Optional[torch.Tensor]:
        if labels is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(labels)) if isinstance(labels, np.ndarray) \
            else torch.as_tensor(labels)
        if t.dim() != 1 or t.shape[0] != n:
            raise ValueError(f"{n} rows but labels of shape {tuple(t.shape)}")
        return t.to(device=self.device, dtype=torch.int32).contiguous()

    # --------------------------------------------------------------- forward
    def _workspace(self, chunk: int):
        """The per-chunk workspaces, sized as NativeMnistEngine.evaluate sizes them."""
        if self._ws is not None and self._ws[0] >= chunk:
            return self._ws[1]
        from ..models import mnist_cnn as M

        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        H, W, Cc = self.shape
        ws = dict(xv=torch.empty(chunk * H * W * Cc, **f32),
                  logits=torch.empty(chunk * self.classes, **f32),
                  acc=torch.empty(chunk * self.classes, **f32),
                  y0=torch.zeros(chunk, dtype=torch.int32, device=dev))
        if self.model == "mnist_cnn":
            if self.bf16:
                cp = (chunk + 7) // 8 * 8
                b16 = dict(dtype=torch.bfloat16, device=dev)
                ws.update(a1=torch.zeros(cp * 18 * 18 * 32, **b16),
                          a2=torch.zeros(cp * M.FC1_IN, **b16),
                          h=torch.empty(chunk * M.FC1_OUT, **f32))
            else:
                ws.update(a1=torch.empty(chunk * 14 * 14 * 32, **f32),
                          a2=torch.empty(chunk * M.FC1_IN, **f32),
                          h=torch.empty(chunk * M.FC1_OUT, **f32))
        self._ws = (chunk, ws)
        return ws

    def _forward_native(self, x_ptr: int, m: int, ws, s: int) -> None:
        """logits of m fp32 rows at x_ptr into ws['logits'] (the labels are a
        zero buffer and no error counter is passed: nothing is counted here)."""
        if self.model == "lenet5":
            self._C.LenetExecutor.eval_chunk(self.ptrs, x_ptr, ptr(ws["y0"]), m, ptr(ws["logits"]),
                                             0, s)
        else:
            self._C.MnistExecutor.eval_chunk(self.ptrs, x_ptr, ptr(ws["y0"]), m, ptr(ws["a1"]),
                                             ptr(ws["a2"]), ptr(ws["h"]), ptr(ws["logits"]), 0,
                                             1.0, 0, s)

    def _forward_torch(self, xb: torch.Tensor) -> torch.Tensor:
        if self.model == "mnist_cnn":
            from ..models import mnist_cnn as M

            return M.forward(self.layout.views(self.params), xb, None)
        pv = self.layout.views(self.params)
        P = {s.name: Fn.Param(pv[s.name], None) for s in self.layout.specs}
        return self._generic.forward(P, {}, xb, False)

    @torch.no_grad()
    def predict(self, x, topk: int = 3, tta: Optional[str] = None, labels=None,
                chunk: int = 2000, return_probs: bool = False) -> PredictResult:
        """x: uint8 or float32, [n, H, W, C] (or [n, H, W] for one channel),
        numpy or torch; a tensor already on the device is used in place.  uint8
        rows are uploaded as uint8 and normalised on the device as
        utils/idx.py extract_data does on the host, bit for bit."""
        views, fill = tta_views(tta, self.model)
        V, k = len(views), int(topk)
        if not 1 <= k <= self.classes:
            raise ValueError(f"topk must be in [1, {self.classes}], got {topk}")
        if chunk < 1:
            raise ValueError("chunk must be positive")
        xd = self._rows(x)
        n = int(xd.shape[0])
        yd = self._labels(labels, n)
        dev, Cn = self.device, self.classes
        chunk = min(int(chunk), max(n, 1))
        run = self._predict_native if self.backend == "native" else self._predict_torch
        out = Fn.PredictHeadOut(torch.empty((n, Cn), device=dev), torch.empty((n, Cn), device=dev),
                                torch.empty((n, k), dtype=torch.int32, device=dev),
                                torch.empty((n, k), device=dev))
        oracle = self.backend != "native"
        mo = Fn.EvalMetricsOut(Cn, dev, oracle=oracle) if yd is not None else None
        self._sync()
        t0 = time.perf_counter()
        run(xd, yd, views, fill, k, chunk, out, mo)
        self._sync()
        seconds = time.perf_counter() - t0
        return PredictResult(pred=out.topk_class[:, 0].contiguous(), topk_class=out.topk_class,
                             topk_prob=out.topk_prob, scores=out.scores, n=n, views=V,
                             seconds=seconds, probs=out.probs if return_probs else None,
                             metrics=mo.result() if mo is not None else None)

    @torch.no_grad()
    def evaluate(self, x, labels, chunk: int = 2000) -> EvalMetrics:
        """The metrics of labelled rows, one view (what predict(x, labels=...)
        reports as `metrics`), for an evaluation that comes round again: the
        result buffers are kept for the next call with as many rows, so with
        fp32 rows and int32 labels already on the device a repeated call
        allocates no device memory."""
        xd = self._rows(x)
        n = int(xd.shape[0])
        yd = self._labels(labels, n)
        if yd is None:
            raise ValueError("evaluate needs labels")
        dev, Cn = self.device, self.classes
        oracle = self.backend != "native"
        if self._eval_out is None or self._eval_out[0] != n:
            out = Fn.PredictHeadOut(torch.empty((n, Cn), device=dev), torch.empty((n, Cn), device=dev),
                                    torch.empty((n, 1), dtype=torch.int32, device=dev),
                                    torch.empty((n, 1), device=dev))
            self._eval_out = (n, out, Fn.EvalMetricsOut(Cn, dev, oracle=oracle))
        _, out, mo = self._eval_out
        mo.zero_()
        run = self._predict_native if self.backend == "native" else self._predict_torch
        run(xd, yd, [(0, 0, False)], 0.0, 1, min(int(chunk), max(n, 1)), out, mo)
        return mo.result()

    def _sync(self) -> None:
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def _predict_native(self, xd, yd, views, fill, k, chunk, out, mo) -> None:
        V, Cn = len(views), self.classes
        H, W, Cc = self.shape
        row = H * W * Cc
        ws = self._workspace(chunk)
        s = stream_handle()
        if self.bf16:  # re-derived from the weights as they are now
            W_, off = ptr(self.params), self.layout.offsets
            sh = self._shadows
            self._C.mnist.shadows_bf16(W_ + 4 * off["fc1_weight"], W_ + 4 * off["conv2_weight"],
                                       ptr(sh["w1b"]), ptr(sh["w1t"]), ptr(sh["w2tb"]),
                                       ptr(sh["w2b"]), s)
        direct = xd.dtype == torch.float32 and V == 1 and views[0] == (0, 0, False)
        n = int(xd.shape[0])
        for a in range(0, n, chunk):
            m = min(chunk, n - a)
            part = Fn.PredictHeadOut(out.probs[a:a + m], out.scores[a:a + m],
                                     out.topk_class[a:a + m], out.topk_prob[a:a + m])
            lg = ws["logits"][:m * Cn].view(m, Cn)
            for v, (dy, dx, fl) in enumerate(views):
                if direct:
                    x_ptr = ptr(xd) + 4 * row * a
                else:
                    Fn.predict_prep(xd[a:a + m], dy, dx, fl, fill, out=ws["xv"])
                    x_ptr = ptr(ws["xv"])
                self._forward_native(x_ptr, m, ws, s)
                Fn.predict_head_view(lg, v, V, k, part, ws["acc"])
            if mo is not None:
                Fn.eval_metrics(part.scores, yd[a:a + m], out=mo)

    def _predict_torch(self, xd, yd, views, fill, k, chunk, out, mo) -> None:
        direct = xd.dtype == torch.float32 and len(views) == 1 and views[0] == (0, 0, False)
        n = int(xd.shape[0])
        with Fn.oracle_mode():
            for a in range(0, n, chunk):
                m = min(chunk, n - a)
                lgs = []
                for dy, dx, fl in views:
                    xv = xd[a:a + m] if direct else Fn.predict_prep(xd[a:a + m], dy, dx, fl, fill)
                    lgs.append(self._forward_torch(xv))
                part = Fn.PredictHeadOut(out.probs[a:a + m], out.scores[a:a + m],
                                         out.topk_class[a:a + m], out.topk_prob[a:a + m])
                Fn.predict_head(lgs, k, out=part)
                if mo is not None:
                    Fn.eval_metrics(part.scores, yd[a:a + m], out=mo)


# ------------------------------------------------------------------ sources --
def _is_idx(path: str) -> bool:
    from ..utils.idx import read_idx_header

    try:
        magic, dims = read_idx_header(path)
    except Exception:
        return False
    return (magic >> 8) == 0x08 and len(dims) == (magic & 0xFF) and len(dims) >= 1


def _file_rows(path: str):
    """(row count, reader(a, b) -> rows [a, b)) of a .npy or IDX ubyte file."""
    if not os.path.exists(path):
        raise ValueError(f"--predict: no such file {path!r}")
    if path.endswith(".npy"):
        arr = np.load(path, mmap_mode="r", allow_pickle=False)
        return int(arr.shape[0]), lambda a, b: np.array(arr[a:b])  # (a copy of the mapped rows)
    if not _is_idx(path):
        raise ValueError(f"--predict: {path!r} is neither a .npy file nor an IDX ubyte file")
    from ..ops import native_available
    from ..utils.idx import read_idx_header, read_idx_raw

    n = int(read_idx_header(path)[1][0])
    if native_available():  # reads the row range only
        return n, lambda a, b: native().idx_read_u8(path, a, b)
    return n, lambda a, b: np.ascontiguousarray(read_idx_raw(path, b)[a:])


def _own_split(cfg: C.TrainConfig, split: str, rank: int, world: int):
    """Rows [n r // W, n (r + 1) // W) of this configuration's test or
    validation split with their labels, from the files or the synthetic
    generator exactly as a training run of `world` ranks takes them."""
    from ..utils import data as Dm

    if cfg.model == "mnist_cnn":
        sizes = Dm.split_sizes(world)
        n = sizes.ts_size if split == "test" else sizes.val_size
        a, b = n * rank // world, n * (rank + 1) // world
        use_syn = (not Dm.mnist_files_present(cfg.data_dir)) if cfg.synthetic is None else cfg.synthetic
        if use_syn:
            x, y = Dm.synthetic_rows("test" if split == "test" else "train", a, b, seed=cfg.seed)
            return n, x, y, f"{split} (synthetic)"
        kind = "test" if split == "test" else "train"
        fx = os.path.join(cfg.data_dir, C.MNIST_FILES[kind + "_images"])
        fy = os.path.join(cfg.data_dir, C.MNIST_FILES[kind + "_labels"])
        _, rx = _file_rows(fx)
        _, ry = _file_rows(fy)
        return n, rx(a, b), ry(a, b).astype(np.int64), f"{split} ({fx})"
    if split == "val":
        raise ValueError(f"--predict val: the {cfg.model} shards have no validation rows")
    per = 8192 // 4  # the trainer's synthetic LeNet-5 shard: 8192 train / 2048 test rows a rank
    n = per * world
    x, y = Dm.synthetic_rows("test", rank * per, (rank + 1) * per, cfg.seed, C.NUM_CLASSES,
                             input_shape(cfg.model))
    return n, x, y, f"{split} (synthetic)"


def load_source(cfg: C.TrainConfig, rank: int = 0, world: int = 1):
    """(global rows n, first row a, this rank's rows, its labels or None, description)."""
    src = cfg.predict
    if src in C.PREDICT_SPLITS:
        n, x, y, desc = _own_split(cfg, src, rank, world)
        a = n * rank // world
        if cfg.predict_labels:
            raise ValueError(f"--predict-labels: --predict {src} brings its own labels")
        return n, a, x, y, desc
    n, rx = _file_rows(src)
    a, b = n * rank // world, n * (rank + 1) // world
    y = None
    if cfg.predict_labels:
        ny, ry = _file_rows(cfg.predict_labels)
        if ny != n:
            raise ValueError(f"--predict-labels: {ny} labels for {n} rows")
        y = np.asarray(ry(a, b)).astype(np.int64).reshape(-1)
    return n, a, rx(a, b), y, src


def predict_main(cfg: C.TrainConfig, di: Optional[D.DistInfo] = None) -> Dict:
    """`mpipy.py --predict`: rank r predicts rows [n r // W, n (r + 1) // W) of
    the source with the checkpoint `cfg.resume`; rank 0 gets the whole result
    (host all-reduce over zero-filled arrays: float64 carries every float32
    exactly), writes `cfg.predict_out` and returns the record it prints."""
    cfg = cfg.validate()
    if not cfg.predict:
        raise ValueError("predict_main needs cfg.predict")
    device = D.resolve_device(cfg.device)
    di = di or D.init(str(device), timeout_s=cfg.collective_timeout_s)
    rank, world = di.rank, di.world
    pr = Predictor.from_checkpoint(cfg.resume, model=cfg.model, dtype=cfg.dtype, device=device,
                                   backend=cfg.backend, weights=cfg.predict_weights or "raw")
    n, a, x, y, desc = load_source(cfg, rank, world)
    views = len(tta_views(cfg.predict_tta, cfg.model)[0])
    res = pr.predict(x, topk=cfg.predict_topk, tta=cfg.predict_tta, labels=y,
                     return_probs=cfg.predict_probs)
    host = res.numpy()
    seconds = D.allreduce_max_host(res.seconds)
    metrics = res.metrics
    if world > 1:
        full = {}
        for name, arr in host.items():
            z = np.zeros((n,) + arr.shape[1:], arr.dtype)
            z[a:a + arr.shape[0]] = arr
            full[name] = D.allreduce_sum_host_array(z).astype(arr.dtype)
        host = full
        if metrics is not None:
            ints, sums = metrics.pack()
            metrics = EvalMetrics.unpack(D.allreduce_sum_host_array(ints),
                                         D.allreduce_sum_host_array(sums), metrics.classes)
    rec = {"model": pr.model, "dtype": pr.dtype, "n": n, "views": views, "world": world,
           "checkpoint_step": pr.step, "images_per_sec": n / max(seconds, 1e-9),
           "out": cfg.predict_out}
    if cfg.predict_weights is not None:  # (a record without the flag is what it always was)
        rec["weights"] = pr.weights
    if metrics is not None:
        rec.update(error=metrics.error, loss=metrics.loss, top3_error=metrics.topk_error(3),
                   confusion=metrics.confusion.tolist())
    if cfg.predict_out and rank == 0:
        arrays = dict(host)
        meta = {"model": pr.model, "dtype": pr.dtype, "step": pr.step,
                "tta": cfg.predict_tta or "", "views": views, "source": desc}
        for key, val in meta.items():
            arrays[ckpt_mod.META_PREFIX + key] = np.array(str(val))
        path = cfg.predict_out
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        tmp = path + ".tmp.npz"
        np.savez(tmp, **arrays)
        os.replace(tmp, path)
    D.barrier()
    return {"predict": rec}
