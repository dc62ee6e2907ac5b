"""Inference from a checkpoint: `Predictor`, and `predict_main` behind
`mpipy.py --predict`.

A `Predictor` holds the flat parameter buffer of a trained model and nothing
of training: no shard, no communicator, no gradient / momentum / backward
buffers, no graphs, no extra streams.  On the GPU a chunk of rows goes through

    predict_prep  (uint8 -> fp32 normalisation and / or one test-time-
                   augmentation view; csrc/kernels/predict.hip)
    eval_chunk    the engines' own static forward (MnistExecutor /
                   LenetExecutor): the same launches on the same operands as
                   `engine.evaluate`, so the logits are bit-identical to it;
                   ResNet-18 (bf16): ResnetInfer, the inference forward with
                   every BatchNorm folded into its conv's epilogue
                   (docs/ACCURACY.md "ResNet-18 inference forward");
                   ResNet-18 (fp8): the same chain with the 19 convs behind
                   the max pool on calibrated e4m3 operands
                   (docs/ACCURACY.md "ResNet-18 fp8 inference");
                   ResNet-18 (mxfp4): the fp8 chain with MXFP4 weights, e2m1
                   codes and one E8M0 scale per 32 input channels
                   (docs/ACCURACY.md "ResNet-18 mxfp4 inference");
                   ResNet-18 (bf16x3): the whole chain on split tensors, every
                   fp32 value a bf16 hi + lo pair, three bf16 MFMA products a
                   multiply (docs/ACCURACY.md "ResNet-18 bf16x3 inference")
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

PREDICT_MODELS = ("mnist_cnn", "lenet5", "resnet18")
RESNET_CHUNK = 256  # rows a ResNet-18 chunk holds at most (154 MB of fp32 input)
BN_EPS = 1e-5  # Fn.batchnorm's default


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
                 weights: str = "raw",
                 bn: Optional[Dict[str, Tuple[torch.Tensor, torch.Tensor]]] = None,
                 calib_rows: int = C.PREDICT_CALIB_ROWS):
        """`params`: the flat fp32 parameter buffer in the model's layout, on
        the device the predictions run on (used in place).  `weights` names
        what it holds: the trained weights ("raw") or their moving average
        ("ema", --ema); the forward is the same.  `bn` (resnet18): every
        BatchNorm's (running mean, running variance) on the same device, used
        in place.  resnet18 runs as dtype "bf16", "fp8", "mxfp4" or "bf16x3" on the native
        backend or as "fp32" on the torch backend.  fp8, mxfp4: the activation scales come from
        `calibrate`; a predictor that has not been calibrated calibrates itself
        on the leading min(n, calib_rows) rows of its first input."""
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
        if model == "resnet18" and backend == "native" and dtype == "fp32":
            raise ValueError("resnet18: the native inference forward is bf16 (--dtype bf16); fp32 "
                             "runs on the torch backend only, or --dtype bf16x3 for fp32-class "
                             "results")
        if dtype in ("fp8", "mxfp4", "bf16x3") and model != "resnet18":
            raise ValueError(f"dtype {dtype} supports resnet18 only, not {model}")
        if calib_rows < 1:
            raise ValueError("calib_rows must be positive")
        if dtype != "fp32" and (backend != "native" or model == "lenet5"):
            raise NotImplementedError(f"dtype {dtype} needs the native (GPU) MNIST or ResNet-18 "
                                      "forward")
        self.backend = backend
        if params.dtype != torch.float32 or params.dim() != 1 or params.numel() != self.layout.total:
            raise ValueError(f"params must be the flat fp32 buffer of {self.layout.total} floats")
        self.params = params.detach()
        self.step, self.meta = int(step), dict(meta or {})
        self.shape = input_shape(model)
        self.classes = C.NUM_CLASSES
        self.bf16 = dtype == "bf16"
        self.mx4 = dtype == "mxfp4"  # the fp8 chain (e4m3 activations) on MXFP4 weights
        self.fp8 = dtype == "fp8" or self.mx4
        self.x3 = dtype == "bf16x3"
        self.calib_rows = int(calib_rows)
        self.calibrated_on = 0  # rows of the last calibration (fp8)
        self._ws: Optional[tuple] = None
        self._eval_out: Optional[tuple] = None
        self._shadows = None
        self.bn = None
        if model == "resnet18":
            want = self._generic.bn_channels
            if bn is None or set(bn) != set(want):
                raise ValueError("resnet18 needs the BatchNorm statistics `bn` of "
                                 f"{sorted(want)}")
            for name, c in want.items():
                for t in bn[name]:
                    if t.dtype != torch.float32 or tuple(t.shape) != (c,) or t.device != self.device:
                        raise ValueError(f"bn[{name!r}] must be two fp32 [{c}] tensors on "
                                         f"{self.device}")
            self.bn = {name: (bn[name][0].detach(), bn[name][1].detach()) for name in want}
        if backend == "native":
            self._C = native()
            self.ptrs = self._make_ptrs()

    # ---------------------------------------------------------- construction
    @classmethod
    def from_checkpoint(cls, path: str, model: Optional[str] = None, dtype: str = "fp32",
                        device: str = "auto", backend: str = "auto",
                        weights: str = "raw",
                        calib_rows: int = C.PREDICT_CALIB_ROWS) -> "Predictor":
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
            bn = None
            if model == "resnet18":  # the names GenericEngine.extra_state saves them under
                bn = {}
                for name, c in _layout_of(model)[1].bn_channels.items():
                    pair = []
                    for key in (name + "/moving_mean", name + "/moving_variance"):
                        if key not in z.files:
                            raise ValueError(f"{path}: missing {key}")
                        a = z[key]
                        if tuple(a.shape) != (c,):
                            raise ValueError(f"{path}: {key} has shape {a.shape}, expected ({c},)")
                        pair.append(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev))
                    bn[name] = tuple(pair)
            if ckpt_mod.STEP_META in z.files:
                step = int(z[ckpt_mod.STEP_META])
            else:
                step = int(float(z[ckpt_mod.STEP_NAME])) if ckpt_mod.STEP_NAME in z.files else 0
        return cls(model, host.to(dev), dtype, backend, step, meta, weights, bn, calib_rows)

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
        bn = None
        if cfg.model == "resnet18":  # the engine's own statistics tensors, shared too
            bn = engine.bn
            native_kind = bool(engine.bf16 and engine.on_gpu)
            dtype = "bf16" if native_kind else "fp32"
        return cls(cfg.model, buf, dtype, "native" if native_kind else "torch",
                   step=getattr(engine, "step", 0), meta={"model": cfg.model}, weights=weights,
                   bn=bn)

    def _make_ptrs(self):
        C_, off = self._C, self.layout.offsets
        if self.model == "resnet18":
            return self._make_resnet_ptrs()
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

    def _make_resnet_ptrs(self):
        """The operands of ResnetInfer that are derived from the weights: one
        buffer of bf16 forward weight copies with its wcvt_batch job table
        (mode 0 only), the stem's space-to-depth filter, and bn_fold's job
        table and (a, b) table.  predict() re-derives them all.  fp8: wq_f8's
        codes and scales and f8_fold's tables as well; the bf16 copies are then
        held only while `calibrate` runs.  bf16x3: wsplit_x3's plane pairs and
        the split stem filter instead of the bf16 copies."""
        C_, dev = self._C, self.device
        pv = self.layout.views(self.params)
        convs, folds = [], ["bn1"]
        for name, cin, c, s, down in self._generic._blocks():
            convs += [name + "c1_w", name + "c2_w"] + ([name + "ds_w"] if down else [])
            folds += [name + "n1", name + "n2"] + ([name + "nd"] if down else [])
        self._convs = convs
        self._wcopy = None
        self._wt8 = torch.empty(64 * 256, dtype=torch.bfloat16, device=dev)
        p = C_.ResnetInferPtrs()
        p.H, p.W, p.classes = self.shape[0], self.shape[1], self.classes
        self.ptrs = p
        if self.x3:
            self._make_x3_planes(pv, convs)
        elif not self.fp8:
            self._hold_bf16_copies(True)
        rows, offs, o = [], [], 0
        for n in folds:
            rm, rv = self.bn[n]
            rows.append([ptr(pv[n + "_g"]), ptr(pv[n + "_b"]), ptr(rm), ptr(rv), rm.numel(), o, 0, 0])
            offs.append(o)
            o += rm.numel()
        self._fjobs = torch.tensor(rows, dtype=torch.int64).to(dev)
        self._fold = torch.empty(2 * o, dtype=torch.float32, device=dev)
        p.wt8 = ptr(self._wt8)
        p.fold, p.fold_total, p.fold_off = ptr(self._fold), o, offs
        p.fc_w, p.fc_b = ptr(pv["fc_w"]), ptr(pv["fc_b"])
        if self.fp8:
            self._make_fp8_tables(pv, convs, offs, o)
        return p

    def _hold_bf16_copies(self, on: bool) -> None:
        """Allocates (or drops) the bf16 forward weight copies and their job table."""
        p, dev = self.ptrs, self.device
        if not on:
            self._wcopy, self._wjobs, p.wt = None, None, []
            return
        pv = self.layout.views(self.params)
        self._wcopy = torch.empty(sum(pv[n].numel() for n in self._convs), dtype=torch.bfloat16,
                                  device=dev)
        rows, wt, o, blocks = [], [], 0, 0
        for n in self._convs:
            R, S, Ci, K = pv[n].shape
            out = self._wcopy[o:o + pv[n].numel()]
            o += pv[n].numel()
            wt.append(ptr(out))
            rows.append([ptr(pv[n]), ptr(out), R * S, Ci, K, 0, blocks, 0])
            blocks += self._C.ops.wcvt_blocks(R * S, Ci, K)
        self._wjobs = torch.tensor(rows, dtype=torch.int64).to(dev)
        self._wblocks = blocks
        p.wt = wt

    def _make_x3_planes(self, pv, convs) -> None:
        """wsplit_x3's job table and the hi / lo plane pairs [2][tap][k][c] of the
        19 convs in one buffer; the split stem filter [2][64][256]."""
        p, dev = self.ptrs, self.device
        self._wx3 = torch.empty(2 * sum(pv[n].numel() for n in convs), dtype=torch.bfloat16,
                                device=dev)
        self._wt8x3 = torch.empty(2 * 64 * 256, dtype=torch.bfloat16, device=dev)
        rows, wx3, o, blocks = [], [], 0, 0
        for n in convs:
            R, S, Ci, K = pv[n].shape
            out = self._wx3[o:o + 2 * pv[n].numel()]
            o += 2 * pv[n].numel()
            wx3.append(ptr(out))
            rows.append([ptr(pv[n]), ptr(out), R * S, Ci, K, 0, blocks, 0])
            blocks += K // 32
        self._xjobs, self._xblocks = torch.tensor(rows, dtype=torch.int64).to(dev), blocks
        p.wx3, p.wt8x3, p.x3 = wx3, ptr(self._wt8x3), True

    def _make_fp8_tables(self, pv, convs, offs, total) -> None:
        """wq_f8's job table, codes and scales; the calibration table (slot 0
        the pool output, 1 + i the output of conv i); f8_fold's job table (which
        tensor each conv reads, writes and adds) and its outputs.  mxfp4:
        wq_mx4's job table and slabs (a block per slab, taps * 2176 bytes:
        half a byte a weight and a scale byte per 32) and a weight-scale
        table of ones, which no launch writes."""
        p, dev = self.ptrs, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        sizes = [pv[n].numel() * 17 // 32 if self.mx4 else pv[n].numel() for n in convs]
        self._w8 = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
        self._sw = torch.ones(total, **f32) if self.mx4 else torch.empty(total, **f32)
        self._a2 = torch.empty(total, **f32)
        self._amax, self._scal = torch.zeros(len(convs) + 1, **f32), torch.empty(2 * len(convs) + 1, **f32)
        rows, w8, o, blocks = [], [], 0, 0
        for i, n in enumerate(convs):
            R, S, Ci, K = pv[n].shape
            out = self._w8[o:o + sizes[i]]
            o += sizes[i]
            w8.append(ptr(out))
            rows.append([ptr(pv[n]), ptr(out), R * S, Ci, K, offs[1 + i], blocks, 0])
            blocks += (K // 64) * (Ci // 64) if self.mx4 else K // 32
        self._qjobs, self._qblocks = torch.tensor(rows, dtype=torch.int64).to(dev), blocks
        rows, i, src = [], 0, 0  # src: the slot of the block input
        for name, cin, c, s, down in self._generic._blocks():
            res = 1 + i + 2 if down else src
            rows.append([offs[1 + i], c, src, 1 + i, -1, 0, 0, 0])  # c1
            rows.append([offs[2 + i], c, 1 + i, 2 + i, res, 0, 0, 0])  # c2 -> the block output
            if down:
                rows.append([offs[3 + i], c, src, 3 + i, -1, 0, 0, 0])  # ds
            src, i = 2 + i, i + (3 if down else 2)
        self._f8jobs = torch.tensor(rows, dtype=torch.int64).to(dev)
        p.w8, p.amax, p.a2, p.scal = w8, ptr(self._amax), ptr(self._a2), ptr(self._scal)
        p.mx4 = self.mx4

    def _derive_resnet(self, s: int) -> None:
        """The bf16 weight operands and the folded BatchNorms, from the
        weights and statistics as they are now (three launches)."""
        ops = self._C.ops
        if self._wcopy is not None:
            ops.wcvt_batch(ptr(self._wjobs), self._wjobs.shape[0], self._wblocks, s)
        w1 = ptr(self.layout.views(self.params)["conv1_w"])
        if self.x3:
            ops.wsplit_x3(ptr(self._xjobs), self._xjobs.shape[0], self._xblocks, s)
            ops.s2d_stem_weight_x3(w1, 64, ptr(self._wt8x3), s)
        else:
            ops.s2d_stem_weight(w1, 64, ptr(self._wt8), s)
        ops.bn_fold(ptr(self._fjobs), self._fjobs.shape[0], self.ptrs.fold_total, BN_EPS,
                    ptr(self._fold), s)
        if self.fp8:
            if self.mx4:
                ops.wq_mx4(ptr(self._qjobs), self._qjobs.shape[0], self._qblocks, s)
            else:
                ops.wq_f8(ptr(self._qjobs), self._qjobs.shape[0], self._qblocks, ptr(self._sw), s)
            if self.ptrs.calibrated:
                self._f8_fold(s)

    def _f8_fold(self, s: int) -> None:
        self._C.ops.f8_fold(ptr(self._f8jobs), self._f8jobs.shape[0], ptr(self._fold),
                            ptr(self._sw), ptr(self._amax), ptr(self._a2), ptr(self._scal), s)

    @torch.no_grad()
    def calibrate(self, x, chunk: int = RESNET_CHUNK) -> int:
        """fp8, mxfp4: the activation scales from the rows x.  Zeroes the amax table,
        runs the bf16 forward over x with a max |value| launch behind every
        tensor the fp8 forward quantises (calibrate_chunk), and folds.  The
        scales stay until the next call.  -> the rows used."""
        if not self.fp8:
            raise ValueError("calibrate: only a dtype fp8 or mxfp4 predictor has scales to "
                             "calibrate")
        xd = self._rows(x)
        n = int(xd.shape[0])
        if n < 1 or chunk < 1:
            raise ValueError("calibrate needs at least one row and a positive chunk")
        chunk = self._chunk(chunk, n)
        ws, s, p = self._workspace(chunk), stream_handle(), self.ptrs
        row = int(np.prod(self.shape))
        self._hold_bf16_copies(True)
        try:
            p.calibrated = False
            self._amax.zero_()
            self._derive_resnet(s)
            for a in range(0, n, chunk):
                m = min(chunk, n - a)
                if xd.dtype == torch.float32:
                    x_ptr = ptr(xd) + 4 * row * a
                else:
                    Fn.predict_prep(xd[a:a + m], 0, 0, False, 0.0, out=ws["xv"])
                    x_ptr = ptr(ws["xv"])
                self._C.ResnetInfer.calibrate_chunk(p, x_ptr, m, ptr(ws["act0"]), ptr(ws["act1"]),
                                                    ptr(ws["act2"]), ptr(ws["conv_ws"]),
                                                    ws["conv_ws"].numel(), ptr(ws["logits"]), s)
            self._f8_fold(s)
            self._sync()  # the copies are dropped below: their readers have finished
        finally:
            self._hold_bf16_copies(False)
        p.calibrated, self.calibrated_on = True, n
        return n

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
        if self.model == "resnet18":
            sizes = self._C.ResnetInfer.ws_bytes(self.ptrs, chunk)
            for i in range(3):
                ws[f"act{i}"] = torch.empty(sizes[i] // 2, dtype=torch.bfloat16, device=dev)
            ws["conv_ws"] = torch.empty(max(sizes[3] // 4, 4), **f32)
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
        if self.x3:
            self._C.ResnetInfer.eval_chunk_x3(self.ptrs, x_ptr, m, ptr(ws["act0"]), ptr(ws["act1"]),
                                              ptr(ws["act2"]), ptr(ws["logits"]), s)
        elif self.fp8:
            self._C.ResnetInfer.eval_chunk_f8(self.ptrs, x_ptr, m, ptr(ws["act0"]), ptr(ws["act1"]),
                                              ptr(ws["act2"]), ptr(ws["logits"]), s)
        elif self.model == "resnet18":
            self._C.ResnetInfer.eval_chunk(self.ptrs, x_ptr, m, ptr(ws["act0"]), ptr(ws["act1"]),
                                           ptr(ws["act2"]), ptr(ws["conv_ws"]),
                                           ws["conv_ws"].numel(), ptr(ws["logits"]), s)
        elif self.model == "lenet5":
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
        return self._generic.forward(P, self.bn or {}, xb, False)

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
        chunk = self._chunk(chunk, n)
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
        run(xd, yd, [(0, 0, False)], 0.0, 1, self._chunk(chunk, n), out, mo)
        return mo.result()

    def _chunk(self, chunk: int, n: int) -> int:
        chunk = min(int(chunk), max(n, 1))
        return min(chunk, RESNET_CHUNK) if self.model == "resnet18" else chunk

    def _sync(self) -> None:
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def _predict_native(self, xd, yd, views, fill, k, chunk, out, mo) -> None:
        V, Cn = len(views), self.classes
        H, W, Cc = self.shape
        row = H * W * Cc
        ws = self._workspace(chunk)
        s = stream_handle()
        if self.fp8 and not self.ptrs.calibrated:
            self.calibrate(xd[:min(int(xd.shape[0]), self.calib_rows)], chunk)
        if self.model == "resnet18":
            self._derive_resnet(s)
        elif self.bf16:  # re-derived from the weights as they are now
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
    if cfg.model == "resnet18":  # the trainer's synthetic shard (runtime/trainer.py)
        per = C.RESNET_SYNTH_ROWS[1]
        x, y = Dm.synthetic_images_torch(per, input_shape(cfg.model), seed=cfg.seed, split="test",
                                         start=rank * per)
        return per * world, x.numpy(), y.numpy().astype(np.int64), f"{split} (synthetic)"
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
                                   backend=cfg.backend, weights=cfg.predict_weights or "raw",
                                   calib_rows=cfg.predict_calib or C.PREDICT_CALIB_ROWS)
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
    if pr.fp8:  # the rows this rank's activation scales were calibrated on
        rec["calib_rows"] = pr.calibrated_on
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
