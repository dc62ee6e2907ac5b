"""Evaluation metrics of a split: what `ops.functional.eval_metrics` counts.

Definitions, for a row of C logits x with label t (docs/ACCURACY.md):

* prediction: the LOWEST index among the maximal logits (the rule of the
  engines' own error counters);
* rank of the label: the classes with a strictly greater logit plus those with
  an equal logit and a lower index; rank 0 = top-1 correct, top-k correct =
  rank < k;
* loss: logsumexp(x) - x[t], the softmax cross-entropy;
* a label outside [0, C) makes the row `ignored`: it counts nowhere else.

`EvalMetrics` holds the sums, so shards (ranks) and chunks merge with `+`.
"""

from __future__ import annotations

import dataclasses
from typing import Dict

import numpy as np


@dataclasses.dataclass
class EvalMetrics:
    n: int  # rows counted (the ignored ones excluded)
    ignored: int
    loss_sum: float
    confusion: np.ndarray  # int64 [C, C]: [label, prediction]
    rank_hist: np.ndarray  # int64 [C]: rows by the rank of their label

    def __post_init__(self):
        self.n, self.ignored, self.loss_sum = int(self.n), int(self.ignored), float(self.loss_sum)
        self.confusion = np.asarray(self.confusion, dtype=np.int64)
        self.rank_hist = np.asarray(self.rank_hist, dtype=np.int64)
        c = self.rank_hist.shape[0]
        if self.confusion.shape != (c, c):
            raise ValueError(f"confusion {self.confusion.shape} does not match rank_hist [{c}]")

    @classmethod
    def zeros(cls, classes: int) -> "EvalMetrics":
        return cls(0, 0, 0.0, np.zeros((classes, classes), np.int64), np.zeros(classes, np.int64))

    @property
    def classes(self) -> int:
        return int(self.rank_hist.shape[0])

    @property
    def wrong(self) -> int:
        return self.n - int(np.trace(self.confusion))

    @property
    def error(self) -> float:
        """top-1 error in percent"""
        return 100.0 * self.wrong / self.n if self.n else float("nan")

    @property
    def loss(self) -> float:
        """mean cross-entropy"""
        return self.loss_sum / self.n if self.n else float("nan")

    def topk_error(self, k: int) -> float:
        """percent of rows whose label is not among the k best classes"""
        if k < 1:
            raise ValueError(f"k must be at least 1, got {k}")
        if not self.n:
            return float("nan")
        return 100.0 * (self.n - int(self.rank_hist[:k].sum())) / self.n

    @property
    def per_class_recall(self) -> np.ndarray:
        """diag / row sum for every label class (nan for a class without rows)"""
        rows = self.confusion.sum(axis=1).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.diag(self.confusion).astype(np.float64) / rows

    def __add__(self, o: "EvalMetrics") -> "EvalMetrics":
        if not isinstance(o, EvalMetrics):
            return NotImplemented
        if o.classes != self.classes:
            raise ValueError(f"cannot merge metrics of {self.classes} and {o.classes} classes")
        return EvalMetrics(self.n + o.n, self.ignored + o.ignored, self.loss_sum + o.loss_sum,
                           self.confusion + o.confusion, self.rank_hist + o.rank_hist)

    def to_json(self) -> Dict:
        recall = [None if r != r else float(r) for r in self.per_class_recall]
        return {"n": self.n, "ignored": self.ignored, "loss_sum": self.loss_sum,
                "confusion": self.confusion.tolist(), "rank_hist": self.rank_hist.tolist(),
                "error": self.error, "loss": self.loss, "per_class_recall": recall}

    # the sums as two flat arrays, for a host all-reduce over the ranks
    def pack(self):
        ints = np.concatenate([self.confusion.ravel(), self.rank_hist,
                               np.array([self.n, self.ignored], np.int64)])
        return ints, np.array([self.loss_sum], np.float64)

    @classmethod
    def unpack(cls, ints: np.ndarray, floats: np.ndarray, classes: int) -> "EvalMetrics":
        c = classes
        return cls(int(ints[c * c + c]), int(ints[c * c + c + 1]), float(floats[0]),
                   ints[:c * c].reshape(c, c), ints[c * c:c * c + c])
