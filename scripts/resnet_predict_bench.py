"""ResNet-18 bf16 inference: Predictor.predict (the native ResnetInfer forward)
against GenericEngine.evaluate on the same weights, rows and device, in one
process, the two alternating (docs/PERF_NOTES.md holds a run's figures).

    python scripts/resnet_predict_bench.py [--rows 1000] [--chunk 256] [--reps 25] [--windows 5]

A window is `reps` passes over the `rows` device-resident fp32 rows between two
synchronisations (a few hundred ms); the first window of each path is the
warm-up and is dropped.  Prints one JSON line: per path the windows'
images/sec as min / median / max."""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpi_tensorflow_amd import config as C  # noqa: E402
from mpi_tensorflow_amd.runtime.generic_engine import GenericEngine  # noqa: E402
from mpi_tensorflow_amd.runtime.predict import Predictor  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    cfg = C.TrainConfig(model="resnet18", dtype="bf16", batch_size=2, graph=False).validate()
    eng = GenericEngine(cfg, np.zeros((4, 224, 224, 3), np.float32), np.zeros(4, np.int64), dev)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # statistics that make the BatchNorms matter
        for rm, rv in eng.bn.values():
            rm.copy_(torch.randn(rm.shape, generator=g) * 0.5)
            rv.copy_(torch.rand(rv.shape, generator=g) * 1.5 + 0.5)
    x = torch.randn(a.rows, 224, 224, 3, generator=g).numpy()
    y = np.zeros(a.rows, np.int64)
    xd = torch.from_numpy(x).to(dev)
    pr = Predictor.from_engine(eng)

    def window(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return a.rows * a.reps / (time.perf_counter() - t)

    paths = {"evaluate": lambda: eng.evaluate(x, y, chunk=a.chunk),  # (x stays cached on the device)
             "predict": lambda: pr.predict(xd, chunk=a.chunk)}
    rate = {k: [] for k in paths}
    for _ in range(a.windows + 1):
        for k, fn in paths.items():
            rate[k].append(window(fn))
    rec = {"rows": a.rows, "chunk": a.chunk, "reps": a.reps, "windows": a.windows}
    for k, v in rate.items():
        v = v[1:]
        rec[k + "_img_s"] = {"min": round(min(v)), "median": round(statistics.median(v)), "max": round(max(v))}
    rec["ratio_of_medians"] = round(rec["predict_img_s"]["median"] / rec["evaluate_img_s"]["median"], 3)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
