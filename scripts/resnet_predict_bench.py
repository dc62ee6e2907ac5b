"""ResNet-18 bf16 inference: Predictor.predict (the native ResnetInfer forward)
against GenericEngine.evaluate on the same weights, rows and device, in one
process, the two alternating (docs/PERF_NOTES.md holds a run's figures).

    python scripts/resnet_predict_bench.py [--rows 1000] [--chunk 256] [--reps 25] [--windows 5]
                                           [--dtype bf16|fp8|bf16x3|mxfp4] [--with-torch-fp32]

--dtype fp8: the bf16 Predictor against an fp8 one on the same weights
(calibrated on the leading 256 rows), and with it the fp8 A/Bs - the MFMA form
(32x32x16 fp8_fp8 / 32x32x64 f8f6f4) and the loader of the 3x3 stride-1 convs
(gather / halo) - all alternating in the one process.

--dtype mxfp4: the bf16, fp8 and mxfp4 Predictors on the same weights, the two
quantised ones calibrated on the same leading 256 rows, alternating; the record
adds mxfp4 over fp8 and the bytes of the two weight buffers.

--dtype bf16x3: the bf16 Predictor against a bf16x3 one on the same weights;
--with-torch-fp32 adds the torch-backend fp32 Predictor (the forward that serves
fp32 checkpoints without bf16x3) to the same alternating windows.

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
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp8", "bf16x3", "mxfp4"))
    ap.add_argument("--with-torch-fp32", action="store_true")
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
    if a.dtype == "fp8":
        from mpi_tensorflow_amd.ops import native

        ops = native().ops
        pr8 = Predictor("resnet18", eng.params, dtype="fp8", bn=eng.bn)
        pr8.calibrate(xd[:256], chunk=a.chunk)

        def fp8(mfma, form):
            def run():
                ops.f8conv_set_mfma(mfma)
                ops.f8conv_set_form(form)
                pr8.predict(xd, chunk=a.chunk)
            return run

        paths = {"predict": paths["predict"], "fp8_x16_gather": fp8(2, 1), "fp8_x64_gather": fp8(1, 1),
                 "fp8_x16_halo": fp8(2, 2), "fp8_x64_halo": fp8(1, 2)}
    if a.dtype == "mxfp4":
        pr8 = Predictor("resnet18", eng.params, dtype="fp8", bn=eng.bn)
        pr4 = Predictor("resnet18", eng.params, dtype="mxfp4", bn=eng.bn)
        pr8.calibrate(xd[:256], chunk=a.chunk)
        pr4.calibrate(xd[:256], chunk=a.chunk)
        paths = {"predict": paths["predict"], "fp8": lambda: pr8.predict(xd, chunk=a.chunk),
                 "mxfp4": lambda: pr4.predict(xd, chunk=a.chunk)}
    if a.dtype == "bf16x3":
        prx = Predictor("resnet18", eng.params, dtype="bf16x3", bn=eng.bn)
        paths = {"predict": paths["predict"], "bf16x3": lambda: prx.predict(xd, chunk=a.chunk)}
        if a.with_torch_fp32:
            prt = Predictor("resnet18", eng.params, dtype="fp32", backend="torch", bn=eng.bn)
            paths["torch_fp32"] = lambda: prt.predict(xd, chunk=a.chunk)
    rate = {k: [] for k in paths}
    for _ in range(a.windows + 1):
        for k, fn in paths.items():
            rate[k].append(window(fn))
    rec = {"rows": a.rows, "chunk": a.chunk, "reps": a.reps, "windows": a.windows}
    for k, v in rate.items():
        v = v[1:]
        rec[k + "_img_s"] = {"min": round(min(v)), "median": round(statistics.median(v)), "max": round(max(v))}
    base = "evaluate" if a.dtype == "bf16" else "predict"
    for k in rate:
        if k != base and (a.dtype != "bf16" or k == "predict"):
            name = "ratio_of_medians" if a.dtype == "bf16" else k + "_over_bf16"
            rec[name] = round(rec[k + "_img_s"]["median"] / rec[base + "_img_s"]["median"], 3)
    if "mxfp4" in rate:  # the weight operands' bytes, read from the allocated buffers
        rec["mxfp4_over_fp8"] = round(rec["mxfp4_img_s"]["median"] / rec["fp8_img_s"]["median"], 3)
        rec["weight_bytes"] = {"fp8": pr8._w8.numel(), "mxfp4": pr4._w8.numel()}
    if "torch_fp32" in rate:
        rec["bf16x3_over_torch_fp32"] = round(rec["bf16x3_img_s"]["median"]
                                              / rec["torch_fp32_img_s"]["median"], 3)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
