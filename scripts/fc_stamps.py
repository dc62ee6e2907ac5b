"""Per-role block timeline of the three FC launches of the fp32 MNIST step
(fc1_fwd_t_kernel, fc_head_train*_kernel, fc1_bwd_kernel; lab): eager training
steps with per-block [start, end] clock stamps (100 MHz), then per launch and
role the start / end spread relative to the launch's first block, the median
block time and the block that ends last.  --chain MASK picks the forms the
launchers take (native().mnist.set_fc_chain; default: the shipped ones), so
the older and the shorter forms are compared on one build.
    python scripts/fc_stamps.py [--chain 0]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpi_tensorflow_amd import config as C  # noqa: E402
from mpi_tensorflow_amd.ops import native  # noqa: E402
from mpi_tensorflow_amd.runtime.mnist_engine import NativeMnistEngine  # noqa: E402
from mpi_tensorflow_amd.utils.data import load_mnist_shard  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chain", type=int, default=-1)
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--feature-major", action="store_true",
                help="the lab step whose fc1 forward is fc1_fwd_t_kernel")
args = ap.parse_args()

B, SLOTS = 64, 1024
cfg = C.TrainConfig(batch_size=B, graph=False).validate()
sh = load_mnist_shard(0, 1, synthetic=True, seed=cfg.seed)
k = native().mnist
k.set_fc_chain(args.chain)
eng = NativeMnistEngine(cfg, sh.train_x, sh.train_y, torch.device("cuda"),
                        fc1_feature_major=args.feature_major)
buf = torch.zeros(3 * 2 * SLOTS, dtype=torch.int64, device="cuda")
eng.train(20)
torch.cuda.synchronize()
k.set_fc_prof(buf.data_ptr())
n_dx = (B // 32) * (3136 // 32)
print(f"fc chain mask {k.fc_chain()}")
try:
    spans = {}
    for rep in range(args.reps):
        buf.zero_()
        eng.train(1)
        torch.cuda.synchronize()
        st = buf.cpu().numpy().reshape(3, SLOTS, 2)
        print(f"rep {rep}:")
        for li, lname in enumerate(("fc1 fwd", "head", "fc1 bwd")):
            s = st[li]
            nb = int((s[:, 1] > 0).sum())
            if nb == 0:
                continue
            s = s[:nb]
            rel = (s - s[:, 0].min()) / 100.0  # us
            if li == 0:
                roles = [("tiles", nb)]
            elif li == 1:
                # the older head forms lr in block 0, the shorter one in an extra block
                roles = ([("rows", nb - 1), ("lr block", 1)] if nb % 32 == 1 else
                         [("row 0 (lr)", 1), ("rows 1..", nb - 1)])
            else:
                n_dw = nb - n_dx - 8
                roles = [("dX", n_dx), ("dW1", n_dw), ("small", 8)]
            span = rel[:, 1].max()
            spans.setdefault(lname, []).append(span)
            print(f"  {lname}: {nb} blocks, span {span:.2f} us, last end: block "
                  f"{int(rel[:, 1].argmax())}")
            o = 0
            for name, n in roles:
                if n <= 0:
                    continue
                r = rel[o:o + n]
                dur = r[:, 1] - r[:, 0]
                print(f"    {name:10s} n={n:4d} start {r[:, 0].min():5.2f}-{r[:, 0].max():5.2f}  "
                      f"end {r[:, 1].min():5.2f}-{r[:, 1].max():5.2f}  dur med "
                      f"{np.median(dur):5.2f} max {dur.max():5.2f} us")
                o += n
    print("median span, us: " + ", ".join(f"{n} {np.median(v):.2f}" for n, v in spans.items()))
finally:
    k.set_fc_prof(0)
    k.set_fc_chain(-1)
