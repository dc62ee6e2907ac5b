"""What the per-pass augmentation launch costs: `augment_rows` (shuffle + shift /
flip in one pass) and `affine_rows` (the same with rotate:10,scale:10 on top)
against `shuffle_rows` on the three device-resident shards.

Method of PERF_NOTES round 10: HIP events around 100 launches, 10 blocks of
each kernel alternating after 20 warm-up launches of both; median and range of
the blocks.

    python scripts/augment_lab.py
"""

import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mpi_tensorflow_amd.ops import native, ptr, stream_handle  # noqa: E402
from mpi_tensorflow_amd.utils import rng  # noqa: E402

SHARDS = (("MNIST", 55000, (28, 28, 1), 2, False, -0.5),
          ("LeNet-5", 8192, (32, 32, 3), 4, True, 0.0),
          ("ResNet-18", 512, (224, 224, 3), 16, True, 0.0))
LAUNCHES, BLOCKS, WARM = 100, 10, 20
PERM_KEY, AUG_KEY = 0xde56f3b3, 0x0bc45ed0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / LAUNCHES  # us a launch


def main():
    ops, dev = native().ops, torch.device("cuda:0")
    for name, n, shape, K, flip, fill in SHARDS:
        if len(sys.argv) > 1 and name not in sys.argv[1:]:
            continue
        row = shape[0] * shape[1] * shape[2]
        src_x = torch.rand((n,) + shape, device=dev) - 0.5
        src_y = torch.randint(0, 10, (n,), dtype=torch.int32, device=dev)
        dst_x, dst_y = torch.empty_like(src_x), torch.empty_like(src_y)
        st = stream_handle()
        args = (ptr(src_x), ptr(src_y), ptr(dst_x), ptr(dst_y), n)
        tables = torch.from_numpy(rng.affine_tables(10.0, 10.0)).to(dev)
        kernels = {
            "shuffle_rows": lambda: ops.shuffle_rows(*args, row, PERM_KEY, st),
            "augment_rows": lambda: ops.augment_rows(*args, *shape, True, PERM_KEY, AUG_KEY, K,
                                                     flip, fill, st),
            "augment_rows, file order": lambda: ops.augment_rows(*args, *shape, False, 0, AUG_KEY,
                                                                 K, flip, fill, st),
            "affine_rows": lambda: ops.affine_rows(*args, *shape, True, PERM_KEY, AUG_KEY, K,
                                                   flip, fill, ptr(tables), 0, st),
            "affine_rows, file order": lambda: ops.affine_rows(*args, *shape, False, 0, AUG_KEY, K,
                                                               flip, fill, ptr(tables), 0, st),
        }
        for fn in kernels.values():
            for _ in range(WARM):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in kernels}
        for _ in range(BLOCKS):
            for k, fn in kernels.items():
                us[k].append(timed(fn))
        moved = 2 * n * row * 4
        base = statistics.median(us["shuffle_rows"])
        for k, v in us.items():
            med = statistics.median(v)
            print(f"{name:10s} {n} x {row}  {k:26s} {med:8.1f} us ({min(v):.1f}-{max(v):.1f})  "
                  f"{moved / med / 1e6:5.2f} TB/s  x{med / base:.2f} of shuffle_rows", flush=True)


if __name__ == "__main__":
    main()
