"""The launch plans of the generic engine's convs over a fixed sweep, as a table:
one row per query - the route of each op (ops.conv_route with its positional
arguments), conv_ws_floats with and without epilogue, conv_filter_splits,
conv_fwd_stats_rows, conv_bwd_data_stats_rows, the TiledPlan variants of
tests/test_conv_routes_gpu.py on that file's shape lists, and the stem queries
with s2d_stem_ws_floats.  A thrown error is recorded as its message.

tests/test_conv_plan_cpu.py regenerates the table and compares it with
tests/golden/conv_plan_table.json: full rows for a sample that holds every
(family, kernel) pair and every TiledPlan variant, a SHA-256 over all rows.
The golden file is recorded on a build of the PARENT commit of a deliberate
plan change (never on the code under test), in a checkout of its own:

    python scripts/conv_plan_table.py --root <parent checkout> --parent <hash> \\
        --record tests/golden/conv_plan_table.json

The planners are host code: no GPU is needed."""
import argparse
import hashlib
import importlib.util
import itertools
import json
import os
import sys

SAMPLE_EVERY = 60  # one sweep row in this many is stored in full

NS, HS = (1, 2, 32), (7, 14, 28, 56, 224)
CS, KS = (3, 6, 16, 32, 64, 128, 192, 256, 512), (6, 16, 64, 128, 192, 512)
RSP = ((1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1), (5, 1, 0), (7, 2, 3))

# the TiledPlan variants and shape lists of tests/test_conv_routes_gpu.py
_spec = importlib.util.spec_from_file_location(
    "conv_plan_cases", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests",
                                    "helpers", "conv_plan_cases.py"))
_cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cases)
HALO_VARIANTS, HALO_SHAPES, XCD_SHAPES = _cases._halo_variants(), _cases.HALO_SHAPES, _cases.XCD_SHAPES
S2_SHAPES, XCD_VARIANTS, S2_VARIANTS = _cases.S2_SHAPES, _cases.XCD_VARIANTS, _cases.S2_VARIANTS
ROUTE_KEYS = ("family", "kernel", "bm", "bn", "z", "halo", "stem")


def _call(f, *a, **k):
    try:
        return f(*a, **k)
    except Exception as e:  # the message is the row
        return f"error: {e}"


def _route(ops, sh, op, bf16, epi=False, wcopy=False, stem=0):
    d = _call(ops.conv_route, sh, op, bf16, epi, wcopy, stem)
    if isinstance(d, str):
        return d
    return "{} {} {}x{} z{} h{:d}s{:d}".format(*(d[k] for k in ROUTE_KEYS))


def _tag(t):
    return ",".join(str(int(v)) for v in t)


def _sizes(ops, sh):
    return [_call(ops.conv_ws_floats, sh, False), _call(ops.conv_ws_floats, sh, True),
            _call(ops.conv_filter_splits, sh), _call(ops.conv_fwd_stats_rows, sh, True),
            _call(ops.conv_fwd_stats_rows, sh, False), _call(ops.conv_bwd_data_stats_rows, sh)]


def sweep(ops):
    """Yields (key, row) over the main sweep: 16 routes and a sizes row per shape."""
    for N, H, C, K, (R, st, pd) in itertools.product(NS, HS, CS, KS, RSP):
        if H + 2 * pd < R:
            continue
        t = (N, H, H, C, K, R, st, pd)
        sh = ops.ConvShape(N, H, H, C, K, R, R, st, pd)
        for b, e, w in itertools.product((False, True), repeat=3):
            yield f"{_tag(t)}|fwd|{_tag((b, e, w))}", _route(ops, sh, "fwd", b, e, w)
        for op in ("dgrad", "wgrad"):
            for b, w in itertools.product((False, True), repeat=2):
                yield f"{_tag(t)}|{op}|{_tag((b, w))}", _route(ops, sh, op, b, False, w)
        yield f"{_tag(t)}|sizes", _sizes(ops, sh)


def variants(ops):
    """Yields (key, row) for the TiledPlan variants and the stem queries: all stored in full."""
    runs = ([((N, H, W, C, K, 3, 1, 1), HALO_VARIANTS) for N, H, W, C, K in HALO_SHAPES] +
            [((N, H, H, C, K, R, st, pd), XCD_VARIANTS) for N, H, C, K, R, st, pd in XCD_SHAPES] +
            [((N, H, H, C, K, 3, 2, 1), S2_VARIANTS) for N, H, C, K in S2_SHAPES])
    saved = ops.get_tiled_plan()
    try:
        for t, vs in runs:
            N, H, W, C, K, R, st, pd = t
            sh = ops.ConvShape(N, H, W, C, K, R, R, st, pd)
            for fields in vs:
                p = ops.get_tiled_plan()
                for k, v in fields.items():
                    setattr(p, k, v)
                ops.set_tiled_plan(p)
                name = ";".join(f"{k}={int(v)}" for k, v in sorted(fields.items()))
                for op, w in itertools.product(("fwd", "dgrad", "wgrad"), (False, True)):
                    yield f"{_tag(t)}|{op}|fp32,wcopy={int(w)}|{name}", _route(ops, sh, op, False, False, w)
                yield f"{_tag(t)}|sizes|{name}", _sizes(ops, sh)
                ops.set_tiled_plan(saved)
    finally:
        ops.set_tiled_plan(saved)
    try:
        for N, OH, OW, K in itertools.product((2, 32), (16, 19, 112), (16, 21, 112), (64, 128)):
            si = ops.ConvShape(N, OH + 3, OW + 3, 16, K, 4, 4, 1, 0)
            for pre in (True, False):
                ops.s2d_stem_set_preload(pre)
                yield f"{_tag((N, OH, OW, K))}|s2d|fwd|preload={int(pre)}", _route(ops, si, "fwd", True, stem=2)
            yield f"{_tag((N, OH, OW, K))}|s2d|wgrad", _route(ops, si, "wgrad", True, stem=2)
            yield f"{_tag((N, OH, OW, K))}|s2d|ws", _call(ops.s2d_stem_ws_floats, si)
            for kp in (64, 192):
                s1 = ops.ConvShape(N, OH, OW, kp, K, 1, 1, 1, 0)
                for op in ("fwd", "wgrad"):
                    yield f"{_tag((N, OH, OW, kp, K))}|stem|{op}", _route(ops, s1, op, True, stem=1)
                yield f"{_tag((N, OH, OW, kp, K))}|stem|rows", _call(ops.conv_fwd_stem_stats_rows, s1)
    finally:
        ops.s2d_stem_set_preload(True)


def build_table(ops):
    """(sampled rows {key: row}, sha256 over every row, row count)."""
    h = hashlib.sha256()
    rows, seen, n = {}, set(), 0
    for i, (key, row) in enumerate(sweep(ops)):
        h.update(json.dumps([key, row]).encode())
        pair = row.split(" ")[:2] if isinstance(row, str) else None
        first = pair is not None and tuple(pair) not in seen
        if first:
            seen.add(tuple(pair))
        if first or i % SAMPLE_EVERY == 0:
            rows[key] = row
        n += 1
    for key, row in variants(ops):
        h.update(json.dumps([key, row]).encode())
        rows[key] = row
        n += 1
    return rows, h.hexdigest(), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose built extension answers")
    ap.add_argument("--parent", default="", help="commit hash of that checkout, stored in the table")
    ap.add_argument("--record", default="", help="write the table there (else: print its digest)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch  # noqa: F401

    from mpi_tensorflow_amd.ops import native

    rows, sha, n = build_table(native().ops)
    print(f"{n} rows, {len(rows)} stored, sha256 {sha}")
    if a.record:
        with open(a.record, "w") as f:
            json.dump({"parent": a.parent, "count": n, "sha256": sha, "rows": rows}, f, indent=0,
                      sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
