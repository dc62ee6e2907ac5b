"""The conv launch plans against the table recorded from the parent commit
(tests/golden/conv_plan_table.json, scripts/conv_plan_table.py): every route,
workspace size, split count and statistics-row count of the sweep is what it
was.  The planners are host code, so this runs without a GPU."""

import glob
import importlib.util
import itertools
import json
import os

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def _ops():
    """Skips only when the extension is not built; one that is built has to load."""
    if not glob.glob(os.path.join(_ROOT, "mpi_tensorflow_amd", "_C*.so")):
        pytest.skip("native extension not built")
    import torch  # noqa: F401
    from mpi_tensorflow_amd.ops import native

    return native().ops


def _script():
    spec = importlib.util.spec_from_file_location("conv_plan_table",
                                                  os.path.join(_ROOT, "scripts", "conv_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RERECORD = ("the table is only re-recorded for a deliberate plan change, on a build of that change's "
            "parent commit (scripts/conv_plan_table.py)")


def test_plans_match_the_recorded_table():
    ops = _ops()
    with open(os.path.join(_HERE, "golden", "conv_plan_table.json")) as f:
        gold = json.load(f)
    rows, sha, n = _script().build_table(ops)
    assert set(rows) == set(gold["rows"]), f"the sweep itself changed; {RERECORD}"
    for key in rows:  # in sweep order
        want, got = gold["rows"][key], rows[key]
        if want != got:
            print(f"first differing query: {key}\n  recorded (parent {gold['parent'][:12]}): {want}\n"
                  f"  now:                              {got}\n{RERECORD}")
        assert want == got, key
    assert n == gold["count"]
    assert sha == gold["sha256"], (f"a row outside the stored sample differs (digest over all {n} rows); "
                                   f"{RERECORD}")


def test_route_flags_name_what_the_call_provides():
    """The keyword flags of ops.conv_route reach the planners (the routes the
    positional form cannot name), and the defaults are the positional form."""
    ops = _ops()
    sh = ops.ConvShape(2, 14, 14, 64, 64, 3, 3, 1, 1)
    assert ops.conv_route(sh, "fwd", False, wcopy=True)["kernel"] == "conv3f_kernel"
    assert ops.conv_route(sh, "fwd", False, wcopy=True, stats=True)["kernel"] == "fwd_kernel"
    assert ops.conv_route(sh, "fwd", True)["kernel"] == "conv3_kernel"
    assert ops.conv_route(sh, "fwd", True, act16=False)["kernel"] == "fwd_kernel"
    s2 = ops.ConvShape(2, 14, 14, 64, 128, 3, 3, 2, 1)
    assert ops.conv_route(s2, "dgrad", True)["kernel"] == "dgrad3s2_kernel"
    d = ops.conv_route(s2, "dgrad", True, act16=False)
    assert (d["family"], d["kernel"]) == ("tiled", "data_kernel")
    assert ops.conv_route(s2, "dgrad", False, dy32=False)["kernel"] == "data_b16_kernel"
    s4 = ops.ConvShape(4, 14, 14, 64, 64, 3, 3, 1, 1)
    assert ops.conv_route(s4, "wgrad", True)["kernel"] == "wgrad3_kernel"
    assert ops.conv_route(s4, "wgrad", True, dy16=False)["kernel"] == "wgrad_kernel"
    # without a workspace the fp32 stride-1 dgrad does not go through the forward kernels
    assert ops.conv_route(sh, "dgrad", False)["kernel"] == "conv3f_kernel"
    assert ops.conv_route(sh, "dgrad", False, ws=False)["kernel"] == "data_kernel"
    for op in ("fwd", "dgrad", "wgrad"):
        for b in (False, True):
            a = ops.conv_route(sh, op, b)
            assert a == ops.conv_route(sh, op, b, False, False, 0, act16=True, dy16=True, dy32=True,
                                       ws=True, stats=False)
            assert a["ws_floats"] <= ops.conv_ws_floats(sh, False)


def test_every_plan_fits_the_layer_workspace():
    """Over the whole sweep, in both conv modes and with every operand copy
    present or left out: the workspace a plan needs (its slabs behind their
    offset included) is within conv_ws_floats of the layer, which is what the
    engine allocates before it knows which calls will come."""
    ops = _ops()
    T = _script()
    flags = [dict(act16=a, dy16=d, wcopy=w) for a, d, w in itertools.product((True, False), repeat=3)]
    for N, H, C, K, (R, st, pd) in itertools.product(T.NS, T.HS, T.CS, T.KS, T.RSP):
        if H + 2 * pd < R:
            continue
        sh = ops.ConvShape(N, H, H, C, K, R, R, st, pd)
        room = {e: ops.conv_ws_floats(sh, e) for e in (False, True)}
        for b in (False, True):
            for f in flags:
                for e in (False, True):
                    r = ops.conv_route(sh, "fwd", b, e, **f)
                    assert r["ws_floats"] <= room[e], (N, H, C, K, R, st, pd, "fwd", b, e, f, r)
                for op in ("dgrad", "wgrad"):
                    r = ops.conv_route(sh, op, b, **f)
                    assert r["ws_floats"] <= room[False], (N, H, C, K, R, st, pd, op, b, f, r)
                    assert r["ws_floats"] <= room[True], (N, H, C, K, R, st, pd, op, b, f, r)
