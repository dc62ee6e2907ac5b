"""What tests/test_resnet_{fp8,mx4,x3}_gpu.py share: the loader of sibling helper modules, e4m3
codes, the canary-checked read-back, the epilogue operands and the run of a byte-row conv."""

import importlib.util
import os

import torch

F64, BF, F8 = torch.float64, torch.bfloat16, torch.float8_e4m3fn


def load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = load("conv_ref")


def codes(t, dev):  # e4m3-exact values -> their codes, uploaded as bytes
    return t.to(torch.float32).to(F8).view(torch.uint8).to(dev)


def checked(y, n, canary):
    """Device buffer y on the host once the stream is idle; the canaries behind its first n elements intact."""
    torch.cuda.synchronize()
    got = y.cpu()
    assert R.guard_hits(got.float() if got.dtype == BF else got, n, canary) == 0
    return got


def epilogue_ops(shape, seed, q, wq):
    """Random e4m3-exact x (q rounds to e4m3), weights wq(randn, taps * C), a2, b, an e4m3 residual
    with its scale, and the fp64 conv."""
    N, H, W, C, K, Rr, stride, pad = shape
    g = torch.Generator().manual_seed(seed)
    x = q(torch.randn(N, H, W, C, generator=g).to(F64) * 2)
    w = wq(torch.randn(Rr, Rr, C, K, generator=g), Rr * Rr * C)
    a2 = (torch.rand(K, generator=g) * 1.5 + 0.5) * (torch.randint(0, 2, (K,), generator=g) * 2 - 1) / 16
    b = torch.rand(K, generator=g) * 2 - 1
    ref = R.conv_fwd(x, w, stride, pad)
    return x, w, a2, b, q(torch.randn(ref[0].shape, generator=g).to(F64) * 4), 0.5, ref


def run_byte_conv(name, dev, shape, x, w, a2, b, res, s_res, inv, relu, out_bf16, canary, **kw):
    """ops.<name> (f8conv, mx4conv) on host x, res (e4m3-exact) and the weight bytes w as the kernel
    takes them -> the output [N][OH][OW][K] (bf16, or e4m3 codes) and ops.<name>_plan's record."""
    from mpi_tensorflow_amd.ops import native, ptr, stream_handle

    ops, (N, H, W, C, K, Rr, stride, pad) = native().ops, shape
    sh = ops.ConvShape(N, H, W, C, K, Rr, Rr, stride, pad)
    M = N * sh.OH * sh.OW
    y = torch.full((M * K + 4096,), canary, dtype=BF if out_bf16 else torch.uint8, device=dev)
    t = [codes(x, dev), w.to(dev), a2.to(dev), b.to(dev), codes(res, dev) if res is not None else None,
         torch.tensor([s_res, inv], dtype=torch.float32, device=dev)]
    getattr(ops, name)(sh, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), ptr(t[4]), ptr(t[5]), ptr(t[5]) + 4,
                       relu, ptr(y), out_bf16, stream_handle(), **kw)
    got = checked(y, M * K, canary)
    return got[:M * K].reshape(N, sh.OH, sh.OW, K), getattr(ops, name + "_plan")(sh, kw["form"])
