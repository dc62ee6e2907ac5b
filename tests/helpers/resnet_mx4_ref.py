"""The MXFP4 weight format of docs/ACCURACY.md "ResNet-18 mxfp4 inference" in plain torch: the
quantiser from its definition, the host packer into conv_mx4.hip's slabs, and the float64 emulation
of the mxfp4 forward (the fp8 emulation on MX-dequantised weights)."""

import importlib.util
import os

import torch

_spec = importlib.util.spec_from_file_location(
    "resnet_fp8_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "resnet_fp8_ref.py"))
E8 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(E8)
F64 = torch.float64
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=F64)  # e2m1 magnitudes by index


def mx4_quantise(w):
    """HWIO -> (codes [R, S, C, K], the e2m1 values as float64, -0.0 for a negative weight that
    rounds to zero; E [R, S, C / 32, K] int64).  A block: 32 consecutive c of one (tap, k)."""
    R, S, C, K = w.shape
    wb = w.to(F64).reshape(R, S, C // 32, 32, K)
    amax = wb.abs().amax(3, keepdim=True)
    m, e = torch.frexp(amax)  # 6 = 0.75 2^3: the least E with 6 2^E >= m 2^e
    E = torch.where(amax > 0, torch.where(m <= 0.75, e - 3, e - 2), 0).clamp(-100, 100).long()
    d = ((wb / 2.0 ** E.to(F64)).abs().unsqueeze(-1) - GRID).abs()
    near = d == d.amin(-1, keepdim=True)  # the nearest grid value; of two equally near, the even index
    even = near & (torch.arange(8) % 2 == 0)
    g = GRID[torch.where(even.any(-1), even.int().argmax(-1), near.int().argmax(-1))]
    return torch.where(wb < 0, -g, g).reshape(R, S, C, K), E.reshape(R, S, C // 32, K)


def mx4_dequant(codes, E):
    return codes * 2.0 ** E.to(F64).repeat_interleave(32, dim=2)


def pack(codes, E):
    """The slabs of one conv as bytes: slab nt (C / 64) + ch holds, per tap, column group g, half
    h, column r, the 16 bytes of channels 64 ch + 32 h + [0, 32) of output channel 64 nt + 32 g
    + r (even channel low), then in the same order one byte E + 127 a block."""
    (R, S, C, K), T = codes.shape, codes.shape[0] * codes.shape[1]
    nib = (GRID == codes.abs().unsqueeze(-1)).int().argmax(-1) | (torch.signbit(codes).int() << 3)
    nib = nib.reshape(T, C // 64, 2, 16, 2, K // 64, 2, 32)  # tap, ch, h, byte, parity, nt, g, r
    by = (nib[:, :, :, :, 0] | (nib[:, :, :, :, 1] << 4)).permute(4, 1, 0, 5, 2, 6, 3)
    sc = (E + 127).reshape(T, C // 64, 2, K // 64, 2, 32).permute(3, 1, 0, 4, 2, 5)
    return torch.cat([by.reshape(-1, T * 2048), sc.reshape(-1, T * 128)], 1).to(torch.uint8).flatten()


def emulate(model, params, bn, x, amax):
    """resnet_fp8_ref.emulate on the MX-dequantised conv weights.  Exact, not approximate: those
    values have two significant bits, so f8_conv's per-channel e4m3 re-encoding returns them
    unchanged - asserted on every conv."""
    params = params.clone()
    pv = model.layout.views(params)
    for name in [b[0] + n for b in model._blocks() for n in ("c1_w", "c2_w") + (("ds_w",) if b[4] else ())]:
        wd = mx4_dequant(*mx4_quantise(pv[name]))
        sw = torch.tensor([E8.scale(a) for a in wd.abs().amax(dim=(0, 1, 2))], dtype=F64)
        assert torch.equal(E8.q(wd / sw) * sw, wd), name
        pv[name].copy_(wd)
    return E8.emulate(model, params, bn, x, amax)
