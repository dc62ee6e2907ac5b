"""Float64 emulation of the ResNet-18 fp8 forward as docs/ACCURACY.md defines it:
eval_chunk_f8's quantisation points and scales, float64 between them; plain torch.
`quantise=False` makes q the identity: the scales cancel, the plain forward is left."""

import math

import torch
import torch.nn.functional as F

F64 = torch.float64
EPS_BN = float(torch.tensor(1e-5, dtype=torch.float32))


def scale(amax):
    """2^j, j the least integer with 448 2^j >= amax (held to [-100, 100]); scale(0) = 1."""
    amax = float(amax)
    if not amax > 0.0:
        return 1.0
    m, e = math.frexp(amax)
    return 2.0 ** min(max(e - 9 if m <= 0.875 else e - 8, -100), 100)


def q(v):
    """e4m3_rne(clamp(v, -448, 448)) as float64 values."""
    return v.clamp(-448.0, 448.0).to(torch.float32).to(torch.float8_e4m3fn).to(F64)


def quantise_weight(w):
    """HWIO fp32 -> (sw [K], codes [tap][k][c] as float64 values)."""
    sw = torch.tensor([scale(a) for a in w.abs().amax(dim=(0, 1, 2))], dtype=F64)
    codes = q(w.to(F64) / sw)
    return sw, codes.reshape(-1, w.shape[2], w.shape[3]).permute(0, 2, 1).contiguous()


def conv(x, w, stride, pad):
    """NHWC x, HWIO w, float64."""
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), None, stride, pad).permute(0, 2, 3, 1)


def f8_conv(xc, s_in, w, a, b, stride, pad, res=None, s_res=0.0, relu=False, s_out=None,
            quant=q):
    """One fp8 conv on codes xc (scale s_in) -> codes (scale s_out), or v where s_out is None."""
    sw = torch.tensor([scale(m) for m in w.abs().amax(dim=(0, 1, 2))], dtype=F64)
    v = conv(xc, quant(w.to(F64) / sw), stride, pad) * (a * sw * s_in) + b
    if res is not None:
        v = v + s_res * res
    if relu:
        v = v.clamp_min(0)
    return v if s_out is None else quant(v / s_out)


def emulate(model, params, bn, x, amax, quantise=True):
    """Logits (float64) of fp32 rows x [n, H, W, 3]; amax: the calibration table (slot 0 the
    pool output, 1 + i the output of conv i, in the order c1, c2, ds per block)."""
    quant = q if quantise else (lambda v: v)
    pv = {k: v.to(F64) for k, v in model.layout.views(params).items()}
    raw = model.layout.views(params)

    def fold(nm):
        rm, rv = (t.to(F64) for t in bn[nm])
        a = pv[nm + "_g"] / torch.sqrt(rv + EPS_BN)
        return a, pv[nm + "_b"] - rm * a

    s = [scale(v) for v in amax]
    a, b = fold("bn1")  # the bf16 stem, its output stored as bf16
    h = (conv(x.to(F64), pv["conv1_w"], 2, 3) * a + b).clamp_min(0)
    if quantise:
        h = h.to(torch.float32).to(torch.bfloat16).to(F64)
    h = F.max_pool2d(h.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    h, src, i = quant(h / s[0]), 0, 0
    blocks = model._blocks()
    for name, cin, c, st, down in blocks:
        last = name == blocks[-1][0]
        t = f8_conv(h, s[src], raw[name + "c1_w"], *fold(name + "n1"), st, 1, relu=True,
                    s_out=s[1 + i], quant=quant)
        res, rslot = h, src
        if down:
            res = f8_conv(h, s[src], raw[name + "ds_w"], *fold(name + "nd"), st, 0,
                          s_out=s[3 + i], quant=quant)
            rslot = 3 + i
        h = f8_conv(t, s[1 + i], raw[name + "c2_w"], *fold(name + "n2"), 1, 1, res=res,
                    s_res=s[rslot], relu=True, s_out=None if last else s[2 + i], quant=quant)
        src, i = 2 + i, i + (3 if down else 2)
    if quantise:
        h = h.to(torch.float32).to(torch.bfloat16).to(F64)
    return h.mean(dim=(1, 2)) @ pv["fc_w"] + pv["fc_b"]
