#include "resnet_infer.h"

#include <algorithm>
#include <stdexcept>

#include "kernels/ops_generic.h"

namespace {

using gops::ConvShape;

template <class T>
inline T* P(uintptr_t v) {
  return reinterpret_cast<T*>(v);
}

ConvShape conv_shape(int N, int H, int W, int C, int K, int R, int stride, int pad) {
  return ConvShape{N, H, W, C, K, R, R, stride, pad, (H + 2 * pad - R) / stride + 1,
                   (W + 2 * pad - R) / stride + 1};
}

struct Block {
  ConvShape c1, c2, ds;
  bool down;
};

// the layer shapes of a chunk of m rows (models/generic.py ResNet18)
struct Net {
  ConvShape stem, s2d;  // the 7x7 / 2 / 3 conv and its 4x4 space-to-depth form
  gops::PoolShape pool;
  Block blocks[8];
  int fh, fw;  // the final feature map
  Net(const ResnetInferPtrs& p, int m) {
    stem = conv_shape(m, p.H, p.W, 3, 64, 7, 2, 3);
    s2d = ConvShape{m, stem.OH + 3, stem.OW + 3, 16, 64, 4, 4, 1, 0, stem.OH, stem.OW};
    pool = gops::PoolShape{m, stem.OH, stem.OW, 64, 3, 2, 1, (stem.OH + 2 - 3) / 2 + 1,
                           (stem.OW + 2 - 3) / 2 + 1};
    const int stages[4][2] = {{64, 1}, {128, 2}, {256, 2}, {512, 2}};
    int h = pool.OH, w = pool.OW, cin = 64, b = 0;
    for (const auto& st : stages)
      for (int bi = 0; bi < 2; ++bi, ++b) {
        const int c = st[0], s = bi == 0 ? st[1] : 1;
        Block& k = blocks[b];
        k.down = s != 1 || cin != c;
        k.c1 = conv_shape(m, h, w, cin, c, 3, s, 1);
        k.c2 = conv_shape(m, k.c1.OH, k.c1.OW, c, c, 3, 1, 1);
        k.ds = conv_shape(m, h, w, cin, c, 1, s, 0);
        h = k.c1.OH, w = k.c1.OW, cin = c;
      }
    fh = h, fw = w;
  }
};

long long out_elems(const ConvShape& s) { return (long long)s.N * s.OH * s.OW * s.K; }

void check(const ResnetInferPtrs& p, int m) {
  if (p.H < 32 || p.W < 32) throw std::runtime_error("ResnetInfer: the image must be 32 x 32 or larger");
  if (m < 1 || m > ResnetInfer::max_rows(p))
    throw std::runtime_error("ResnetInfer: chunk rows outside [1, max_rows]");
}

// the convs of a chunk, in launch order
template <class F>
void each_conv(const Net& n, F f) {
  for (const Block& b : n.blocks) {
    if (b.down) f(b.ds);
    f(b.c1);
    f(b.c2);
  }
}

// workspace floats of a chunk of exactly m rows.  NOT monotone in m: small
// chunks split K (slabs behind the weight-copy region) where large ones do not
long long ws_floats_at(const ResnetInferPtrs& p, int m) {
  long long f = 0;
  each_conv(Net(p, m), [&](const ConvShape& s) {
    f = std::max(f, gops::plan_fwd_bf16(s, gops::ConvHave{}).ws_floats);
  });
  return f;
}

void conv(const ConvShape& s, const void* x, uintptr_t wt, const ResnetInferPtrs& p, int bn,
          const void* res, bool relu, void* y, float* ws, hipStream_t st) {
  const float* fold = P<const float>(p.fold);
  const int off = p.fold_off[bn];
  gops::conv_fwd_affine_bf16(gops::plan_fwd_bf16(s, gops::ConvHave{}), x, P<const void>(wt),
                             fold + off, fold + p.fold_total + off, res, relu, y, ws, st);
}

// The 19 convs of the eight residual blocks in launch order (a down block: ds,
// c1, c2), on the three rotating buffers: conv(shape, in, out, i, res, relu,
// last), i the conv's place in the weight order (a block's c1, c2, ds; its
// BatchNorm is 1 + i), last set for the final block output.  Returns the index
// of the buffer that holds that output.
template <class F>
int walk_blocks(const Net& n, void* const (&act)[3], F conv) {
  int h = 1, t = 0, u = 2;  // the block input, c1's output, the shortcut / the next input
  size_t wi = 0;
  for (const Block& b : n.blocks) {
    const bool last = &b == &n.blocks[7];
    if (b.down) {
      conv(b.ds, act[h], act[u], wi + 2, nullptr, false, false);
      conv(b.c1, act[h], act[t], wi, nullptr, true, false);
      conv(b.c2, act[t], act[h], wi + 1, act[u], true, last);
      wi += 3;
    } else {
      conv(b.c1, act[h], act[t], wi, nullptr, true, false);
      conv(b.c2, act[t], act[u], wi + 1, act[h], true, last);
      std::swap(h, u);
      wi += 2;
    }
  }
  return h;
}

}  // namespace

int ResnetInfer::max_rows(const ResnetInferPtrs& p) {
  const Net n(p, 1);
  const long long per = std::max((long long)n.stem.OH * n.stem.OW * 64,
                                 (long long)n.s2d.H * n.s2d.W * 16);
  return (int)std::min<long long>(((1LL << 31) - 1) / per, 1 << 20);
}

ResnetInferSizes ResnetInfer::ws_sizes(const ResnetInferPtrs& p, int m) {
  check(p, m);
  const Net n(p, m);
  ResnetInferSizes z;
  long long blk = (long long)m * n.pool.OH * n.pool.OW * 64;
  each_conv(n, [&](const ConvShape& s) { blk = std::max(blk, out_elems(s)); });
  // the buffers serve every chunk of up to m rows (a ragged tail, a later
  // smaller call): the activations grow with the rows, the workspace does not,
  // so it is the maximum over every row count
  if (p.x3)
    z.act_bytes = 4;
  else
    for (int r = 1; r <= m; ++r) z.ws_floats = std::max(z.ws_floats, ws_floats_at(p, r));
  z.act[0] = std::max(blk, out_elems(n.stem));
  z.act[1] = std::max(blk, (long long)m * n.s2d.H * n.s2d.W * 16);
  z.act[2] = blk;
  return z;
}

namespace {

void check_bf16(const ResnetInferPtrs& p, int m, uintptr_t x, uintptr_t act0, uintptr_t act1,
                uintptr_t act2, uintptr_t ws, long long ws_floats, uintptr_t logits) {
  check(p, m);
  if (ws_floats < ws_floats_at(p, m))
    throw std::runtime_error("ResnetInfer: the split-K workspace is smaller than this chunk's "
                             "plans need (size it with ws_sizes)");
  if (p.wt.size() != 19 || p.fold_off.size() != 20 || !p.wt8 || !p.fold || !p.fc_w || !p.fc_b ||
      std::find(p.wt.begin(), p.wt.end(), (uintptr_t)0) != p.wt.end())
    throw std::runtime_error("ResnetInfer: 19 conv weight copies, the stem filter, 20 fold "
                             "offsets, the fold table and the FC are required");
  if (!x || !act0 || !act1 || !act2 || !ws || !logits)
    throw std::runtime_error("ResnetInfer: null buffer");
}

// the bf16 chain; amax (calibration): max |v| of every tensor the fp8 forward
// quantises joined into its slot - 0 the pool output, 1 + i the output of conv
// i (weight order: a block's c1, c2 = the block output, ds)
void run_bf16(const ResnetInferPtrs& p, uintptr_t x, int m, uintptr_t act0, uintptr_t act1,
              uintptr_t act2, uintptr_t ws, uintptr_t logits, float* amax, hipStream_t s) {
  const Net n(p, m);
  void* act[3] = {P<void>(act0), P<void>(act1), P<void>(act2)};
  float* wsf = P<float>(ws);
  const float* fold = P<const float>(p.fold);
  auto seen = [&](const void* t, long long elems, size_t slot) {
    if (amax) gops::amax_b16(t, elems, amax + slot, s);
  };
  gops::s2d_stem_input(P<const float>(x), m, p.H, p.W, n.stem.OH, n.stem.OW, act[1], s);
  gops::conv_fwd_s2d_stem_affine_bf16(n.s2d, act[1], P<const void>(p.wt8), fold + p.fold_off[0],
                                      fold + p.fold_total + p.fold_off[0], true, act[0], s);
  gops::maxpool_infer_b16(n.pool, act[0], act[1], s);
  seen(act[1], (long long)m * n.pool.OH * n.pool.OW * 64, 0);
  const int h = walk_blocks(n, act, [&](const ConvShape& cs, const void* in, void* out, size_t i,
                                        const void* res, bool relu, bool) {
    conv(cs, in, p.wt[i], p, 1 + (int)i, res, relu, out, wsf, s);
    seen(out, out_elems(cs), 1 + i);
  });
  gops::avgpool_fc(act[h], P<const float>(p.fc_w), P<const float>(p.fc_b), P<float>(logits), m,
                   n.fh * n.fw, 512, p.classes, s);
}

}  // namespace

void ResnetInfer::eval_chunk(const ResnetInferPtrs& p, uintptr_t x, int m, uintptr_t act0,
                             uintptr_t act1, uintptr_t act2, uintptr_t ws, long long ws_floats,
                             uintptr_t logits, hipStream_t s) {
  check_bf16(p, m, x, act0, act1, act2, ws, ws_floats, logits);
  run_bf16(p, x, m, act0, act1, act2, ws, logits, nullptr, s);
}

void ResnetInfer::calibrate_chunk(const ResnetInferPtrs& p, uintptr_t x, int m, uintptr_t act0,
                                  uintptr_t act1, uintptr_t act2, uintptr_t ws,
                                  long long ws_floats, uintptr_t logits, hipStream_t s) {
  check_bf16(p, m, x, act0, act1, act2, ws, ws_floats, logits);
  if (!p.amax) throw std::runtime_error("ResnetInfer: calibrate_chunk needs the amax table");
  run_bf16(p, x, m, act0, act1, act2, ws, logits, P<float>(p.amax), s);
}

void ResnetInfer::eval_chunk_f8(const ResnetInferPtrs& p, uintptr_t x, int m, uintptr_t act0,
                                uintptr_t act1, uintptr_t act2, uintptr_t logits, hipStream_t s) {
  check(p, m);
  if (!p.calibrated)
    throw std::runtime_error("ResnetInfer: the fp8 forward is not calibrated (calibrate_chunk, "
                             "then f8_fold)");
  if (p.w8.size() != 19 || p.fold_off.size() != 20 || !p.wt8 || !p.fold || !p.a2 || !p.scal ||
      !p.fc_w || !p.fc_b || std::find(p.w8.begin(), p.w8.end(), (uintptr_t)0) != p.w8.end())
    throw std::runtime_error("ResnetInfer: 19 fp8 weight codes, the stem filter, 20 fold offsets, "
                             "the fold, a2 and scale tables and the FC are required");
  if (!x || !act0 || !act1 || !act2 || !logits) throw std::runtime_error("ResnetInfer: null buffer");
  const Net n(p, m);
  void* act[3] = {P<void>(act0), P<void>(act1), P<void>(act2)};
  const float* fold = P<const float>(p.fold);
  const float* a2 = P<const float>(p.a2);
  const float* scal = P<const float>(p.scal);
  gops::s2d_stem_input(P<const float>(x), m, p.H, p.W, n.stem.OH, n.stem.OW, act[1], s);
  gops::conv_fwd_s2d_stem_affine_bf16(n.s2d, act[1], P<const void>(p.wt8), fold + p.fold_off[0],
                                      fold + p.fold_total + p.fold_off[0], true, act[0], s);
  gops::maxpool_infer_f8(n.pool, act[0], scal + 2 * 19, act[1], s);
  // conv i of the weight order: BatchNorm 1 + i, scales scal[i] / scal[19 + i]
  // (the final block output stays bf16 for avgpool_fc)
  auto conv8 = [&](const ConvShape& cs, const void* xin, void* y, size_t i, const void* res,
                   bool relu, bool last) {
    gops::F8Epi e;
    const int off = p.fold_off[1 + i];
    e.a2 = a2 + off, e.b = fold + p.fold_total + off;
    e.res = res, e.s_res = scal + i, e.inv_s_out = scal + 19 + i, e.relu = relu ? 1 : 0;
    if (p.mx4)
      gops::mx4conv(cs, xin, P<const void>(p.w8[i]), e, y, last, 0, s);
    else
      gops::f8conv(cs, xin, P<const void>(p.w8[i]), e, y, last, 0, 0, s);
  };
  const int h = walk_blocks(n, act, conv8);
  gops::avgpool_fc(act[h], P<const float>(p.fc_w), P<const float>(p.fc_b), P<float>(logits), m,
                   n.fh * n.fw, 512, p.classes, s);
}

void ResnetInfer::eval_chunk_x3(const ResnetInferPtrs& p, uintptr_t x, int m, uintptr_t act0,
                                uintptr_t act1, uintptr_t act2, uintptr_t logits, hipStream_t s) {
  check(p, m);
  if (!p.x3 || p.wx3.size() != 19 || p.fold_off.size() != 20 || !p.wt8x3 || !p.fold || !p.fc_w ||
      !p.fc_b || std::find(p.wx3.begin(), p.wx3.end(), (uintptr_t)0) != p.wx3.end())
    throw std::runtime_error("ResnetInfer: the bf16x3 forward needs x3 set (buffers of 4-byte "
                             "elements), 19 split weight plane pairs, the split stem filter, 20 "
                             "fold offsets, the fold table and the FC");
  if (!x || !act0 || !act1 || !act2 || !logits) throw std::runtime_error("ResnetInfer: null buffer");
  const Net n(p, m);
  void* act[3] = {P<void>(act0), P<void>(act1), P<void>(act2)};
  const float* fold = P<const float>(p.fold);
  // BatchNorm bn: 0 the stem's, 1 + i conv i's of the weight order
  auto conv3 = [&](const ConvShape& cs, const void* xin, void* y, uintptr_t w, int bn,
                   const void* res, bool relu) {
    gops::X3Epi e;
    const int off = p.fold_off[bn];
    e.a = fold + off, e.b = fold + p.fold_total + off, e.res = res, e.relu = relu ? 1 : 0;
    gops::x3conv(cs, xin, P<const void>(w), e, y, 0, s);
  };
  gops::s2d_stem_input_x3(P<const float>(x), m, p.H, p.W, n.stem.OH, n.stem.OW, act[1], s);
  conv3(n.s2d, act[1], act[0], p.wt8x3, 0, nullptr, true);
  gops::maxpool_infer_x3(n.pool, act[0], act[1], s);
  const int h = walk_blocks(n, act, [&](const ConvShape& cs, const void* in, void* out, size_t i,
                                        const void* res, bool relu, bool) {
    conv3(cs, in, out, p.wx3[i], 1 + (int)i, res, relu);
  });
  gops::avgpool_fc_x3(act[h], P<const float>(p.fc_w), P<const float>(p.fc_b), P<float>(logits), m,
                      n.fh * n.fw, 512, p.classes, s);
}
