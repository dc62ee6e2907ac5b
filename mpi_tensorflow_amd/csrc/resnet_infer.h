// Native bf16 inference forward of ResNet-18 (models/generic.py ResNet18).
//
// Like LenetExecutor::eval_chunk: one static call enqueues the forward of a
// chunk of rows on a HIP stream, in plain C++ - no allocation, no host
// synchronisation, one stream, a linear chain of launches (capturable):
//   s2d_stem_input -> stem conv (bn1 + ReLU in its epilogue) -> max pool
//   -> 8 BasicBlocks -> avgpool_fc
// A BasicBlock on input h:
//   sc = affine(conv_ds(h))            (blocks with a shortcut conv; no ReLU)
//   t  = relu(affine(conv_c1(h)))
//   h' = relu(affine(conv_c2(t)) + res),  res = sc or h
// Every BatchNorm is a folded per-channel (a, b) pair of bn_fold's table,
// applied in the producing conv's epilogue (conv_fwd_affine_bf16); every
// activation between two launches is bf16 (eval_chunk) or, behind the max pool
// of eval_chunk_f8, e4m3 with one calibrated scale a tensor; eval_chunk_x3 runs
// the same chain on bf16 hi / lo pairs (conv_x3.hip).  Each bf16 conv runs the plan
// plan_fwd_bf16(shape, ConvHave{}) gives - what ops.conv_route reports.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

struct ResnetInferPtrs {
  int H = 224, W = 224;  // input image (3 channels, NHWC fp32)
  int classes = 10;
  // bf16 weight operands: the stem's 8x8-extended filter (s2d_stem_weight) and
  // the forward copies (wcvt_batch mode 0) in forward order - per block c1,
  // c2, then ds where the block has a shortcut conv (19 in all)
  uintptr_t wt8 = 0;
  std::vector<uintptr_t> wt;
  // bn_fold's table [2][fold_total] and the channel offset of every BatchNorm:
  // bn1, then per block n1, n2, then nd where it has one (20 in all)
  uintptr_t fold = 0;
  int fold_total = 0;
  std::vector<int> fold_off;
  uintptr_t fc_w = 0, fc_b = 0;  // fp32 [512][classes], [classes]
  // the fp8 forward (docs/ACCURACY.md "ResNet-18 fp8 inference"): wq_f8's e4m3
  // codes [tap][k][c] in the order of wt; amax, the calibration table of 20
  // floats (slot 0 the pool output, 1 + i the output of conv i); f8_fold's a2
  // [fold_total] (conv i at fold_off[1 + i]) and scal [2 * 19 + 1] (s_res,
  // 1 / s_out per conv, 1 / s_pool); calibrated: amax has been filled and folded
  std::vector<uintptr_t> w8;
  uintptr_t amax = 0, a2 = 0, scal = 0;
  bool calibrated = false;
  // the mxfp4 forward (docs/ACCURACY.md "ResNet-18 mxfp4 inference") is the fp8
  // forward with MXFP4 weights: w8 holds wq_mx4's slabs, the convs are mx4conv,
  // and f8_fold ran on a weight-scale table of ones
  bool mx4 = false;
  // the bf16x3 forward (docs/ACCURACY.md "ResNet-18 bf16x3 inference"): the
  // split stem filter (s2d_stem_weight_x3, planes [2][64][256]) and wsplit_x3's
  // plane pairs [2][tap][k][c] in the order of wt.  x3: the buffers are sized
  // for it - an activation element is a hi / lo pair, 4 bytes, and no conv
  // takes a workspace
  uintptr_t wt8x3 = 0;
  std::vector<uintptr_t> wx3;
  bool x3 = false;
};

struct ResnetInferSizes {
  // three activation buffers (elements of act_bytes bytes: bf16, or a bf16x3
  // pair) and the fp32 split-K workspace (floats)
  long long act[3] = {0, 0, 0};
  long long ws_floats = 0;
  int act_bytes = 2;
};

class ResnetInfer {
 public:
  // rows a chunk may hold: the 32-bit pixel x channel offsets of the halo conv
  // (conv3_ok) and of the pool on the 112 x 112 x 64 stem output
  static int max_rows(const ResnetInferPtrs& p);
  // buffers that serve every chunk of 1 .. m rows (the workspace a chunk
  // needs does not grow with its rows: small chunks split K, large ones do not)
  static ResnetInferSizes ws_sizes(const ResnetInferPtrs& p, int m);
  // logits [m][classes] of the m fp32 rows at x; ws holds ws_floats floats,
  // and a chunk whose plans need more is refused
  static void eval_chunk(const ResnetInferPtrs& p, uintptr_t x, int m, uintptr_t act0,
                         uintptr_t act1, uintptr_t act2, uintptr_t ws, long long ws_floats,
                         uintptr_t logits, hipStream_t s);
  // eval_chunk with an amax_b16 launch behind every tensor the fp8 forward
  // quantises, joined into p.amax (which accumulates across chunks)
  static void calibrate_chunk(const ResnetInferPtrs& p, uintptr_t x, int m, uintptr_t act0,
                              uintptr_t act1, uintptr_t act2, uintptr_t ws, long long ws_floats,
                              uintptr_t logits, hipStream_t s);
  // the fp8 forward: the bf16 stem, maxpool_infer_f8, 19 f8conv launches (the
  // last one writes bf16), avgpool_fc.  The same three buffers (their bytes
  // suffice), no workspace: no conv splits K, so a row's logits do not depend
  // on the chunk it arrives in.  Refuses an uncalibrated or incomplete p.
  // p.mx4: the same chain with 19 mx4conv launches on wq_mx4's slabs.
  static void eval_chunk_f8(const ResnetInferPtrs& p, uintptr_t x, int m, uintptr_t act0,
                            uintptr_t act1, uintptr_t act2, uintptr_t logits, hipStream_t s);
  // the bf16x3 forward: s2d_stem_input_x3, the stem, maxpool_infer_x3, 19
  // x3conv launches in eval_chunk's order, avgpool_fc_x3.  Every activation is
  // a split tensor at the start of its buffer (ws_sizes with p.x3), no
  // workspace: no conv splits K, so a row's logits do not depend on the chunk
  // it arrives in.  Refuses an incomplete p.
  static void eval_chunk_x3(const ResnetInferPtrs& p, uintptr_t x, int m, uintptr_t act0,
                            uintptr_t act1, uintptr_t act2, uintptr_t logits, hipStream_t s);
};
