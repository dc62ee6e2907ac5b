// Inference from a checkpoint (runtime/predict.py): the two kernels around the
// engines' forward launches.
//
//   prep : one view of n source rows [n][H][W][C] (uint8 or fp32) as fp32 NHWC:
//          dst[i][y][x][c] = norm(src[i][y + dy][(flip ? W - 1 - x : x) + dx][c]),
//          or fill where that pixel lies outside the image - the definitions of
//          augment.h / utils/rng.py augment_np with one (dy, dx, flip) for the
//          whole launch (a test-time-augmentation view; (0, 0, false) is the
//          plain uint8 -> fp32 normalisation).  The flip mirrors x, never c.
//          norm: uint8 p -> lut[p] (256 floats, made on the host by the
//          expression of utils/data.py extract_data, so bit-identical to it);
//          fp32 -> identity.
//   head : per row, acc += softmax(logits) over the views in view order, and
//          after the last view the averaged probabilities, the scores and the
//          top k classes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace predict {

// src_u8: src is uint8 (lut must hold 256 floats), else fp32 (lut unused).
// Rows of dst at n and above and all of src are not written.  |dy| < H,
// |dx| < W.  One launch, no allocation, no sync.
void prep(const void* src, bool src_u8, float* dst, long long n, int H, int W, int C, int dy,
          int dx, bool flip, float fill, const float* lut, hipStream_t st);

// logits [n][C] of view `view` (0 <= view < views), 1 <= C <= 64, 1 <= k <= C.
// views == 1: acc is not touched (may be null).  views > 1: acc [n][C] is set
// by view 0 and added to by the later ones.  The last view writes
//   probs [n][C]     acc / views (views == 1: the softmax itself); may be null
//   scores [n][C]    views == 1: the logits; else logf(max(probs, FLT_MIN)); may be null
//   topk_class [n][k], topk_prob [n][k]: k rounds of "lowest index among the
//                    maximal keys not taken yet", key = logits (views == 1) or
//                    probs; topk_prob = probs at those classes.
// One launch, no allocation, no sync.
void head(const float* logits, float* acc, int n, int C, int view, int views, int k, float* probs,
          float* scores, int* topk_class, float* topk_prob, hipStream_t st);

}  // namespace predict
