// Per-pass training augmentation of a device-resident shard (--augment):
// random shift (translation, the pixels shifted in are `fill`) and horizontal
// flip of NHWC fp32 images, fused with the row shuffle.
//
// The draw of a row is a pure function of (aug_key, pristine row index s):
//   h0 = mix32(aug_key ^ s), h1 = mix32(h0 + GOLDEN), h2 = mix32(h1 + GOLDEN)
//   dy = h0 % (2K + 1) - K, dx = h1 % (2K + 1) - K, flipped = flip && (h2 >> 31)
//   out[y][x][c] = src[y + dy][(flipped ? W - 1 - x : x) + dx][c], or fill
//   where that pixel lies outside the image.
// Identical to utils/rng.py augment_params / augment_np.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace augment {

// dst row i = transform of src row s, s = perm(i) of shuffle.h with perm_key
// when use_perm is set, else s = i; dst_y[i] = src_y[s] (src_y may be null).
// n rows of H x W x C floats.  Rows of dst at n and above and all of src are
// not written.  One launch, no allocation, no sync: capturable into a hipGraph.
void augment_rows(const float* src_x, const int* src_y, float* dst_x, int* dst_y, long long n,
                  int H, int W, int C, bool use_perm, uint32_t perm_key, uint32_t aug_key, int K,
                  bool flip, float fill, hipStream_t st);

}  // namespace augment
