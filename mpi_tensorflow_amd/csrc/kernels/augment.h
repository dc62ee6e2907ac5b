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

// The same load with a random rotation, zoom and erased square on top (rotate:D,
// scale:P, cutout:S): a per-row inverse affine map with bilinear sampling.  The
// draw chain goes on, h_{k+1} = mix32(h_k + GOLDEN) up to h6:
//   ia = h3 % 129, ib = h4 % 129    levels into `tables` = cosT | sinT | invT,
//                                   3 x 129 device int32 in Q16 (rng.affine_tables)
//   cy0 = h5 % (H - S + 1), cx0 = h6 % (W - S + 1)    the cutout's corner, S > 0
//   m00 = m11 = r(cosT[ia] invT[ib]), m01 = r(sinT[ia] invT[ib]),
//   m10 = r(-sinT[ia] invT[ib]),  r(v) = (v + 32768) >> 16 in 64 bits
// Source coordinate of output pixel (y, x) in Q17, u2 = 2x - (W-1), v2 = 2y - (H-1):
//   SX = m00 u2 + m01 v2 + ((W-1) << 16); flipped: SX = ((W-1) << 17) - SX; SX += dx << 17
//   SY = m10 u2 + m11 v2 + ((H-1) << 16);                                   SY += dy << 17
//   ix = SX >> 17, fx = (SX & 0x1FFFF) 2^-17, likewise iy, fy; taps outside = fill
//   out = (1 - fy) ((1 - fx) p00 + fx p01) + fy ((1 - fx) p10 + fx p11)
// with every -, * and + one rounded fp32 operation (no fused multiply-add), and
// fill inside the cutout square.  Identical to utils/rng.py affine_params /
// affine_np, bit for bit.  H, W <= 1024 (the coordinates are 32-bit); S = 0: no
// cutout.  Otherwise the contract of augment_rows.
void affine_rows(const float* src_x, const int* src_y, float* dst_x, int* dst_y, long long n,
                 int H, int W, int C, bool use_perm, uint32_t perm_key, uint32_t aug_key, int K,
                 bool flip, float fill, const int* tables, int S, hipStream_t st);

// mixup / cutmix of a loaded pass (--mix): dst row i = src row i blended with
// its partner row j of the same pass.  The draw of row i (rng.mix_params):
//   g0 = mix32(mix_key ^ i), g1 = mix32(g0 + GOLDEN), g2 = mix32(g1 + GOLDEN)
//   level = g0 % 129 into `table` = wq | bh | bw, 3 x 129 device int32 (rng.mix_table)
//   j = perm(i) of shuffle.h under the key mix32(mix_key ^ GOLDEN)
//   cy = g1 % (H - bh + 1), cx = g2 % (W - bw + 1)
//   lam = (65536 - wq) 2^-16, w = wq 2^-16
//   mixup:  dst = lam src[i] + w src[j], each product and the sum one rounded
//           fp32 operation (no fused multiply-add)
//   cutmix: dst = src[j] for cy <= y < cy + bh, cx <= x < cx + bw, src[i] elsewhere
//   dst_y[i] = src_y[i], dst_y2[i] = src_y[j], dst_lam[i] = lam
// Identical to utils/rng.py mix_np, bit for bit.  H, W <= 1024.  Rows of dst at n
// and above and all of src are not written.  One launch, no allocation, no
// sync: capturable into a hipGraph.
void mix_rows(const float* src_x, const int* src_y, float* dst_x, int* dst_y, int* dst_y2,
              float* dst_lam, long long n, int H, int W, int C, bool cutmix, uint32_t mix_key,
              const int* table, hipStream_t st);

}  // namespace augment
