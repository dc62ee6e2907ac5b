// Per-pass row shuffle of a device-resident shard (--shuffle).
//
// perm is a pure function of (key, n): a balanced 4-round Feistel network over
// [0, 2^bits), bits = the even bit length of n - 1 (at least 2), walked along
// its cycle until it lands below n.  Identical to utils/rng.py shuffle_perm.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace shuffle {

// dst_x[i] = src_x[perm(i)], dst_y[i] = src_y[perm(i)] for i < n; rows of
// row_elems floats.  Rows of dst at n and above and all of src are not written.
// No index buffer and no host state: capturable into a hipGraph.
void shuffle_rows(const float* src_x, const int* src_y, float* dst_x, int* dst_y, long long n,
                  long long row_elems, uint32_t key, hipStream_t st);

// out[i] = perm(i) for i < n
void shuffle_perm(int* out, long long n, uint32_t key, hipStream_t st);

}  // namespace shuffle

// The permutation itself, for the kernels that walk it (shuffle.hip,
// augment.hip); common.h holds device code, so HIP translation units only.
#ifdef __HIPCC__
#include <algorithm>

#include "common.h"

namespace shuffle {

struct Perm {
  uint32_t n, h, mask, rk[4];
};

inline Perm make_perm(uint32_t key, long long n) {
  Perm p;
  p.n = (uint32_t)n;
  uint32_t bits = 0;
  for (uint64_t v = (uint64_t)(n - 1); v; v >>= 1) ++bits;
  bits = std::max(bits, 2u);
  bits += bits & 1u;
  p.h = bits / 2;
  p.mask = (1u << p.h) - 1u;
  for (uint32_t r = 0; r < 4; ++r) p.rk[r] = mix32(key + r * 0x9E3779B9u);
  return p;
}

__host__ __device__ __forceinline__ uint32_t feistel(const Perm& p, uint32_t x) {
  uint32_t l = x >> p.h, r = x & p.mask;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t t = l ^ (mix32(r ^ p.rk[k]) & p.mask);
    l = r;
    r = t;
  }
  return (l << p.h) | r;
}

// F is a bijection of [0, 2^bits) and i < n: the walk stays on the cycle of i,
// which holds i itself, so it ends.
__host__ __device__ __forceinline__ uint32_t perm_of(const Perm& p, uint32_t i) {
  uint32_t x = feistel(p, i);
  while (x >= p.n) x = feistel(p, x);
  return x;
}

}  // namespace shuffle
#endif  // __HIPCC__
