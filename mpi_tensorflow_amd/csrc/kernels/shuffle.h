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
