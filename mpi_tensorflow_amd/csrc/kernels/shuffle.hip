// Per-pass row shuffle of the device-resident shard (shuffle.h).
//
// A memory-bound gather of whole rows: one workgroup copies a 16 KB piece of
// one row (blockIdx.y picks the piece, so a 602 KB ResNet row spreads over 37
// workgroups and a 3 KB MNIST row is one piece) and walks the rows with a grid
// stride, two rows in flight per trip.  perm(i) depends on blockIdx and the
// trip only, so it is uniform over the workgroup and the compiler keeps the
// Feistel walk in scalar registers: once per row piece, not per element.
#include "shuffle.h"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "common.h"

namespace shuffle {

namespace {

constexpr int THREADS = 256;
constexpr int PER_THREAD = 4;                  // vectors a thread moves per row piece
constexpr int PIECE = THREADS * PER_THREAD;    // vectors per row piece
constexpr int MAX_BLOCKS = 2048;               // 256 CUs x 8 resident workgroups

// V = f32x4 (row_vecs = row_elems / 4; the ext vector, not the float4 struct, whose
// predicated copies clang parks in scratch) or float (row_vecs = row_elems)
template <class V>
__global__ __launch_bounds__(THREADS) void rows_kernel(const V* __restrict__ src_x,
                                                       const int* __restrict__ src_y,
                                                       V* __restrict__ dst_x,
                                                       int* __restrict__ dst_y, Perm p,
                                                       long long row_vecs) {
  const long long v0 = (long long)blockIdx.y * PIECE + threadIdx.x;
  const long long n = p.n;
  for (long long i0 = blockIdx.x; i0 < n; i0 += 2ll * gridDim.x) {
    const long long i1 = i0 + gridDim.x;
    const bool two = i1 < n;
    const long long s0 = perm_of(p, (uint32_t)i0);
    const long long s1 = two ? (long long)perm_of(p, (uint32_t)i1) : s0;
    const V* a0 = src_x + s0 * row_vecs;
    const V* a1 = src_x + s1 * row_vecs;
    V r0[PER_THREAD], r1[PER_THREAD];
#pragma unroll
    for (int u = 0; u < PER_THREAD; ++u) {
      const long long v = v0 + u * THREADS;
      if (v < row_vecs) {
        r0[u] = a0[v];
        if (two) r1[u] = a1[v];
      }
    }
    V* d0 = dst_x + i0 * row_vecs;
    V* d1 = dst_x + i1 * row_vecs;
#pragma unroll
    for (int u = 0; u < PER_THREAD; ++u) {
      const long long v = v0 + u * THREADS;
      if (v < row_vecs) {
        d0[v] = r0[u];
        if (two) d1[v] = r1[u];
      }
    }
    if (src_y && blockIdx.y == 0 && threadIdx.x == 0) {
      dst_y[i0] = src_y[s0];
      if (two) dst_y[i1] = src_y[s1];
    }
  }
}

__global__ __launch_bounds__(THREADS) void perm_kernel(int* __restrict__ out, Perm p) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += stride)
    out[i] = (int)perm_of(p, (uint32_t)i);
}

void check_n(long long n, const char* what) {
  if (n < 0 || n > 0x7FFFFFFFll) throw std::runtime_error(std::string(what) + ": n out of range");
}

template <class V>
void launch_rows(const float* src_x, const int* src_y, float* dst_x, int* dst_y, const Perm& p,
                 long long row_vecs, hipStream_t st) {
  const long long pieces = (row_vecs + PIECE - 1) / PIECE;
  if (pieces > 65535) throw std::runtime_error("shuffle_rows: row too long");
  const long long gx = std::max(1ll, std::min((long long)p.n, MAX_BLOCKS / pieces));
  rows_kernel<V><<<dim3((unsigned)gx, (unsigned)pieces), THREADS, 0, st>>>(
      reinterpret_cast<const V*>(src_x), src_y, reinterpret_cast<V*>(dst_x), dst_y, p, row_vecs);
}

}  // namespace

void shuffle_rows(const float* src_x, const int* src_y, float* dst_x, int* dst_y, long long n,
                  long long row_elems, uint32_t key, hipStream_t st) {
  check_n(n, "shuffle_rows");
  if (row_elems <= 0) throw std::runtime_error("shuffle_rows: row_elems must be positive");
  if (n == 0) return;
  if (!src_x || !dst_x || (src_y && !dst_y)) throw std::runtime_error("shuffle_rows: null buffer");
  const Perm p = make_perm(key, n);
  const bool vec = row_elems % 4 == 0 && (reinterpret_cast<uintptr_t>(src_x) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(dst_x) & 15) == 0;
  if (vec)
    launch_rows<f32x4>(src_x, src_y, dst_x, dst_y, p, row_elems / 4, st);
  else
    launch_rows<float>(src_x, src_y, dst_x, dst_y, p, row_elems, st);
}

void shuffle_perm(int* out, long long n, uint32_t key, hipStream_t st) {
  check_n(n, "shuffle_perm");
  if (n == 0) return;
  if (!out) throw std::runtime_error("shuffle_perm: null buffer");
  const Perm p = make_perm(key, n);
  const long long blocks = std::min<long long>((n + THREADS - 1) / THREADS, MAX_BLOCKS);
  perm_kernel<<<(unsigned)blocks, THREADS, 0, st>>>(out, p);
}

}  // namespace shuffle
