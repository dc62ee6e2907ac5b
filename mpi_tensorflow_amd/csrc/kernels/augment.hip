// Per-pass shift / flip augmentation fused with the row shuffle (augment.h).
//
// The same memory-bound gather of whole rows as shuffle.hip: one workgroup
// writes a 16 KB piece of one destination row (blockIdx.y picks the piece) and
// walks the rows with a grid stride.  The source row s = perm(i), its draw
// (dy, dx, flipped) and the row bases depend on blockIdx and the trip only, so
// they are uniform over the workgroup and live in scalar registers: the
// Feistel walk, the three hashes and the two modulos run once per row piece.
//
// A thread owns 4 consecutive destination floats (one aligned 16-byte store).
// Without a flip their sources are 4 consecutive floats at the uniform element
// distance dy * W * C + dx * C, in general not 16-byte aligned: one unaligned
// 16-byte load when all four lie inside the image, so consecutive lanes read
// consecutive 16-byte runs and a wave covers 1 KB of whole lines.  Around the
// fill border, and in flipped rows (pixel order reversed, channel order kept),
// the four are single loads: the lines they touch are the same ones.
#include "augment.h"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "common.h"
#include "shuffle.h"

namespace augment {

namespace {

constexpr int THREADS = 256;
constexpr int PER_THREAD = 4;                  // stores a thread issues per row piece
constexpr int PIECE = THREADS * PER_THREAD;    // ... of a workgroup
constexpr int MAX_BLOCKS = 2048;               // 256 CUs x 8 resident workgroups

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

struct Geo {
  uint32_t H, W, C, wc;  // wc = W * C floats an image line
  uint32_t m_wc, m_c;    // floor(2^32 / d) + 1 for d = wc, C
  uint32_t key, span;    // span = 2 K + 1
  int K, flip;
  float fill;
};

uint32_t magic(uint32_t d) { return d > 1 ? (uint32_t)((1ull << 32) / d) + 1u : 0u; }

// n / d for n < 2^31 with m = floor(2^32 / d) + 1: m d = 2^32 + e, 0 < e <= d, so
// n m / 2^32 = n / d + n e / (d 2^32) overshoots n / d by less than 1: the
// estimate is the quotient or one more, and then the remainder is negative.
__device__ __forceinline__ uint32_t div_by(uint32_t n, uint32_t d, uint32_t m) {
  if (d == 1) return n;
  uint32_t q = __umulhi(n, m);
  if ((int)(n - q * d) < 0) --q;
  return q;
}

// The U destination floats from element e of a row: their source floats, or fill.
template <int U>
__device__ __forceinline__ void gather(const float* __restrict__ a, const Geo& g, uint32_t e,
                                       int dy, int dx, bool fl, float* o) {
  uint32_t y = div_by(e, g.wc, g.m_wc);
  uint32_t r = e - y * g.wc;
  uint32_t off[U];
  bool ok[U];
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const uint32_t sy = y + (uint32_t)dy;  // (a negative coordinate wraps past H, W)
    uint32_t sr;
    bool in;
    if (fl) {
      const uint32_t x = div_by(r, g.C, g.m_c), c = r - x * g.C;
      const uint32_t sx = g.W - 1u - x + (uint32_t)dx;
      in = sx < g.W;
      sr = sx * g.C + c;
    } else {
      sr = r + (uint32_t)(dx * (int)g.C);
      in = sr < g.wc;
    }
    ok[k] = in && sy < g.H;
    off[k] = sy * g.wc + sr;
    if (++r == g.wc) {
      r = 0;
      ++y;
    }
  }
  if constexpr (U == 4) {
    // not flipped and all inside: off[k] = e + k + dy * wc + dx * C, also across a line end
    if (!fl && ok[0] && ok[1] && ok[2] && ok[3]) {
      const f32x4u v = *reinterpret_cast<const f32x4u*>(a + off[0]);
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = v[k];
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < U; ++k) o[k] = ok[k] ? a[off[k]] : g.fill;
}

// U = 4 (row_vecs = row_elems / 4, aligned f32x4 stores) or 1 (row_vecs = row_elems)
template <int U>
__global__ __launch_bounds__(THREADS) void rows_kernel(const float* __restrict__ src_x,
                                                       const int* __restrict__ src_y,
                                                       float* __restrict__ dst_x,
                                                       int* __restrict__ dst_y, shuffle::Perm p,
                                                       int use_perm, Geo g, long long row_vecs) {
  const long long v0 = (long long)blockIdx.y * PIECE + threadIdx.x;
  const long long row_elems = row_vecs * U;
  const long long n = p.n;
  for (long long i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t s = use_perm ? shuffle::perm_of(p, (uint32_t)i) : (uint32_t)i;
    const uint32_t h0 = mix32(g.key ^ s), h1 = mix32(h0 + 0x9E3779B9u),
                   h2 = mix32(h1 + 0x9E3779B9u);
    const int dy = (int)(h0 % g.span) - g.K, dx = (int)(h1 % g.span) - g.K;
    const bool fl = g.flip && (h2 >> 31);
    const float* a = src_x + (long long)s * row_elems;
    float* d = dst_x + i * row_elems;
    float o[PER_THREAD][U];
#pragma unroll
    for (int u = 0; u < PER_THREAD; ++u) {
      const long long v = v0 + u * THREADS;
      if (v < row_vecs) gather<U>(a, g, (uint32_t)(v * U), dy, dx, fl, o[u]);
    }
#pragma unroll
    for (int u = 0; u < PER_THREAD; ++u) {
      const long long v = v0 + u * THREADS;
      if (v < row_vecs) {
        if constexpr (U == 4) {
          const f32x4 t = {o[u][0], o[u][1], o[u][2], o[u][3]};
          reinterpret_cast<f32x4*>(d)[v] = t;
        } else {
          d[v] = o[u][0];
        }
      }
    }
    if (src_y && blockIdx.y == 0 && threadIdx.x == 0) dst_y[i] = src_y[s];
  }
}

template <int U>
void launch_rows(const float* src_x, const int* src_y, float* dst_x, int* dst_y,
                 const shuffle::Perm& p, bool use_perm, const Geo& g, long long row_vecs,
                 hipStream_t st) {
  const long long pieces = (row_vecs + PIECE - 1) / PIECE;
  if (pieces > 65535) throw std::runtime_error("augment_rows: row too long");
  const long long gx = std::max(1ll, std::min((long long)p.n, MAX_BLOCKS / pieces));
  rows_kernel<U><<<dim3((unsigned)gx, (unsigned)pieces), THREADS, 0, st>>>(
      src_x, src_y, dst_x, dst_y, p, use_perm ? 1 : 0, g, row_vecs);
}

bool overlap(const void* a, const void* b, unsigned long long bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + bytes && y < x + bytes;
}

}  // namespace

void augment_rows(const float* src_x, const int* src_y, float* dst_x, int* dst_y, long long n,
                  int H, int W, int C, bool use_perm, uint32_t perm_key, uint32_t aug_key, int K,
                  bool flip, float fill, hipStream_t st) {
  if (n < 0 || n > 0x7FFFFFFFll) throw std::runtime_error("augment_rows: n out of range");
  if (H <= 0 || W <= 0 || C <= 0) throw std::runtime_error("augment_rows: H, W, C must be positive");
  const long long row_elems = (long long)H * W * C;
  if (row_elems > 0x7FFFFFFFll) throw std::runtime_error("augment_rows: image too large");
  if (K < 0 || K >= std::min(H, W))
    throw std::runtime_error("augment_rows: shift K must be in [0, min(H, W))");
  if (!src_x || !dst_x || (src_y && !dst_y)) throw std::runtime_error("augment_rows: null buffer");
  if (n == 0) return;
  if (overlap(src_x, dst_x, (unsigned long long)n * row_elems * sizeof(float)) ||
      (src_y && overlap(src_y, dst_y, (unsigned long long)n * sizeof(int))))
    throw std::runtime_error("augment_rows: src and dst overlap");
  const shuffle::Perm p = shuffle::make_perm(perm_key, n);
  Geo g;
  g.H = H, g.W = W, g.C = C, g.wc = (uint32_t)W * C;
  g.m_wc = magic(g.wc), g.m_c = magic(g.C);
  g.key = aug_key, g.span = 2u * K + 1u;
  g.K = K, g.flip = flip ? 1 : 0, g.fill = fill;
  const bool vec = row_elems % 4 == 0 && (reinterpret_cast<uintptr_t>(src_x) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(dst_x) & 15) == 0;
  if (vec)
    launch_rows<4>(src_x, src_y, dst_x, dst_y, p, use_perm, g, row_elems / 4, st);
  else
    launch_rows<1>(src_x, src_y, dst_x, dst_y, p, use_perm, g, row_elems, st);
}

}  // namespace augment
