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
//
// affine_rows (rotate / scale / cutout) keeps that shape; the seven hashes, the
// table reads and the Q16 matrix are per row and scalar as well, and each
// destination float is four guarded single loads and seven fp32 operations.
//
// mix_rows (mixup / cutmix) keeps that shape too: it blends the rows of one
// loaded pass with partner rows of the same pass.
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

// ---- rotate / scale / cutout: per-row inverse affine map, bilinear taps ----
// The draw of a row in the form the lanes use it: SX = ax u2 + bx v2 + cx and
// SY = ay u2 + by v2 + cy in Q17 pixels (augment.h; a flip negates ax and bx:
// ((W-1) << 17) - (A + ((W-1) << 16)) = -A + ((W-1) << 16)).  32-bit: with
// |m| <= 2^17, H, W <= 1024 and |dy|, |dx| < 1024 every sum stays below 2^29.
struct Row {
  int ax, bx, cx, ay, by, cy;
  int cy0, cx0;  // the cutout's corner
};

constexpr int LEVELS = 129;
constexpr int MAX_SIDE = 1024;

__device__ __forceinline__ int q16(long long v) { return (int)((v + 32768) >> 16); }

// One destination float: pixel (y, x), channel c of the row whose source row is a.
__device__ __forceinline__ float sample(const float* __restrict__ a, const Geo& g, const Row& r,
                                        int S, uint32_t y, uint32_t x, uint32_t c) {
#pragma clang fp contract(off)  // every *, +, - below is one rounded fp32 operation
  if (S > 0 && y - (uint32_t)r.cy0 < (uint32_t)S && x - (uint32_t)r.cx0 < (uint32_t)S)
    return g.fill;
  const int u2 = 2 * (int)x - (int)(g.W - 1u), v2 = 2 * (int)y - (int)(g.H - 1u);
  const int sx = r.ax * u2 + r.bx * v2 + r.cx, sy = r.ay * u2 + r.by * v2 + r.cy;
  const int ix = sx >> 17, iy = sy >> 17;  // floor
  const float fx = (float)(sx & 0x1FFFF) * 0x1p-17f, fy = (float)(sy & 0x1FFFF) * 0x1p-17f;
  const bool x0 = (uint32_t)ix < g.W, x1 = (uint32_t)(ix + 1) < g.W;
  const bool y0 = (uint32_t)iy < g.H, y1 = (uint32_t)(iy + 1) < g.H;
  const float* q = a + ((long long)iy * (int)g.W + ix) * (int)g.C + (int)c;  // tap (iy, ix)
  const float p00 = y0 && x0 ? q[0] : g.fill;
  const float p01 = y0 && x1 ? q[g.C] : g.fill;
  const float p10 = y1 && x0 ? q[g.wc] : g.fill;
  const float p11 = y1 && x1 ? q[g.wc + g.C] : g.fill;
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  const float t = gx * p00 + fx * p01;
  const float b = gx * p10 + fx * p11;
  return gy * t + fy * b;
}

// As rows_kernel: a workgroup per 16 KB piece of a destination row, the draw in
// scalar registers, U = 4 floats and one aligned 16-byte store a thread (or U = 1).
// The taps are read straight from the source row: the 4 floats of a thread and
// the 4 taps of each share cache lines with their neighbours in the wave.
template <int U>
__global__ __launch_bounds__(THREADS) void affine_kernel(const float* __restrict__ src_x,
                                                         const int* __restrict__ src_y,
                                                         float* __restrict__ dst_x,
                                                         int* __restrict__ dst_y, shuffle::Perm p,
                                                         int use_perm, Geo g,
                                                         const int* __restrict__ tab, int S,
                                                         long long row_vecs) {
  const long long v0 = (long long)blockIdx.y * PIECE + threadIdx.x;
  const long long row_elems = row_vecs * U;
  const long long n = p.n;
  for (long long i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t s = use_perm ? shuffle::perm_of(p, (uint32_t)i) : (uint32_t)i;
    uint32_t h[7];
    h[0] = mix32(g.key ^ s);
#pragma unroll
    for (int k = 1; k < 7; ++k) h[k] = mix32(h[k - 1] + 0x9E3779B9u);
    const int dy = (int)(h[0] % g.span) - g.K, dx = (int)(h[1] % g.span) - g.K;
    const bool fl = g.flip && (h[2] >> 31);
    const uint32_t ia = h[3] % LEVELS, ib = h[4] % LEVELS;
    const long long co = tab[ia], si = tab[LEVELS + ia], inv = tab[2 * LEVELS + ib];
    const int m00 = q16(co * inv), m01 = q16(si * inv), m10 = q16(-si * inv);
    Row r;
    r.ax = fl ? -m00 : m00, r.bx = fl ? -m01 : m01;
    r.cx = (int)((g.W - 1u) << 16) + dx * (1 << 17);
    r.ay = m10, r.by = m00;
    r.cy = (int)((g.H - 1u) << 16) + dy * (1 << 17);
    r.cy0 = S > 0 ? (int)(h[5] % (g.H - (uint32_t)S + 1u)) : 0;
    r.cx0 = S > 0 ? (int)(h[6] % (g.W - (uint32_t)S + 1u)) : 0;
    const float* a = src_x + (long long)s * row_elems;
    float* d = dst_x + i * row_elems;
    float o[PER_THREAD][U];
#pragma unroll
    for (int u = 0; u < PER_THREAD; ++u) {
      const long long v = v0 + u * THREADS;
      if (v < row_vecs) {
        const uint32_t e = (uint32_t)(v * U);
        uint32_t y = div_by(e, g.wc, g.m_wc);
        uint32_t x = div_by(e - y * g.wc, g.C, g.m_c);
        uint32_t c = e - y * g.wc - x * g.C;
#pragma unroll
        for (int k = 0; k < U; ++k) {
          o[u][k] = sample(a, g, r, S, y, x, c);
          if (++c == g.C) {
            c = 0;
            if (++x == g.W) x = 0, ++y;
          }
        }
      }
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

// ---- mixup / cutmix (--mix): blend the rows of a pass with partner rows ----
// The draw of working row i in scalar registers, as above: three hashes, the
// level's table entries, the Feistel walk to the partner j and the box corner.
// mixup: lam a + w b, each product and the sum one rounded fp32 operation;
// cutmix: b inside the box, a elsewhere.  Both rows are read as whole vectors
// (rows of one pass: the partner's lines are some other workgroup's own lines).
struct MixGeo {
  uint32_t H, W, C, wc;
  uint32_t m_wc, m_c;
  uint32_t key;
  int cutmix;
};

template <int U>
__global__ __launch_bounds__(THREADS) void mix_kernel(
    const float* __restrict__ src_x, const int* __restrict__ src_y, float* __restrict__ dst_x,
    int* __restrict__ dst_y, int* __restrict__ dst_y2, float* __restrict__ dst_lam,
    shuffle::Perm p, MixGeo g, const int* __restrict__ tab, long long row_vecs) {
#pragma clang fp contract(off)  // every * and + below is one rounded fp32 operation
  const long long v0 = (long long)blockIdx.y * PIECE + threadIdx.x;
  const long long row_elems = row_vecs * U;
  const long long n = p.n;
  for (long long i = blockIdx.x; i < n; i += gridDim.x) {
    const uint32_t g0 = mix32(g.key ^ (uint32_t)i), g1 = mix32(g0 + 0x9E3779B9u),
                   g2 = mix32(g1 + 0x9E3779B9u);
    const uint32_t level = g0 % LEVELS;
    const int wq = tab[level];
    const uint32_t bh = (uint32_t)tab[LEVELS + level], bw = (uint32_t)tab[2 * LEVELS + level];
    const uint32_t j = shuffle::perm_of(p, (uint32_t)i);
    const uint32_t cy = g1 % (g.H - bh + 1u), cx = g2 % (g.W - bw + 1u);
    const float lam = (float)(65536 - wq) * 0x1p-16f, w = (float)wq * 0x1p-16f;
    const float* a = src_x + i * row_elems;
    const float* b = src_x + (long long)j * row_elems;
    float* d = dst_x + i * row_elems;
    float o[PER_THREAD][U];
#pragma unroll
    for (int u = 0; u < PER_THREAD; ++u) {
      const long long v = v0 + u * THREADS;
      if (v < row_vecs) {
        float va[U], vb[U];
        if constexpr (U == 4) {
          const f32x4 ta = reinterpret_cast<const f32x4*>(a)[v];
          const f32x4 tb = reinterpret_cast<const f32x4*>(b)[v];
#pragma unroll
          for (int k = 0; k < 4; ++k) va[k] = ta[k], vb[k] = tb[k];
        } else {
          va[0] = a[v], vb[0] = b[v];
        }
        if (g.cutmix) {
          const uint32_t e = (uint32_t)(v * U);
          uint32_t y = div_by(e, g.wc, g.m_wc);
          uint32_t x = div_by(e - y * g.wc, g.C, g.m_c);
          uint32_t c = e - y * g.wc - x * g.C;
#pragma unroll
          for (int k = 0; k < U; ++k) {
            o[u][k] = (y - cy < bh && x - cx < bw) ? vb[k] : va[k];
            if (++c == g.C) {
              c = 0;
              if (++x == g.W) x = 0, ++y;
            }
          }
        } else {
#pragma unroll
          for (int k = 0; k < U; ++k) {
            const float pa = lam * va[k], pb = w * vb[k];
            o[u][k] = pa + pb;
          }
        }
      }
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
    if (blockIdx.y == 0 && threadIdx.x == 0) {
      dst_y[i] = src_y[i];
      dst_y2[i] = src_y[j];
      dst_lam[i] = lam;
    }
  }
}

// the grid of both kernels: (rows in flight, 16 KB pieces of a row)
dim3 rows_grid(const char* who, long long n, long long row_vecs) {
  const long long pieces = (row_vecs + PIECE - 1) / PIECE;
  if (pieces > 65535) throw std::runtime_error(std::string(who) + ": row too long");
  const long long gx = std::max(1ll, std::min(n, MAX_BLOCKS / pieces));
  return dim3((unsigned)gx, (unsigned)pieces);
}

template <int U>
void launch_rows(const float* src_x, const int* src_y, float* dst_x, int* dst_y,
                 const shuffle::Perm& p, bool use_perm, const Geo& g, long long row_vecs,
                 hipStream_t st) {
  rows_kernel<U><<<rows_grid("augment_rows", p.n, row_vecs), THREADS, 0, st>>>(
      src_x, src_y, dst_x, dst_y, p, use_perm ? 1 : 0, g, row_vecs);
}

template <int U>
void launch_affine(const float* src_x, const int* src_y, float* dst_x, int* dst_y,
                   const shuffle::Perm& p, bool use_perm, const Geo& g, const int* tab, int S,
                   long long row_vecs, hipStream_t st) {
  affine_kernel<U><<<rows_grid("affine_rows", p.n, row_vecs), THREADS, 0, st>>>(
      src_x, src_y, dst_x, dst_y, p, use_perm ? 1 : 0, g, tab, S, row_vecs);
}

bool overlap(const void* a, const void* b, unsigned long long bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + bytes && y < x + bytes;
}

bool range_overlap(const void* a, unsigned long long na, const void* b, unsigned long long nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

// The checks both entries share, thrown before anything is launched; false: nothing to do.
bool check_rows(const std::string& who, const float* src_x, const int* src_y, float* dst_x,
                int* dst_y, long long n, int H, int W, int C, int K) {
  if (n < 0 || n > 0x7FFFFFFFll) throw std::runtime_error(who + ": n out of range");
  if (H <= 0 || W <= 0 || C <= 0) throw std::runtime_error(who + ": H, W, C must be positive");
  const long long row_elems = (long long)H * W * C;
  if (row_elems > 0x7FFFFFFFll) throw std::runtime_error(who + ": image too large");
  if (K < 0 || K >= std::min(H, W))
    throw std::runtime_error(who + ": shift K must be in [0, min(H, W))");
  if (!src_x || !dst_x || (src_y && !dst_y)) throw std::runtime_error(who + ": null buffer");
  if (n == 0) return false;
  if (overlap(src_x, dst_x, (unsigned long long)n * row_elems * sizeof(float)) ||
      (src_y && overlap(src_y, dst_y, (unsigned long long)n * sizeof(int))))
    throw std::runtime_error(who + ": src and dst overlap");
  return true;
}

Geo make_geo(int H, int W, int C, uint32_t aug_key, int K, bool flip, float fill) {
  Geo g;
  g.H = H, g.W = W, g.C = C, g.wc = (uint32_t)W * C;
  g.m_wc = magic(g.wc), g.m_c = magic(g.C);
  g.key = aug_key, g.span = 2u * K + 1u;
  g.K = K, g.flip = flip ? 1 : 0, g.fill = fill;
  return g;
}

// rows of whole 16-byte vectors between 16-byte aligned bases
bool vector_rows(const float* src_x, const float* dst_x, long long row_elems) {
  return row_elems % 4 == 0 && (reinterpret_cast<uintptr_t>(src_x) & 15) == 0 &&
         (reinterpret_cast<uintptr_t>(dst_x) & 15) == 0;
}

}  // namespace

void augment_rows(const float* src_x, const int* src_y, float* dst_x, int* dst_y, long long n,
                  int H, int W, int C, bool use_perm, uint32_t perm_key, uint32_t aug_key, int K,
                  bool flip, float fill, hipStream_t st) {
  if (!check_rows("augment_rows", src_x, src_y, dst_x, dst_y, n, H, W, C, K)) return;
  const long long row_elems = (long long)H * W * C;
  const shuffle::Perm p = shuffle::make_perm(perm_key, n);
  const Geo g = make_geo(H, W, C, aug_key, K, flip, fill);
  if (vector_rows(src_x, dst_x, row_elems))
    launch_rows<4>(src_x, src_y, dst_x, dst_y, p, use_perm, g, row_elems / 4, st);
  else
    launch_rows<1>(src_x, src_y, dst_x, dst_y, p, use_perm, g, row_elems, st);
}

void affine_rows(const float* src_x, const int* src_y, float* dst_x, int* dst_y, long long n,
                 int H, int W, int C, bool use_perm, uint32_t perm_key, uint32_t aug_key, int K,
                 bool flip, float fill, const int* tables, int S, hipStream_t st) {
  if (H > MAX_SIDE || W > MAX_SIDE)
    throw std::runtime_error("affine_rows: H, W above 1024 (32-bit source coordinates)");
  if (!tables) throw std::runtime_error("affine_rows: null table");
  if (H > 0 && W > 0 && (S < 0 || S >= std::min(H, W)))
    throw std::runtime_error("affine_rows: cutout S must be in [0, min(H, W))");
  if (!check_rows("affine_rows", src_x, src_y, dst_x, dst_y, n, H, W, C, K)) return;
  const long long row_elems = (long long)H * W * C;
  const shuffle::Perm p = shuffle::make_perm(perm_key, n);
  const Geo g = make_geo(H, W, C, aug_key, K, flip, fill);
  if (vector_rows(src_x, dst_x, row_elems))
    launch_affine<4>(src_x, src_y, dst_x, dst_y, p, use_perm, g, tables, S, row_elems / 4, st);
  else
    launch_affine<1>(src_x, src_y, dst_x, dst_y, p, use_perm, g, tables, S, row_elems, st);
}

void mix_rows(const float* src_x, const int* src_y, float* dst_x, int* dst_y, int* dst_y2,
              float* dst_lam, long long n, int H, int W, int C, bool cutmix, uint32_t mix_key,
              const int* table, hipStream_t st) {
  if (H > MAX_SIDE || W > MAX_SIDE) throw std::runtime_error("mix_rows: H, W above 1024");
  if (!table || !src_y || !dst_y || !dst_y2 || !dst_lam)
    throw std::runtime_error("mix_rows: null buffer");
  if (!check_rows("mix_rows", src_x, src_y, dst_x, dst_y, n, H, W, C, 0)) return;
  // every output against every input and against the other outputs (4-byte rows of n)
  const unsigned long long yb = (unsigned long long)n * sizeof(int);
  const unsigned long long xb = (unsigned long long)n * H * W * C * sizeof(float);
  const void* small[4] = {src_y, dst_y, dst_y2, dst_lam};
  for (int a = 0; a < 4; ++a) {
    for (int b = a + 1; b < 4; ++b)
      if (overlap(small[a], small[b], yb)) throw std::runtime_error("mix_rows: src and dst overlap");
    if (a > 0 && (range_overlap(small[a], yb, src_x, xb) ||
                  range_overlap(small[a], yb, dst_x, xb)))
      throw std::runtime_error("mix_rows: src and dst overlap");
  }
  const long long row_elems = (long long)H * W * C;
  // the partner permutation has a key of its own, derived from the pass's
  const shuffle::Perm p = shuffle::make_perm(mix32(mix_key ^ 0x9E3779B9u), n);
  MixGeo g;
  g.H = H, g.W = W, g.C = C, g.wc = (uint32_t)W * C;
  g.m_wc = magic(g.wc), g.m_c = magic(g.C);
  g.key = mix_key, g.cutmix = cutmix ? 1 : 0;
  if (vector_rows(src_x, dst_x, row_elems))
    mix_kernel<4><<<rows_grid("mix_rows", n, row_elems / 4), THREADS, 0, st>>>(
        src_x, src_y, dst_x, dst_y, dst_y2, dst_lam, p, g, table, row_elems / 4);
  else
    mix_kernel<1><<<rows_grid("mix_rows", n, row_elems), THREADS, 0, st>>>(
        src_x, src_y, dst_x, dst_y, dst_y2, dst_lam, p, g, table, row_elems);
}

}  // namespace augment
