// Inference kernels (predict.h): the input view and the prediction head.
//
// prep is the memory-bound gather of augment.hip without the per-row draw: one
// workgroup writes a 16 KB piece of one destination row (blockIdx.y picks the
// piece) and walks the rows with a grid stride; a thread owns 4 consecutive
// destination floats (one aligned 16-byte store).  A uint8 source is a quarter
// of the bytes read; its 256-entry normalisation table sits in LDS.
//
// head has the shape of eval_metrics_kernel: one wave per row, one lane per
// class (C <= 64), 256-thread blocks, a bounded grid striding over the rows.
#include "predict.h"

#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <stdexcept>

#include "common.h"

namespace predict {

namespace {

constexpr int THREADS = 256;
constexpr int PER_THREAD = 4;                // stores a thread issues per row piece
constexpr int PIECE = THREADS * PER_THREAD;  // ... of a workgroup
constexpr int MAX_BLOCKS = 2048;             // 256 CUs x 8 resident workgroups
constexpr int HEAD_MAX_C = 64;
constexpr int HEAD_MAX_BLOCKS = 1024;

struct Geo {
  uint32_t H, W, C, wc;  // wc = W * C elements an image line
  uint32_t m_wc, m_c;    // floor(2^32 / d) + 1 for d = wc, C
  int dy, dx, flip;
  float fill;
};

uint32_t magic(uint32_t d) { return d > 1 ? (uint32_t)((1ull << 32) / d) + 1u : 0u; }

// n / d for n < 2^31 with m = floor(2^32 / d) + 1 (augment.hip div_by): the
// estimate is the quotient or one more, and then the remainder is negative.
__device__ __forceinline__ uint32_t div_by(uint32_t n, uint32_t d, uint32_t m) {
  if (d == 1) return n;
  uint32_t q = __umulhi(n, m);
  if ((int)(n - q * d) < 0) --q;
  return q;
}

__device__ __forceinline__ float norm_of(float v, const float*) { return v; }
__device__ __forceinline__ float norm_of(uint8_t v, const float* lut) { return lut[v]; }

// The U destination floats from element e of a row: their normalised source
// elements, or fill.  Every source index read is inside the row: sy < H and
// sx < W (unsigned: a negative coordinate wraps past them).
template <class T, int U>
__device__ __forceinline__ void gather(const T* __restrict__ a, const Geo& g, uint32_t e,
                                       const float* lut, float* o) {
  uint32_t y = div_by(e, g.wc, g.m_wc);
  uint32_t r = e - y * g.wc;
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const uint32_t sy = y + (uint32_t)g.dy;
    const uint32_t x = div_by(r, g.C, g.m_c), c = r - x * g.C;
    const uint32_t sx = (g.flip ? g.W - 1u - x : x) + (uint32_t)g.dx;
    const bool ok = sy < g.H && sx < g.W;
    o[k] = ok ? norm_of(a[sy * g.wc + sx * g.C + c], lut) : g.fill;
    if (++r == g.wc) {
      r = 0;
      ++y;
    }
  }
}

// U = 4 (row_vecs = row_elems / 4, aligned f32x4 stores) or 1 (row_vecs = row_elems)
template <class T, int U>
__global__ __launch_bounds__(THREADS) void prep_kernel(const T* __restrict__ src,
                                                       float* __restrict__ dst, long long n, Geo g,
                                                       long long row_vecs,
                                                       const float* __restrict__ lut_g) {
  __shared__ float lut[256];
  if constexpr (sizeof(T) == 1) {
    lut[threadIdx.x] = lut_g[threadIdx.x];  // THREADS == 256 entries
    __syncthreads();
  }
  const long long v0 = (long long)blockIdx.y * PIECE + threadIdx.x;
  const long long row_elems = row_vecs * U;
  for (long long i = blockIdx.x; i < n; i += gridDim.x) {
    const T* a = src + i * row_elems;
    float* d = dst + i * row_elems;
    float o[PER_THREAD][U];
#pragma unroll
    for (int u = 0; u < PER_THREAD; ++u) {
      const long long v = v0 + u * THREADS;
      if (v < row_vecs) gather<T, U>(a, g, (uint32_t)(v * U), lut, o[u]);
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
  }
}

template <class T>
void launch_prep(const T* src, float* dst, long long n, const Geo& g, long long row_elems,
                 const float* lut, hipStream_t st) {
  const bool vec = row_elems % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  const long long row_vecs = vec ? row_elems / 4 : row_elems;
  const long long pieces = (row_vecs + PIECE - 1) / PIECE;
  if (pieces > 65535) throw std::runtime_error("predict_prep: row too long");
  const long long gx = std::max(1ll, std::min(n, MAX_BLOCKS / pieces));
  const dim3 grid((unsigned)gx, (unsigned)pieces);
  if (vec)
    prep_kernel<T, 4><<<grid, THREADS, 0, st>>>(src, dst, n, g, row_vecs, lut);
  else
    prep_kernel<T, 1><<<grid, THREADS, 0, st>>>(src, dst, n, g, row_vecs, lut);
}

__global__ __launch_bounds__(256) void head_kernel(const float* __restrict__ logits,
                                                   float* __restrict__ acc, int n, int C, int view,
                                                   int views, int k, float* __restrict__ probs,
                                                   float* __restrict__ scores,
                                                   int* __restrict__ topk_class,
                                                   float* __restrict__ topk_prob) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool live = lane < C;
  const bool last = view == views - 1;
  const float nviews = (float)views;
  for (long long row = (long long)blockIdx.x * 4 + wave; row < n; row += (long long)gridDim.x * 4) {
    const size_t at = (size_t)row * C + lane;
    const float v = live ? logits[at] : -INFINITY;
    const float mx = wave_max(v);
    const float e = live ? expf(v - mx) : 0.f;
    float p = e / wave_sum(e);
    float key = v;
    if (views > 1) {  // uniform over the launch
      if (live) {
        if (view > 0) p += acc[at];
        if (!last) acc[at] = p;
      }
      if (!last) continue;
      p = p / nviews;
      key = p;
    }
    if (live) {
      if (probs) probs[at] = p;
      if (scores) scores[at] = views > 1 ? logf(fmaxf(p, FLT_MIN)) : v;
    }
    // k rounds: the lowest index among the maximal keys not taken yet
    bool free_ = live;
    for (int r = 0; r < k; ++r) {
      const float m = wave_max(free_ ? key : -INFINITY);
      unsigned long long top = __ballot(free_ && key == m);
      // no lane matches only on NaN keys (outside the contract): the lowest
      // free class then, so the classes stay distinct and inside [0, C)
      if (!top) top = __ballot(free_);
      const int c = __ffsll(top) - 1;
      const float pc = __shfl(p, c, 64);
      if (lane == 0) {
        topk_class[(size_t)row * k + r] = c;
        topk_prob[(size_t)row * k + r] = pc;
      }
      if (lane == c) free_ = false;
    }
  }
}

}  // namespace

void prep(const void* src, bool src_u8, float* dst, long long n, int H, int W, int C, int dy,
          int dx, bool flip, float fill, const float* lut, hipStream_t st) {
  if (n < 0 || n > 0x7FFFFFFFll) throw std::runtime_error("predict_prep: n out of range");
  if (H <= 0 || W <= 0 || C <= 0) throw std::runtime_error("predict_prep: H, W, C must be positive");
  const long long row_elems = (long long)H * W * C;
  if (row_elems > 0x7FFFFFFFll) throw std::runtime_error("predict_prep: image too large");
  if (std::abs(dy) >= H || std::abs(dx) >= W)
    throw std::runtime_error("predict_prep: |dy| < H and |dx| < W");
  if (!src || !dst || (src_u8 && !lut)) throw std::runtime_error("predict_prep: null buffer");
  if (n == 0) return;
  Geo g;
  g.H = H, g.W = W, g.C = C, g.wc = (uint32_t)W * C;
  g.m_wc = magic(g.wc), g.m_c = magic(g.C);
  g.dy = dy, g.dx = dx, g.flip = flip ? 1 : 0, g.fill = fill;
  if (src_u8)
    launch_prep(static_cast<const uint8_t*>(src), dst, n, g, row_elems, lut, st);
  else
    launch_prep(static_cast<const float*>(src), dst, n, g, row_elems, lut, st);
}

void head(const float* logits, float* acc, int n, int C, int view, int views, int k, float* probs,
          float* scores, int* topk_class, float* topk_prob, hipStream_t st) {
  if (C < 1 || C > HEAD_MAX_C) throw std::runtime_error("predict_head: 1 <= C <= 64 classes");
  if (k < 1 || k > C) throw std::runtime_error("predict_head: 1 <= k <= C");
  if (views < 1 || view < 0 || view >= views)
    throw std::runtime_error("predict_head: 0 <= view < views");
  if (n < 0) throw std::runtime_error("predict_head: negative row count");
  if (!logits || (views > 1 && !acc) || (view == views - 1 && (!topk_class || !topk_prob)))
    throw std::runtime_error("predict_head: null buffer");
  if (n == 0) return;
  const int blocks = (int)std::min<long long>(((long long)n + 3) / 4, HEAD_MAX_BLOCKS);
  head_kernel<<<blocks, 256, 0, st>>>(logits, acc, n, C, view, views, k, probs, scores, topk_class,
                                      topk_prob);
}

}  // namespace predict
