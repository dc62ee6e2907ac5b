// LARS on the flat parameter / gradient / momentum buffers (lars.h has the
// definition and the segment table).
//
// The update is not elementwise: a weight moves by a rate that depends on the
// 2-norms of its whole tensor and of that tensor's gradient.  Two launches over
// the same grid, one 256-lane block per 4096-float chunk of one tensor:
//
//   lars_norms_kernel   (sum w^2, sum g'^2) of the chunk -> part[chunk]
//   lars_update_kernel  the first wave sums the pairs of the block's own tensor
//                       (fp64, fixed order; at most a few KB out of L2) while the
//                       chunk's w / g / m loads are in flight, r goes through
//                       LDS, then the chunk is updated
//
// The kernel boundary is the only synchronisation: no float atomics (the sums
// would depend on arrival order) and no grid barrier.  A lane's 16-byte loads
// of its chunk (four each of w and g in the first kernel, of w, g and m in the
// second) are issued together before anything consumes them.
#include <stdexcept>

#include "common.h"
#include "lars.h"

namespace optim {

// Row of the chunk b: the last row whose first chunk (column 3) is <= b.  One
// ballot per 64 rows (the table_lookup idiom of conv_bf16.hip); every lane of
// the wave takes part and gets the same answer.
__device__ __forceinline__ int lars_row_of(const long long* tab, int n, long long b) {
  int j = 0;
  for (int base = 0; base < n; base += 64) {
    const int jj = base + (int)(threadIdx.x & 63);
    const bool le = jj < n && tab[kLarsRow * min(jj, n - 1) + 3] <= b;
    const int cnt = __popcll(__ballot(le));
    j = base + cnt - 1;
    if (cnt < 64) break;
  }
  return max(j, 0);
}

// What a block owns: floats [base, base + len) of the flat buffers, len in
// [1, kLarsChunk]; base is a multiple of 64 floats (offset % 64 == 0 and the
// chunk size is one), so float4 accesses from it are 16-byte aligned.
struct LarsChunk {
  long long base;
  int len;
};

__device__ __forceinline__ LarsChunk lars_chunk(const long long* T, long long b) {
  const long long lc = b - T[3];
  const long long left = T[1] - lc * kLarsChunk;
  return {T[0] + lc * kLarsChunk, (int)(left < kLarsChunk ? left : kLarsChunk)};
}

__global__ __launch_bounds__(256) void lars_norms_kernel(const float* __restrict__ w,
                                                         const float* __restrict__ g,
                                                         const long long* __restrict__ tab,
                                                         int ntensors, float gscale,
                                                         float2* __restrict__ part) {
  __shared__ float2 red[4];
  const int tid = threadIdx.x;
  const long long* T = tab + kLarsRow * lars_row_of(tab, ntensors, blockIdx.x);
  if (T[2] == 0) return;  // not adapted: r = 1, nobody reads this pair (block-uniform)
  const LarsChunk c = lars_chunk(T, blockIdx.x);
  const float4* w4 = reinterpret_cast<const float4*>(w + c.base);
  const float4* g4 = reinterpret_cast<const float4*>(g + c.base);
  float4 wv[4], gv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // whole float4s only: all eight loads in flight together
    const int q = tid + 256 * i;
    const bool in = 4 * q + 4 <= c.len;
    wv[i] = in ? w4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    gv[i] = in ? g4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float sw = 0.f, sg = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a0 = gv[i].x * gscale, a1 = gv[i].y * gscale, a2 = gv[i].z * gscale,
                a3 = gv[i].w * gscale;
    sw = __builtin_fmaf(wv[i].x, wv[i].x, sw);
    sw = __builtin_fmaf(wv[i].y, wv[i].y, sw);
    sw = __builtin_fmaf(wv[i].z, wv[i].z, sw);
    sw = __builtin_fmaf(wv[i].w, wv[i].w, sw);
    sg = __builtin_fmaf(a0, a0, sg);
    sg = __builtin_fmaf(a1, a1, sg);
    sg = __builtin_fmaf(a2, a2, sg);
    sg = __builtin_fmaf(a3, a3, sg);
  }
  // the len % 4 floats past the last whole float4, one by one, by the lane whose
  // (skipped) float4 they would have been: the padding behind them is not read
  const int e0 = c.len & ~3;
  if (e0 < c.len && tid == ((e0 >> 2) & 255)) {
    for (int e = e0; e < c.len; ++e) {
      const float x = w[c.base + e], a = g[c.base + e] * gscale;
      sw = __builtin_fmaf(x, x, sw);
      sg = __builtin_fmaf(a, a, sg);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sw += __shfl_xor(sw, o, 64);
    sg += __shfl_xor(sg, o, 64);
  }
  if ((tid & 63) == 0) red[tid >> 6] = make_float2(sw, sg);
  __syncthreads();
  if (tid == 0)
    part[blockIdx.x] = make_float2((red[0].x + red[1].x) + (red[2].x + red[3].x),
                                   (red[0].y + red[1].y) + (red[2].y + red[3].y));
}

// One element of the update; every operation is one rounded fp32 operation
// (docs/ACCURACY.md counts them): g' = g * gscale, e = fma(wd, w, g'), u = r * e,
// m = fma(mu, m, u), [nesterov: d = fma(mu, m, u)], w = fma(-lr, d or m, w).
__device__ __forceinline__ void lars_elem(float& w, float g, float& m, float r, float wd, float mu,
                                          float gscale, float nlr, bool nesterov) {
  const float u = r * __builtin_fmaf(wd, w, g * gscale);
  m = __builtin_fmaf(mu, m, u);
  const float d = nesterov ? __builtin_fmaf(mu, m, u) : m;
  w = __builtin_fmaf(nlr, d, w);
}

__global__ __launch_bounds__(256) void lars_update_kernel(
    float* __restrict__ w, const float* __restrict__ g, float* __restrict__ mom,
    const long long* __restrict__ tab, int ntensors, const float2* __restrict__ part,
    float* __restrict__ ratio, double eta, double wd, int nesterov, float momentum, float gscale,
    const float* __restrict__ lr_ptr, long long* step_ptr) {
  __shared__ float r_sh;
  const int tid = threadIdx.x;
  const int t = lars_row_of(tab, ntensors, blockIdx.x);
  const long long* T = tab + kLarsRow * t;
  const bool adapted = T[2] != 0;
  const LarsChunk c = lars_chunk(T, blockIdx.x);
  const float nlr = -*lr_ptr;
  float4* w4 = reinterpret_cast<float4*>(w + c.base);
  float4* m4 = reinterpret_cast<float4*>(mom + c.base);
  const float4* g4 = reinterpret_cast<const float4*>(g + c.base);
  float4 wv[4], gv[4], mv[4];
  bool in[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // issued before the reduction below: it hides under them
    const int q = tid + 256 * i;
    in[i] = 4 * q + 4 <= c.len;
    if (in[i]) {
      wv[i] = w4[q];
      gv[i] = g4[q];
      mv[i] = m4[q];
    }
  }
  if (tid < 64) {
    float r = 1.f;
    if (adapted) {  // (wave-uniform)
      // lane l sums the pairs l, l + 64, ... in order, then the xor butterfly:
      // the same additions in the same order in every block of the tensor,
      // and a + b == b + a bit for bit, so all lanes and blocks agree
      const float2* p = part + T[3];
      const int nc = (int)T[4];
      double sw = 0.0, sg = 0.0;
      for (int j = tid; j < nc; j += 64) {
        const float2 v = p[j];
        sw += (double)v.x;
        sg += (double)v.y;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        sw += __shfl_xor(sw, o, 64);
        sg += __shfl_xor(sg, o, 64);
      }
      const double nw = sqrt(sw), ng = sqrt(sg);
      if (nw > 0.0 && ng > 0.0) r = (float)(eta * nw / (ng + wd * nw));
    }
    if (tid == 0) {
      r_sh = r;
      if (blockIdx.x == T[3]) ratio[t] = r;  // the block of the tensor's first chunk
    }
  }
  __syncthreads();
  const float r = r_sh;
  const float wdf = adapted ? (float)wd : 0.f;  // no decay on the tensors not adapted
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!in[i]) continue;
    lars_elem(wv[i].x, gv[i].x, mv[i].x, r, wdf, momentum, gscale, nlr, nesterov);
    lars_elem(wv[i].y, gv[i].y, mv[i].y, r, wdf, momentum, gscale, nlr, nesterov);
    lars_elem(wv[i].z, gv[i].z, mv[i].z, r, wdf, momentum, gscale, nlr, nesterov);
    lars_elem(wv[i].w, gv[i].w, mv[i].w, r, wdf, momentum, gscale, nlr, nesterov);
    const int q = tid + 256 * i;
    w4[q] = wv[i];
    m4[q] = mv[i];
  }
  const int e0 = c.len & ~3;  // the ragged tail, as in the norms
  if (e0 < c.len && tid == ((e0 >> 2) & 255)) {
    for (int e = e0; e < c.len; ++e) {
      float x = w[c.base + e], m = mom[c.base + e];
      lars_elem(x, g[c.base + e], m, r, wdf, momentum, gscale, nlr, nesterov);
      w[c.base + e] = x;
      mom[c.base + e] = m;
    }
  }
  if (step_ptr && blockIdx.x == 0 && tid == 0) *step_ptr += 1;
}

void launch_lars_step(float* w, const float* g, float* mom, const long long* table, int ntensors,
                      int nchunks, float* part, float* ratio, double eta, double wd,
                      bool nesterov, float momentum, float gscale, const float* lr_ptr,
                      long long* step_ptr, hipStream_t s) {
  if (!w || !g || !mom || !table || !part || !ratio || !lr_ptr)
    throw std::runtime_error("lars_step: null buffer");
  if (ntensors < 1 || nchunks < ntensors)
    throw std::runtime_error("lars_step: needs ntensors >= 1 and a chunk per tensor");
  if (((uintptr_t)w | (uintptr_t)g | (uintptr_t)mom) % 16 || (uintptr_t)part % 8)
    throw std::runtime_error("lars_step: w, g, mom must be 16-byte and part 8-byte aligned");
  if (!(eta > 0.0 && eta <= 1.0) || !(wd >= 0.0))
    throw std::runtime_error("lars_step: needs 0 < eta <= 1 and wd >= 0");
  lars_norms_kernel<<<nchunks, 256, 0, s>>>(w, g, table, ntensors, gscale,
                                            reinterpret_cast<float2*>(part));
  lars_update_kernel<<<nchunks, 256, 0, s>>>(w, g, mom, table, ntensors,
                                             reinterpret_cast<const float2*>(part), ratio, eta, wd,
                                             nesterov ? 1 : 0, momentum, gscale, lr_ptr, step_ptr);
}

}  // namespace optim
