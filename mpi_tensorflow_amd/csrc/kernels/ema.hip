// Exponential moving average of the flat parameter buffer (ema.h has the
// definition).  One memory-bound pass, 16 B per lane: reads w and ema, writes
// ema.  The step comes from the device counter, so the launch is captured
// into the step graphs as it stands; a step that is no multiple of K costs
// one scalar load per wave and the launch.
#include <stdexcept>

#include "common.h"
#include "ema.h"

namespace optim {

__global__ __launch_bounds__(256) void ema_flat_kernel(float4* __restrict__ ema,
                                                       const float4* __restrict__ w, long long n4,
                                                       float decay, long long K,
                                                       const long long* step_ptr,
                                                       long long step_const) {
  // wave-uniform: a scalar load of the step, then the early return
  const long long t = step_ptr ? *step_ptr : step_const;
  if (t % K != 0) return;
  const float u = (float)(t / K - 1);  // earlier updates
  const float d = fminf(decay, (1.0f + u) / (10.0f + u));  // TF's num_updates warm-up
  const float omd = 1.0f - d;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 wv = w[i];
    float4 ev = ema[i];
    ev.x = __builtin_fmaf(omd, wv.x - ev.x, ev.x);
    ev.y = __builtin_fmaf(omd, wv.y - ev.y, ev.y);
    ev.z = __builtin_fmaf(omd, wv.z - ev.z, ev.z);
    ev.w = __builtin_fmaf(omd, wv.w - ev.w, ev.w);
    ema[i] = ev;
  }
}

// (the grid of sgd.hip: at most 2048 blocks, grid-stride beyond)
static inline int grid_for(long long n4) {
  long long b = (n4 + 255) / 256;
  return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

void launch_ema(float* ema, const float* w, long long n, float decay, long long K,
                const long long* step_ptr, long long step_const, hipStream_t s) {
  if (n % 4) throw std::runtime_error("ema: n % 4 != 0");
  if (K < 1) throw std::runtime_error("ema: K < 1");
  if (n == 0) return;
  ema_flat_kernel<<<grid_for(n / 4), 256, 0, s>>>(reinterpret_cast<float4*>(ema),
                                                  reinterpret_cast<const float4*>(w), n / 4, decay,
                                                  K, step_ptr, step_const);
}

}  // namespace optim
