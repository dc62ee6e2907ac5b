// Exponential moving average of the flat parameter buffer (--ema, TF1's
// tf.train.ExponentialMovingAverage with num_updates; docs/ACCURACY.md).
//
// t = the step counter after the step's SGD incremented it (optimizer steps
// applied).  t % K != 0: nothing.  Else u = t / K - 1 earlier updates,
//   d   = min(decay, (1 + u) / (10 + u))    fp32
//   omd = 1 - d
//   ema = fma(omd, w - ema, ema)            per element, fp32
// Everything derives from the step counter: no state besides `ema`.
#pragma once

#include <hip/hip_runtime.h>

namespace optim {
// ema, w: flat fp32 buffers of n floats (n % 4 == 0, else throws; 16-B
// aligned).  t is read from step_ptr when non-null (the device step counter:
// graph-replayable), else step_const.  One launch, no allocation, no sync.
void launch_ema(float* ema, const float* w, long long n, float decay, long long K,
                const long long* step_ptr, long long step_const, hipStream_t s);
}  // namespace optim
