// Layer-wise adaptive rate scaling on the flat buffers (--optimizer lars; You
// et al. 2017, the "scaled gradient" form; docs/ACCURACY.md has the definition).
//
// g' = gscale * g.  Adapted tensors (table column 2):
//   nw = ||w||_2, ng = ||g'||_2 over the tensor's real elements
//   r  = eta * nw / (ng + wd * nw)   when nw > 0 and ng > 0, else 1
//   u  = r * (g' + wd * w)
// other tensors: r = 1, u = g'.  Then m = momentum * m + u and w -= lr * m, or
// with nesterov w -= lr * (u + momentum * m) on the new m.
//
// The segment table holds one row of kLarsRow int64 per tensor,
//   {offset, numel, adapted, first chunk, nchunks},
// offsets in floats and 64-float aligned, rows in ascending offset order.  A
// tensor is cut into chunks of kLarsChunk floats (the last one ragged); a chunk
// never spans two tensors; `first chunk` numbers them through the table.
#pragma once

#include <hip/hip_runtime.h>

namespace optim {
constexpr int kLarsChunk = 4096;  // floats a block owns: 256 lanes x 4 float4
constexpr int kLarsRow = 5;

// Two launches on s, no allocation, no sync, no atomics: the per-chunk sums of
// squares into part[nchunks][2], then the update of every chunk, whose block
// first reduces its own tensor's pairs in a fixed order (fp64), so every block
// of a tensor - and every rank holding the same summed gradient - derives the
// same r.  ratio[ntensors] receives r (1 for the tensors not adapted).  Floats
// between a tensor's end and the next offset are neither read nor written.
// lr is read from lr_ptr; one thread adds 1 to *step_ptr when it is non-null.
// The table is trusted (the caller builds and checks it); everything else
// throws std::runtime_error.
void launch_lars_step(float* w, const float* g, float* mom, const long long* table, int ntensors,
                      int nchunks, float* part, float* ratio, double eta, double wd,
                      bool nesterov, float momentum, float gscale, const float* lr_ptr,
                      long long* step_ptr, hipStream_t s);
}  // namespace optim
