// Evaluation metrics over a chunk of logits: confusion matrix, histogram of
// the label's rank, summed cross-entropy, ignored rows.  Every output is
// accumulated into (one evaluation = one launch pair per chunk, zeroed once by
// the caller), so a whole split ends in one copy of C * C + C + 4 words.
//
// One wave per row, one lane per class (C <= 64: a row is one load), 256-thread
// blocks, a bounded grid striding over the rows.  Definitions (the tie rule of
// fc_head_eval_kernel's `v > best` and fc_head_train_kernel's ballot / ffs):
//   prediction = the lowest index among the maximal logits
//   rank       = #{j : x[j] > x[label]} + #{j < label : x[j] == x[label]}
//   loss       = logsumexp(x) - x[label], fp32 per row, max-subtracted
// Rows whose label is outside [0, C) only count as ignored.
//
// Counts go to a per-block LDS table (10,000 rows of a 10-class test set would
// otherwise be 10,000 global atomics on ~10 addresses); only its non-zero
// cells are flushed, with integer atomics: exact, order-independent.  The loss
// takes no floating-point atomic: per-block fp64 partials go to a workspace, a
// one-thread launch adds them in block order into loss_sum (launches of one
// evaluation are ordered on the stream, so the total is reproducible).
#include <algorithm>
#include <stdexcept>

#include "common.h"
#include "ops_generic.h"

namespace gops {

namespace {

constexpr int EM_MAX_C = 64;
constexpr int EM_MAX_BLOCKS = 256;

__global__ __launch_bounds__(256) void eval_metrics_kernel(
    const float* __restrict__ logits, const int* __restrict__ labels, int n, int C,
    int* __restrict__ conf, int* __restrict__ rank_hist, int* __restrict__ ignored,
    double* __restrict__ part, float* __restrict__ loss_rows) {
  __shared__ int s_conf[EM_MAX_C * EM_MAX_C];
  __shared__ int s_rank[EM_MAX_C];
  __shared__ int s_ign;
  __shared__ double s_loss[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int cells = C * C;
  for (int i = tid; i < cells; i += 256) s_conf[i] = 0;
  if (tid < EM_MAX_C) s_rank[tid] = 0;
  if (tid == 0) s_ign = 0;
  __syncthreads();

  const bool live = lane < C;
  double acc = 0.0;  // wave-uniform
  for (long long row = blockIdx.x * 4 + wave; row < n; row += gridDim.x * 4) {
    const int label = labels[row];
    const float v = live ? logits[(size_t)row * C + lane] : -INFINITY;
    if (label < 0 || label >= C) {  // wave-uniform
      if (lane == 0) {
        atomicAdd(&s_ign, 1);
        if (loss_rows) loss_rows[row] = 0.f;
      }
      continue;
    }
    const float mx = wave_max(v);
    const float s = wave_sum(live ? expf(v - mx) : 0.f);
    // no lane matches only on NaN logits (outside the contract): class 0 then,
    // so the index stays inside the table
    const unsigned long long top = __ballot(live && v == mx);
    const int pred = top ? __ffsll(top) - 1 : 0;
    const float vl = __shfl(v, label, 64);
    // the label's own lane is in neither mask: rank <= C - 1
    const unsigned long long gt = __ballot(live && v > vl);
    const unsigned long long eq = __ballot(live && v == vl && lane < label);
    const int rank = __popcll(gt) + __popcll(eq);
    const float loss = logf(s) + (mx - vl);
    acc += (double)loss;
    if (lane == 0) {
      atomicAdd(&s_conf[label * C + pred], 1);
      atomicAdd(&s_rank[rank], 1);
      if (loss_rows) loss_rows[row] = loss;
    }
  }
  if (lane == 0) s_loss[wave] = acc;
  __syncthreads();

  for (int i = tid; i < cells; i += 256) {
    const int c = s_conf[i];
    if (c) atomicAdd(&conf[i], c);
  }
  if (tid < C) {
    const int c = s_rank[tid];
    if (c) atomicAdd(&rank_hist[tid], c);
  }
  if (tid == 0) {
    if (s_ign) atomicAdd(ignored, s_ign);
    part[blockIdx.x] = ((s_loss[0] + s_loss[1]) + s_loss[2]) + s_loss[3];
  }
}

__global__ void eval_metrics_loss_kernel(const double* __restrict__ part, int blocks,
                                         double* __restrict__ loss_sum) {
  double t = 0.0;
  for (int i = 0; i < blocks; ++i) t += part[i];
  *loss_sum = *loss_sum + t;
}

}  // namespace

int eval_metrics_ws_doubles() { return EM_MAX_BLOCKS; }

void eval_metrics(const float* logits, const int* labels, int n, int C, int* conf, int* rank_hist,
                  double* loss_sum, int* ignored, double* ws, float* loss_rows, hipStream_t st) {
  if (C < 1 || C > EM_MAX_C) throw std::runtime_error("eval_metrics: 1 <= C <= 64 classes");
  if (n < 0) throw std::runtime_error("eval_metrics: negative row count");
  if (n == 0) return;
  const int blocks = (int)std::min<long long>(((long long)n + 3) / 4, EM_MAX_BLOCKS);
  eval_metrics_kernel<<<blocks, 256, 0, st>>>(logits, labels, n, C, conf, rank_hist, ignored, ws,
                                              loss_rows);
  eval_metrics_loss_kernel<<<1, 1, 0, st>>>(ws, blocks, loss_sum);
}

}  // namespace gops
