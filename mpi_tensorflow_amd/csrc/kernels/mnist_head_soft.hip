// The MNIST train head against a soft target (--label-smoothing, --mix;
// docs/ACCURACY.md), in a translation unit of its own: the code object of
// mnist.hip, which the tuned hard-label step runs, stays what it was.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "common.h"
#include "mnist.h"
#include "mnist_shared.h"

namespace mnist {

// The head against a soft target (--label-smoothing, --mix), derived from
// fc_head_train_kernel: per class t = (1 - eps) (lam [c == y1] + (1 - lam) [c == y2])
// + eps / classes, loss = logsumexp - sum t z, dlogits = (softmax - t) / B;
// `correct` stays argmax against y1.  labels2 / lam_rows null: lam = 1.  With
// eps = 0 and lam = 1, t is the one-hot row and every output carries the hard
// kernels' bits.  Both chain forms of set_fc_chain bit 0 take this one kernel
// (it carries no fc_stamps profiling slots).
template <int NS>
__global__ __launch_bounds__(256) void fc_head_train_soft_kernel(
    const float* __restrict__ part, const float* __restrict__ b3, const float* __restrict__ w4,
    const float* __restrict__ b4, const int* __restrict__ labels, int n_local,
    const long long* step_ptr, int batch, float keep_prob, uint32_t seed, uint32_t rank,
    float base_lr, float lr_decay, float* __restrict__ hd_out, float* __restrict__ dh_out,
    float* __restrict__ dlog_out, float* __restrict__ loss_rows, float* __restrict__ lr_out,
    int* __restrict__ correct, __bf16* __restrict__ dh16, __bf16* __restrict__ dht16,
    int lbatch, const int* __restrict__ labels2, const float* __restrict__ lam_rows, float eps) {
  __shared__ float red[4][NCLS];
  __shared__ float dlog_s[NCLS];
  const int row = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long step = step_ptr ? *step_ptr : 0;
  const int lb = logical_batch(lbatch, batch);
  const bool valid = row < lb;
  const long long off = batch_offset_dev(step_ptr, n_local, lb);
  const uint32_t key = dropout_key(seed, rank, (uint32_t)step, 0u);
  const float scale = 1.f / keep_prob;
  const int label = labels[off + row];
  const int label2 = lam_rows ? labels2[off + row] : label;
  const float lam = lam_rows ? lam_rows[off + row] : 1.f;
  const float b4l = lane < NCLS ? b4[lane] : 0.f;
  float ps[2][NS];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int q = 0; q < NS; ++q)
      ps[u][q] = part[((size_t)q * batch + row) * FC1_OUT + tid + 256 * u];
  float w4r[2][NCLS];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int c = 0; c < NCLS; ++c) w4r[u][c] = w4[(tid + 256 * u) * NCLS + c];
  float z[2], hd[2];
  bool kp[2];
  float lg[NCLS];
#pragma unroll
  for (int c = 0; c < NCLS; ++c) lg[c] = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = tid + 256 * u;
    float s = b3[j];
#pragma unroll
    for (int q = 0; q < NS; ++q) s += ps[u][q];
    z[u] = s;
    const float h = fmaxf(s, 0.f);
    kp[u] = dropout_keep(key, (uint32_t)(row * FC1_OUT + j), keep_prob);
    hd[u] = kp[u] ? h * scale : 0.f;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) lg[c] += hd[u] * w4r[u][c];
  }
#pragma unroll
  for (int c = 0; c < NCLS; ++c) {
    float v = wave_sum(lg[c]);
    if (lane == 0) red[wv][c] = v;
  }
  __syncthreads();
  if (tid < 64) {
    float logit = -INFINITY;
    if (lane < NCLS) logit = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane] + b4l;
    const float mx = wave_max(logit);
    const float e = lane < NCLS ? __expf(logit - mx) : 0.f;
    const float se = wave_sum(e);
    const float p = e / se;
    // the target of this lane's class
    const float a = (lane == label ? lam : 0.f) + (lane == label2 ? 1.f - lam : 0.f);
    const float t = (1.f - eps) * a + eps / (float)NCLS;
    const float tz = wave_sum(lane < NCLS ? t * logit : 0.f);
    if (lane < NCLS) dlog_s[lane] = valid ? (p - t) / (float)lb : 0.f;
    const unsigned long long bal = __ballot(lane < NCLS && logit == mx);
    const int am = __ffsll((long long)bal) - 1;
    if (lane == 0) {
      loss_rows[row] = valid ? (logf(se) + mx) - tz : 0.f;  // logsumexp - sum t z
      if (correct && valid) atomicAdd(correct, am == label ? 1 : 0);
      if (row == 0 && lr_out) {
        const float e2 = (float)((step * lb) / n_local);
        lr_out[0] = base_lr * powf(lr_decay, e2);
      }
    }
  }
  __syncthreads();
  float dl[NCLS];
#pragma unroll
  for (int c = 0; c < NCLS; ++c) dl[c] = dlog_s[c];
  if (tid < NCLS) dlog_out[row * NCLS + tid] = dl[tid];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = tid + 256 * u;
    float d = 0.f;
#pragma unroll
    for (int c = 0; c < NCLS; ++c) d += dl[c] * w4r[u][c];
    d = (kp[u] && z[u] > 0.f) ? d * scale : 0.f;  // pad row: dl == 0, so d == +0.f
    hd_out[row * FC1_OUT + j] = hd[u];
    dh_out[row * FC1_OUT + j] = d;
    if (dh16) {  // K-packed layouts of mnist_bf16.h
      dh16[((j >> 4) * batch + row) * 16 + (j & 15)] = (__bf16)d;
      dht16[((row >> 4) * FC1_OUT + j) * 16 + (row & 15)] = (__bf16)d;
    }
  }
}

void launch_fc_head_train_soft(const float* part, const float* b3, const float* w4,
                               const float* b4, const int* labels, int n_local,
                               const long long* step, int batch, float keep_prob, uint32_t seed,
                               uint32_t rank, float base_lr, float lr_decay, float* hd, float* dh,
                               float* dlog, float* loss_rows, float* lr_out, int* correct,
                               hipStream_t s, uint16_t* dh16, uint16_t* dht16, int splits,
                               int lbatch, const int* labels2, const float* lam, float eps) {
  if (lbatch < 0 || lbatch > batch) throw std::runtime_error("fc_head_train: lbatch > batch");
  if (lam && !labels2) throw std::runtime_error("fc_head_train: lam without labels2");
  if (!(eps >= 0.f && eps < 1.f)) throw std::runtime_error("fc_head_train: eps not in [0, 1)");
#define HEAD_SOFT(NS_)                                                                          \
  fc_head_train_soft_kernel<NS_><<<batch, 256, 0, s>>>(                                         \
      part, b3, w4, b4, labels, n_local, step, batch, keep_prob, seed, rank, base_lr, lr_decay, \
      hd, dh, dlog, loss_rows, lr_out, correct, reinterpret_cast<__bf16*>(dh16),                \
      reinterpret_cast<__bf16*>(dht16), lbatch, labels2, lam, eps)
  if (splits == FC1T_SPLITS)
    HEAD_SOFT(FC1T_SPLITS);
  else if (splits == FC1_SPLITS)
    HEAD_SOFT(FC1_SPLITS);
  else
    throw std::runtime_error("fc_head_train: unsupported slab count");
#undef HEAD_SOFT
}

}  // namespace mnist
