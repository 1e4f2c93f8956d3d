// TempScaling's one-parameter fit (reference trainers/calibration/tempscaling.py:146-169) from cosine logits computed once.  The reference
// runs both frozen towers on every step of every epoch over the same val split; the loss only ever sees the same [N, C] cosine matrix
// c, so the whole run is a function of c, the labels and the optimiser settings.  With theta = logit_scale, s = exp(theta) and
// p = softmax(s c_i.):
//   loss_i = logsumexp_j(s c_ij) - s c_iy,      d loss_i / d theta = s (sum_j p_ij c_ij - c_iy)
// and a step is F.cross_entropy's batch mean followed by torch.optim.SGD's rule on the scalar, in fp32.
//
// Two launches per step, ordered by the stream alone (DESIGN.md "TempScaling fit"):
//   tempscale_rows_kernel    one wave per row, four rows per workgroup, over a grid: z_j = s c_ij rounded once, m = max_j z_j,
//                            S = sum_j exp(z_j - m), T = sum_j exp(z_j - m) c_ij, lane-strided in fp32;  the row's
//                            (log S - (z_y - m),  s (T / S - c_iy)) goes to rows[r].  A row's pair does not depend on its batch.
//   tempscale_finish_kernel  one workgroup: the batch's pairs summed in float64 in a fixed order (thread t takes r = t, t + 256, ...;
//                            then a tree over LDS), the means rounded to fp32, and the SGD update of the state in fp32.
// Both read theta from the state buffer; no workgroup waits for another, nothing is accumulated with atomics, and the same inputs
// give the same bits.  state: four 32-bit words {theta fp32, momentum buffer fp32, steps taken int32, last batch loss fp32}.
#include <cmath>

#include "common.h"
#include "train_rules.h"   // SgdArgs (the first step is state[2] == 0 here, not first_step), check_sgd, block_sum_f64

namespace clipmi {
namespace {

// rows[r] for batch position r: sample order[r], or first + r without an order.  A sample index outside [0, N) or a label outside
// [0, C) is never used as an address: the pair is NaN (the host checks both before it launches anything).
__global__ __launch_bounds__(256) void tempscale_rows_kernel(const float* __restrict__ cosine, int64_t ld, const int64_t* __restrict__ labels,
                                                             const int32_t* __restrict__ order, int first, int rows, int N, int C,
                                                             const float* __restrict__ theta, float2* __restrict__ out) {
#pragma clang fp contract(off)   // z = s * c is rounded before the maximum is subtracted: the largest term is exp(0) exactly
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int i = order ? order[r] : first + r;
  float loss = NAN, grad = NAN;
  if (i >= 0 && i < N) {
    const float* __restrict__ row = cosine + (int64_t)i * ld;
    const float s = expf(*theta);
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, s * row[c]);
    m = wave_max(m);
    float S = 0.f, T = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float v = row[c];
      const float e = __expf(s * v - m);
      S += e;
      T += e * v;
    }
    S = wave_sum(S);
    T = wave_sum(T);
    const int64_t y = labels[i];
    if (y >= 0 && y < C) {
      const float cy = row[y];
      loss = logf(S) - (s * cy - m);
      grad = s * (T / S - cy);
    }
  }
  if (lane == 0) out[r] = make_float2(loss, grad);
}

// lr == nullptr: evaluate only (batch_out receives {mean loss, mean d theta}).  Otherwise torch.optim.SGD.step on the state with *lr.
__global__ __launch_bounds__(256) void tempscale_finish_kernel(const float2* __restrict__ rows, int n, float* __restrict__ state,
                                                               const float* __restrict__ lr, SgdArgs a, float* __restrict__ loss_out,
                                                               float* __restrict__ batch_out) {
#pragma clang fp contract(off)   // torch's add(other, alpha) rounds the product
  __shared__ double sl[2][256];
  const int t = threadIdx.x;
  double lg[2] = {0.0, 0.0};   // the losses, the gradients
  for (int r = t; r < n; r += 256) {
    const float2 v = rows[r];
    lg[0] += (double)v.x;
    lg[1] += (double)v.y;
  }
  block_sum_f64(lg, sl);
  if (t != 0) return;
  const float loss = (float)(lg[0] / (double)n);
  float grad = (float)(lg[1] / (double)n);
  if (batch_out) {
    batch_out[0] = loss;
    batch_out[1] = grad;
  }
  if (loss_out) *loss_out = loss;
  if (!lr) return;
  const float th = state[0];
  int32_t* steps = reinterpret_cast<int32_t*>(state) + 2;
  if (a.weight_decay != 0.f) grad = grad + a.weight_decay * th;
  if (a.momentum != 0.f) {
    const float buf = *steps == 0 ? grad : a.momentum * state[1] + a.one_minus_dampening * grad;
    state[1] = buf;
    grad = a.nesterov ? grad + a.momentum * buf : buf;
  }
  state[0] = th - *lr * grad;
  *steps += 1;
  state[3] = loss;
}

int check_matrix(const char* who, const float* cosine, int64_t ld, const int64_t* labels, int n, int C) {
  CLIPMI_REQUIRE(cosine && labels, CLIPMI_ERR_ARG, "%s: null pointer (cosine and labels are required)", who);
  CLIPMI_REQUIRE(n >= 1, CLIPMI_ERR_SHAPE, "%s: n=%d (>= 1)", who, n);
  CLIPMI_REQUIRE(C >= 2, CLIPMI_ERR_SHAPE, "%s: C=%d (>= 2 classes)", who, C);
  CLIPMI_REQUIRE(ld >= C, CLIPMI_ERR_SHAPE, "%s: ld=%lld < C=%d", who, (long long)ld, C);
  return CLIPMI_OK;
}

int check_workspace(const char* who, const void* workspace, size_t bytes, int rows) {
  CLIPMI_REQUIRE(workspace, CLIPMI_ERR_ARG, "%s: null workspace", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 8 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 8-byte aligned", who);
  CLIPMI_REQUIRE(bytes >= clipmi_tempscale_workspace_bytes(rows), CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, bytes,
                 clipmi_tempscale_workspace_bytes(rows));
  return CLIPMI_OK;
}

int launch_rows(const float* cosine, int64_t ld, const int64_t* labels, const int32_t* order, int first, int rows, int n, int C,
                const float* theta, float2* out, hipStream_t s) {
  hipLaunchKernelGGL(tempscale_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, cosine, ld, labels, order, first, rows, n, C, theta, out);
  return check_launch("tempscale_rows_kernel");
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

size_t clipmi_tempscale_workspace_bytes(int rows) { return rows < 1 ? 0 : align256((size_t)rows * sizeof(float2)); }

int clipmi_tempscale_batch(const float* cosine, int64_t ld, const int64_t* labels, const int32_t* order, int rows, int n, int C,
                           const float* theta, float* out, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_matrix("tempscale_batch", cosine, ld, labels, n, C)) return rc;
  CLIPMI_REQUIRE(theta && out, CLIPMI_ERR_ARG, "tempscale_batch: null pointer (theta and out are required)");
  CLIPMI_REQUIRE(rows >= 1, CLIPMI_ERR_SHAPE, "tempscale_batch: rows=%d (>= 1)", rows);
  CLIPMI_REQUIRE(order || rows <= n, CLIPMI_ERR_SHAPE, "tempscale_batch: rows=%d of n=%d without an order", rows, n);
  if (int rc = check_workspace("tempscale_batch", workspace, workspace_bytes, rows)) return rc;
  float2* pairs = static_cast<float2*>(workspace);
  if (int rc = launch_rows(cosine, ld, labels, order, 0, rows, n, C, theta, pairs, s)) return rc;
  hipLaunchKernelGGL(tempscale_finish_kernel, dim3(1), dim3(256), 0, s, pairs, rows, nullptr, nullptr, SgdArgs{}, nullptr, out);
  return check_launch("tempscale_finish_kernel");
}

int clipmi_tempscale_fit(const float* cosine, int64_t ld, const int64_t* labels, const int32_t* order, int n, int C, int batch, int epochs,
                         int drop_last, const float* lr, float momentum, float dampening, float weight_decay, int nesterov, float* state,
                         float* losses, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_matrix("tempscale_fit", cosine, ld, labels, n, C)) return rc;
  CLIPMI_REQUIRE(lr && state, CLIPMI_ERR_ARG, "tempscale_fit: null pointer (lr and state are required)");
  CLIPMI_REQUIRE((uintptr_t)state % 4 == 0, CLIPMI_ERR_ARG, "tempscale_fit: the state must be 4-byte aligned");
  CLIPMI_REQUIRE(batch >= 1, CLIPMI_ERR_SHAPE, "tempscale_fit: batch=%d (>= 1)", batch);
  CLIPMI_REQUIRE(epochs >= 0, CLIPMI_ERR_ARG, "tempscale_fit: epochs=%d (>= 0)", epochs);
  if (int rc = check_sgd("tempscale_fit", momentum, dampening, weight_decay, nesterov)) return rc;
  const int width = batch < n ? batch : n;   // the widest batch of the run
  if (int rc = check_workspace("tempscale_fit", workspace, workspace_bytes, width)) return rc;
  const int per_epoch = drop_last ? n / batch : (int)(((int64_t)n + batch - 1) / batch);
  const SgdArgs a = make_sgd_args(momentum, dampening, weight_decay, nesterov, 0);
  float2* pairs = static_cast<float2*>(workspace);
  int64_t step = 0;
  for (int e = 0; e < epochs; ++e) {
    const int32_t* epoch_order = order ? order + (int64_t)e * n : nullptr;
    for (int k = 0; k < per_epoch; ++k, ++step) {
      const int first = k * batch;   // k < per_epoch <= n: no overflow
      const int rows = n - first < batch ? n - first : batch;
      if (int rc = launch_rows(cosine, ld, labels, epoch_order ? epoch_order + first : nullptr, first, rows, n, C, state, pairs, s)) return rc;
      hipLaunchKernelGGL(tempscale_finish_kernel, dim3(1), dim3(256), 0, s, pairs, rows, state, lr + step, a, losses ? losses + step : nullptr,
                         nullptr);
      if (int rc = check_launch("tempscale_finish_kernel")) return rc;
    }
  }
  return CLIPMI_OK;
}

}  // extern "C"
