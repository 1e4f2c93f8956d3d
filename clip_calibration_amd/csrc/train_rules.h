// What the training translation units share (adapter_train.hip, taskres_train.hip, tempscale.hip, prompt_train.hip): torch.optim.SGD's
// hyper-parameter rules on the host, torch's optimiser rules on one fp32 element, the workgroup reductions, the cross-entropy row and the
// batch loss as the float64 mean of the fp32 row losses.  Every device rule is compiled with contraction off, so each product is rounded
// before it is added, as torch's own kernels round it.
#pragma once
#include <cmath>

#include "common.h"

namespace clipmi {

struct SgdArgs {
  float momentum, one_minus_dampening, weight_decay;
  int nesterov, first_step;   // first_step: the momentum buffers are initialised from this step's gradient (torch's buf is None)
};

// torch.optim.Adam (no amsgrad), the constants as torch's single-tensor path forms them: in double on the host, once per step
struct AdamArgs {
  float one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
  double bias_correction1, bias_correction2_sqrt;   // 1 - beta1^t, sqrt(1 - beta2^t) of this step's t (1 on the first)
};

// torch.optim.SGD's own refusals (torch/optim/sgd.py); a momentum's buffer is the caller's to check, since the buffers differ
inline int check_sgd(const char* who, float momentum, float dampening, float weight_decay, int nesterov) {
  CLIPMI_REQUIRE(momentum >= 0.f && momentum < 1.f, CLIPMI_ERR_ARG, "%s: momentum=%g (in [0, 1))", who, momentum);
  CLIPMI_REQUIRE(dampening >= 0.f && dampening < 1.f, CLIPMI_ERR_ARG, "%s: dampening=%g (in [0, 1))", who, dampening);
  CLIPMI_REQUIRE(weight_decay >= 0.f && std::isfinite(weight_decay), CLIPMI_ERR_ARG, "%s: weight_decay=%g (finite, >= 0)", who, weight_decay);
  CLIPMI_REQUIRE(!nesterov || (momentum > 0.f && dampening == 0.f), CLIPMI_ERR_ARG,
                 "%s: nesterov needs a momentum and zero dampening (momentum=%g, dampening=%g)", who, momentum, dampening);
  return CLIPMI_OK;
}
// what a block's step (clipmi_maple_step, clipmi_promptsrc_step) asks of the optimiser's arguments; their one-call step asks it before
// anything is enqueued
inline int check_step_args(const char* who, const float* block, const float* buf, const float* grad_out, int apply, const float* lr, float grad_scale,
                           float momentum, float dampening, float weight_decay, int nesterov) {
  CLIPMI_REQUIRE(block, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(apply || grad_out, CLIPMI_ERR_ARG, "%s: null pointer (nothing to write)", who);
  CLIPMI_REQUIRE(!apply || lr, CLIPMI_ERR_ARG, "%s: null pointer (a step needs lr)", who);
  CLIPMI_REQUIRE(std::isfinite(grad_scale) && grad_scale > 0.f, CLIPMI_ERR_ARG, "%s: grad_scale=%g (finite, > 0)", who, grad_scale);
  if (int rc = check_sgd(who, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE(!apply || momentum == 0.f || buf, CLIPMI_ERR_ARG, "%s: null pointer (a momentum needs the buffer)", who);
  return CLIPMI_OK;
}
inline SgdArgs make_sgd_args(float momentum, float dampening, float weight_decay, int nesterov, int first_step) {
  return SgdArgs{momentum, (float)(1.0 - (double)dampening), weight_decay, nesterov ? 1 : 0, first_step ? 1 : 0};
}

// ProGrad's float64 dots: the first launch's grid is at most this many workgroups, a function of the context's size alone
constexpr int PROGRAD_DOT_BLOCKS = 256;

#ifdef __HIPCC__
// torch.optim.SGD's rule on one element (torch rounds the products of add(other, alpha) before it adds)
__device__ __forceinline__ void sgd_element(float* __restrict__ w, float* __restrict__ buf, int64_t idx, float grad, float lr, const SgdArgs& a) {
#pragma clang fp contract(off)
  const float v = w[idx];
  if (a.weight_decay != 0.f) grad = grad + a.weight_decay * v;
  if (a.momentum != 0.f) {
    const float b = a.first_step ? grad : a.momentum * buf[idx] + a.one_minus_dampening * grad;
    buf[idx] = b;
    grad = a.nesterov ? grad + a.momentum * b : b;
  }
  w[idx] = v - lr * grad;
}

// The same rule as torch's foreach kernels on the GPU evaluate it, for a caller that is held to torch.optim.SGD bit for bit (ctx_step_kernel,
// prompt_train.hip): every add(other, alpha) is ONE fused multiply-add there -- g + wd w, mul_(momentum) rounded and then
// buf + (1 - dampening) g, g + momentum buf, w + (-lr) g -- as measured on the MI355X (tests/test_gpu_text_backward.py).
__device__ __forceinline__ void sgd_element_fma(float* __restrict__ w, float* __restrict__ buf, int64_t idx, float grad, float lr, const SgdArgs& a) {
#pragma clang fp contract(off)
  const float v = w[idx];
  if (a.weight_decay != 0.f) grad = fmaf(a.weight_decay, v, grad);
  if (a.momentum != 0.f) {
    const float b = a.first_step ? grad : fmaf(a.one_minus_dampening, grad, a.momentum * buf[idx]);
    buf[idx] = b;
    grad = a.nesterov ? fmaf(a.momentum, b, grad) : b;
  }
  w[idx] = fmaf(-lr, grad, v);
}

// Element idx of the context's gradient from d_embed fp32 [C * L, D] (prompt_train.hip's ctx_step_kernel and ProGrad's step, grad_scaler.hip):
// row 1 + j of every prompt belongs to context vector j; the classes' rows added in ascending order (generic context) or the class's own
// row (per_class), times inv_scale
__device__ __forceinline__ float ctx_grad_element(const float* __restrict__ d_embed, int64_t idx, int C, int L, int D, int n_ctx, int per_class,
                                                  float inv_scale) {
  const int64_t per = (int64_t)n_ctx * D;
  const int d = (int)(idx % D), j = (int)((idx / D) % n_ctx);
  float g = 0.f;
  if (per_class) {
    const int64_t c = idx / per;
    g = d_embed[((c * L) + 1 + j) * D + d];
  } else {
    for (int64_t c = 0; c < C; ++c) g += d_embed[((c * L) + 1 + j) * D + d];
  }
  return g * inv_scale;
}

// The balanced split of the class-sharded fits (shard_train.hip, proda_train.hip): the first C mod G of the G ranks own one item more.
// Returns the rank that owns item c of C; *lo: that rank's first item
__device__ __forceinline__ int shard_owner(int c, int C, int G, int* lo) {
  const int base = C / G, rem = C % G, cut = rem * (base + 1);
  const int r = c < cut ? c / (base + 1) : rem + (c - cut) / base;   // base >= 1: C >= G
  *lo = r * base + (r < rem ? r : rem);
  return r;
}

// ProGrad's rule (reference prograd.py:371-409) on the float64 dots a.a, b.b, a.b of its two context gradients (prompt_train.hip's
// prograd_step_kernel, shard_train.hip): the reference compares dot(a / |a|, b / |b|) with 0, which is a.b < 0 unless a norm is zero or
// something is not finite, where its comparison is false and the plain a is applied.  The element: a - lambda (a.b / b.b) b, the scalar
// in float64, the product rounded before the subtraction
__device__ __forceinline__ bool prograd_projects(double aa, double bb, double ab) {
  return isfinite(aa) && isfinite(bb) && isfinite(ab) && ab < 0.0 && aa > 0.0 && bb > 0.0;
}
__device__ __forceinline__ float prograd_element(float a, float b, bool project, float lambda, double ab, double bb) {
#pragma clang fp contract(off)
  if (!project) return a;
  const float k = (float)((double)lambda * (ab / bb));
  return a - k * b;
}

// torch.optim.Adam's rule on one element: g += wd w;  m += (g - m)(1 - b1)  (lerp_ with a weight below one half);
// v = b2 v + ((1 - b2) g) g  (mul_, addcmul_);  w -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)  (addcdiv_)
__device__ __forceinline__ void adam_element(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v, int64_t idx, float grad, float lr,
                                             const AdamArgs& a) {
#pragma clang fp contract(off)
  const float p = w[idx];
  if (a.weight_decay != 0.f) grad = grad + a.weight_decay * p;
  const float m0 = m[idx];
  const float m1 = m0 + (grad - m0) * a.one_minus_beta1;
  const float v1 = a.beta2 * v[idx] + (a.one_minus_beta2 * grad) * grad;
  m[idx] = m1;
  v[idx] = v1;
  const float step_size = (float)((double)lr / a.bias_correction1);
  const float denom = sqrtf(v1) / (float)a.bias_correction2_sqrt + a.eps;
  w[idx] = p - step_size * m1 / denom;
}

// torch.optim.AdamW's rule on one element (Adam with decoupled_weight_decay): w *= 1 - lr wd, the factor formed in double and rounded
// once as torch's Python scalar is, then Adam's rule above on the decayed value with no weight decay in the gradient
__device__ __forceinline__ void adamw_element(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v, int64_t idx, float grad, float lr,
                                              const AdamArgs& a) {
#pragma clang fp contract(off)
  float p = w[idx];
  if (a.weight_decay != 0.f) p = p * (float)(1.0 - (double)lr * (double)a.weight_decay);
  const float m0 = m[idx];
  const float m1 = m0 + (grad - m0) * a.one_minus_beta1;
  const float v1 = a.beta2 * v[idx] + (a.one_minus_beta2 * grad) * grad;
  m[idx] = m1;
  v[idx] = v1;
  const float step_size = (float)((double)lr / a.bias_correction1);
  const float denom = sqrtf(v1) / (float)a.bias_correction2_sqrt + a.eps;
  w[idx] = p - step_size * m1 / denom;
}

// One value per wave (the same in every lane) to the sum / maximum over the workgroup's WAVES waves, in ascending wave order through sw
// (WAVES floats of LDS): one barrier.  Every thread of the workgroup calls it and holds the result.  There is no barrier in front: a
// caller that reduces twice gives each reduction WAVES floats of its own, or puts a barrier between the two.
template <int WAVES>
__device__ __forceinline__ float waves_sum(float v, float* sw) {
#pragma clang fp contract(off)
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
  __syncthreads();
  v = sw[0];
  for (int w = 1; w < WAVES; ++w) v += sw[w];
  return v;
}
template <int WAVES>
__device__ __forceinline__ float waves_max(float v, float* sw) {
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
  __syncthreads();
  v = sw[0];
  for (int w = 1; w < WAVES; ++w) v = fmaxf(v, sw[w]);
  return v;
}
// the same over the WAVES * 64 threads' own values: the wave tree first
template <int WAVES>
__device__ __forceinline__ float block_sum(float v, float* sw) { return waves_sum<WAVES>(wave_sum(v), sw); }
template <int WAVES>
__device__ __forceinline__ float block_max(float v, float* sw) { return waves_max<WAVES>(wave_max(v), sw); }

// N float64 sums over the 256 threads of a workgroup by one binary tree over LDS -- a fixed order.  Every thread calls it and holds the
// results.  No barrier in front either: a second use of the same sl waits for a barrier behind the first.
template <int N>
__device__ __forceinline__ void block_sum_f64(double (&v)[N], double (*sl)[256]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < N; ++i) sl[i][t] = v[i];
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
#pragma unroll
      for (int i = 0; i < N; ++i) sl[i][t] += sl[i][t + h];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = sl[i][0];
}

// float64 sum of x[0 .. n) by the 256 threads of one workgroup: thread-strided float64 partial sums, then the tree over sl
__device__ __forceinline__ double sum_f64_256(const float* __restrict__ x, int n, double (*sl)[256]) {
  double s[1] = {0.0};
  for (int i = threadIdx.x; i < n; i += 256) s[0] += (double)x[i];
  block_sum_f64(s, sl);
  return s[0];
}

// *loss_out = float(float64 mean of loss[0 .. rows)).  Every thread of the 256-thread workgroup calls it.
__device__ __forceinline__ void mean_loss_256(const float* __restrict__ loss, int rows, float* __restrict__ loss_out) {
  __shared__ double sl[1][256];
  const double s = sum_f64_256(loss, rows, sl);
  if (threadIdx.x == 0) *loss_out = (float)(s / (double)rows);
}

// The cross-entropy of one row of C logits z with the row maximum m and the label y in [0, C): S = sum_c exp(z_c - m) thread-strided, then
// block_sum through sw (WAVES floats no earlier reduction still reads); *loss = log S - (z_y - m); dz_c = (exp(z_c - m) / S - [c == y]) k,
// the caller's factor k already formed.  dz may be z itself (z_y is read before the barrier, the stores follow it), so neither is
// __restrict__.  One barrier.  Every thread of the WAVES * 64 calls it, the logits final and visible to the workgroup.
template <int WAVES>
__device__ __forceinline__ void xent_row(const float* z, float* dz, int C, float m, int64_t y, float k, float* sw, float* loss) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  const float zy = t == 0 ? z[y] : 0.f;   // thread 0 writes the loss
  float S = 0.f;
  for (int c = t; c < C; c += WAVES * 64) S += __expf(z[c] - m);
  S = block_sum<WAVES>(S, sw);
  if (t == 0) *loss = logf(S) - (zy - m);
  for (int c = t; c < C; c += WAVES * 64) {
    const float p = __expf(z[c] - m) / S;
    dz[c] = (c == y ? p - 1.f : p) * k;
  }
}
#endif

}  // namespace clipmi
