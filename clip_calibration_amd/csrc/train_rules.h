// What the training translation units share (adapter_train.hip, taskres_train.hip): torch's optimiser rules on one fp32 element and the
// batch loss as the float64 mean of the fp32 row losses.  Device code only; every rule is compiled with contraction off, so each product
// is rounded before it is added, as torch's own kernels round it.
#pragma once
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
// text_backward.hip): every add(other, alpha) is ONE fused multiply-add there -- g + wd w, mul_(momentum) rounded and then
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

// *loss_out = float(float64 mean of loss[0 .. rows)) by the 256 threads of one workgroup: thread-strided float64 partial sums, then a
// binary tree over LDS -- a fixed order.  Every thread of the workgroup calls it.
__device__ __forceinline__ void mean_loss_256(const float* __restrict__ loss, int rows, float* __restrict__ loss_out) {
  __shared__ double sl[256];
  const int t = threadIdx.x;
  double l = 0.0;
  for (int b = t; b < rows; b += 256) l += (double)loss[b];
  sl[t] = l;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) sl[t] += sl[t + w];
    __syncthreads();
  }
  if (t == 0) *loss_out = (float)(sl[0] / (double)rows);
}
#endif

}  // namespace clipmi
