// torch.optim.Adam's and torch.optim.AdamW's step on a whole fp32 master block, for the prompt fits whose own launches form the block's
// gradient without applying it (CoOp, KgCoOp, ProGrad, ProDA, CoCoOp, VPT, MaPLe, PromptSRC).  DESIGN.md "Adam steps for the prompt fits".
//   block_adam_kernel          the static-scale step: g = grad / grad_scale, then adam_element / adamw_element (train_rules.h), one launch
//   scaled_adam_apply_kernel   the third launch of the dynamic-scale step, behind grad_scaler.hip's block_unscale_kernel and
//                              scaler_update_kernel: the same rule on the workspace's unscaled gradient, only when the decision record says
//                              the step is clean
// The bias corrections 1 - beta1^t and sqrt(1 - beta2^t) come from a float64 table [table_len, 2] that the host fills for t = 1 ..
// table_len as Python forms them: no pow on the device, and under the dynamic scale t is the number of APPLIED steps, which only the
// device knows.  One thread per element, integer flags, no atomics: the same inputs give the same bits.
#include <cmath>

#include "common.h"
#include "model.h"
#include "train_rules.h"

namespace clipmi {
namespace {

constexpr int THREADS = SCALED_THREADS;

// what both kernels take of the rule; the two corrections are read from the table on the device
struct AdamRule {
  float one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
  int decoupled;
};

__device__ __forceinline__ AdamArgs adam_args(const AdamRule& r, const double* __restrict__ table, int64_t t) {
  return AdamArgs{r.one_minus_beta1, r.beta2, r.one_minus_beta2, r.eps, r.weight_decay, table[2 * (t - 1)], table[2 * (t - 1) + 1]};
}

// one thread per element; t in 1 .. table_len has been checked on the host.  grad_out may be grad itself: an element is read and
// written by one thread
__global__ __launch_bounds__(THREADS) void block_adam_kernel(const float* grad, float* __restrict__ params, float* __restrict__ exp_avg,
                                                             float* __restrict__ exp_avg_sq, float* grad_out, int64_t total, float inv_scale,
                                                             const float* __restrict__ lr, int64_t t, const double* __restrict__ table, AdamRule r) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= total) return;
  const float g = grad[idx] * inv_scale;
  if (grad_out) grad_out[idx] = g;
  const AdamArgs a = adam_args(r, table, t);
  if (r.decoupled) adamw_element(params, exp_avg, exp_avg_sq, idx, g, *lr, a);
  else adam_element(params, exp_avg, exp_avg_sq, idx, g, *lr, a);
}

// one thread per element: nothing is written on a skipped step.  scaler_update_kernel has counted this step into applied_steps before
// this launch reads it, so on a clean step Adam's step number t IS st->applied_steps (1 on the first applied step), not applied_steps + 1.
// A t outside the table writes nothing: the caller keeps the table longer than the steps it has enqueued
__global__ __launch_bounds__(THREADS) void scaled_adam_apply_kernel(ScaledWs w, float* __restrict__ params, float* __restrict__ exp_avg,
                                                                    float* __restrict__ exp_avg_sq, int64_t total, const float* __restrict__ lr,
                                                                    const clipmi_scaler_state* __restrict__ st, const double* __restrict__ table,
                                                                    int64_t table_len, AdamRule r) {
  if (w.decision[0]) return;   // the same for every thread of the launch
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= total) return;
  const int64_t t = st->applied_steps;
  if (t < 1 || t > table_len) return;
  const AdamArgs a = adam_args(r, table, t);
  if (r.decoupled) adamw_element(params, exp_avg, exp_avg_sq, idx, w.grad[idx], *lr, a);
  else adam_element(params, exp_avg, exp_avg_sq, idx, w.grad[idx], *lr, a);
}

// torch.optim.Adam's own refusals (torch/optim/adam.py) and what both steps ask of their pointers and the shape
int check_adam_common(const char* who, const float* grad, const float* params, const float* exp_avg, const float* exp_avg_sq, const float* grad_out,
                      const float* lr, const double* table, int64_t table_len, int64_t total, double beta1, double beta2, double eps, float weight_decay) {
  CLIPMI_REQUIRE(grad && params && exp_avg && exp_avg_sq && lr && table, CLIPMI_ERR_ARG,
                 "%s: null pointer (grad, params, exp_avg, exp_avg_sq, lr and bias_table are required)", who);
  CLIPMI_REQUIRE(((uintptr_t)grad | (uintptr_t)params | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)grad_out | (uintptr_t)lr) % 4 == 0,
                 CLIPMI_ERR_ARG, "%s: grad, params, exp_avg, exp_avg_sq, grad_out and lr must be 4-byte aligned", who);
  CLIPMI_REQUIRE((uintptr_t)table % 8 == 0, CLIPMI_ERR_ARG, "%s: bias_table must be 8-byte aligned", who);
  CLIPMI_REQUIRE(table_len >= 1, CLIPMI_ERR_ARG, "%s: table_len=%lld (>= 1)", who, (long long)table_len);
  CLIPMI_REQUIRE(total >= 1, CLIPMI_ERR_SHAPE, "%s: total=%lld (>= 1)", who, (long long)total);
  CLIPMI_REQUIRE(total < (1ll << 31) * THREADS, CLIPMI_ERR_SHAPE, "%s: %lld elements are too many", who, (long long)total);
  CLIPMI_REQUIRE(beta1 >= 0.0 && beta1 < 1.0, CLIPMI_ERR_ARG, "%s: beta1=%g (in [0, 1))", who, beta1);
  CLIPMI_REQUIRE(beta2 >= 0.0 && beta2 < 1.0, CLIPMI_ERR_ARG, "%s: beta2=%g (in [0, 1))", who, beta2);
  CLIPMI_REQUIRE(std::isfinite(eps) && eps > 0.0, CLIPMI_ERR_ARG, "%s: eps=%g (finite, > 0)", who, eps);
  CLIPMI_REQUIRE(weight_decay >= 0.f && std::isfinite(weight_decay), CLIPMI_ERR_ARG, "%s: weight_decay=%g (finite, >= 0)", who, weight_decay);
  return CLIPMI_OK;
}

// the constants as torch's single-tensor path hands them to its kernels: 1 - beta in double, then rounded
AdamRule make_rule(double beta1, double beta2, double eps, float weight_decay, int decoupled) {
  return AdamRule{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, weight_decay, decoupled ? 1 : 0};
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

int clipmi_block_step_adam(const float* grad, float* params, float* exp_avg, float* exp_avg_sq, float* grad_out, int64_t total, float grad_scale,
                           const float* lr, int64_t t, const double* bias_table, int64_t table_len, double beta1, double beta2, double eps,
                           float weight_decay, int decoupled, clipmi_stream_t stream) {
  const char* who = "block_step_adam";
  if (int rc = check_adam_common(who, grad, params, exp_avg, exp_avg_sq, grad_out, lr, bias_table, table_len, total, beta1, beta2, eps, weight_decay))
    return rc;
  CLIPMI_REQUIRE(std::isfinite(grad_scale) && grad_scale > 0.f, CLIPMI_ERR_ARG, "%s: grad_scale=%g (finite, > 0)", who, grad_scale);
  CLIPMI_REQUIRE(t >= 1, CLIPMI_ERR_ARG, "%s: t=%lld (Adam's step number, >= 1)", who, (long long)t);
  CLIPMI_REQUIRE(t <= table_len, CLIPMI_ERR_ARG, "%s: t=%lld lies behind the bias table of %lld steps", who, (long long)t, (long long)table_len);
  hipLaunchKernelGGL(block_adam_kernel, dim3((unsigned)scaled_grad_blocks(total)), dim3(THREADS), 0, (hipStream_t)stream, grad, params, exp_avg, exp_avg_sq,
                     grad_out, total, 1.f / grad_scale, lr, t, bias_table, make_rule(beta1, beta2, eps, weight_decay, decoupled));
  return check_launch("block_adam_kernel");
}

size_t clipmi_block_step_adam_scaled_workspace_bytes(int64_t total) { return block_step_scaled_bytes(total); }

int clipmi_block_step_adam_scaled(const float* grad, float* params, float* exp_avg, float* exp_avg_sq, float* grad_out, int64_t total,
                                  clipmi_scaler_state* state, float growth_factor, float backoff_factor, int growth_interval, const float* lr,
                                  const double* bias_table, int64_t table_len, double beta1, double beta2, double eps, float weight_decay, int decoupled,
                                  void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  const char* who = "block_step_adam_scaled";
  const ScalerCall sc{state, growth_factor, backoff_factor, growth_interval};
  if (int rc = check_adam_common(who, grad, params, exp_avg, exp_avg_sq, grad_out, lr, bias_table, table_len, total, beta1, beta2, eps, weight_decay))
    return rc;
  if (int rc = check_scaler(who, sc)) return rc;
  CLIPMI_REQUIRE(workspace, CLIPMI_ERR_ARG, "%s: null pointer (the workspace)", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 256-byte aligned", who);
  CLIPMI_REQUIRE(workspace_bytes >= scaled_step_bytes(total), CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
                 scaled_step_bytes(total));
  hipStream_t s = (hipStream_t)stream;
  const ScaledWs w = scaled_carve(workspace, total);
  if (int rc = launch_block_unscale(grad, grad_out, total, sc, w, s)) return rc;
  if (int rc = launch_scaler_update(w, total, sc, s)) return rc;
  hipLaunchKernelGGL(scaled_adam_apply_kernel, dim3((unsigned)scaled_grad_blocks(total)), dim3(THREADS), 0, s, w, params, exp_avg, exp_avg_sq, total, lr,
                     (const clipmi_scaler_state*)state, bias_table, table_len, make_rule(beta1, beta2, eps, weight_decay, decoupled));
  return check_launch("scaled_adam_apply_kernel");
}

}  // extern "C"
