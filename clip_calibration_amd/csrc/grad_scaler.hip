// torch.cuda.amp.GradScaler's rule on the device for the fits that step through clipmi_ctx_step (CoOp, KgCoOp; reference
// trainers/classification/coop.py:286-291): the backward carries scale * gradient with the scale in a device block, a step whose gradient
// holds an inf or a NaN is skipped, and the scale backs off and grows again -- without a host read.  DESIGN.md "Dynamic loss scale".
//   grad_scale_rows_kernel    x *= state->scale: the head runs at grad_scale = 1 and its d_text is multiplied here (exact for a power of two)
//   scaled_grad_kernel        the context's unscaled gradient (ctx_step_kernel's arithmetic) into the workspace, one found-non-finite flag per workgroup
//   block_unscale_kernel      the same for a fit whose own launches formed scale * gradient of a whole master block (clipmi_block_step_scaled)
//   scaler_update_kernel      ONE workgroup: ORs the flags, writes the decision record of this step, applies _amp_update_scale_'s rule to the block
//   scaled_apply_kernel       torch.optim.SGD's rule (sgd_element_fma) on every element, only when the decision record says the step is clean
// The state block is read by the first launch and written by the second alone; the third reads the decision record only: no workgroup
// reads what another workgroup of the same launch writes.  Integer flags, no atomics: the same inputs give the same bits.
#include <cmath>

#include "common.h"
#include "model.h"
#include "train_rules.h"

namespace clipmi {
namespace {

constexpr int THREADS = SCALED_THREADS;   // one found-non-finite flag per workgroup (model.h)

enum { MODE_COOP = 0, MODE_KGCOOP = 1, MODE_PROGRAD = 2 };   // `mode` of clipmi_prompt_head (include/clipmi.h)

__global__ __launch_bounds__(THREADS) void grad_scale_rows_kernel(float* __restrict__ x, int64_t n, const clipmi_scaler_state* __restrict__ st) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx < n) x[idx] *= st->scale;
}

// one thread per element of ctx: g = (the context row's sum) / scale, as ctx_step_kernel forms it at grad_scale = scale; the workgroup's
// flag is set when any of its elements is an inf or a NaN (a non-finite sum stays non-finite through the division)
__global__ __launch_bounds__(THREADS) void scaled_grad_kernel(const float* __restrict__ d_embed, float* __restrict__ grad_out, int C, int L, int D, int n_ctx,
                                                              int per_class, int64_t total, const clipmi_scaler_state* __restrict__ st, ScaledWs w) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  int bad = 0;
  if (idx < total) {
    const float g = ctx_grad_element(d_embed, idx, C, L, D, n_ctx, per_class, 1.f / st->scale);
    w.grad[idx] = g;
    if (grad_out) grad_out[idx] = g;
    bad = !isfinite(g);
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) w.flags[blockIdx.x] = bad ? 1 : 0;
}

// one thread per element of a master block: g = grad / scale for a gradient that the fit's own launches formed at grad_scale = 1 from a
// backward carrying scale * gradient (CoCoOp, VPT, MaPLe, PromptSRC); the flag as above.  grad_out may be grad itself: an element is read
// and written by one thread
__global__ __launch_bounds__(THREADS) void block_unscale_kernel(const float* grad, float* grad_out, int64_t total, const clipmi_scaler_state* __restrict__ st,
                                                                ScaledWs w) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  int bad = 0;
  if (idx < total) {
    const float g = grad[idx] * (1.f / st->scale);
    w.grad[idx] = g;
    if (grad_out) grad_out[idx] = g;
    bad = !isfinite(g);
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) w.flags[blockIdx.x] = bad ? 1 : 0;
}

// grid (1).  torch's _amp_update_scale_: found -> scale *= backoff, tracker = 0; else the tracker counts up to growth_interval, where the
// scale grows (only to a finite value) and the tracker starts again.  The counters are this library's own.
__global__ __launch_bounds__(THREADS) void scaler_update_kernel(ScaledWs w, int64_t blocks, clipmi_scaler_state* __restrict__ st, float growth, float backoff,
                                                                int growth_interval) {
  int bad = 0;
  for (int64_t b = threadIdx.x; b < blocks; b += THREADS) bad |= w.flags[b];
  bad = __syncthreads_or(bad);
  if (threadIdx.x != 0) return;
  w.decision[0] = bad ? 1 : 0;
  w.decision[1] = st->applied_steps == 0 ? 1 : 0;
  st->found_inf = bad ? 1 : 0;
  if (bad) {
    st->scale = st->scale * backoff;
    st->growth_tracker = 0;
    st->skipped_steps += 1;
    return;
  }
  st->applied_steps += 1;
  const int successful = st->growth_tracker + 1;
  if (successful == growth_interval) {
    const float grown = st->scale * growth;
    if (isfinite(grown)) st->scale = grown;
    st->growth_tracker = 0;
  } else {
    st->growth_tracker = successful;
  }
}

// one thread per element of ctx: nothing is written on a skipped step; the momentum buffer starts from the first APPLIED step's gradient
__global__ __launch_bounds__(THREADS) void scaled_apply_kernel(ScaledWs w, float* __restrict__ ctx, float* __restrict__ buf, int64_t total,
                                                               const float* __restrict__ lr, SgdArgs sgd) {
  if (w.decision[0]) return;   // the same for every thread of the launch
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= total) return;
  sgd.first_step = w.decision[1];
  sgd_element_fma(ctx, buf, idx, w.grad[idx], *lr, sgd);
}

// what every scaled step refuses behind its caller's own first lines (the required pointers and the shape), before anything is launched
int check_scaled_common(const char* who, const ScalerCall& sc, const float* buf, int64_t total, float momentum, float dampening, float weight_decay,
                        int nesterov, const void* workspace, size_t workspace_bytes) {
  if (int rc = check_scaler(who, sc)) return rc;
  if (int rc = check_sgd(who, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE(momentum == 0.f || buf, CLIPMI_ERR_ARG, "%s: null pointer (a momentum needs the buffer)", who);
  CLIPMI_REQUIRE(total < (1ll << 31) * THREADS, CLIPMI_ERR_SHAPE, "%s: %lld elements are too many", who, (long long)total);
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 256-byte aligned", who);
  CLIPMI_REQUIRE(workspace_bytes >= scaled_step_bytes(total), CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
                 scaled_step_bytes(total));
  return CLIPMI_OK;
}

}  // namespace

// ---- what every scaled step shares (model.h)
int check_scaler(const char* who, const ScalerCall& sc) {
  CLIPMI_REQUIRE(sc.state, CLIPMI_ERR_ARG, "%s: null pointer (the scaler's state block)", who);
  CLIPMI_REQUIRE((uintptr_t)sc.state % 4 == 0, CLIPMI_ERR_ARG, "%s: the scaler's state block must be 4-byte aligned", who);
  CLIPMI_REQUIRE(std::isfinite(sc.growth) && sc.growth > 0.f && std::isfinite(sc.backoff) && sc.backoff > 0.f, CLIPMI_ERR_ARG,
                 "%s: growth_factor=%g, backoff_factor=%g (both finite, > 0)", who, sc.growth, sc.backoff);
  CLIPMI_REQUIRE(sc.interval >= 1, CLIPMI_ERR_ARG, "%s: growth_interval=%d (>= 1)", who, sc.interval);
  return CLIPMI_OK;
}

// the first two launches of a block's scaled step, for the callers that apply a rule of their own behind them (optim_step.hip): the
// unscale-and-flag launch over a block of scale * gradient, and the decision launch; every argument has been checked
int launch_block_unscale(const float* grad, float* grad_out, int64_t total, const ScalerCall& sc, const ScaledWs& w, hipStream_t s) {
  hipLaunchKernelGGL(block_unscale_kernel, dim3((unsigned)scaled_grad_blocks(total)), dim3(THREADS), 0, s, grad, grad_out, total,
                     (const clipmi_scaler_state*)sc.state, w);
  return check_launch("block_unscale_kernel");
}
int launch_scaler_update(const ScaledWs& w, int64_t total, const ScalerCall& sc, hipStream_t s) {
  hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(THREADS), 0, s, w, scaled_grad_blocks(total), sc.state, sc.growth, sc.backoff, sc.interval);
  return check_launch("scaler_update_kernel");
}

// the decision launch and the step launch behind a first launch that has filled w.grad and w.flags; every argument has been checked
int launch_scaled_decide_apply(const ScaledWs& w, int64_t total, float* params, float* buf, const ScalerCall& sc, const float* lr, float momentum,
                               float dampening, float weight_decay, int nesterov, hipStream_t s) {
  if (int rc = launch_scaler_update(w, total, sc, s)) return rc;
  hipLaunchKernelGGL(scaled_apply_kernel, dim3((unsigned)scaled_grad_blocks(total)), dim3(THREADS), 0, s, w, params, buf, total, lr,
                     make_sgd_args(momentum, dampening, weight_decay, nesterov, 0));
  return check_launch("scaled_apply_kernel");
}

// ---- what the fits' one-call steps share (model.h)
int launch_grad_scale_rows(const char* who, float* x, int rows, int cols, const clipmi_scaler_state* st, hipStream_t s) {
  CLIPMI_REQUIRE(x && st, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(rows >= 1 && cols >= 1, CLIPMI_ERR_SHAPE, "%s: rows=%d cols=%d", who, rows, cols);
  const int64_t n = (int64_t)rows * cols;
  hipLaunchKernelGGL(grad_scale_rows_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, x, n, st);
  return check_launch("grad_scale_rows_kernel");
}

// everything clipmi_ctx_step_scaled refuses, before anything is launched; *total: the elements of ctx
int check_ctx_step_scaled(const char* who, const float* d_embed, const float* ctx, const float* buf, const float* lr, int C, int L, int D, int n_ctx, int per_class,
                          const ScalerCall& sc, float momentum, float dampening, float weight_decay, int nesterov, const void* workspace, size_t workspace_bytes,
                          int64_t* total) {
  CLIPMI_REQUIRE(d_embed && ctx && lr && workspace, CLIPMI_ERR_ARG, "%s: null pointer (d_embed, ctx, lr and the workspace are required)", who);
  CLIPMI_REQUIRE(C >= 1 && D >= 1 && n_ctx >= 1 && 1 + n_ctx <= L, CLIPMI_ERR_SHAPE, "%s: C=%d L=%d D=%d n_ctx=%d", who, C, L, D, n_ctx);
  *total = (int64_t)n_ctx * D * (per_class ? C : 1);
  return check_scaled_common(who, sc, buf, *total, momentum, dampening, weight_decay, nesterov, workspace, workspace_bytes);
}

// the three launches; every argument has been checked
int launch_ctx_step_scaled(const float* d_embed, float* ctx, float* buf, float* grad_out, int C, int L, int D, int n_ctx, int per_class, int64_t total,
                           const ScalerCall& sc, const float* lr, float momentum, float dampening, float weight_decay, int nesterov, void* workspace,
                           hipStream_t s) {
  const ScaledWs w = scaled_carve(workspace, total);
  hipLaunchKernelGGL(scaled_grad_kernel, dim3((unsigned)scaled_grad_blocks(total)), dim3(THREADS), 0, s, d_embed, grad_out, C, L, D, n_ctx, per_class ? 1 : 0,
                     total, (const clipmi_scaler_state*)sc.state, w);
  if (int rc = check_launch("scaled_grad_kernel")) return rc;
  return launch_scaled_decide_apply(w, total, ctx, buf, sc, lr, momentum, dampening, weight_decay, nesterov, s);
}

size_t block_step_scaled_bytes(int64_t total) { return total >= 1 && total < (1ll << 31) * THREADS ? scaled_step_bytes(total) : 0; }

// everything clipmi_block_step_scaled refuses, before anything is launched
int check_block_step_scaled(const char* who, const float* grad, const float* params, const float* buf, const float* grad_out, const float* lr, int64_t total,
                            const ScalerCall& sc, float momentum, float dampening, float weight_decay, int nesterov, const void* workspace,
                            size_t workspace_bytes) {
  CLIPMI_REQUIRE(grad && params && lr && workspace, CLIPMI_ERR_ARG, "%s: null pointer (grad, params, lr and the workspace are required)", who);
  CLIPMI_REQUIRE(((uintptr_t)grad | (uintptr_t)params | (uintptr_t)buf | (uintptr_t)grad_out | (uintptr_t)lr) % 4 == 0, CLIPMI_ERR_ARG,
                 "%s: grad, params, buf, grad_out and lr must be 4-byte aligned", who);
  CLIPMI_REQUIRE(total >= 1, CLIPMI_ERR_SHAPE, "%s: total=%lld (>= 1)", who, (long long)total);
  return check_scaled_common(who, sc, buf, total, momentum, dampening, weight_decay, nesterov, workspace, workspace_bytes);
}

// the three launches; every argument has been checked
int launch_block_step_scaled(const float* grad, float* params, float* buf, float* grad_out, int64_t total, const ScalerCall& sc, const float* lr, float momentum,
                             float dampening, float weight_decay, int nesterov, void* workspace, hipStream_t s) {
  const ScaledWs w = scaled_carve(workspace, total);
  if (int rc = launch_block_unscale(grad, grad_out, total, sc, w, s)) return rc;
  return launch_scaled_decide_apply(w, total, params, buf, sc, lr, momentum, dampening, weight_decay, nesterov, s);
}

}  // namespace clipmi

using namespace clipmi;

extern "C" {

int clipmi_grad_scale_rows(float* x, int rows, int cols, const clipmi_scaler_state* state, clipmi_stream_t stream) {
  return launch_grad_scale_rows("grad_scale_rows", x, rows, cols, state, (hipStream_t)stream);
}

size_t clipmi_ctx_step_scaled_workspace_bytes(int C, int D, int n_ctx, int per_class) {
  if (C < 1 || D < 1 || n_ctx < 1) return 0;
  const int64_t total = (int64_t)n_ctx * D * (per_class ? C : 1);
  if (total >= (1ll << 31) * THREADS) return 0;
  return scaled_step_bytes(total);
}

int clipmi_ctx_step_scaled(const float* d_embed, float* ctx, float* buf, float* grad_out, int C, int L, int D, int n_ctx, int per_class,
                           clipmi_scaler_state* state, float growth_factor, float backoff_factor, int growth_interval, const float* lr, float momentum,
                           float dampening, float weight_decay, int nesterov, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  const ScalerCall sc{state, growth_factor, backoff_factor, growth_interval};
  int64_t total;
  if (int rc = check_ctx_step_scaled("ctx_step_scaled", d_embed, ctx, buf, lr, C, L, D, n_ctx, per_class, sc, momentum, dampening, weight_decay, nesterov,
                                     workspace, workspace_bytes, &total))
    return rc;
  return launch_ctx_step_scaled(d_embed, ctx, buf, grad_out, C, L, D, n_ctx, per_class, total, sc, lr, momentum, dampening, weight_decay, nesterov, workspace,
                                (hipStream_t)stream);
}

size_t clipmi_block_step_scaled_workspace_bytes(int64_t total) { return block_step_scaled_bytes(total); }

int clipmi_block_step_scaled(const float* grad, float* params, float* buf, float* grad_out, int64_t total, clipmi_scaler_state* state, float growth_factor,
                             float backoff_factor, int growth_interval, const float* lr, float momentum, float dampening, float weight_decay, int nesterov,
                             void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  const ScalerCall sc{state, growth_factor, backoff_factor, growth_interval};
  if (int rc = check_block_step_scaled("block_step_scaled", grad, params, buf, grad_out, lr, total, sc, momentum, dampening, weight_decay, nesterov, workspace,
                                       workspace_bytes))
    return rc;
  return launch_block_step_scaled(grad, params, buf, grad_out, total, sc, lr, momentum, dampening, weight_decay, nesterov, workspace, (hipStream_t)stream);
}

size_t clipmi_prompt_train_step_scaled_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int mode, int n_ctx, int ctx_per_class) {
  if (mode != MODE_COOP && mode != MODE_KGCOOP) return 0;
  const size_t base = clipmi_prompt_train_step_bytes(m, n_prompts, seq_rows, B, mode, n_ctx, ctx_per_class);
  const size_t step = m ? clipmi_ctx_step_scaled_workspace_bytes(n_prompts, m->g.text_width, n_ctx, ctx_per_class) : 0;
  return base && step ? base + step : 0;
}

// workspace: clipmi_prompt_train_step's of the same mode | clipmi_ctx_step_scaled's
int clipmi_prompt_train_step_scaled(clipmi_model* m, const clipmi_text_dgrad* wt, const void* prompts, int dtype, float* ctx, float* buf, int n_ctx,
                                    int ctx_per_class, const int32_t* eot, int n_prompts, int seq_rows, const float* feats, int64_t ld,
                                    const int64_t* labels, int B, float scale, clipmi_scaler_state* state, float growth_factor, float backoff_factor,
                                    int growth_interval, int mode, const float* teacher, float w, const float* lr, float momentum, float dampening,
                                    float weight_decay, int nesterov, float* losses, float* grad_out, void* workspace, size_t workspace_bytes, void* stash,
                                    size_t stash_bytes, clipmi_stream_t stream) {
  const ScalerCall sc{state, growth_factor, backoff_factor, growth_interval};
  return prompt_train_step("prompt_train_step_scaled", true, clipmi_prompt_train_step_scaled_bytes(m, n_prompts, seq_rows, B, mode, n_ctx, ctx_per_class), &sc,
                           nullptr, m, wt, prompts, dtype, ctx, buf, n_ctx, ctx_per_class, eot, n_prompts, seq_rows, feats, ld, labels, B, scale, 1.f, mode, teacher,
                           w, 1.f, 0.f, lr, 0, momentum, dampening, weight_decay, nesterov, losses, grad_out, nullptr, nullptr, workspace, workspace_bytes, stash,
                           stash_bytes, (hipStream_t)stream);
}

}  // extern "C"
