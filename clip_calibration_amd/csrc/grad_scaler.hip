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

// everything clipmi_ctx_step_scaled refuses, before anything is launched; *total: the elements of ctx
int check_scaled_step(const char* who, const float* d_embed, const float* ctx, const float* buf, const float* lr, int C, int L, int D, int n_ctx, int per_class,
                      const clipmi_scaler_state* st, float growth, float backoff, int growth_interval, float momentum, float dampening, float weight_decay,
                      int nesterov, const void* workspace, size_t workspace_bytes, int64_t* total) {
  CLIPMI_REQUIRE(d_embed && ctx && lr && workspace, CLIPMI_ERR_ARG, "%s: null pointer (d_embed, ctx, lr and the workspace are required)", who);
  if (int rc = check_scaler(who, st, growth, backoff, growth_interval)) return rc;
  CLIPMI_REQUIRE(C >= 1 && D >= 1 && n_ctx >= 1 && 1 + n_ctx <= L, CLIPMI_ERR_SHAPE, "%s: C=%d L=%d D=%d n_ctx=%d", who, C, L, D, n_ctx);
  if (int rc = check_sgd(who, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE(momentum == 0.f || buf, CLIPMI_ERR_ARG, "%s: null pointer (a momentum needs the buffer)", who);
  *total = (int64_t)n_ctx * D * (per_class ? C : 1);
  CLIPMI_REQUIRE(*total < (1ll << 31) * THREADS, CLIPMI_ERR_SHAPE, "%s: context too large", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 256-byte aligned", who);
  CLIPMI_REQUIRE(workspace_bytes >= scaled_step_bytes(*total), CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
                 scaled_step_bytes(*total));
  return CLIPMI_OK;
}

// the three launches; every argument has been checked
int launch_scaled_step(const float* d_embed, float* ctx, float* buf, float* grad_out, int C, int L, int D, int n_ctx, int per_class, int64_t total,
                       clipmi_scaler_state* st, float growth, float backoff, int growth_interval, const float* lr, float momentum, float dampening,
                       float weight_decay, int nesterov, void* workspace, hipStream_t s) {
  const ScaledWs w = scaled_carve(workspace, total);
  const int64_t blocks = scaled_grad_blocks(total);
  hipLaunchKernelGGL(scaled_grad_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, s, d_embed, grad_out, C, L, D, n_ctx, per_class ? 1 : 0, total,
                     (const clipmi_scaler_state*)st, w);
  if (int rc = check_launch("scaled_grad_kernel")) return rc;
  return launch_scaled_decide_apply(w, total, ctx, buf, st, growth, backoff, growth_interval, lr, momentum, dampening, weight_decay, nesterov, s);
}

}  // namespace

// ---- what every scaled step shares (model.h)
int check_scaler(const char* who, const clipmi_scaler_state* st, float growth, float backoff, int growth_interval) {
  CLIPMI_REQUIRE(st, CLIPMI_ERR_ARG, "%s: null pointer (the scaler's state block)", who);
  CLIPMI_REQUIRE((uintptr_t)st % 4 == 0, CLIPMI_ERR_ARG, "%s: the scaler's state block must be 4-byte aligned", who);
  CLIPMI_REQUIRE(std::isfinite(growth) && growth > 0.f && std::isfinite(backoff) && backoff > 0.f, CLIPMI_ERR_ARG,
                 "%s: growth_factor=%g, backoff_factor=%g (both finite, > 0)", who, growth, backoff);
  CLIPMI_REQUIRE(growth_interval >= 1, CLIPMI_ERR_ARG, "%s: growth_interval=%d (>= 1)", who, growth_interval);
  return CLIPMI_OK;
}

// the decision launch and the step launch behind a first launch that has filled w.grad and w.flags; every argument has been checked
int launch_scaled_decide_apply(const ScaledWs& w, int64_t total, float* params, float* buf, clipmi_scaler_state* st, float growth, float backoff,
                               int growth_interval, const float* lr, float momentum, float dampening, float weight_decay, int nesterov, hipStream_t s) {
  const int64_t blocks = scaled_grad_blocks(total);
  hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(THREADS), 0, s, w, blocks, st, growth, backoff, growth_interval);
  if (int rc = check_launch("scaler_update_kernel")) return rc;
  hipLaunchKernelGGL(scaled_apply_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, s, w, params, buf, total, lr,
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

size_t block_step_scaled_bytes(int64_t total) { return total >= 1 && total < (1ll << 31) * THREADS ? scaled_step_bytes(total) : 0; }

// everything clipmi_block_step_scaled refuses, before anything is launched
int check_block_step_scaled(const char* who, const float* grad, const float* params, const float* buf, const float* grad_out, const float* lr, int64_t total,
                            const clipmi_scaler_state* st, float growth, float backoff, int growth_interval, float momentum, float dampening,
                            float weight_decay, int nesterov, const void* workspace, size_t workspace_bytes) {
  CLIPMI_REQUIRE(grad && params && lr && workspace, CLIPMI_ERR_ARG, "%s: null pointer (grad, params, lr and the workspace are required)", who);
  CLIPMI_REQUIRE(((uintptr_t)grad | (uintptr_t)params | (uintptr_t)buf | (uintptr_t)grad_out | (uintptr_t)lr) % 4 == 0, CLIPMI_ERR_ARG,
                 "%s: grad, params, buf, grad_out and lr must be 4-byte aligned", who);
  if (int rc = check_scaler(who, st, growth, backoff, growth_interval)) return rc;
  CLIPMI_REQUIRE(total >= 1, CLIPMI_ERR_SHAPE, "%s: total=%lld (>= 1)", who, (long long)total);
  if (int rc = check_sgd(who, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE(momentum == 0.f || buf, CLIPMI_ERR_ARG, "%s: null pointer (a momentum needs the buffer)", who);
  CLIPMI_REQUIRE(total < (1ll << 31) * THREADS, CLIPMI_ERR_SHAPE, "%s: block too large", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 256-byte aligned", who);
  CLIPMI_REQUIRE(workspace_bytes >= scaled_step_bytes(total), CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
                 scaled_step_bytes(total));
  return CLIPMI_OK;
}

// the three launches; every argument has been checked
int launch_block_step_scaled(const float* grad, float* params, float* buf, float* grad_out, int64_t total, clipmi_scaler_state* st, float growth, float backoff,
                             int growth_interval, const float* lr, float momentum, float dampening, float weight_decay, int nesterov, void* workspace,
                             hipStream_t s) {
  const ScaledWs w = scaled_carve(workspace, total);
  const int64_t blocks = scaled_grad_blocks(total);
  hipLaunchKernelGGL(block_unscale_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, s, grad, grad_out, total, (const clipmi_scaler_state*)st, w);
  if (int rc = check_launch("block_unscale_kernel")) return rc;
  return launch_scaled_decide_apply(w, total, params, buf, st, growth, backoff, growth_interval, lr, momentum, dampening, weight_decay, nesterov, s);
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
  int64_t total;
  if (int rc = check_scaled_step("ctx_step_scaled", d_embed, ctx, buf, lr, C, L, D, n_ctx, per_class, state, growth_factor, backoff_factor, growth_interval,
                                 momentum, dampening, weight_decay, nesterov, workspace, workspace_bytes, &total))
    return rc;
  return launch_scaled_step(d_embed, ctx, buf, grad_out, C, L, D, n_ctx, per_class, total, state, growth_factor, backoff_factor, growth_interval, lr, momentum,
                            dampening, weight_decay, nesterov, workspace, (hipStream_t)stream);
}

size_t clipmi_block_step_scaled_workspace_bytes(int64_t total) { return block_step_scaled_bytes(total); }

int clipmi_block_step_scaled(const float* grad, float* params, float* buf, float* grad_out, int64_t total, clipmi_scaler_state* state, float growth_factor,
                             float backoff_factor, int growth_interval, const float* lr, float momentum, float dampening, float weight_decay, int nesterov,
                             void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  if (int rc = check_block_step_scaled("block_step_scaled", grad, params, buf, grad_out, lr, total, state, growth_factor, backoff_factor, growth_interval,
                                       momentum, dampening, weight_decay, nesterov, workspace, workspace_bytes))
    return rc;
  return launch_block_step_scaled(grad, params, buf, grad_out, total, state, growth_factor, backoff_factor, growth_interval, lr, momentum, dampening,
                                  weight_decay, nesterov, workspace, (hipStream_t)stream);
}

size_t clipmi_prompt_train_step_scaled_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int mode, int n_ctx, int ctx_per_class) {
  if (mode != MODE_COOP && mode != MODE_KGCOOP) return 0;
  const size_t base = clipmi_prompt_train_step_bytes(m, n_prompts, seq_rows, B, mode, n_ctx, ctx_per_class);
  const size_t step = m ? clipmi_ctx_step_scaled_workspace_bytes(n_prompts, m->g.text_width, n_ctx, ctx_per_class) : 0;
  return base && step ? base + step : 0;
}

// workspace: clipmi_prompt_train_step's of the same mode (the tower's workspace | text features | their gradient | d_embed | the head's
// workspace) | clipmi_ctx_step_scaled's
int clipmi_prompt_train_step_scaled(clipmi_model* m, const clipmi_text_dgrad* wt, const void* prompts, int dtype, float* ctx, float* buf, int n_ctx,
                                    int ctx_per_class, const int32_t* eot, int n_prompts, int seq_rows, const float* feats, int64_t ld,
                                    const int64_t* labels, int B, float scale, clipmi_scaler_state* state, float growth_factor, float backoff_factor,
                                    int growth_interval, int mode, const float* teacher, float w, const float* lr, float momentum, float dampening,
                                    float weight_decay, int nesterov, float* losses, float* grad_out, void* workspace, size_t workspace_bytes, void* stash,
                                    size_t stash_bytes, clipmi_stream_t stream) {
  const char* who = "prompt_train_step_scaled";
  const int C = n_prompts;
  hipStream_t s = (hipStream_t)stream;
  CLIPMI_REQUIRE(mode != MODE_PROGRAD, CLIPMI_ERR_ARG, "%s: ProGrad's mode has no dynamic loss scale (its two gradients share one step)", who);
  CLIPMI_REQUIRE(mode == MODE_COOP || mode == MODE_KGCOOP, CLIPMI_ERR_ARG, "%s: bad mode %d", who, mode);
  if (int rc = check_scaler(who, state, growth_factor, backoff_factor, growth_interval)) return rc;
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "%s: null model", who);
  CLIPMI_REQUIRE(C >= 2 && B >= 1, CLIPMI_ERR_SHAPE, "%s: n_prompts=%d (>= 2), B=%d (>= 1)", who, C, B);
  CLIPMI_REQUIRE(feats && labels && losses, CLIPMI_ERR_ARG, "%s: null pointer (feats, labels and losses are required)", who);
  CLIPMI_REQUIRE(mode == MODE_COOP || teacher, CLIPMI_ERR_ARG, "%s: null pointer (KgCoOp needs the teacher)", who);
  CLIPMI_REQUIRE(std::isfinite(scale), CLIPMI_ERR_ARG, "%s: scale=%g (finite)", who, scale);
  CLIPMI_REQUIRE(mode != MODE_KGCOOP || (std::isfinite(w) && w >= 0.f), CLIPMI_ERR_ARG, "%s: w=%g (finite, >= 0)", who, w);
  const size_t need = clipmi_prompt_train_step_scaled_bytes(m, C, seq_rows, B, mode, n_ctx, ctx_per_class);
  CLIPMI_REQUIRE(need > 0 && workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  size_t tower = 0;
  clipmi_text_train_bytes(m, C, seq_rows, &tower, nullptr);
  if (int rc = check_train_call(who, m, C, workspace, tower, stash, stash_bytes, seq_rows)) return rc;
  if (int rc = check_train_inputs(who, m, prompts, dtype, ctx, n_ctx, eot, seq_rows, nullptr, 0)) return rc;
  if (int rc = check_dgrad(who, m, wt)) return rc;
  const int L = live_rows(m, seq_rows), D = m->g.text_width, E = m->g.embed_dim;
  CLIPMI_REQUIRE(L <= AB_MAX_L, CLIPMI_ERR_SHAPE, "%s: %d token rows per prompt (at most %d)", who, L, AB_MAX_L);
  CLIPMI_REQUIRE(ld >= E && (int64_t)B * C < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: B=%d C=%d E=%d ld=%lld", who, B, C, E, (long long)ld);
  const size_t head_bytes = clipmi_prompt_head_workspace_bytes(B, E, C, mode);
  const size_t step_bytes = clipmi_ctx_step_scaled_workspace_bytes(C, D, n_ctx, ctx_per_class);
  Carver c(static_cast<char*>(workspace) + tower);
  float* text = c.take<float>((size_t)C * E * 4);
  float* d_text = c.take<float>((size_t)C * E * 4);
  float* d_embed = c.take<float>((size_t)C * L * D * 4);
  void* head_ws = c.take<char>(head_bytes);
  void* step_ws = c.take<char>(step_bytes);
  int64_t total;
  if (int rc = check_scaled_step(who, d_embed, ctx, buf, lr, C, L, D, n_ctx, ctx_per_class, state, growth_factor, backoff_factor, growth_interval, momentum,
                                 dampening, weight_decay, nesterov, step_ws, step_bytes, &total))
    return rc;
  if (int rc = run_train_forward(m, prompts, dtype, ctx, n_ctx, ctx_per_class, eot, C, seq_rows, text, workspace, stash, s)) return rc;
  if (int rc = clipmi_prompt_head(feats, ld, labels, text, B, E, C, scale, 1.f, mode, teacher, w, 1.f, losses, d_text, nullptr, nullptr, head_ws, head_bytes,
                                  stream))
    return rc;
  if (int rc = launch_grad_scale_rows(who, d_text, C, E, state, s)) return rc;
  if (int rc = run_backward(m, wt, d_text, C, seq_rows, d_embed, workspace, stash, nullptr, s)) return rc;
  return launch_scaled_step(d_embed, ctx, buf, grad_out, C, L, D, n_ctx, ctx_per_class, total, state, growth_factor, backoff_factor, growth_interval, lr,
                            momentum, dampening, weight_decay, nesterov, step_ws, s);
}

}  // extern "C"
