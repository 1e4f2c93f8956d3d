// MaPLe's multi-modal prompts trained on the device (reference trainers/classification/maple.py:77-216; clip/model.py:259-331): the
// coupling functions that make the image tower's prompt rows from the text-side prompts, their backward inside torch.optim.SGD's step over
// one fp32 master block, and the one-call step that puts both frozen towers' training forwards and backwards (text_backward.hip with deep
// prompts, vision_backward.hip) and the joint head (prompt_train.hip) between them.  DESIGN.md "MaPLe fit" has the data flow.
//
// The master block, fp32, d = the prompt depth:
//   [ ctx [n_ctx, Dt] | compound_prompts_text [d - 1, n_ctx, Dt] | proj.weight [Dv, Dt] | proj.bias [Dv] |
//     compound_prompt_projections.weight [d - 1, Dv, Dt] | compound_prompt_projections.bias [d - 1, Dv] ]
// so the text-side prompts are one [d, n_ctx, Dt] array t at its front, and Linear i (0: proj) maps t[i] to the image tower's slot i.
//   maple_couple_kernel       vis[i] = t[i] W_i^T + b_i, slot 0 on operands rounded through fp16 (proj is a half Linear)
//   maple_text_grad_kernel    the gradient of t: the text tower's (d_embed rows 1 .. n_ctx summed over the classes, d_deep) plus d_vis[i] W_i;
//                             keeps it and a copy of t, so that the step below multiplies what the forward multiplied
//   maple_step_kernel         every element of the block: its gradient (dW and db formed here, never written to memory unless asked),
//                             1 / grad_scale and the SGD rule
// No float atomics and no workgroup waits for another: the same inputs give the same bits.
#include <cmath>

#include "common.h"
#include "model.h"
#include "train_rules.h"

namespace clipmi {
namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

struct MapleShape {
  int n_ctx, d, Dt, Dv;
  __host__ __device__ int64_t text() const { return (int64_t)d * n_ctx * Dt; }                       // floats of t
  __host__ __device__ int64_t w(int i) const { return text() + (i == 0 ? 0 : (int64_t)Dv * Dt + Dv + (int64_t)(i - 1) * Dv * Dt); }
  __host__ __device__ int64_t b(int i) const {
    return text() + (int64_t)Dv * Dt + (i == 0 ? 0 : Dv + (int64_t)(d - 1) * Dv * Dt + (int64_t)(i - 1) * Dv);
  }
  __host__ __device__ int64_t total() const { return text() + (int64_t)d * Dv * Dt + (int64_t)d * Dv; }
};

// what Linear 0 multiplies: proj runs in fp16 (maple.py:111-112), the other Linears in fp32
__device__ __forceinline__ float through_half(float v) { return (float)(half_t)v; }
__device__ __forceinline__ float operand(float v, int i) { return i == 0 ? through_half(v) : v; }

// one wave per (i, v): lane-strided fmaf chains over k ascending and the wave tree, one output per context row j
__global__ __launch_bounds__(THREADS) void maple_couple_kernel(const float* __restrict__ block, MapleShape sh, float* __restrict__ vis) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (item >= (int64_t)sh.d * sh.Dv) return;   // no barrier below
  const int i = (int)(item / sh.Dv), v = (int)(item % sh.Dv);
  const float* w = block + sh.w(i) + (int64_t)v * sh.Dt;
  const float bias = operand(block[sh.b(i) + v], i);
  for (int j = 0; j < sh.n_ctx; ++j) {
    const float* t = block + ((int64_t)i * sh.n_ctx + j) * sh.Dt;
    float s = 0.f;
    for (int k = lane; k < sh.Dt; k += 64) s = fmaf(operand(t[k], i), operand(w[k], i), s);
    s = wave_sum(s);
    if (lane == 0) vis[((int64_t)i * sh.n_ctx + j) * sh.Dv + v] = s + bias;
  }
}

// one thread per element (i, j, k) of t: g = text tower's gradient + sum_v d_vis[i, j, v] W_i[v, k] (v ascending), still times grad_scale
__global__ __launch_bounds__(THREADS) void maple_text_grad_kernel(const float* __restrict__ block, MapleShape sh, const float* __restrict__ d_embed,
                                                                  const float* __restrict__ d_deep, const float* __restrict__ d_vis, int C, int L,
                                                                  float* __restrict__ d_t, float* __restrict__ t_keep) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= sh.text()) return;
  const int k = (int)(idx % sh.Dt), j = (int)((idx / sh.Dt) % sh.n_ctx), i = (int)(idx / ((int64_t)sh.Dt * sh.n_ctx));
  float g = 0.f;
  if (i == 0) {
    for (int64_t c = 0; c < C; ++c) g += d_embed[(c * L + 1 + j) * sh.Dt + k];   // as ctx_step_kernel sums
  } else {
    g = d_deep[idx - (int64_t)sh.n_ctx * sh.Dt];
  }
  const float* w = block + sh.w(i) + k;
  const float* dv = d_vis + ((int64_t)i * sh.n_ctx + j) * sh.Dv;
  float s = 0.f;
  for (int v = 0; v < sh.Dv; ++v) s = fmaf(dv[v], operand(w[(int64_t)v * sh.Dt], i), s);
  d_t[idx] = g + s;
  t_keep[idx] = block[idx];
}

// one thread per element of the block
__global__ __launch_bounds__(THREADS) void maple_step_kernel(float* __restrict__ block, float* __restrict__ buf, float* __restrict__ grad_out, MapleShape sh,
                                                             const float* __restrict__ d_vis, const float* __restrict__ d_t,
                                                             const float* __restrict__ t_keep, int apply, float inv_scale, const float* __restrict__ lr,
                                                             SgdArgs sgd) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= sh.total()) return;
  const int64_t nt = sh.text(), nw = (int64_t)sh.Dv * sh.Dt;
  float g;
  if (idx < nt) {
    g = d_t[idx];
  } else {
    int64_t r = idx - nt;
    int i = 0, v = 0, k = -1;   // k < 0: a bias element
    if (r < nw) { i = 0; v = (int)(r / sh.Dt); k = (int)(r % sh.Dt); }
    else if ((r -= nw) < sh.Dv) { i = 0; v = (int)r; }
    else if ((r -= sh.Dv) < (int64_t)(sh.d - 1) * nw) { i = 1 + (int)(r / nw); v = (int)((r % nw) / sh.Dt); k = (int)(r % sh.Dt); }
    else { r -= (int64_t)(sh.d - 1) * nw; i = 1 + (int)(r / sh.Dv); v = (int)(r % sh.Dv); }
    g = 0.f;
    for (int j = 0; j < sh.n_ctx; ++j) {   // dW_i[v, k] = sum_j d_vis[i, j, v] t_i[j, k];  db_i[v] = sum_j d_vis[i, j, v]
      const float dv = d_vis[((int64_t)i * sh.n_ctx + j) * sh.Dv + v];
      g = k < 0 ? g + dv : fmaf(dv, operand(t_keep[((int64_t)i * sh.n_ctx + j) * sh.Dt + k], i), g);
    }
  }
  g *= inv_scale;
  if (grad_out) grad_out[idx] = g;
  if (apply) sgd_element_fma(block, buf, idx, g, *lr, sgd);
}

int check_shape(const char* who, int n_ctx, int depth, int Dt, int Dv) {
  CLIPMI_REQUIRE(n_ctx >= 1 && depth >= 1 && Dt >= 1 && Dv >= 1, CLIPMI_ERR_SHAPE, "%s: n_ctx=%d depth=%d Dt=%d Dv=%d", who, n_ctx, depth, Dt, Dv);
  const MapleShape sh{n_ctx, depth, Dt, Dv};
  CLIPMI_REQUIRE(sh.total() < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: block too large", who);
  return CLIPMI_OK;
}

int launch_couple(const char* who, const float* block, int n_ctx, int depth, int Dt, int Dv, float* vis, hipStream_t s) {
  if (int rc = check_shape(who, n_ctx, depth, Dt, Dv)) return rc;
  CLIPMI_REQUIRE(block && vis, CLIPMI_ERR_ARG, "%s: null pointer", who);
  const MapleShape sh{n_ctx, depth, Dt, Dv};
  hipLaunchKernelGGL(maple_couple_kernel, dim3((unsigned)(((int64_t)depth * Dv + WAVES - 1) / WAVES)), dim3(THREADS), 0, s, block, sh, vis);
  return check_launch("maple_couple_kernel");
}

inline size_t step_bytes(int n_ctx, int depth, int Dt) { return 2 * align256((size_t)depth * n_ctx * Dt * 4); }

int launch_step(const char* who, const float* d_embed, const float* d_deep, const float* d_vis, float* block, float* buf, float* grad_out, int apply, int C,
                int L, int n_ctx, int depth, int Dt, int Dv, float grad_scale, const float* lr, int first_step, float momentum, float dampening,
                float weight_decay, int nesterov, void* workspace, size_t workspace_bytes, hipStream_t s) {
  if (int rc = check_shape(who, n_ctx, depth, Dt, Dv)) return rc;
  CLIPMI_REQUIRE(C >= 1 && 1 + n_ctx <= L, CLIPMI_ERR_SHAPE, "%s: C=%d L=%d n_ctx=%d", who, C, L, n_ctx);
  CLIPMI_REQUIRE(d_embed && d_vis && block && workspace && (depth == 1 || d_deep), CLIPMI_ERR_ARG, "%s: null pointer", who);
  if (int rc = check_step_args(who, block, buf, grad_out, apply, lr, grad_scale, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 256-byte aligned", who);
  CLIPMI_REQUIRE(workspace_bytes >= step_bytes(n_ctx, depth, Dt), CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
                 step_bytes(n_ctx, depth, Dt));
  const MapleShape sh{n_ctx, depth, Dt, Dv};
  Carver c(workspace);
  float* d_t = c.take<float>((size_t)sh.text() * 4);
  float* t_keep = c.take<float>((size_t)sh.text() * 4);
  hipLaunchKernelGGL(maple_text_grad_kernel, dim3((unsigned)((sh.text() + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, (const float*)block, sh, d_embed, d_deep,
                     d_vis, C, L, d_t, t_keep);
  if (int rc = check_launch("maple_text_grad_kernel")) return rc;
  hipLaunchKernelGGL(maple_step_kernel, dim3((unsigned)((sh.total() + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, block, buf, grad_out, sh, d_vis,
                     (const float*)d_t, (const float*)t_keep, apply ? 1 : 0, 1.f / grad_scale, lr,
                     make_sgd_args(momentum, dampening, weight_decay, nesterov, first_step));
  return check_launch("maple_step_kernel");
}

// the one-call step's workspace: the text tower's | the image tower's | the buffers between the calls.  vis and d_vis have room for every
// layer of the image tower, whatever the depth.  Carving and sizing go through this one function.
struct StepWs {
  size_t tws, vws, head_bytes, step_bytes, bytes;
  char* vision;
  float *text, *d_text, *feats, *d_feats, *d_embed, *d_deep, *vis, *d_vis;
  void *head, *step;
};
int carve_step(const clipmi_model* m, void* p, int C, int seq_rows, int B, int n_ctx, int depth, StepWs* w) {
  if (int rc = clipmi_text_train_bytes(m, C, seq_rows, &w->tws, nullptr)) return rc;
  if (int rc = clipmi_vision_train_bytes(m, B, n_ctx, &w->vws, nullptr)) return rc;
  const int E = m->g.embed_dim, Dt = m->g.text_width, Dv = m->g.vision_width;
  w->vision = p ? static_cast<char*>(p) + w->tws : nullptr;
  Carver c(w->vision);
  c.off = w->vws;
  w->text = c.take<float>((size_t)C * E * 4);
  w->d_text = c.take<float>((size_t)C * E * 4);
  w->feats = c.take<float>((size_t)B * E * 4);
  w->d_feats = c.take<float>((size_t)B * E * 4);
  w->d_embed = c.take<float>((size_t)C * live_rows(m, seq_rows) * Dt * 4);
  w->d_deep = c.take<float>((size_t)depth * n_ctx * Dt * 4);
  w->vis = c.take<float>((size_t)m->g.vision_layers * n_ctx * Dv * 4);
  w->d_vis = c.take<float>((size_t)m->g.vision_layers * n_ctx * Dv * 4);
  w->head_bytes = clipmi_maple_head_workspace_bytes(B, E, C);
  w->head = c.take<char>(w->head_bytes);
  w->step_bytes = step_bytes(n_ctx, depth, Dt);
  w->step = c.take<char>(w->step_bytes);
  w->bytes = w->tws + c.off;
  return CLIPMI_OK;
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

size_t clipmi_maple_block_floats(int n_ctx, int depth, int Dt, int Dv) {
  if (n_ctx < 1 || depth < 1 || Dt < 1 || Dv < 1) return 0;
  return (size_t)MapleShape{n_ctx, depth, Dt, Dv}.total();
}

int clipmi_maple_couple(const float* block, int n_ctx, int depth, int Dt, int Dv, float* vis, clipmi_stream_t stream) {
  return launch_couple("maple_couple", block, n_ctx, depth, Dt, Dv, vis, (hipStream_t)stream);
}

size_t clipmi_maple_step_workspace_bytes(int n_ctx, int depth, int Dt) {
  if (n_ctx < 1 || depth < 1 || Dt < 1) return 0;
  return step_bytes(n_ctx, depth, Dt);
}

int clipmi_maple_step(const float* d_embed, const float* d_deep, const float* d_vis, float* block, float* buf, float* grad_out, int apply, int C, int L,
                      int n_ctx, int depth, int Dt, int Dv, float grad_scale, const float* lr, int first_step, float momentum, float dampening,
                      float weight_decay, int nesterov, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  return launch_step("maple_step", d_embed, d_deep, d_vis, block, buf, grad_out, apply, C, L, n_ctx, depth, Dt, Dv, grad_scale, lr, first_step, momentum,
                     dampening, weight_decay, nesterov, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t clipmi_maple_train_step_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int n_ctx, int depth) {
  StepWs w;
  if (!m || n_prompts < 2 || B < 1 || n_ctx < 1 || depth < 1 || carve_step(m, nullptr, n_prompts, seq_rows, B, n_ctx, depth, &w) != CLIPMI_OK) return 0;
  return w.bytes;
}

// the static call's workspace | the block of scale * gradient that clipmi_maple_step leaves with apply = 0 | clipmi_block_step_scaled's
size_t clipmi_maple_train_step_scaled_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int n_ctx, int depth) {
  const size_t base = clipmi_maple_train_step_bytes(m, n_prompts, seq_rows, B, n_ctx, depth);
  if (!base) return 0;
  const int64_t total = MapleShape{n_ctx, depth, m->g.text_width, m->g.vision_width}.total();
  const size_t step = block_step_scaled_bytes(total);
  return step ? base + align256((size_t)total * 4) + step : 0;
}

}  // extern "C"

// MaPLe's one-call step, static (sc == NULL) or under the dynamic loss scale (sc: the head at grad_scale = 1, d_text and d_feats times the block's
// scale, both backwards, the step's two launches at grad_scale = 1 without applying, and the block step on the gradient they leave)
static int maple_train_step(const char* who, const ScalerCall* sc, size_t need, clipmi_model* m, const clipmi_text_dgrad* wt, const clipmi_vision_dgrad* wv,
                            const void* prompts, int dtype, const int32_t* eot, int n_prompts, int seq_rows, const void* image, int image_dtype, int B,
                            const int64_t* labels, float* block, float* buf, int n_ctx, int depth, float scale, float grad_scale, const float* lr,
                            int first_step, float momentum, float dampening, float weight_decay, int nesterov, float* loss, float* grad_out, void* workspace,
                            size_t workspace_bytes, void* text_stash, size_t text_stash_bytes, void* vision_stash, size_t vision_stash_bytes, hipStream_t s) {
  const int C = n_prompts;
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "%s: null model", who);
  CLIPMI_REQUIRE(C >= 2 && B >= 1, CLIPMI_ERR_SHAPE, "%s: n_prompts=%d (>= 2), B=%d (>= 1)", who, C, B);
  CLIPMI_REQUIRE(block && lr && labels && image, CLIPMI_ERR_ARG, "%s: null pointer", who);
  const int E = m->g.embed_dim, Dt = m->g.text_width, Dv = m->g.vision_width, L = live_rows(m, seq_rows);
  if (int rc = check_shape(who, n_ctx, depth, Dt, Dv)) return rc;
  StepWs w;
  if (int rc = carve_step(m, workspace, C, seq_rows, B, n_ctx, depth, &w)) return rc;
  CLIPMI_REQUIRE(need > 0 && workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  if (int rc = check_train_call(who, m, C, workspace, w.tws, text_stash, text_stash_bytes, seq_rows)) return rc;
  if (int rc = check_deep(who, m, n_ctx, depth - 1, block, seq_rows)) return rc;
  if (int rc = check_train_inputs(who, m, prompts, dtype, block, n_ctx, eot, seq_rows, nullptr, 0)) return rc;
  if (int rc = check_dgrad(who, m, wt)) return rc;
  CLIPMI_REQUIRE(L <= AB_MAX_L, CLIPMI_ERR_SHAPE, "%s: %d token rows per prompt (at most %d)", who, L, AB_MAX_L);
  if (int rc = check_vision_train_call(who, m, B, n_ctx, depth, w.vision, w.vws, vision_stash, vision_stash_bytes)) return rc;
  if (int rc = check_vision_dgrad(who, m, wv)) return rc;
  CLIPMI_REQUIRE(image_dtype == CLIPMI_F16 || image_dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "%s: image dtype %d", who, image_dtype);
  CLIPMI_REQUIRE(std::isfinite(scale), CLIPMI_ERR_ARG, "%s: scale=%g (finite)", who, scale);
  if (!sc)
    if (int rc = check_step_args(who, block, buf, grad_out, 1, lr, grad_scale, momentum, dampening, weight_decay, nesterov)) return rc;
  const int64_t total = MapleShape{n_ctx, depth, Dt, Dv}.total();
  const size_t scaled_bytes = sc ? block_step_scaled_bytes(total) : 0;
  Carver behind(workspace ? static_cast<char*>(workspace) + w.bytes : nullptr);
  float* scaled_grad = behind.take<float>(sc ? (size_t)total * 4 : 0);
  void* scaled_ws = behind.take<char>(scaled_bytes);
  if (sc)   // the scaler's and the optimiser's refusals come ahead of the first launch
    if (int rc = check_block_step_scaled(who, scaled_grad, block, buf, grad_out, lr, total, *sc, momentum,
                                         dampening, weight_decay, nesterov, scaled_ws, scaled_bytes))
      return rc;
  const float* deep = block + (int64_t)n_ctx * Dt;
  if (int rc = launch_couple(who, block, n_ctx, depth, Dt, Dv, w.vis, s)) return rc;
  if (int rc = run_train_forward(m, prompts, dtype, block, n_ctx, 0, eot, C, seq_rows, w.text, workspace, text_stash, s, deep, depth - 1)) return rc;
  if (int rc = run_vision_train_forward(m, image, image_dtype, B, w.vis, n_ctx, depth, w.feats, w.vision, vision_stash, s)) return rc;
  if (int rc = launch_maple_head(who, w.feats, E, labels, w.text, B, E, C, scale, grad_scale, loss, w.d_feats, w.d_text, nullptr, w.head, w.head_bytes, s))
    return rc;
  if (sc) {
    if (int rc = launch_grad_scale_rows(who, w.d_text, C, E, sc->state, s)) return rc;
    if (int rc = launch_grad_scale_rows(who, w.d_feats, B, E, sc->state, s)) return rc;
  }
  if (int rc = run_backward(m, wt, w.d_text, C, seq_rows, w.d_embed, workspace, text_stash, nullptr, s, n_ctx, depth - 1, w.d_deep)) return rc;
  if (int rc = run_vision_backward(m, wv, w.d_feats, B, n_ctx, depth, w.d_vis, w.vision, vision_stash, nullptr, s)) return rc;
  if (sc) {
    if (int rc = launch_step(who, w.d_embed, w.d_deep, w.d_vis, block, nullptr, scaled_grad, 0, C, L, n_ctx, depth, Dt, Dv, 1.f, nullptr, 0, momentum, dampening,
                             weight_decay, nesterov, w.step, w.step_bytes, s))
      return rc;
    return launch_block_step_scaled(scaled_grad, block, buf, grad_out, total, *sc, lr, momentum, dampening,
                                    weight_decay, nesterov, scaled_ws, s);
  }
  return launch_step(who, w.d_embed, w.d_deep, w.d_vis, block, buf, grad_out, 1, C, L, n_ctx, depth, Dt, Dv, grad_scale, lr, first_step, momentum, dampening,
                     weight_decay, nesterov, w.step, w.step_bytes, s);
}

extern "C" {

int clipmi_maple_train_step(clipmi_model* m, const clipmi_text_dgrad* wt, const clipmi_vision_dgrad* wv, const void* prompts, int dtype, const int32_t* eot,
                            int n_prompts, int seq_rows, const void* image, int image_dtype, int B, const int64_t* labels, float* block, float* buf,
                            int n_ctx, int depth, float scale, float grad_scale, const float* lr, int first_step, float momentum, float dampening,
                            float weight_decay, int nesterov, float* loss, float* grad_out, void* workspace, size_t workspace_bytes, void* text_stash,
                            size_t text_stash_bytes, void* vision_stash, size_t vision_stash_bytes, clipmi_stream_t stream) {
  return maple_train_step("maple_train_step", nullptr, clipmi_maple_train_step_bytes(m, n_prompts, seq_rows, B, n_ctx, depth), m, wt, wv, prompts, dtype, eot,
                          n_prompts, seq_rows, image, image_dtype, B, labels, block, buf, n_ctx, depth, scale, grad_scale, lr, first_step, momentum, dampening,
                          weight_decay, nesterov, loss, grad_out, workspace, workspace_bytes, text_stash, text_stash_bytes, vision_stash, vision_stash_bytes,
                          (hipStream_t)stream);
}

int clipmi_maple_train_step_scaled(clipmi_model* m, const clipmi_text_dgrad* wt, const clipmi_vision_dgrad* wv, const void* prompts, int dtype,
                                   const int32_t* eot, int n_prompts, int seq_rows, const void* image, int image_dtype, int B, const int64_t* labels,
                                   float* block, float* buf, int n_ctx, int depth, float scale, clipmi_scaler_state* state, float growth_factor,
                                   float backoff_factor, int growth_interval, const float* lr, float momentum, float dampening, float weight_decay,
                                   int nesterov, float* loss, float* grad_out, void* workspace, size_t workspace_bytes, void* text_stash,
                                   size_t text_stash_bytes, void* vision_stash, size_t vision_stash_bytes, clipmi_stream_t stream) {
  const ScalerCall sc{state, growth_factor, backoff_factor, growth_interval};
  return maple_train_step("maple_train_step_scaled", &sc, clipmi_maple_train_step_scaled_bytes(m, n_prompts, seq_rows, B, n_ctx, depth), m, wt, wv, prompts,
                          dtype, eot, n_prompts, seq_rows, image, image_dtype, B, labels, block, buf, n_ctx, depth, scale, 1.f, lr, 0, momentum, dampening,
                          weight_decay, nesterov, loss, grad_out, workspace, workspace_bytes, text_stash, text_stash_bytes, vision_stash, vision_stash_bytes,
                          (hipStream_t)stream);
}

}  // extern "C"
