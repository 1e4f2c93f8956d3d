// PromptSRC's and IVLP's independent prompts trained on the device (reference trainers/classification/promptsrc.py:73-317; clip/model.py
// 191-256): torch.optim.SGD's step over one fp32 master block of text and image prompts, the Gaussian-weighted prompt aggregation over the
// epochs, and the one-call step that puts the frozen plain image tower, both prompted towers' training forwards and backwards
// (text_backward.hip with deep prompts, vision_backward.hip) and the four-term head (prompt_train.hip) in front of it.  DESIGN.md
// "PromptSRC fit" has the data flow.
//
// The master block, fp32, dt / dv = the text / image prompt depth:
//   [ ctx [nt, Dt] | transformer.resblocks.{i}.VPT_shallow [dt - 1, nt, Dt] | visual.VPT and visual...resblocks.{i}.VPT_shallow [dv, nv, Dv] ]
// so its text part is the [ctx; deep] pair of clipmi_text_encoder_train_deep and its image part the block of clipmi_vision_encoder_train.
//   promptsrc_step_kernel     every element of the block: its gradient (ctx: d_embed rows 1 .. nt summed over the classes as
//                             ctx_step_kernel sums them; the others: d_deep, d_vis), 1 / grad_scale and the SGD rule
//   gpa_accumulate_kernel     gpa = weight block (the first epoch) or fmaf(weight, block, gpa)
// No float atomics and no workgroup waits for another: the same inputs give the same bits.
#include <cmath>

#include "common.h"
#include "model.h"
#include "train_rules.h"

namespace clipmi {
namespace {

constexpr int THREADS = 256;

struct SrcShape {
  int nt, dt, Dt, nv, dv, Dv;
  __host__ __device__ int64_t ctx() const { return (int64_t)nt * Dt; }
  __host__ __device__ int64_t text() const { return (int64_t)dt * nt * Dt; }
  __host__ __device__ int64_t total() const { return text() + (int64_t)dv * nv * Dv; }
};

// one thread per element of the block
__global__ __launch_bounds__(THREADS) void promptsrc_step_kernel(float* __restrict__ block, float* __restrict__ buf, float* __restrict__ grad_out, SrcShape sh,
                                                                 const float* __restrict__ d_embed, const float* __restrict__ d_deep,
                                                                 const float* __restrict__ d_vis, int C, int L, int apply, float inv_scale,
                                                                 const float* __restrict__ lr, SgdArgs sgd) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= sh.total()) return;
  float g;
  if (idx < sh.ctx()) {
    const int k = (int)(idx % sh.Dt), j = (int)(idx / sh.Dt);
    g = 0.f;
    for (int64_t c = 0; c < C; ++c) g += d_embed[(c * L + 1 + j) * sh.Dt + k];   // as ctx_step_kernel sums
  } else if (idx < sh.text()) {
    g = d_deep[idx - sh.ctx()];
  } else {
    g = d_vis[idx - sh.text()];
  }
  g = g * inv_scale;
  if (grad_out) grad_out[idx] = g;
  if (apply) sgd_element_fma(block, buf, idx, g, *lr, sgd);
}

__global__ __launch_bounds__(THREADS) void gpa_accumulate_kernel(const float* __restrict__ block, float* __restrict__ gpa, int64_t n, float weight, int first) {
#pragma clang fp contract(off)
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= n) return;
  gpa[idx] = first ? weight * block[idx] : fmaf(weight, block[idx], gpa[idx]);
}

int check_shape(const char* who, int nt, int dt, int Dt, int nv, int dv, int Dv) {
  CLIPMI_REQUIRE(nt >= 1 && dt >= 1 && Dt >= 1 && nv >= 1 && dv >= 1 && Dv >= 1, CLIPMI_ERR_SHAPE, "%s: nt=%d dt=%d Dt=%d nv=%d dv=%d Dv=%d", who, nt, dt, Dt, nv,
                 dv, Dv);
  CLIPMI_REQUIRE((SrcShape{nt, dt, Dt, nv, dv, Dv}.total()) < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: block too large", who);
  return CLIPMI_OK;
}

int launch_step(const char* who, const float* d_embed, const float* d_deep, const float* d_vis, float* block, float* buf, float* grad_out, int apply, int C,
                int L, int nt, int dt, int Dt, int nv, int dv, int Dv, float grad_scale, const float* lr, int first_step, float momentum, float dampening,
                float weight_decay, int nesterov, hipStream_t s) {
  if (int rc = check_shape(who, nt, dt, Dt, nv, dv, Dv)) return rc;
  CLIPMI_REQUIRE(C >= 1 && 1 + nt <= L, CLIPMI_ERR_SHAPE, "%s: C=%d L=%d nt=%d", who, C, L, nt);
  CLIPMI_REQUIRE(d_embed && d_vis && (dt == 1 || d_deep), CLIPMI_ERR_ARG, "%s: null pointer", who);
  if (int rc = check_step_args(who, block, buf, grad_out, apply, lr, grad_scale, momentum, dampening, weight_decay, nesterov)) return rc;
  const SrcShape sh{nt, dt, Dt, nv, dv, Dv};
  hipLaunchKernelGGL(promptsrc_step_kernel, dim3((unsigned)((sh.total() + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, block, buf, grad_out, sh, d_embed,
                     d_deep, d_vis, C, L, apply ? 1 : 0, 1.f / grad_scale, lr, make_sgd_args(momentum, dampening, weight_decay, nesterov, first_step));
  return check_launch("promptsrc_step_kernel");
}

// the one-call step's workspace: the text tower's | the image tower's, which the frozen forward uses first | the buffers between the calls.
// The sizing function does not know dv, so d_vis has room for every layer, as clipmi_maple_train_step's has; d_deep keeps that function's
// dt slots where dt - 1 are written.  Both are over-allocations on purpose: carving and sizing go through this one function.
struct StepWs {
  size_t tws, vws, bytes;
  char* vision;
  float *zs, *text, *d_text, *feats, *d_feats, *d_embed, *d_deep, *d_vis;
  void* head;
  size_t head_bytes;
};
int carve_step(const clipmi_model* m, void* p, int C, int seq_rows, int B, int nt, int dt, int nv, StepWs* w) {
  size_t tws = 0, vws = 0;
  if (int rc = clipmi_text_train_bytes(m, C, seq_rows, &tws, nullptr)) return rc;
  if (int rc = clipmi_vision_train_bytes(m, B, nv, &vws, nullptr)) return rc;
  const size_t fws = align256(clipmi_vision_workspace_bytes(m, B, 0));
  const int E = m->g.embed_dim, Dt = m->g.text_width, Dv = m->g.vision_width;
  w->tws = tws;
  w->vws = vws > fws ? vws : fws;
  w->vision = p ? static_cast<char*>(p) + tws : nullptr;
  Carver c(w->vision);
  c.off = w->vws;
  w->zs = c.take<float>((size_t)B * E * 4);
  w->text = c.take<float>((size_t)C * E * 4);
  w->d_text = c.take<float>((size_t)C * E * 4);
  w->feats = c.take<float>((size_t)B * E * 4);
  w->d_feats = c.take<float>((size_t)B * E * 4);
  w->d_embed = c.take<float>((size_t)C * live_rows(m, seq_rows) * Dt * 4);
  w->d_deep = c.take<float>((size_t)dt * nt * Dt * 4);
  w->d_vis = c.take<float>((size_t)m->g.vision_layers * nv * Dv * 4);
  w->head_bytes = promptsrc_head_bytes(B, E, C);
  w->head = c.take<char>(w->head_bytes);
  w->bytes = tws + c.off;
  return CLIPMI_OK;
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

size_t clipmi_promptsrc_head_workspace_bytes(int B, int E, int C) { return promptsrc_head_bytes(B, E, C); }

int clipmi_promptsrc_head(const float* feats, int64_t ld, const float* zs_feats, const float* text, const float* teacher, const int64_t* labels, int B, int E,
                          int C, float scale, float grad_scale, float w_text, float w_image, float w_logit, float* losses, float* d_feats, float* d_text,
                          void* d_text16, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  return launch_promptsrc_head("promptsrc_head", feats, ld, zs_feats, labels, text, teacher, B, E, C, scale, grad_scale, w_text, w_image, w_logit, losses,
                               d_feats, d_text, static_cast<half_t*>(d_text16), workspace, workspace_bytes, (hipStream_t)stream);
}

size_t clipmi_promptsrc_block_floats(int nt, int dt, int Dt, int nv, int dv, int Dv) {
  if (nt < 1 || dt < 1 || Dt < 1 || nv < 1 || dv < 1 || Dv < 1) return 0;
  return (size_t)SrcShape{nt, dt, Dt, nv, dv, Dv}.total();
}

int clipmi_promptsrc_step(const float* d_embed, const float* d_deep, const float* d_vis, float* block, float* buf, float* grad_out, int apply, int C, int L,
                          int nt, int dt, int Dt, int nv, int dv, int Dv, float grad_scale, const float* lr, int first_step, float momentum,
                          float dampening, float weight_decay, int nesterov, clipmi_stream_t stream) {
  return launch_step("promptsrc_step", d_embed, d_deep, d_vis, block, buf, grad_out, apply, C, L, nt, dt, Dt, nv, dv, Dv, grad_scale, lr, first_step, momentum,
                     dampening, weight_decay, nesterov, (hipStream_t)stream);
}

int clipmi_gpa_accumulate(const float* block, float* gpa, int64_t n, float weight, int first, clipmi_stream_t stream) {
  CLIPMI_REQUIRE(block && gpa, CLIPMI_ERR_ARG, "gpa_accumulate: null pointer");
  CLIPMI_REQUIRE(n >= 0 && n < (1ll << 31) * THREADS, CLIPMI_ERR_SHAPE, "gpa_accumulate: n=%lld", (long long)n);
  CLIPMI_REQUIRE(std::isfinite(weight), CLIPMI_ERR_ARG, "gpa_accumulate: weight=%g (finite)", weight);
  if (n == 0) return CLIPMI_OK;
  hipLaunchKernelGGL(gpa_accumulate_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, block, gpa, n, weight,
                     first ? 1 : 0);
  return check_launch("gpa_accumulate_kernel");
}

size_t clipmi_promptsrc_train_step_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int nt, int dt, int nv) {
  StepWs w;
  if (!m || n_prompts < 2 || B < 1 || nt < 1 || dt < 1 || nv < 1 || carve_step(m, nullptr, n_prompts, seq_rows, B, nt, dt, nv, &w) != CLIPMI_OK) return 0;
  return w.bytes;
}

// the static call's workspace | the block of scale * gradient that clipmi_promptsrc_step leaves with apply = 0 | clipmi_block_step_scaled's
size_t clipmi_promptsrc_train_step_scaled_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int nt, int dt, int nv, int dv) {
  const size_t base = clipmi_promptsrc_train_step_bytes(m, n_prompts, seq_rows, B, nt, dt, nv);
  if (!base || dv < 1) return 0;
  const int64_t total = SrcShape{nt, dt, m->g.text_width, nv, dv, m->g.vision_width}.total();
  const size_t step = block_step_scaled_bytes(total);
  return step ? base + align256((size_t)total * 4) + step : 0;
}

}  // extern "C"

// PromptSRC's and IVLP's one-call step, static (sc == NULL) or under the dynamic loss scale (sc: the head at grad_scale = 1, d_text and d_feats
// times the block's scale, both backwards, the step's launch at grad_scale = 1 without applying, and the block step on the gradient it leaves)
static int promptsrc_train_step(const char* who, const ScalerCall* sc, clipmi_model* m, const clipmi_text_dgrad* wt, const clipmi_vision_dgrad* wv,
                                const void* prompts, int dtype, const int32_t* eot, int n_prompts, int seq_rows, const void* image, int image_dtype, int B,
                                const int64_t* labels, const float* teacher, float* block, float* buf, int nt, int dt, int nv, int dv, float scale,
                                float grad_scale, float w_text, float w_image, float w_logit, const float* lr, int first_step, float momentum, float dampening,
                                float weight_decay, int nesterov, float* losses, float* grad_out, void* workspace, size_t workspace_bytes, void* text_stash,
                                size_t text_stash_bytes, void* vision_stash, size_t vision_stash_bytes, clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  const int C = n_prompts;
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "%s: null model", who);
  CLIPMI_REQUIRE(C >= 2 && B >= 1, CLIPMI_ERR_SHAPE, "%s: n_prompts=%d (>= 2), B=%d (>= 1)", who, C, B);
  CLIPMI_REQUIRE(block && lr && labels && image && teacher && losses, CLIPMI_ERR_ARG, "%s: null pointer", who);
  const int E = m->g.embed_dim, Dt = m->g.text_width, Dv = m->g.vision_width, L = live_rows(m, seq_rows);
  if (int rc = check_shape(who, nt, dt, Dt, nv, dv, Dv)) return rc;
  StepWs w;
  if (int rc = carve_step(m, workspace, C, seq_rows, B, nt, dt, nv, &w)) return rc;
  const int64_t total = SrcShape{nt, dt, Dt, nv, dv, Dv}.total();
  const size_t scaled_bytes = sc ? block_step_scaled_bytes(total) : 0;
  Carver behind(workspace ? static_cast<char*>(workspace) + w.bytes : nullptr);
  float* scaled_grad = behind.take<float>(sc ? (size_t)total * 4 : 0);
  void* scaled_ws = behind.take<char>(scaled_bytes);
  const size_t need = w.bytes + behind.off;
  CLIPMI_REQUIRE(workspace && workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  if (int rc = check_train_call(who, m, C, workspace, w.tws, text_stash, text_stash_bytes, seq_rows)) return rc;
  if (int rc = check_deep(who, m, nt, dt - 1, block, seq_rows)) return rc;
  if (int rc = check_train_inputs(who, m, prompts, dtype, block, nt, eot, seq_rows, nullptr, 0)) return rc;
  if (int rc = check_dgrad(who, m, wt)) return rc;
  CLIPMI_REQUIRE(L <= AB_MAX_L, CLIPMI_ERR_SHAPE, "%s: %d token rows per prompt (at most %d)", who, L, AB_MAX_L);
  if (int rc = check_vision_train_call(who, m, B, nv, dv, w.vision, w.vws, vision_stash, vision_stash_bytes)) return rc;
  if (int rc = check_vision_dgrad(who, m, wv)) return rc;
  CLIPMI_REQUIRE(image_dtype == CLIPMI_F16 || image_dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "%s: image dtype %d", who, image_dtype);
  if (sc) {
    if (int rc = check_block_step_scaled(who, scaled_grad, block, buf, grad_out, lr, total, *sc, momentum,
                                         dampening, weight_decay, nesterov, scaled_ws, scaled_bytes))
      return rc;
  } else if (int rc = check_step_args(who, block, buf, grad_out, 1, lr, grad_scale, momentum, dampening, weight_decay, nesterov)) {
    return rc;
  }
  if (int rc = check_promptsrc_head(who, w.feats, E, w.zs, labels, w.text, teacher, B, E, C, scale, grad_scale, w_text, w_image, w_logit, losses, w.d_feats,
                                    w.d_text, w.head, w.head_bytes))
    return rc;
  float* vis = block + SrcShape{nt, dt, Dt, nv, dv, Dv}.text();
  CLIPMI_REQUIRE((uintptr_t)vis % 16 == 0, CLIPMI_ERR_ARG, "%s: the block's image part must be 16-byte aligned", who);
  const float* deep = block + (int64_t)nt * Dt;
  // the frozen plain tower first, in the image tower's workspace: the training forward behind it on the stream overwrites that
  if (int rc = clipmi_encode_image(m, image, image_dtype, B, nullptr, w.zs, w.vision, w.vws, CLIPMI_CALL_STREAM_F32, stream)) return rc;
  if (int rc = run_train_forward(m, prompts, dtype, block, nt, 0, eot, C, seq_rows, w.text, workspace, text_stash, s, deep, dt - 1)) return rc;
  if (int rc = run_vision_train_forward(m, image, image_dtype, B, vis, nv, dv, w.feats, w.vision, vision_stash, s)) return rc;
  if (int rc = launch_promptsrc_head(who, w.feats, E, w.zs, labels, w.text, teacher, B, E, C, scale, grad_scale, w_text, w_image, w_logit, losses, w.d_feats,
                                     w.d_text, nullptr, w.head, w.head_bytes, s))
    return rc;
  if (sc) {
    if (int rc = launch_grad_scale_rows(who, w.d_text, C, E, sc->state, s)) return rc;
    if (int rc = launch_grad_scale_rows(who, w.d_feats, B, E, sc->state, s)) return rc;
  }
  if (int rc = run_backward(m, wt, w.d_text, C, seq_rows, w.d_embed, workspace, text_stash, nullptr, s, nt, dt - 1, w.d_deep)) return rc;
  if (int rc = run_vision_backward(m, wv, w.d_feats, B, nv, dv, w.d_vis, w.vision, vision_stash, nullptr, s)) return rc;
  if (sc) {
    if (int rc = launch_step(who, w.d_embed, w.d_deep, w.d_vis, block, nullptr, scaled_grad, 0, C, L, nt, dt, Dt, nv, dv, Dv, 1.f, nullptr, 0, momentum,
                             dampening, weight_decay, nesterov, s))
      return rc;
    return launch_block_step_scaled(scaled_grad, block, buf, grad_out, total, *sc, lr, momentum, dampening,
                                    weight_decay, nesterov, scaled_ws, s);
  }
  return launch_step(who, w.d_embed, w.d_deep, w.d_vis, block, buf, grad_out, 1, C, L, nt, dt, Dt, nv, dv, Dv, grad_scale, lr, first_step, momentum, dampening,
                     weight_decay, nesterov, s);
}

extern "C" {

int clipmi_promptsrc_train_step(clipmi_model* m, const clipmi_text_dgrad* wt, const clipmi_vision_dgrad* wv, const void* prompts, int dtype, const int32_t* eot,
                                int n_prompts, int seq_rows, const void* image, int image_dtype, int B, const int64_t* labels, const float* teacher,
                                float* block, float* buf, int nt, int dt, int nv, int dv, float scale, float grad_scale, float w_text, float w_image,
                                float w_logit, const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov,
                                float* losses, float* grad_out, void* workspace, size_t workspace_bytes, void* text_stash, size_t text_stash_bytes,
                                void* vision_stash, size_t vision_stash_bytes, clipmi_stream_t stream) {
  return promptsrc_train_step("promptsrc_train_step", nullptr, m, wt, wv, prompts, dtype, eot, n_prompts, seq_rows, image, image_dtype, B, labels, teacher, block,
                              buf, nt, dt, nv, dv, scale, grad_scale, w_text, w_image, w_logit, lr, first_step, momentum, dampening, weight_decay, nesterov,
                              losses, grad_out, workspace, workspace_bytes, text_stash, text_stash_bytes, vision_stash, vision_stash_bytes, stream);
}

int clipmi_promptsrc_train_step_scaled(clipmi_model* m, const clipmi_text_dgrad* wt, const clipmi_vision_dgrad* wv, const void* prompts, int dtype,
                                       const int32_t* eot, int n_prompts, int seq_rows, const void* image, int image_dtype, int B, const int64_t* labels,
                                       const float* teacher, float* block, float* buf, int nt, int dt, int nv, int dv, float scale,
                                       clipmi_scaler_state* state, float growth_factor, float backoff_factor, int growth_interval, float w_text,
                                       float w_image, float w_logit, const float* lr, float momentum, float dampening, float weight_decay, int nesterov,
                                       float* losses, float* grad_out, void* workspace, size_t workspace_bytes, void* text_stash, size_t text_stash_bytes,
                                       void* vision_stash, size_t vision_stash_bytes, clipmi_stream_t stream) {
  const ScalerCall sc{state, growth_factor, backoff_factor, growth_interval};
  return promptsrc_train_step("promptsrc_train_step_scaled", &sc, m, wt, wv, prompts, dtype, eot, n_prompts, seq_rows, image, image_dtype, B, labels, teacher,
                              block, buf, nt, dt, nv, dv, scale, 1.f, w_text, w_image, w_logit, lr, 0, momentum, dampening, weight_decay, nesterov, losses,
                              grad_out, workspace, workspace_bytes, text_stash, text_stash_bytes, vision_stash, vision_stash_bytes, stream);
}

}  // extern "C"
