// The class token at the front or in the middle of a CoOp, KgCoOp or ProGrad prompt (reference trainers/classification/coop.py:128-192,
// kgcoop.py:172-230, prograd.py:150-210: PromptLearner.forward's three torch.cat layouts), for one context per class or one for all.  Two
// copy kernels around the frozen tower's training forward and backward, and the one-call steps that put them there.  DESIGN.md "CoOp fit".
//   prompt_place_kernel     the C prompts as fp32 embeddings [C, Lc, D] with the context and the class name on the rows of the position
//   prompt_unplace_kernel   the inverse on the gradient stream: d_embed [C L, D] -> [C (1 + n_ctx), D], row 1 + j of class c the row of prompt c
//                           that holds context vector j, row 0 zeros -- the layout clipmi_ctx_step, clipmi_ctx_step_scaled and clipmi_prograd_step
//                           read at L = 1 + n_ctx, so the class sums, the SGD rule, the scaler's rule and ProGrad's projection are theirs
// The position codes and the row rule are ProDA's (include/clipmi.h, "clipmi_proda_embed").  Plain copies, no atomics: the same inputs give
// the same bits.
#include <cmath>

#include "common.h"
#include "model.h"
#include "train_rules.h"

namespace clipmi {
namespace {

constexpr int THREADS = 256;
enum { POS_FRONT = 0, POS_MIDDLE = 1, POS_END = 2 };
enum { MODE_COOP = 0, MODE_KGCOOP = 1, MODE_PROGRAD = 2 };   // `mode` of clipmi_prompt_head (include/clipmi.h)

// a class's name length as both kernels read it: inside [0, L - 2 - n_ctx], so that no row index computed from it leaves [1, L - 1) (the
// callers check the values on the host; a bad one on the device moves tokens, it is never an address out of bounds)
__device__ __forceinline__ int clamp_name_len(int nl, int L, int n_ctx) { return min(max(nl, 0), L - 2 - n_ctx); }

// THE ROW RULE, once.  A prompt of the position `ps` whose class name is nl tokens long holds, on the rows [1, 1 + n_ctx + nl), f context
// vectors, the nl name tokens and the other n_ctx - f context vectors, in this order; f is all of them (end), none (front) or h = n_ctx / 2
// (middle).  row < 0: the token row of context vector j.  row >= 1: what that row holds -- context vector j >= 0, or -(1 + t) for name token
// t, or INT_MIN for a row the base prompt keeps (SOS; '.', EOT and the padding from 1 + n_ctx + nl on).
constexpr int BASE_ROW = -2147483647 - 1;
__device__ __forceinline__ int place_rule(int ps, int n_ctx, int nl, int j, int row) {
  const int f = ps == POS_END ? n_ctx : ps == POS_MIDDLE ? n_ctx / 2 : 0;
  if (row < 0) return j < f ? 1 + j : 1 + nl + j;
  const int r = row - 1;
  if (r < 0 || r >= n_ctx + nl) return BASE_ROW;
  if (r < f) return r;
  if (r < f + nl) return -(1 + (r - f));
  return r - nl;
}
__device__ __forceinline__ int ctx_row(int ps, int n_ctx, int nl, int j) { return place_rule(ps, n_ctx, nl, j, -1); }
__device__ __forceinline__ int row_source(int ps, int n_ctx, int nl, int row) { return place_rule(ps, n_ctx, nl, 0, row); }

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ld4(const half_t* p) {
  const f16x4 h = *reinterpret_cast<const f16x4*>(p);
  return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}

// one thread per four elements of the live rows: out[c, l, 4 i ..] of the prompt buffer [C, Lc, D].  A context row is copied from the fp32
// master as it is; a base row is widened (exact).  Name token t is base row 1 + n_ctx + t: base holds "X .. X name ."
template <typename T>
__global__ __launch_bounds__(THREADS) void prompt_place_kernel(const T* __restrict__ base, const float* __restrict__ ctx, const int32_t* __restrict__ name_lens,
                                                               float* __restrict__ out, int C, int L, int Lc, int D, int n_ctx, int per_class, int ps) {
  const int D4 = D / 4;
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)C * L * D4) return;
  const int d = (int)(idx % D4) * 4, l = (int)((idx / D4) % L);
  const int64_t c = idx / ((int64_t)D4 * L);
  const int nl = clamp_name_len(name_lens[c], L, n_ctx);
  const int src = row_source(ps, n_ctx, nl, l);
  const T* cls = base + c * Lc * D + d;
  f32x4 v;
  if (src >= 0) v = ld4(ctx + ((per_class ? c * n_ctx : 0) + src) * D + d);
  else if (src == BASE_ROW) v = ld4(cls + (int64_t)l * D);
  else v = ld4(cls + (int64_t)(1 + n_ctx + (-src - 1)) * D);
  *reinterpret_cast<f32x4*>(out + (c * Lc + l) * D + d) = v;
}

// one thread per four elements of out [C, 1 + n_ctx, D]: row 0 zeros, row 1 + j the row of d_embed [C, L, D] that holds context vector j
__global__ __launch_bounds__(THREADS) void prompt_unplace_kernel(const float* __restrict__ d_embed, const int32_t* __restrict__ name_lens, float* __restrict__ out,
                                                                 int C, int L, int D, int n_ctx, int ps) {
  const int D4 = D / 4, R = 1 + n_ctx;
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)C * R * D4) return;
  const int d = (int)(idx % D4) * 4, row = (int)((idx / D4) % R);
  const int64_t c = idx / ((int64_t)D4 * R);
  f32x4 v{0.f, 0.f, 0.f, 0.f};
  if (row >= 1) {
    const int nl = clamp_name_len(name_lens[c], L, n_ctx);
    v = ld4(d_embed + (c * L + ctx_row(ps, n_ctx, nl, row - 1)) * D + d);
  }
  *reinterpret_cast<f32x4*>(out + (c * R + row) * D + d) = v;
}

// what both kernels ask of the position and the shape
int check_position(const char* who, int position, const int32_t* name_lens, int C, int L, int Lc, int D, int n_ctx) {
  CLIPMI_REQUIRE(name_lens, CLIPMI_ERR_ARG, "%s: null pointer (name_lens)", who);
  CLIPMI_REQUIRE(position == POS_FRONT || position == POS_MIDDLE || position == POS_END, CLIPMI_ERR_ARG,
                 "%s: position=%d (0 front, 1 middle, 2 end)", who, position);
  CLIPMI_REQUIRE((uintptr_t)name_lens % 4 == 0, CLIPMI_ERR_ARG, "%s: name_lens must be 4-byte aligned", who);
  CLIPMI_REQUIRE(C >= 1 && n_ctx >= 1 && 2 + n_ctx <= L && L <= Lc, CLIPMI_ERR_SHAPE,
                 "%s: C=%d (>= 1), n_ctx=%d (>= 1), L=%d of Lc=%d rows (SOS, the context and EOT must fit)", who, C, n_ctx, L, Lc);
  CLIPMI_REQUIRE(D >= 4 && D % 4 == 0, CLIPMI_ERR_SHAPE, "%s: D=%d (a multiple of 4)", who, D);
  CLIPMI_REQUIRE((int64_t)C * Lc < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: too many prompt tokens", who);
  return CLIPMI_OK;
}

int check_place(const char* who, const void* base, int dtype, const float* ctx, int position, const int32_t* name_lens, const float* out, int C, int L, int Lc,
                int D, int n_ctx) {
  CLIPMI_REQUIRE(base && ctx && out, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(dtype == CLIPMI_F16 || dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "%s: bad dtype %d", who, dtype);
  if (int rc = check_position(who, position, name_lens, C, L, Lc, D, n_ctx)) return rc;
  CLIPMI_REQUIRE((uintptr_t)base % 16 == 0 && (uintptr_t)ctx % 16 == 0 && (uintptr_t)out % 16 == 0, CLIPMI_ERR_ARG,
                 "%s: base, ctx and the prompt buffer must be 16-byte aligned", who);
  return CLIPMI_OK;
}

int check_unplace(const char* who, const float* d_embed, int position, const int32_t* name_lens, const float* out, int C, int L, int D, int n_ctx) {
  CLIPMI_REQUIRE(d_embed && out, CLIPMI_ERR_ARG, "%s: null pointer", who);
  if (int rc = check_position(who, position, name_lens, C, L, L, D, n_ctx)) return rc;
  CLIPMI_REQUIRE((uintptr_t)d_embed % 16 == 0 && (uintptr_t)out % 16 == 0, CLIPMI_ERR_ARG, "%s: d_embed and the output must be 16-byte aligned", who);
  return CLIPMI_OK;
}

// the launches alone: the caller has passed the checks
int enqueue_place(const void* base, int dtype, const float* ctx, int per_class, int position, const int32_t* name_lens, float* out, int C, int L, int Lc, int D,
                  int n_ctx, hipStream_t s) {
  const int64_t total = (int64_t)C * L * (D / 4);
  const dim3 grid((unsigned)((total + THREADS - 1) / THREADS)), threads(THREADS);
  if (dtype == CLIPMI_F16)
    hipLaunchKernelGGL(prompt_place_kernel<half_t>, grid, threads, 0, s, (const half_t*)base, ctx, name_lens, out, C, L, Lc, D, n_ctx, per_class ? 1 : 0,
                       position);
  else
    hipLaunchKernelGGL(prompt_place_kernel<float>, grid, threads, 0, s, (const float*)base, ctx, name_lens, out, C, L, Lc, D, n_ctx, per_class ? 1 : 0, position);
  return check_launch("prompt_place_kernel");
}

int enqueue_unplace(const float* d_embed, int position, const int32_t* name_lens, float* out, int C, int L, int D, int n_ctx, hipStream_t s) {
  const int64_t total = (int64_t)C * (1 + n_ctx) * (D / 4);
  hipLaunchKernelGGL(prompt_unplace_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, d_embed, name_lens, out, C, L, D, n_ctx,
                     position);
  return check_launch("prompt_unplace_kernel");
}

// ------------------------------------------------------------------------------------------------------------ the one-call steps
// workspace: the unplaced step's of the same arguments (clipmi_prompt_train_step's or clipmi_prompt_train_step_scaled's, carved as those
// carve it) | the placed prompts fp32 [C, Lc, D] | the compact gradient [C (1 + n_ctx), D] and, for ProGrad, | the second one
struct PlacedWs {
  float *text, *d_text, *d_embed, *d_text_kl, *d_embed_kl, *prompts, *compact, *compact_kl;
  void *head, *step;
  size_t head_bytes, step_bytes;
};
inline size_t placed_extra_bytes(const clipmi_model* m, int C, int mode, int n_ctx) {
  const int D = m->g.text_width;
  return align256((size_t)C * m->g.context_length * D * 4) + (mode == MODE_PROGRAD ? 2 : 1) * align256((size_t)C * (1 + n_ctx) * D * 4);
}
inline PlacedWs placed_carve(void* workspace, size_t tower, size_t unplaced, const clipmi_model* m, int C, int L, int B, int mode, int n_ctx, int per_class,
                             bool scaled) {
  const int D = m->g.text_width, E = m->g.embed_dim;
  PlacedWs w{};
  w.head_bytes = clipmi_prompt_head_workspace_bytes(B, E, C, mode);
  Carver c(static_cast<char*>(workspace) + tower);
  w.text = c.take<float>((size_t)C * E * 4);
  w.d_text = c.take<float>((size_t)C * E * 4);
  w.d_embed = c.take<float>((size_t)C * L * D * 4);
  w.head = c.take<char>(w.head_bytes);
  if (scaled) {
    w.step_bytes = clipmi_ctx_step_scaled_workspace_bytes(C, D, n_ctx, per_class);
    w.step = c.take<char>(w.step_bytes);
  } else if (mode == MODE_PROGRAD) {
    w.d_text_kl = c.take<float>((size_t)C * E * 4);
    w.d_embed_kl = c.take<float>((size_t)C * L * D * 4);
    w.step_bytes = clipmi_prograd_step_workspace_bytes(C, D, n_ctx, per_class);
    w.step = c.take<char>(w.step_bytes);
  }
  Carver x(static_cast<char*>(workspace) + unplaced);
  w.prompts = x.take<float>((size_t)C * m->g.context_length * D * 4);
  w.compact = x.take<float>((size_t)C * (1 + n_ctx) * D * 4);
  if (mode == MODE_PROGRAD) w.compact_kl = x.take<float>((size_t)C * (1 + n_ctx) * D * 4);
  return w;
}

// what the two placed steps refuse alike, before anything is launched: the tower's, the placement's and the head's checks (the step's own
// follow in each caller).  need: the placed sizer's report; *tower: the tower's share of the workspace
int check_placed_call(const char* who, const clipmi_model* m, const clipmi_text_dgrad* wt, const void* base, int dtype, const float* ctx, const float* buf,
                      int n_ctx, const int32_t* eot, int C, int seq_rows, int position, const int32_t* name_lens, const float* feats, int64_t ld,
                      const int64_t* labels, int B, float scale, int mode, const float* teacher, float w, const float* lr, float momentum, float dampening,
                      float weight_decay, int nesterov, const float* losses, size_t need, const void* workspace, size_t workspace_bytes, const void* stash,
                      size_t stash_bytes, size_t* tower) {
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "%s: null model", who);
  CLIPMI_REQUIRE(C >= 2 && B >= 1, CLIPMI_ERR_SHAPE, "%s: n_prompts=%d (>= 2), B=%d (>= 1)", who, C, B);
  CLIPMI_REQUIRE(base && ctx && lr && losses && feats && labels && eot && workspace && stash, CLIPMI_ERR_ARG,
                 "%s: null pointer (prompts, ctx, lr, losses, feats, labels, eot, the workspace and the stash are required)", who);
  CLIPMI_REQUIRE(mode == MODE_COOP || teacher, CLIPMI_ERR_ARG, "%s: null pointer (KgCoOp and ProGrad need the teacher)", who);
  const int L = live_rows(m, seq_rows), Lc = m->g.context_length, D = m->g.text_width, E = m->g.embed_dim;
  if (int rc = check_place(who, base, dtype, ctx, position, name_lens, static_cast<const float*>(workspace), C, L, Lc, D, n_ctx)) return rc;
  CLIPMI_REQUIRE(std::isfinite(scale), CLIPMI_ERR_ARG, "%s: scale=%g (finite)", who, scale);
  CLIPMI_REQUIRE(mode != MODE_KGCOOP || (std::isfinite(w) && w >= 0.f), CLIPMI_ERR_ARG, "%s: w=%g (finite, >= 0)", who, w);
  CLIPMI_REQUIRE(ld >= E && (int64_t)B * C < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: B=%d C=%d E=%d ld=%lld", who, B, C, E, (long long)ld);
  if (int rc = check_sgd(who, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE(momentum == 0.f || buf, CLIPMI_ERR_ARG, "%s: null pointer (a momentum needs the buffer)", who);
  CLIPMI_REQUIRE(need > 0 && workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  *tower = 0;
  clipmi_text_train_bytes(m, C, seq_rows, tower, nullptr);
  if (int rc = check_train_call(who, m, C, workspace, *tower, stash, stash_bytes, seq_rows)) return rc;
  if (int rc = check_train_inputs(who, m, base, dtype, ctx, n_ctx, eot, seq_rows, nullptr, 0)) return rc;
  if (int rc = check_dgrad(who, m, wt)) return rc;
  CLIPMI_REQUIRE(L <= AB_MAX_L, CLIPMI_ERR_SHAPE, "%s: %d token rows per prompt (at most %d)", who, L, AB_MAX_L);
  return CLIPMI_OK;
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

int clipmi_prompt_place(const void* base, int dtype, const float* ctx, int per_class, int position, const int32_t* name_lens, float* prompts, int C, int L,
                        int Lc, int D, int n_ctx, clipmi_stream_t stream) {
  if (int rc = check_place("prompt_place", base, dtype, ctx, position, name_lens, prompts, C, L, Lc, D, n_ctx)) return rc;
  return enqueue_place(base, dtype, ctx, per_class, position, name_lens, prompts, C, L, Lc, D, n_ctx, (hipStream_t)stream);
}

int clipmi_prompt_unplace(const float* d_embed, int position, const int32_t* name_lens, float* out, int C, int L, int D, int n_ctx, clipmi_stream_t stream) {
  if (int rc = check_unplace("prompt_unplace", d_embed, position, name_lens, out, C, L, D, n_ctx)) return rc;
  return enqueue_unplace(d_embed, position, name_lens, out, C, L, D, n_ctx, (hipStream_t)stream);
}

size_t clipmi_prompt_train_step_placed_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int mode, int n_ctx, int ctx_per_class) {
  const size_t unplaced = clipmi_prompt_train_step_bytes(m, n_prompts, seq_rows, B, mode, n_ctx, ctx_per_class);
  return unplaced ? unplaced + placed_extra_bytes(m, n_prompts, mode, n_ctx) : 0;
}

int clipmi_prompt_train_step_placed(clipmi_model* m, const clipmi_text_dgrad* wt, const void* prompts, int dtype, float* ctx, float* buf, int n_ctx,
                                    int ctx_per_class, int position, const int32_t* name_lens, const int32_t* eot, int n_prompts, int seq_rows,
                                    const float* feats, int64_t ld, const int64_t* labels, int B, float scale, float grad_scale, int mode,
                                    const float* teacher, float w, float T, float lambda, const float* lr, int first_step, float momentum, float dampening,
                                    float weight_decay, int nesterov, float* losses, float* grad_out, int* projected, double* dots, void* workspace,
                                    size_t workspace_bytes, void* stash, size_t stash_bytes, clipmi_stream_t stream) {
  const char* who = "prompt_train_step_placed";
  const int C = n_prompts;
  hipStream_t s = (hipStream_t)stream;
  CLIPMI_REQUIRE(mode == MODE_COOP || mode == MODE_KGCOOP || mode == MODE_PROGRAD, CLIPMI_ERR_ARG, "%s: bad mode %d", who, mode);
  CLIPMI_REQUIRE(std::isfinite(grad_scale) && grad_scale > 0.f, CLIPMI_ERR_ARG, "%s: grad_scale=%g (finite, > 0)", who, grad_scale);
  CLIPMI_REQUIRE(mode != MODE_PROGRAD || (std::isfinite(T) && T > 0.f && std::isfinite(lambda)), CLIPMI_ERR_ARG, "%s: T=%g (finite, > 0), lambda=%g (finite)",
                 who, T, lambda);
  size_t tower = 0;
  if (int rc = check_placed_call(who, m, wt, prompts, dtype, ctx, buf, n_ctx, eot, C, seq_rows, position, name_lens, feats, ld, labels, B, scale, mode, teacher, w,
                                 lr, momentum, dampening, weight_decay, nesterov, losses,
                                 clipmi_prompt_train_step_placed_bytes(m, C, seq_rows, B, mode, n_ctx, ctx_per_class), workspace, workspace_bytes, stash,
                                 stash_bytes, &tower))
    return rc;
  const int L = live_rows(m, seq_rows), Lc = m->g.context_length, D = m->g.text_width, E = m->g.embed_dim, R = 1 + n_ctx;
  const PlacedWs p = placed_carve(workspace, tower, clipmi_prompt_train_step_bytes(m, C, seq_rows, B, mode, n_ctx, ctx_per_class), m, C, L, B, mode, n_ctx,
                                  ctx_per_class, false);
  if (int rc = enqueue_place(prompts, dtype, ctx, ctx_per_class, position, name_lens, p.prompts, C, L, Lc, D, n_ctx, s)) return rc;
  if (int rc = run_train_forward(m, p.prompts, CLIPMI_F32, nullptr, 0, 0, eot, C, seq_rows, p.text, workspace, stash, s)) return rc;
  if (int rc = clipmi_prompt_head(feats, ld, labels, p.text, B, E, C, scale, grad_scale, mode, teacher, w, T, losses, p.d_text, nullptr, p.d_text_kl, p.head,
                                  p.head_bytes, stream))
    return rc;
  if (int rc = run_backward(m, wt, p.d_text, C, seq_rows, p.d_embed, workspace, stash, nullptr, s)) return rc;
  if (mode != MODE_PROGRAD) {
    if (int rc = enqueue_unplace(p.d_embed, position, name_lens, p.compact, C, L, D, n_ctx, s)) return rc;
    return clipmi_ctx_step(p.compact, ctx, buf, grad_out, C, R, D, n_ctx, ctx_per_class, grad_scale, lr, first_step, momentum, dampening, weight_decay, nesterov,
                           stream);
  }
  if (int rc = run_backward(m, wt, p.d_text_kl, C, seq_rows, p.d_embed_kl, workspace, stash, nullptr, s)) return rc;
  if (int rc = enqueue_unplace(p.d_embed, position, name_lens, p.compact, C, L, D, n_ctx, s)) return rc;
  if (int rc = enqueue_unplace(p.d_embed_kl, position, name_lens, p.compact_kl, C, L, D, n_ctx, s)) return rc;
  return clipmi_prograd_step(p.compact, p.compact_kl, ctx, buf, grad_out, projected, dots, C, R, D, n_ctx, ctx_per_class, grad_scale, lambda, lr, first_step,
                             momentum, dampening, weight_decay, nesterov, p.step, p.step_bytes, stream);
}

size_t clipmi_prompt_train_step_scaled_placed_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int mode, int n_ctx, int ctx_per_class) {
  const size_t unplaced = clipmi_prompt_train_step_scaled_bytes(m, n_prompts, seq_rows, B, mode, n_ctx, ctx_per_class);
  return unplaced ? unplaced + placed_extra_bytes(m, n_prompts, mode, n_ctx) : 0;
}

int clipmi_prompt_train_step_scaled_placed(clipmi_model* m, const clipmi_text_dgrad* wt, const void* prompts, int dtype, float* ctx, float* buf, int n_ctx,
                                           int ctx_per_class, int position, const int32_t* name_lens, const int32_t* eot, int n_prompts, int seq_rows,
                                           const float* feats, int64_t ld, const int64_t* labels, int B, float scale, clipmi_scaler_state* state,
                                           float growth_factor, float backoff_factor, int growth_interval, int mode, const float* teacher, float w,
                                           const float* lr, float momentum, float dampening, float weight_decay, int nesterov, float* losses, float* grad_out,
                                           void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes, clipmi_stream_t stream) {
  const char* who = "prompt_train_step_scaled_placed";
  const int C = n_prompts;
  hipStream_t s = (hipStream_t)stream;
  CLIPMI_REQUIRE(mode != MODE_PROGRAD, CLIPMI_ERR_ARG, "%s: ProGrad's mode has no dynamic loss scale (its two gradients share one step)", who);
  CLIPMI_REQUIRE(mode == MODE_COOP || mode == MODE_KGCOOP, CLIPMI_ERR_ARG, "%s: bad mode %d", who, mode);
  CLIPMI_REQUIRE(state, CLIPMI_ERR_ARG, "%s: null pointer (the scaler's state block)", who);
  CLIPMI_REQUIRE((uintptr_t)state % 4 == 0, CLIPMI_ERR_ARG, "%s: the scaler's state block must be 4-byte aligned", who);
  CLIPMI_REQUIRE(std::isfinite(growth_factor) && growth_factor > 0.f && std::isfinite(backoff_factor) && backoff_factor > 0.f, CLIPMI_ERR_ARG,
                 "%s: growth_factor=%g, backoff_factor=%g (both finite, > 0)", who, growth_factor, backoff_factor);
  CLIPMI_REQUIRE(growth_interval >= 1, CLIPMI_ERR_ARG, "%s: growth_interval=%d (>= 1)", who, growth_interval);
  size_t tower = 0;
  if (int rc = check_placed_call(who, m, wt, prompts, dtype, ctx, buf, n_ctx, eot, C, seq_rows, position, name_lens, feats, ld, labels, B, scale, mode, teacher, w,
                                 lr, momentum, dampening, weight_decay, nesterov, losses,
                                 clipmi_prompt_train_step_scaled_placed_bytes(m, C, seq_rows, B, mode, n_ctx, ctx_per_class), workspace, workspace_bytes,
                                 stash, stash_bytes, &tower))
    return rc;
  const int L = live_rows(m, seq_rows), Lc = m->g.context_length, D = m->g.text_width, E = m->g.embed_dim, R = 1 + n_ctx;
  const PlacedWs p = placed_carve(workspace, tower, clipmi_prompt_train_step_scaled_bytes(m, C, seq_rows, B, mode, n_ctx, ctx_per_class), m, C, L, B, mode,
                                  n_ctx, ctx_per_class, true);
  if (int rc = enqueue_place(prompts, dtype, ctx, ctx_per_class, position, name_lens, p.prompts, C, L, Lc, D, n_ctx, s)) return rc;
  if (int rc = run_train_forward(m, p.prompts, CLIPMI_F32, nullptr, 0, 0, eot, C, seq_rows, p.text, workspace, stash, s)) return rc;
  if (int rc = clipmi_prompt_head(feats, ld, labels, p.text, B, E, C, scale, 1.f, mode, teacher, w, 1.f, losses, p.d_text, nullptr, nullptr, p.head, p.head_bytes,
                                  stream))
    return rc;
  if (int rc = launch_grad_scale_rows(who, p.d_text, C, E, state, s)) return rc;
  if (int rc = run_backward(m, wt, p.d_text, C, seq_rows, p.d_embed, workspace, stash, nullptr, s)) return rc;
  if (int rc = enqueue_unplace(p.d_embed, position, name_lens, p.compact, C, L, D, n_ctx, s)) return rc;
  return clipmi_ctx_step_scaled(p.compact, ctx, buf, grad_out, C, R, D, n_ctx, ctx_per_class, state, growth_factor, backoff_factor, growth_interval, lr,
                                momentum, dampening, weight_decay, nesterov, p.step, p.step_bytes, stream);
}

}  // extern "C"
