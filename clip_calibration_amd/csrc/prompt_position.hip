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

int check_unplace(const char* who, const float* d_embed, int position, const int32_t* name_lens, const float* out, int C, int L, int D, int n_ctx) {
  CLIPMI_REQUIRE(d_embed && out, CLIPMI_ERR_ARG, "%s: null pointer", who);
  if (int rc = check_position(who, position, name_lens, C, L, L, D, n_ctx)) return rc;
  CLIPMI_REQUIRE((uintptr_t)d_embed % 16 == 0 && (uintptr_t)out % 16 == 0, CLIPMI_ERR_ARG, "%s: d_embed and the output must be 16-byte aligned", who);
  return CLIPMI_OK;
}

// the unplaced step's workspace of the same arguments | the placed prompts fp32 [C, Lc, D] | the compact gradient [C (1 + n_ctx), D] and,
// for ProGrad, | the second one: what the placed sizers add (prompt_train.hip carves it)
inline size_t placed_extra_bytes(const clipmi_model* m, int C, int mode, int n_ctx) {
  const int D = m->g.text_width;
  return align256((size_t)C * m->g.context_length * D * 4) + (mode == MODE_PROGRAD ? 2 : 1) * align256((size_t)C * (1 + n_ctx) * D * 4);
}

}  // namespace

// ---- what the CoOp family's one-call step shares (model.h)
int check_place(const char* who, const void* base, int dtype, const float* ctx, int position, const int32_t* name_lens, const float* out, int C, int L, int Lc,
                int D, int n_ctx) {
  CLIPMI_REQUIRE(base && ctx && out, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(dtype == CLIPMI_F16 || dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "%s: bad dtype %d", who, dtype);
  if (int rc = check_position(who, position, name_lens, C, L, Lc, D, n_ctx)) return rc;
  CLIPMI_REQUIRE((uintptr_t)base % 16 == 0 && (uintptr_t)ctx % 16 == 0 && (uintptr_t)out % 16 == 0, CLIPMI_ERR_ARG,
                 "%s: base, ctx and the prompt buffer must be 16-byte aligned", who);
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
  const PromptPlacement pl{position, name_lens};
  return prompt_train_step("prompt_train_step_placed", true, clipmi_prompt_train_step_placed_bytes(m, n_prompts, seq_rows, B, mode, n_ctx, ctx_per_class), nullptr,
                           &pl, m, wt, prompts, dtype, ctx, buf, n_ctx, ctx_per_class, eot, n_prompts, seq_rows, feats, ld, labels, B, scale, grad_scale, mode,
                           teacher, w, T, lambda, lr, first_step, momentum, dampening, weight_decay, nesterov, losses, grad_out, projected, dots, workspace,
                           workspace_bytes, stash, stash_bytes, (hipStream_t)stream);
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
  const ScalerCall sc{state, growth_factor, backoff_factor, growth_interval};
  const PromptPlacement pl{position, name_lens};
  return prompt_train_step("prompt_train_step_scaled_placed", true,
                           clipmi_prompt_train_step_scaled_placed_bytes(m, n_prompts, seq_rows, B, mode, n_ctx, ctx_per_class), &sc, &pl, m, wt, prompts, dtype, ctx,
                           buf, n_ctx, ctx_per_class, eot, n_prompts, seq_rows, feats, ld, labels, B, scale, 1.f, mode, teacher, w, 1.f, 0.f, lr, 0, momentum,
                           dampening, weight_decay, nesterov, losses, grad_out, nullptr, nullptr, workspace, workspace_bytes, stash, stash_bytes,
                           (hipStream_t)stream);
}

}  // extern "C"
