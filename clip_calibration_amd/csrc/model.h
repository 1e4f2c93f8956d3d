// The model handle of include/clipmi.h, shared by the translation units that drive a tower (capi.hip: the inference towers;
// text_backward.hip: the text tower's training forward and its backward; prompt_train.hip: the one-call training step around them).
// Host-side C++ only.
#pragma once
#include <vector>

#include "common.h"

struct clipmi_model {
  clipmi_geometry g;
  bool has_vision = false, has_text = false;
  // per-handle settings (clipmi_model_set_option): -1 = follow the process-wide default of the same name
  std::atomic<int> opt_residual_f16{-1}, opt_ln_fold{-1}, opt_cls_only{-1};
  int residual_mode() const { const int v = opt_residual_f16.load(std::memory_order_relaxed); return v >= 0 ? v : clipmi::options().residual_f16.load(std::memory_order_relaxed); }
  int ln_fold() const { const int v = opt_ln_fold.load(std::memory_order_relaxed); return v >= 0 ? v : clipmi::options().ln_fold.load(std::memory_order_relaxed); }
  int cls_only() const { const int v = opt_cls_only.load(std::memory_order_relaxed); return v >= 0 ? v : clipmi::options().cls_only_last_block.load(std::memory_order_relaxed); }
  clipmi_vision_weights vw;
  clipmi_text_weights tw;
  std::vector<clipmi_block_weights> vblocks, tblocks;
  int grid() const { return g.image_resolution / g.patch_size; }
  int tokens0() const { return grid() * grid() + 1; }
  int kpad() const { return clipmi::round_up(3 * g.patch_size * g.patch_size, 64); }
  size_t col_bytes(int batch) const { return (size_t)batch * grid() * grid() * kpad() * 2; }
};

namespace clipmi {

// consecutive 256-byte aligned pieces of a workspace; a null base only counts
struct Carver {
  char* base; size_t off = 0;
  explicit Carver(void* p) : base(static_cast<char*>(p)) {}
  template <typename T> T* take(size_t bytes) {
    T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align256(bytes);
    return r;
  }
};

// rows of a prompt the tower works on: the caller's bound on the last live token (dead-row elimination), else the whole context
inline int live_rows(const clipmi_model* m, int seq_rows) { return seq_rows > 0 && seq_rows < m->g.context_length ? seq_rows : m->g.context_length; }

// ---- what the two training towers share (text_backward.hip defines the launchers; vision_backward.hip drives the image tower with them)
int launch_ln_backward(const float* x, int64_t x_stride, const int32_t* row_idx, const float* gamma, const void* dy, int dy_dtype, float* g,
                       half_t* g16, int64_t rows, int D, float eps, hipStream_t s);
int launch_quickgelu_forward(const half_t* h, half_t* a, int64_t n, hipStream_t s);
int launch_quickgelu_backward(const half_t* h, const half_t* d_a, half_t* d_h, int64_t n, hipStream_t s);
int launch_operand_stats(const half_t* x, int64_t n, unsigned long long* stats, hipStream_t s);

// workspace shared by a tower's training forward and its backward over M = C * L token rows: C sequences (prompts of the text tower,
// images of the image tower) of L token rows, D the tower's width, E the embedding
struct TrainWs {
  half_t* xn;      // [M, D]   LayerNorm output (forward) / fp16 copy of the gradient stream (backward)
  half_t* att;     // [M, D]   attention output / its gradient
  half_t* hid;     // [M, 4D]  QuickGELU output / the gradient of c_fc's output
  half_t* qkv;     // [M, 3D]  backward: dqkv
  float* dy;       // [M, D]   backward: the fp32 output of the dgrad GEMM in front of a LayerNorm backward
  half_t* rows16;  // [C, D]   the output rows of the last LayerNorm (ln_final / ln_post)
  half_t* dfeat16; // [C, E]
  float* dxf;      // [C, D]   d_out projection^T (text_projection / visual.proj)
  size_t bytes;
};
inline TrainWs carve_ws(void* p, int64_t M, int64_t C, int D, int E) {
  Carver c(p);
  TrainWs w;
  w.xn = c.take<half_t>((size_t)M * D * 2);
  w.att = c.take<half_t>((size_t)M * D * 2);
  w.hid = c.take<half_t>((size_t)M * D * 8);
  w.qkv = c.take<half_t>((size_t)M * D * 6);
  w.dy = c.take<float>((size_t)M * D * 4);
  w.rows16 = c.take<half_t>((size_t)C * D * 2);
  w.dfeat16 = c.take<half_t>((size_t)C * E * 2);
  w.dxf = c.take<float>((size_t)C * D * 4);
  w.bytes = c.off;
  return w;
}

// the stash of either tower: x[2 i] = block i's input rows, x[2 i + 1] = its rows before ln_2, x[2 layers] = the last LayerNorm's input
// (ln_final / ln_post); per block qkv and h; idx: the C gathered row indices (EOT rows / class rows)
struct Stash {
  char* base; int64_t M; int D, layers; size_t x_bytes, qkv_bytes, h_bytes;
  float* x(int k) const { return reinterpret_cast<float*>(base + (size_t)k * x_bytes); }
  half_t* qkv(int i) const { return reinterpret_cast<half_t*>(base + (size_t)(2 * layers + 1) * x_bytes + (size_t)i * qkv_bytes); }
  half_t* h(int i) const { return reinterpret_cast<half_t*>(base + (size_t)(2 * layers + 1) * x_bytes + (size_t)layers * qkv_bytes + (size_t)i * h_bytes); }
  int32_t* idx() const { return reinterpret_cast<int32_t*>(base + (size_t)(2 * layers + 1) * x_bytes + (size_t)layers * (qkv_bytes + h_bytes)); }
  size_t bytes(int64_t C) const { return (size_t)(2 * layers + 1) * x_bytes + (size_t)layers * (qkv_bytes + h_bytes) + align256((size_t)C * 8); }
};
inline Stash carve_stash(void* p, int64_t M, int D, int layers) {
  Stash st;
  st.base = static_cast<char*>(p); st.M = M; st.D = D; st.layers = layers;
  st.x_bytes = align256((size_t)M * D * 4);
  st.qkv_bytes = align256((size_t)M * D * 6);
  st.h_bytes = align256((size_t)M * D * 8);
  return st;
}

inline int tower_gemm(const half_t* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* residual, void* out, int64_t ldo,
                      int out_dtype, int64_t M, int N, int K, int epilogue, hipStream_t s) {
  GemmArgs a{};
  a.A = A; a.lda = lda; a.W = static_cast<const half_t*>(W); a.ldw = ldw; a.bias = bias; a.residual = residual; a.out = out; a.ldo = ldo;
  a.out_dtype = out_dtype; a.M = (int)M; a.N = N; a.K = K; a.epilogue = epilogue;
  return launch_gemm(a, s);
}

// vision_backward.hip: the image tower's training forward and backward (VPT), for the one-call step of prompt_train.hip
int check_vision_train_call(const char* who, const clipmi_model* m, int B, int n_ctx, int depth, const void* ws, size_t ws_bytes, const void* stash,
                            size_t stash_bytes);
int check_vision_dgrad(const char* who, const clipmi_model* m, const clipmi_vision_dgrad* wt);
// out[j, :] = sum_b g[b L + first + j, :], b ascending; with `zero` those rows of g and g16 are cleared behind the sum
int launch_splice_reduce(float* g, half_t* g16, float* out, int B, int L, int D, int first, int n_ctx, int zero, hipStream_t s);
int run_vision_train_forward(clipmi_model* m, const void* image, int image_dtype, int B, const float* prompts, int n_ctx, int depth, float* out,
                             void* workspace, void* stash_p, hipStream_t s);
int run_vision_backward(clipmi_model* m, const clipmi_vision_dgrad* wt, const float* d_out, int B, int n_ctx, int depth, float* d_prompts,
                        void* workspace, const void* stash_p, unsigned long long* stats, hipStream_t s);

// text_backward.hip: the training tower's checks and drivers, for the one-call step of prompt_train.hip
int check_train_call(const char* who, const clipmi_model* m, int n_prompts, const void* ws, size_t ws_bytes, const void* stash, size_t stash_bytes,
                     int seq_rows);
int check_train_inputs(const char* who, const clipmi_model* m, const void* prompts, int dtype, const float* ctx, int n_ctx, const int32_t* eot,
                       int seq_rows, const clipmi_prompt_hook* hook, unsigned flags);
int check_dgrad(const char* who, const clipmi_model* m, const clipmi_text_dgrad* wt);
// deep, n_deep (MaPLe): fp32 [n_deep, n_ctx, Dt], rounded through fp16 over the rows 1 .. n_ctx of every prompt in front of block i = 1 .. n_deep;
// the backward then writes d_deep of that shape (the prompts' rows summed in ascending order) and zeroes those rows of the stream
int run_train_forward(clipmi_model* m, const void* prompts, int dtype, const float* ctx, int n_ctx, int per_class, const int32_t* eot, int C, int seq_rows,
                      float* out, void* workspace, void* stash_p, hipStream_t s, const float* deep = nullptr, int n_deep = 0);
int run_backward(clipmi_model* m, const clipmi_text_dgrad* wt, const float* d_out, int C, int seq_rows, float* g, void* workspace, const void* stash_p,
                 unsigned long long* stats, hipStream_t s, int n_ctx = 0, int n_deep = 0, float* d_deep = nullptr);
int check_deep(const char* who, const clipmi_model* m, int n_ctx, int n_deep, const void* deep, int seq_rows);

// prompt_train.hip: MaPLe's joint head (the loss, d_feats [B, E] and d_text [C, E] of one logits matrix), for maple_train.hip
int launch_maple_head(const char* who, const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale,
                      float grad_scale, float* loss, float* d_feats, float* d_text, half_t* d_text16, void* workspace, size_t workspace_bytes, hipStream_t s);

// prompt_train.hip: PromptSRC's head (the joint head plus the two L1 terms and the logit KL against a frozen teacher), for promptsrc_train.hip
size_t promptsrc_head_bytes(int B, int E, int C);
int check_promptsrc_head(const char* who, const float* feats, int64_t ld, const float* zs_feats, const int64_t* labels, const float* text, const float* teacher,
                         int B, int E, int C, float scale, float grad_scale, float w_text, float w_image, float w_logit, const float* losses,
                         const float* d_feats, const float* d_text, const void* workspace, size_t workspace_bytes);
int launch_promptsrc_head(const char* who, const float* feats, int64_t ld, const float* zs_feats, const int64_t* labels, const float* text,
                          const float* teacher, int B, int E, int C, float scale, float grad_scale, float w_text, float w_image, float w_logit,
                          float* losses, float* d_feats, float* d_text, half_t* d_text16, void* workspace, size_t workspace_bytes, hipStream_t s);

// grad_scaler.hip: the dynamic loss scale's launches for the fits' one-call steps.  A ScalerCall is what a `_scaled` step is given in
// grad_scale's place: the device block and torch.cuda.amp.GradScaler's three arguments
struct ScalerCall {
  clipmi_scaler_state* state;
  float growth, backoff;
  int interval;
};
int launch_grad_scale_rows(const char* who, float* x, int rows, int cols, const clipmi_scaler_state* st, hipStream_t s);
// the workspace of one scaled step over `total` elements: the decision record (found, first applied step) | one flag per workgroup of
// SCALED_THREADS elements of the step's first launch | the unscaled gradient
constexpr int SCALED_THREADS = 256;
struct ScaledWs {
  int32_t* decision;   // [2]
  int32_t* flags;      // [blocks]
  float* grad;         // [total]
};
inline int64_t scaled_grad_blocks(int64_t total) { return (total + SCALED_THREADS - 1) / SCALED_THREADS; }
inline size_t scaled_step_bytes(int64_t total) { return 256 + align256((size_t)scaled_grad_blocks(total) * 4) + align256((size_t)total * 4); }
inline ScaledWs scaled_carve(void* ws, int64_t total) {
  char* p = static_cast<char*>(ws);
  ScaledWs w;
  w.decision = reinterpret_cast<int32_t*>(p);
  w.flags = reinterpret_cast<int32_t*>(p + 256);
  w.grad = reinterpret_cast<float*>(p + 256 + align256((size_t)scaled_grad_blocks(total) * 4));
  return w;
}
int check_scaler(const char* who, const ScalerCall& sc);
// the decision launch and the step launch of a scaled step whose own first launch has filled w.grad and w.flags (proda_train.hip)
int launch_scaled_decide_apply(const ScaledWs& w, int64_t total, float* params, float* buf, const ScalerCall& sc, const float* lr, float momentum,
                               float dampening, float weight_decay, int nesterov, hipStream_t s);
// the first two launches of a block's scaled step on their own: unscale and flag (w.grad, w.flags), then the decision and the state's
// update (optim_step.hip applies Adam's rule behind them)
int launch_block_unscale(const float* grad, float* grad_out, int64_t total, const ScalerCall& sc, const ScaledWs& w, hipStream_t s);
int launch_scaler_update(const ScaledWs& w, int64_t total, const ScalerCall& sc, hipStream_t s);
size_t block_step_scaled_bytes(int64_t total);   // 0 for a total the step refuses
int check_block_step_scaled(const char* who, const float* grad, const float* params, const float* buf, const float* grad_out, const float* lr, int64_t total,
                            const ScalerCall& sc, float momentum, float dampening, float weight_decay, int nesterov, const void* workspace,
                            size_t workspace_bytes);
int launch_block_step_scaled(const float* grad, float* params, float* buf, float* grad_out, int64_t total, const ScalerCall& sc, const float* lr, float momentum,
                             float dampening, float weight_decay, int nesterov, void* workspace, hipStream_t s);
// clipmi_ctx_step_scaled's check (*total: the elements of ctx) and its three launches, for the CoOp family's one-call step
int check_ctx_step_scaled(const char* who, const float* d_embed, const float* ctx, const float* buf, const float* lr, int C, int L, int D, int n_ctx, int per_class,
                          const ScalerCall& sc, float momentum, float dampening, float weight_decay, int nesterov, const void* workspace, size_t workspace_bytes,
                          int64_t* total);
int launch_ctx_step_scaled(const float* d_embed, float* ctx, float* buf, float* grad_out, int C, int L, int D, int n_ctx, int per_class, int64_t total,
                           const ScalerCall& sc, const float* lr, float momentum, float dampening, float weight_decay, int nesterov, void* workspace,
                           hipStream_t s);

// prompt_position.hip: the class token at the front or in the middle, for the CoOp family's one-call step.  check_place covers what
// both copy launches ask of the position and the shape (the step's own gradient streams are the unplace launch's other arguments)
struct PromptPlacement {
  int position;
  const int32_t* name_lens;
};
int check_place(const char* who, const void* base, int dtype, const float* ctx, int position, const int32_t* name_lens, const float* out, int C, int L, int Lc,
                int D, int n_ctx);
int enqueue_place(const void* base, int dtype, const float* ctx, int per_class, int position, const int32_t* name_lens, float* out, int C, int L, int Lc, int D,
                  int n_ctx, hipStream_t s);
int enqueue_unplace(const float* d_embed, int position, const int32_t* name_lens, float* out, int C, int L, int D, int n_ctx, hipStream_t s);

// prompt_train.hip: the one-call step of CoOp, KgCoOp and ProGrad behind its six exported symbols.  sc == nullptr: the static step at
// grad_scale; pl == nullptr: the class token at the end, nothing is placed.  need: what the calling symbol's sizing function reports
int prompt_train_step(const char* who, bool need_losses, size_t need, const ScalerCall* sc, const PromptPlacement* pl, clipmi_model* m,
                      const clipmi_text_dgrad* wt, const void* prompts, int dtype, float* ctx, float* buf, int n_ctx, int per_class, const int32_t* eot, int C,
                      int seq_rows, const float* feats, int64_t ld, const int64_t* labels, int B, float scale, float grad_scale, int mode, const float* teacher,
                      float w, float T, float lambda, const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov,
                      float* losses, float* grad_out, int* projected, double* dots, void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes,
                      hipStream_t s);

}  // namespace clipmi
