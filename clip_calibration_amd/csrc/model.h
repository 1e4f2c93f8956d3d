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

// text_backward.hip: the training tower's checks and drivers, for the one-call step of prompt_train.hip
int check_train_call(const char* who, const clipmi_model* m, int n_prompts, const void* ws, size_t ws_bytes, const void* stash, size_t stash_bytes,
                     int seq_rows);
int check_train_inputs(const char* who, const clipmi_model* m, const void* prompts, int dtype, const float* ctx, int n_ctx, const int32_t* eot,
                       int seq_rows, const clipmi_prompt_hook* hook, unsigned flags);
int check_dgrad(const char* who, const clipmi_model* m, const clipmi_text_dgrad* wt);
int run_train_forward(clipmi_model* m, const void* prompts, int dtype, const float* ctx, int n_ctx, int per_class, const int32_t* eot, int C, int seq_rows,
                      float* out, void* workspace, void* stash_p, hipStream_t s);
int run_backward(clipmi_model* m, const clipmi_text_dgrad* wt, const float* d_out, int C, int seq_rows, float* g, void* workspace, const void* stash_p,
                 unsigned long long* stats, hipStream_t s);

}  // namespace clipmi
