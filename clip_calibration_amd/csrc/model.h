// The model handle of include/clipmi.h, shared by the translation units that drive a tower (capi.hip: the inference towers;
// text_backward.hip: the text tower's training forward and its backward).  Host-side C++ only.
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
