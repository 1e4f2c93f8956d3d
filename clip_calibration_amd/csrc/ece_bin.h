// The confidence-bin rule of the library, stated once: the ECE kernels (logits.hip) and the row scores (row_scores.hip) share it, and
// clip_calibration_amd/metrics.py digitize_bins is its host form.
#pragma once
#include <hip/hip_runtime.h>

namespace clipmi {

// bin index = np.digitize(conf, linspace(0, 1, n_bins + 1)) - 1, with conf == 1.0 in bin n_bins (tools/metrics.py:90-130)
__device__ __forceinline__ int ece_bin(double x, int n_bins) {
  const double step = 1.0 / (double)n_bins;  // np.linspace: edge_i = i * step, last edge = 1.0 exactly
  int b = (int)floor(x * n_bins);
  b = b < 0 ? 0 : (b > n_bins ? n_bins : b);
  auto edge = [&](int k) { return k >= n_bins ? 1.0 : (double)k * step; };
  while (b < n_bins && edge(b + 1) <= x) ++b;
  while (b > 0 && edge(b) > x) --b;
  if (!(x < 1.0)) b = n_bins;   // 1.0, and NaN: np.digitize puts it behind the last edge
  return b;
}

}  // namespace clipmi
