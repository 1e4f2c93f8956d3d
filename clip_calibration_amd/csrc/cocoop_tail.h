// CoCoOp's per-pair tail (reference cocoop.py:193-199) as one device function: per_image_logits_kernel (cocoop.hip) and the fused validation
// row kernel (fit_monitor.hip, cocoop_val_rows_kernel) both call it, so a pair's logit does not depend on which of the two formed it.
#pragma once
#include "common.h"

namespace clipmi {

// scale * <f, t / |t|> by one wave: lane e, e + 64, ... in ascending order, then the xor butterfly 32 .. 1; every lane returns the same bits.
// *inv_out (every lane) = 1 / |t|.
__device__ __forceinline__ float pair_logit(const float* __restrict__ f, const float* __restrict__ t, float scale, int E, int lane, float* inv_out) {
  float dot = 0.f, ss = 0.f;
  for (int e = lane; e < E; e += 64) {
    const float tv = t[e];
    dot += tv * f[e];
    ss += tv * tv;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float inv = 1.0f / sqrtf(ss);
  *inv_out = inv;
  return scale * dot * inv;
}

}  // namespace clipmi
