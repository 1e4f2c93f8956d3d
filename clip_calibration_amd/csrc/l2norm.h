// The sum of squares of one row by one wave, in l2norm_kernel's order (elementwise.hip): that kernel and ProDA's normalise-and-mean
// validation kernel (proda_train.hip) both call it, so a row's reciprocal norm does not depend on which of the two formed it.
#pragma once
#include "common.h"

namespace clipmi {

// vec8 (uniform; E % 8 == 0 and 16-byte aligned rows): a lane takes the 8-element chunks lane, lane + 64, ... and adds their squares in
// ascending order with fused multiply-adds; otherwise element lane, lane + 64, ...; then the xor butterfly 32, 16, ..., 1.  Every lane
// returns the same bits.
template <typename TI>
__device__ __forceinline__ float row_sumsq(const TI* __restrict__ x, int E, int vec8, int lane) {
  float ss = 0.f;
  auto load8 = [&](const TI* p8, float (&v)[8]) {
    if constexpr (sizeof(TI) == 4) {
      const f32x4 p = *reinterpret_cast<const f32x4*>(p8), q = *reinterpret_cast<const f32x4*>(p8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] = p[e]; v[4 + e] = q[e]; }
    } else {
      const f16x8 h = *reinterpret_cast<const f16x8*>(p8);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (float)h[e];
    }
  };
  if (vec8) {   // uniform
    for (int c = lane; c < (E >> 3); c += 64) {
      float v[8];
      load8(x + c * 8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) ss = __builtin_fmaf(v[e], v[e], ss);
    }
  } else {
    for (int e = lane; e < E; e += 64) {
      const float v = (float)x[e];
      ss = __builtin_fmaf(v, v, ss);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  return ss;
}

}  // namespace clipmi
