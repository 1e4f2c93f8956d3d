// Multi-class isotonic calibration (reference trainers/calibration/multi_isotonic_regression.py) and its proximity-binned form
// Bin-Mean-Shift (multi_proximity_isotonic.py:130-247), selected by vl_calibrator.py:121-147 on base_calibration_mode "bin_based" with
// base_bin_calibrator_name "multi_isotonic_regression".  Per element of a row the reference computes, on the host in numpy,
//   p = softmax(DAC(logits)),   x = exp(p) / sum_j exp(p_j)   (a SECOND softmax, of the probabilities),   out = g(x) + 1e-9 x
// with g the fitted isotonic function: linear interpolation through the thresholds, clipped outside them; rows are not renormalised.
//
// Shared by every kernel here (row_softmax / row_x), so that fit and predict see bit-identical x:
//   p  the lane-strided form of row_calibrate_kernel (logits.hip) and procal.hip, with or without a DAC factor (f = 1), the product
//      logit * f rounded before the subtraction: a row scaled here and a row that arrives scaled give the same bits;
//   x  expf (the accurate one: the reference's is numpy's float32 exp) over a lane-strided sum, one correctly rounded division.
//
// Fit.  The isotonic fit to 0/1 targets is determined by the N positive keys (x at the label) and, for the N (C - 1) zeros, by
// per-gap statistics: isotonic_keys_kernel writes the positive keys; the host sorts and de-duplicates them per proximity
// bin; isotonic_stats_kernel then does a binary search per element into its bin's keys and accumulates, for a bin with m keys,
//   slot g            (0 <= g <= m)  zeros strictly between key g-1 and key g: count, min and max bit pattern (x > 0: bit order = value order)
//   slot m+1+k        (0 <= k < m)   zeros equal to key k: count
//   slot 2m+1+k                      multiplicity of key k among the positives
// Counts are aggregated per wave before the (vector) atomic; min / max look before they leap.  The pooling of the <= 2m+1 weighted
// points runs on the host in float64.
//
// Predict.  One wave per row, four rows per workgroup; the packed tables (X | Y | slope per table, fp64) sit in LDS when they fit in
// 48 KiB, else they are read from global memory.  g is evaluated in fp64 with numpy.interp's own formula slope * (x - X_j) + Y_j,
// rounded to fp32 once; the 1e-9 x term is added in fp32 as the reference does.  Top-1 with the lowest index among equal maxima.
#include <cmath>

#include "common.h"

namespace clipmi {
namespace {

constexpr int MAXT = CLIPMI_ISOTONIC_MAX_TABLES;
constexpr int LDS_ENTRIES = 2048;   // 2048 thresholds x 3 fp64 = 48 KiB

struct RowSoftmax { float f, M, inv, s2; bool from_probs; };

__device__ __forceinline__ float row_p(const RowSoftmax& r, float v) {
#pragma clang fp contract(off)   // y = logit * f is rounded once: logits that arrive DAC-scaled (runner.test) give the same bits
  return r.from_probs ? v : __expf(v * r.f - r.M) * r.inv;
}
__device__ __forceinline__ float row_x(const RowSoftmax& r, float v) { return expf(row_p(r, v)) / r.s2; }

// a whole wave per row; every lane returns the same parameters
__device__ __forceinline__ RowSoftmax row_softmax(const float* lr, const float* __restrict__ dac, int C, int lane, bool from_probs) {
#pragma clang fp contract(off)
  RowSoftmax r{1.0f, 0.f, 1.0f, 1.0f, from_probs};
  if (!from_probs) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
      const float v = lr[c];
      if (v > best) { best = v; bi = c; }
    }
    wave_argmax(best, bi);
    if (bi == 0x7fffffff) bi = 0;
    if (dac) r.f = dac[bi];   // the factor of the raw argmax (distanse_aware_calibration.py:49-58)
    r.M = best * r.f;
    float se = 0.f;
    for (int c = lane; c < C; c += 64) se += __expf(lr[c] * r.f - r.M);
    r.inv = 1.0f / wave_sum(se);
  }
  float s2 = 0.f;
  for (int c = lane; c < C; c += 64) s2 += expf(row_p(r, lr[c]));
  r.s2 = wave_sum(s2);
  return r;
}

__global__ __launch_bounds__(256) void isotonic_keys_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                            float* __restrict__ keys, int N, int C, int from_probs) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* lr = logits + (int64_t)row * C;
  const RowSoftmax r = row_softmax(lr, nullptr, C, lane, from_probs != 0);
  if (lane == 0) {
    const int64_t lab = labels[row];
    keys[row] = lab >= 0 && lab < C ? row_x(r, lr[lab]) : NAN;   // a label outside the classes: the host refuses the NaN key
  }
}

struct StatsArgs {
  const float* keys;       // the sorted distinct positive keys, bin after bin
  int n_bins;
  int key_off[MAXT + 1];   // bin b owns keys[key_off[b] .. key_off[b + 1])
};

__global__ void isotonic_stats_init_kernel(int32_t* __restrict__ stats, int32_t* __restrict__ status, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < total) {
    stats[i] = 0;
    stats[total + i] = 0x7f800000;   // min: +inf
    stats[2 * total + i] = 0;        // max
  }
  if (i == 0) *status = 0;
}

// status bits: 1 a positive element did not find its own key, 2 an x outside (0, 1] (non-finite logits), 4 a bin index out of range
__global__ __launch_bounds__(256) void isotonic_stats_kernel(StatsArgs a, const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                             const int32_t* __restrict__ bin, int32_t* __restrict__ stats,
                                                             int32_t* __restrict__ status, int total, int N, int C, int from_probs) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const int b = bin ? bin[row] : 0;
  if (b < 0 || b >= a.n_bins) {
    if (lane == 0) atomicOr(status, 4);
    return;
  }
  const float* __restrict__ keys = a.keys + a.key_off[b];
  const int m = a.key_off[b + 1] - a.key_off[b];
  const int base = 3 * a.key_off[b] + b;
  int32_t* cnt = stats;
  uint32_t* lo_bits = reinterpret_cast<uint32_t*>(stats) + total;
  uint32_t* hi_bits = reinterpret_cast<uint32_t*>(stats) + 2 * (int64_t)total;
  const float* lr = logits + (int64_t)row * C;
  const RowSoftmax r = row_softmax(lr, nullptr, C, lane, from_probs != 0);
  const int64_t lab = labels[row];
  int bad = 0;
  for (int c0 = 0; c0 < C; c0 += 64) {
    const int c = c0 + lane;
    int slot = -1;
    if (c < C) {
      const float x = row_x(r, lr[c]);
      if (!(x > 0.f && x <= 1.f)) {
        bad |= 2;
      } else {
        int lo = 0, hi = m;   // g = the number of keys below x
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (keys[mid] < x) lo = mid + 1;
          else hi = mid;
        }
        const bool eq = lo < m && keys[lo] == x;
        if (c == lab) {
          if (eq) slot = base + 2 * m + 1 + lo;
          else bad |= 1;
        } else if (eq) {
          slot = base + m + 1 + lo;
        } else {
          slot = base + lo;
          const uint32_t bits = __builtin_bit_cast(uint32_t, x);
          if (bits < lo_bits[slot]) atomicMin(&lo_bits[slot], bits);   // a stale read only costs a spare atomic: min only falls, max only rises
          if (bits > hi_bits[slot]) atomicMax(&hi_bits[slot], bits);
        }
      }
    }
    // one atomic per distinct slot of the wave (the zeros below the smallest key alone are most of a row)
    uint64_t todo = __ballot(slot >= 0);
    while (todo) {
      const int leader = __ffsll((unsigned long long)todo) - 1;
      const int s0 = __shfl(slot, leader, 64);
      const uint64_t same = __ballot(slot == s0);
      if (lane == leader) atomicAdd(&cnt[s0], (int)__popcll(same));
      todo &= ~same;
    }
  }
  if (bad) atomicOr(status, bad);
}

struct RowsArgs {
  const double* table;
  int n_tables;
  int off[MAXT + 1];
  double edges[MAXT - 1];
};

template <bool IN_LDS>
__global__ __launch_bounds__(256) void isotonic_rows_kernel(RowsArgs a, const float* logits, const float* __restrict__ dac,
                                                            const float* __restrict__ prox, float* probs, float* __restrict__ xs,
                                                            float* __restrict__ conf, int32_t* __restrict__ pred, int N, int C,
                                                            int from_probs) {
#pragma clang fp contract(off)   // numpy.interp rounds the product before the add
  extern __shared__ double sh[];
  if (IN_LDS) {
    const int n = 3 * a.off[a.n_tables];
    for (int i = threadIdx.x; i < n; i += 256) sh[i] = a.table[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  int b = 0;   // np.searchsorted(edges[1:-1], proximity, side="right"): the number of inner edges <= proximity
  if (prox) {
    const double p = (double)prox[row];
    for (int e = 0; e + 1 < a.n_tables; ++e) b += a.edges[e] <= p ? 1 : 0;
  }
  const int T = a.off[b + 1] - a.off[b];
  const double* tab = IN_LDS ? sh : a.table;
  const double* X = tab + 3 * a.off[b];
  const double* Y = X + T;
  const double* S = Y + T;
  const float* lr = logits + (int64_t)row * C;
  const RowSoftmax r = row_softmax(lr, dac, C, lane, from_probs != 0);
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float x = row_x(r, lr[c]);   // read before the write below: probs may alias logits
    const double xd = (double)x;
    int lo = 0, hi = T;   // lo = the number of thresholds <= x
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (X[mid] <= xd) lo = mid + 1;
      else hi = mid;
    }
    const int j = lo - 1;
    const double g = j < 0 ? Y[0] : (j >= T - 1 ? Y[T - 1] : S[j] * (xd - X[j]) + Y[j]);
    const float o = (float)g + 1e-9f * x;
    if (probs) probs[(int64_t)row * C + c] = o;
    if (xs) xs[(int64_t)row * C + c] = x;
    if (o > best) { best = o; bi = c; }   // ascending c: the first of equal values stays
  }
  wave_argmax(best, bi);
  if (lane == 0) {
    conf[row] = bi == 0x7fffffff ? NAN : best;   // no finite maximum
    pred[row] = bi == 0x7fffffff ? 0 : bi;
  }
}

int check_model(const clipmi_isotonic_model* m, RowsArgs& a, bool has_proximity) {
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "isotonic: null model");
  CLIPMI_REQUIRE(m->table, CLIPMI_ERR_ARG, "isotonic: null table");
  CLIPMI_REQUIRE((uintptr_t)m->table % 8 == 0, CLIPMI_ERR_ARG, "isotonic: the table must be 8-byte aligned");
  CLIPMI_REQUIRE(m->n_tables >= 1 && m->n_tables <= MAXT, CLIPMI_ERR_SHAPE, "isotonic: n_tables=%d (1 .. %d)", m->n_tables, MAXT);
  CLIPMI_REQUIRE(m->offset[0] == 0, CLIPMI_ERR_SHAPE, "isotonic: offset[0]=%d (0)", m->offset[0]);
  for (int t = 0; t < m->n_tables; ++t)
    CLIPMI_REQUIRE(m->offset[t + 1] > m->offset[t], CLIPMI_ERR_SHAPE, "isotonic: table %d has %d thresholds (each >= 1)", t,
                   m->offset[t + 1] - m->offset[t]);
  CLIPMI_REQUIRE(m->offset[m->n_tables] <= (1 << 24), CLIPMI_ERR_SHAPE, "isotonic: %d thresholds in all (<= 2^24)", m->offset[m->n_tables]);
  for (int e = 0; e + 1 < m->n_tables; ++e) {
    CLIPMI_REQUIRE(std::isfinite(m->edges[e]), CLIPMI_ERR_ARG, "isotonic: edges[%d]=%g (finite)", e, m->edges[e]);
    CLIPMI_REQUIRE(e == 0 || m->edges[e] >= m->edges[e - 1], CLIPMI_ERR_ARG, "isotonic: edges[%d]=%g < edges[%d]=%g (ascending)", e,
                   m->edges[e], e - 1, m->edges[e - 1]);
  }
  CLIPMI_REQUIRE(m->n_tables == 1 || has_proximity, CLIPMI_ERR_ARG, "isotonic: %d tables need a proximity per row", m->n_tables);
  a.table = m->table;
  a.n_tables = m->n_tables;
  for (int t = 0; t <= MAXT; ++t) a.off[t] = t <= m->n_tables ? m->offset[t] : 0;
  for (int e = 0; e < MAXT - 1; ++e) a.edges[e] = e + 1 < m->n_tables ? m->edges[e] : 0.0;
  return CLIPMI_OK;
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

int clipmi_isotonic_pack(const double* x, const double* y, const int32_t* counts, int n_tables, double* packed) {
  CLIPMI_REQUIRE(x && y && counts && packed, CLIPMI_ERR_ARG, "isotonic_pack: null pointer");
  CLIPMI_REQUIRE(n_tables >= 1 && n_tables <= MAXT, CLIPMI_ERR_SHAPE, "isotonic_pack: n_tables=%d (1 .. %d)", n_tables, MAXT);
  int64_t total = 0;
  for (int t = 0; t < n_tables; ++t) {
    CLIPMI_REQUIRE(counts[t] >= 1, CLIPMI_ERR_SHAPE, "isotonic_pack: table %d has %d thresholds (each >= 1)", t, counts[t]);
    total += counts[t];
  }
  CLIPMI_REQUIRE(total <= (1 << 24), CLIPMI_ERR_SHAPE, "isotonic_pack: %lld thresholds in all (<= 2^24)", (long long)total);
  int64_t o = 0;
  for (int t = 0; t < n_tables; ++t) {
    const int T = counts[t];
    const double *X = x + o, *Y = y + o;
    for (int i = 0; i < T; ++i) {
      CLIPMI_REQUIRE(std::isfinite(X[i]) && std::isfinite(Y[i]), CLIPMI_ERR_ARG, "isotonic_pack: table %d threshold %d is (%g, %g) (finite)", t,
                     i, X[i], Y[i]);
      CLIPMI_REQUIRE(i == 0 || X[i] > X[i - 1], CLIPMI_ERR_ARG, "isotonic_pack: table %d: X[%d]=%g <= X[%d]=%g (strictly ascending)", t, i,
                     X[i], i - 1, X[i - 1]);
    }
    double* P = packed + 3 * o;
    for (int i = 0; i < T; ++i) {
      P[i] = X[i];
      P[T + i] = Y[i];
      P[2 * T + i] = i + 1 < T ? (Y[i + 1] - Y[i]) / (X[i + 1] - X[i]) : 0.0;   // numpy.interp's slope
      CLIPMI_REQUIRE(std::isfinite(P[2 * T + i]), CLIPMI_ERR_ARG, "isotonic_pack: table %d: the slope after threshold %d overflows", t, i);
    }
    o += T;
  }
  return CLIPMI_OK;
}

int clipmi_isotonic_keys(const float* logits, const int64_t* labels, float* keys, int n, int C, int from_probs, clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(n > 0 && C > 0, CLIPMI_ERR_SHAPE, "isotonic_keys: n=%d C=%d", n, C);
  CLIPMI_REQUIRE(logits && labels && keys, CLIPMI_ERR_ARG, "isotonic_keys: null pointer (logits, labels and keys are required)");
  hipLaunchKernelGGL(isotonic_keys_kernel, dim3((n + 3) / 4), dim3(256), 0, s, logits, labels, keys, n, C, from_probs);
  return check_launch("isotonic_keys_kernel");
}

int clipmi_isotonic_gap_stats(const float* logits, const int64_t* labels, const int32_t* bin, const float* keys, const int32_t* key_offset,
                              int n_bins, int32_t* stats, int32_t* status, int n, int C, int from_probs, clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  CLIPMI_REQUIRE(n >= 0 && C > 0, CLIPMI_ERR_SHAPE, "isotonic_gap_stats: n=%d C=%d", n, C);
  CLIPMI_REQUIRE(n_bins >= 1 && n_bins <= MAXT, CLIPMI_ERR_SHAPE, "isotonic_gap_stats: n_bins=%d (1 .. %d)", n_bins, MAXT);
  CLIPMI_REQUIRE(key_offset && keys && stats && status, CLIPMI_ERR_ARG,
                 "isotonic_gap_stats: null pointer (keys, key_offset, stats and status are required)");
  CLIPMI_REQUIRE(n == 0 || (logits && labels), CLIPMI_ERR_ARG, "isotonic_gap_stats: null pointer (logits and labels are required)");
  CLIPMI_REQUIRE(n_bins == 1 || bin || n == 0, CLIPMI_ERR_ARG, "isotonic_gap_stats: %d bins need a bin index per row", n_bins);
  CLIPMI_REQUIRE(key_offset[0] == 0, CLIPMI_ERR_SHAPE, "isotonic_gap_stats: key_offset[0]=%d (0)", key_offset[0]);
  StatsArgs a{};
  a.keys = keys;
  a.n_bins = n_bins;
  for (int b = 0; b < n_bins; ++b) {
    CLIPMI_REQUIRE(key_offset[b + 1] > key_offset[b], CLIPMI_ERR_SHAPE, "isotonic_gap_stats: bin %d has %d keys (each >= 1)", b,
                   key_offset[b + 1] - key_offset[b]);
    a.key_off[b + 1] = key_offset[b + 1];
  }
  CLIPMI_REQUIRE(key_offset[n_bins] <= n || n == 0, CLIPMI_ERR_SHAPE, "isotonic_gap_stats: %d keys for %d rows", key_offset[n_bins], n);
  CLIPMI_REQUIRE((int64_t)n * C < 0x7fffffffll, CLIPMI_ERR_SHAPE, "isotonic_gap_stats: n * C = %lld overflows the int32 counts",
                 (long long)n * C);
  const int total = 3 * key_offset[n_bins] + n_bins;
  hipLaunchKernelGGL(isotonic_stats_init_kernel, dim3((total + 255) / 256), dim3(256), 0, s, stats, status, total);
  if (int rc = check_launch("isotonic_stats_init_kernel")) return rc;
  if (n == 0) return CLIPMI_OK;
  hipLaunchKernelGGL(isotonic_stats_kernel, dim3((n + 3) / 4), dim3(256), 0, s, a, logits, labels, bin, stats, status, total, n, C,
                     from_probs);
  return check_launch("isotonic_stats_kernel");
}

int clipmi_isotonic_rows(const clipmi_isotonic_model* model, const float* logits, const float* dac_conf, const float* proximity,
                         int from_probs, float* probs, float* xs, float* conf, int32_t* pred, int n, int C, clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(n > 0 && C > 0, CLIPMI_ERR_SHAPE, "isotonic_rows: n=%d C=%d", n, C);
  CLIPMI_REQUIRE(logits && conf && pred, CLIPMI_ERR_ARG, "isotonic_rows: null pointer (logits, conf and pred are required)");
  CLIPMI_REQUIRE(!(from_probs && dac_conf), CLIPMI_ERR_ARG, "isotonic_rows: the DAC factor scales logits, not probabilities");
  RowsArgs a;
  if (int rc = check_model(model, a, proximity != nullptr)) return rc;
  const int entries = a.off[a.n_tables];
  const dim3 grid((n + 3) / 4);
  if (entries <= LDS_ENTRIES)
    hipLaunchKernelGGL(isotonic_rows_kernel<true>, grid, dim3(256), (size_t)entries * 3 * sizeof(double), s, a, logits, dac_conf, proximity,
                       probs, xs, conf, pred, n, C, from_probs);
  else
    hipLaunchKernelGGL(isotonic_rows_kernel<false>, grid, dim3(256), 0, s, a, logits, dac_conf, proximity, probs, xs, conf, pred, n, C,
                       from_probs);
  return check_launch("isotonic_rows_kernel");
}

}  // extern "C"
