// Proper scores of whole probability rows at test time (DESIGN.md "Row scores"): per row the negative log-likelihood and the Brier score, and
// per class the confidence bins of the class-wise calibration error (Kull et al. 2019; the "static calibration error" of Nixon et al. 2019).
// The reference has none of the three; the oracle is the float64 restatement in clip_calibration_amd/metrics.py (NLL, Brier, ClasswiseECE).
//   row_scores_kernel<FROM_PROBS>   one workgroup per 64 rows.  Phase A, one wave per row: the row maximum, sum = sum_c exp(z_c - max) (a lane adds
//                                   its columns c = lane, lane + 64, ... in ascending order, then the xor butterfly), nll and Brier -> row_out, and the
//                                   row's (max, 1 / sum, label) into LDS.  Phase B, per tile of W classes: every element's probability again from the
//                                   saved statistics -- the same instructions on the same operands, hence the same bits --, its bin, and ONE 64-bit
//                                   integer LDS atomic that adds {1 << 48 | round(p 2^32)} to the tile's (class, bin) counter; then the non-zero
//                                   counters go to class_acc with 64-bit integer global atomics, contiguous per wave.
//   row_scores_partials_kernel      float64 partial sums of nll and Brier per 4096 rows (thread t its 16 rows in ascending order, then a fixed
//                                   halving tree) and of the classes' gaps per 256 classes (thread t its class's bins in ascending order, same tree)
//   row_scores_reduce_kernel        ONE thread adds the partials in ascending order and writes the four doubles
// class_acc: int64 [3][C][n_bins + 1] = count | conf_sum | hits, bin b being ece_bin's bin b (ece_bin.h: numpy.digitize over linspace(0, 1,
// n_bins + 1), so the last bin, n_bins, holds p == 1.0 and a NaN).  conf_sum is 32.32 fixed point: every element adds round-to-nearest-even
// (p 2^32) with p clamped to [0, 1].  Integer addition is associative and commutative, so the block holds the same bits whatever the order of
// the atomics and however the rows were cut into calls; nothing else is shared between workgroups.  No float atomics anywhere.
// The rule for rows that cannot be scored is clipmi_val_score's (fit_monitor.hip score_row), restated: a label outside [0, C) is never used as
// an address -- the row's nll and Brier are NaN and it counts no hit, its probabilities are binned all the same; a row without a softmax (it
// holds a NaN or a +inf, or nothing but -inf; with FROM_PROBS: any non-finite entry) has a NaN nll and Brier, counts no hit, and each of its
// elements counts in bin n_bins, where a NaN sorts, and adds nothing to conf_sum, which has no NaN.  The NaNs reach the two means.
#include <cfloat>
#include <cmath>

#include "common.h"
#include "ece_bin.h"

namespace clipmi {
namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_WAVE = 64;
constexpr int RS_WAVES = RS_THREADS / RS_WAVE;
constexpr int RS_ROWS = 64;            // rows per workgroup: at most 64 elements meet in one LDS counter
constexpr int RS_TABLE = 6144;         // 64-bit LDS counters (48 KiB)
constexpr int RS_MAX_BINS = 1024;      // clipmi_ece_accumulate's limit
constexpr int RS_COUNT_SHIFT = 48;     // a counter holds {count << 48 | conf_sum}: 64 elements of at most 2^32 stay below 2^39
constexpr unsigned long long RS_CONF_MASK = (1ull << RS_COUNT_SHIFT) - 1;
constexpr int RF_THREADS = 256;
constexpr int RF_ROWS = 4096;          // rows per partial of the finish: 16 per thread

__host__ __device__ inline int table_stride(int n_bins) { return (n_bins + 1) | 1; }   // odd: a wave's 64 classes spread over the LDS banks

__device__ inline float wave_sum_xor(float v) {
  for (int off = 1; off < RS_WAVE; off <<= 1) v += __shfl_xor(v, off, RS_WAVE);   // a + b == b + a: every lane holds the same bits
  return v;
}

// the probability of one element as both phases form it: from the row's saved (max, 1 / sum), or the element itself
template <bool FROM_PROBS>
__device__ __forceinline__ float element_prob(float v, float m, float inv) {
  return FROM_PROBS ? v : expf(v - m) * inv;
}

// round-to-nearest-even (p 2^32) of a probability clamped to [0, 1]: exact in float64 before the one rounding
__device__ __forceinline__ unsigned long long conf_fixed(float p) {
  const double c = p < 0.f ? 0.0 : (p > 1.f ? 1.0 : (double)p);
  return (unsigned long long)__double2ll_rn(c * 4294967296.0);
}

template <bool FROM_PROBS>
__global__ __launch_bounds__(RS_THREADS) void row_scores_kernel(const float* __restrict__ rows, int64_t ld, const int64_t* __restrict__ labels, int N,
                                                                int C, int n_bins, float* __restrict__ row_out,
                                                                unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long s_tab[RS_TABLE];
  __shared__ float s_m[RS_ROWS], s_inv[RS_ROWS];
  __shared__ int s_y[RS_ROWS];     // the label, -1 when it lies outside [0, C)
  __shared__ int s_bad[RS_ROWS];   // a row without a softmax
  const int wave = threadIdx.x / RS_WAVE, lane = threadIdx.x % RS_WAVE;
  const int64_t row0 = (int64_t)blockIdx.x * RS_ROWS;
  const int have = (int)((int64_t)N - row0 < RS_ROWS ? (int64_t)N - row0 : RS_ROWS);

  // ---- phase A: one wave per row
  for (int r = wave; r < have; r += RS_WAVES) {
    const float* z = rows + (row0 + r) * ld;
    float m = -INFINITY;
    int bad = 0;
    for (int c = lane; c < C; c += RS_WAVE) {
      const float v = z[c];
      bad |= FROM_PROBS ? !isfinite(v) : (v != v);
      m = fmaxf(m, v);
    }
    for (int off = 1; off < RS_WAVE; off <<= 1) {
      m = fmaxf(m, __shfl_xor(m, off, RS_WAVE));
      bad |= __shfl_xor(bad, off, RS_WAVE);
    }
    float inv = 1.f, sum = 1.f;
    if (!FROM_PROBS) {
      bad |= m == INFINITY || m == -INFINITY;
      if (bad) m = 0.f;
      float s = 0.f;
      for (int c = lane; c < C; c += RS_WAVE) s += expf(z[c] - m);
      sum = wave_sum_xor(s);
      inv = 1.f / sum;
    }
    const int64_t y64 = labels[row0 + r];
    const bool in_range = y64 >= 0 && y64 < C;   // a label outside [0, C) is never used as an address
    const int y = in_range ? (int)y64 : -1;
    float b = 0.f;
    for (int c = lane; c < C; c += RS_WAVE) {
      const float d = element_prob<FROM_PROBS>(z[c], m, inv) - (c == y ? 1.f : 0.f);
      b += d * d;
    }
    b = wave_sum_xor(b);
    if (lane == 0) {
      float nll = NAN;
      if (in_range) nll = FROM_PROBS ? -logf(fmaxf(z[y], FLT_MIN)) : logf(sum) - (z[y] - m);   // lse - z[y] with the maximum cancelled before the rounding
      const bool ok = in_range && !bad;
      row_out[2 * (row0 + r)] = ok ? nll : NAN;
      row_out[2 * (row0 + r) + 1] = ok ? b : NAN;
      s_m[r] = m;
      s_inv[r] = inv;
      s_y[r] = y;
      s_bad[r] = bad;
    }
  }

  // ---- phase B: the class-wise bins, a tile of W classes at a time
  const int nb1 = n_bins + 1, stride = table_stride(n_bins);
  const int W = RS_TABLE / stride;   // >= 5: stride <= 1025
  const int64_t plane = (int64_t)C * nb1;
  for (int c0 = 0; c0 < C; c0 += W) {
    const int w = C - c0 < W ? C - c0 : W;
    __syncthreads();   // phase A's statistics, and the previous tile's flush
    for (int i = threadIdx.x; i < w * stride; i += RS_THREADS) s_tab[i] = 0ull;
    __syncthreads();
    for (int r = wave; r < have; r += RS_WAVES) {
      const float* z = rows + (row0 + r) * ld;
      const float m = s_m[r], inv = s_inv[r];
      const int y = s_y[r], bad = s_bad[r];
      for (int c = c0 + lane; c < c0 + w; c += RS_WAVE) {
        const float p = element_prob<FROM_PROBS>(z[c], m, inv);
        const int b = bad ? n_bins : ece_bin((double)p, n_bins);
        const unsigned long long fx = bad || !(p == p) ? 0ull : conf_fixed(p);
        atomicAdd(&s_tab[(c - c0) * stride + b], (1ull << RS_COUNT_SHIFT) | fx);
        if (c == y && !bad) atomicAdd(&acc[2 * plane + (int64_t)c * nb1 + b], 1ull);   // one per row
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < w * nb1; i += RS_THREADS) {   // entry i of the tile is entry c0 * nb1 + i of a plane: contiguous per wave
      const unsigned long long v = s_tab[(i / nb1) * stride + i % nb1];
      if (v == 0ull) continue;
      const int64_t e = (int64_t)c0 * nb1 + i;
      atomicAdd(&acc[e], v >> RS_COUNT_SHIFT);
      if (v & RS_CONF_MASK) atomicAdd(&acc[plane + e], v & RS_CONF_MASK);
    }
  }
}

inline int64_t finish_row_blocks(int N) { return ((int64_t)N + RF_ROWS - 1) / RF_ROWS; }
inline int64_t finish_class_blocks(int C) { return ((int64_t)C + RF_THREADS - 1) / RF_THREADS; }

// the fixed halving tree over the workgroup's 256 values; thread 0 returns the sum
__device__ inline double block_tree_sum(double v, double* s) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int off = RF_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
    __syncthreads();
  }
  return s[0];
}

// partials: double [2 row_blocks + class_blocks] = (nll, brier) per row block, then the gap sum per class block
__global__ __launch_bounds__(RF_THREADS) void row_scores_partials_kernel(const float* __restrict__ row_out, int N, const long long* __restrict__ acc, int C,
                                                                        int n_bins, int64_t row_blocks, double* __restrict__ partials) {
  __shared__ double s_a[RF_THREADS], s_b[RF_THREADS];
  if ((int64_t)blockIdx.x < row_blocks) {
    const int64_t first = (int64_t)blockIdx.x * RF_ROWS + (int64_t)threadIdx.x * (RF_ROWS / RF_THREADS);
    double nll = 0.0, brier = 0.0;
    for (int64_t i = first; i < first + RF_ROWS / RF_THREADS && i < N; ++i) {
      nll += (double)row_out[2 * i];
      brier += (double)row_out[2 * i + 1];
    }
    nll = block_tree_sum(nll, s_a);
    brier = block_tree_sum(brier, s_b);
    if (threadIdx.x == 0) {
      partials[2 * blockIdx.x] = nll;
      partials[2 * blockIdx.x + 1] = brier;
    }
  } else {
    // class c's gap: sum_b |hits_cb - conf_cb|, with bin n_bins (p == 1.0) counted into the last interval, [1 - 1 / n_bins, 1], as
    // metrics.mce_from_bins does; (n_cb / N) |hits_cb / n_cb - conf_cb / n_cb| = |hits_cb - conf_cb| / N, the division is the reduce kernel's
    const int64_t cb = (int64_t)blockIdx.x - row_blocks;
    const int64_t c = cb * RF_THREADS + threadIdx.x;
    const int nb1 = n_bins + 1;
    const int64_t plane = (int64_t)C * nb1;
    double gap = 0.0;
    if (c < C) {
      const long long* conf = acc + plane + c * nb1;
      const long long* hits = acc + 2 * plane + c * nb1;
      for (int b = 0; b < n_bins; ++b) {
        long long h = hits[b], f = conf[b];
        if (b == n_bins - 1) {
          h += hits[n_bins];
          f += conf[n_bins];
        }
        gap += fabs((double)h - (double)f * (1.0 / 4294967296.0));
      }
    }
    gap = block_tree_sum(gap, s_a);
    if (threadIdx.x == 0) partials[2 * row_blocks + cb] = gap;
  }
}

__global__ void row_scores_reduce_kernel(const double* __restrict__ partials, int64_t row_blocks, int64_t class_blocks, int N, int C,
                                         double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double nll = 0.0, brier = 0.0, gap = 0.0;
  for (int64_t k = 0; k < row_blocks; ++k) {
    nll += partials[2 * k];
    brier += partials[2 * k + 1];
  }
  for (int64_t k = 0; k < class_blocks; ++k) gap += partials[2 * row_blocks + k];
  out[0] = nll / (double)N;
  out[1] = brier / (double)N;
  out[2] = gap / (double)N / (double)C;
  out[3] = (double)N;
}

size_t finish_bytes(int N, int C) {
  if (N < 1 || C < 1) return 0;
  return align256((size_t)(2 * finish_row_blocks(N) + finish_class_blocks(C)) * sizeof(double));
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

size_t clipmi_row_scores_acc_bytes(int C, int n_bins) {
  if (C < 1 || n_bins < 1 || n_bins > RS_MAX_BINS) return 0;
  return (size_t)3 * (size_t)C * (size_t)(n_bins + 1) * sizeof(int64_t);
}

int clipmi_row_scores(const float* rows, int64_t ld, const int64_t* labels, int N, int C, int from_probs, int n_bins, float* row_out, void* class_acc,
                      clipmi_stream_t stream) {
  CLIPMI_REQUIRE(N >= 0 && C >= 1 && ld >= C, CLIPMI_ERR_SHAPE, "row_scores: N=%d C=%d ld=%lld (N >= 0, C >= 1, ld >= C)", N, C, (long long)ld);
  CLIPMI_REQUIRE(n_bins >= 1 && n_bins <= RS_MAX_BINS, CLIPMI_ERR_ARG, "row_scores: n_bins=%d outside 1..%d", n_bins, RS_MAX_BINS);
  CLIPMI_REQUIRE(from_probs == 0 || from_probs == 1, CLIPMI_ERR_ARG, "row_scores: from_probs=%d (0: logits, 1: probabilities)", from_probs);
  CLIPMI_REQUIRE((int64_t)C * (n_bins + 1) <= 0x7fffffff, CLIPMI_ERR_SHAPE, "row_scores: C=%d x (n_bins=%d + 1) bins exceed 2^31 - 1", C, n_bins);
  if (N == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(rows && labels && row_out && class_acc, CLIPMI_ERR_ARG,
                 "row_scores: null pointer (the rows, labels, the row scores and the class bins are required)");
  CLIPMI_REQUIRE((uintptr_t)rows % 4 == 0, CLIPMI_ERR_ARG, "row_scores: the rows must be 4-byte aligned");
  CLIPMI_REQUIRE(((uintptr_t)labels | (uintptr_t)row_out | (uintptr_t)class_acc) % 8 == 0, CLIPMI_ERR_ARG,
                 "row_scores: labels, the row scores and the class bins must be 8-byte aligned");
  const int64_t blocks = ((int64_t)N + RS_ROWS - 1) / RS_ROWS;
  hipStream_t s = (hipStream_t)stream;
  if (from_probs)
    hipLaunchKernelGGL(row_scores_kernel<true>, dim3((unsigned)blocks), dim3(RS_THREADS), 0, s, rows, ld, labels, N, C, n_bins, row_out,
                       (unsigned long long*)class_acc);
  else
    hipLaunchKernelGGL(row_scores_kernel<false>, dim3((unsigned)blocks), dim3(RS_THREADS), 0, s, rows, ld, labels, N, C, n_bins, row_out,
                       (unsigned long long*)class_acc);
  return check_launch("row_scores_kernel");
}

size_t clipmi_row_scores_finish_workspace_bytes(int N, int C) { return finish_bytes(N, C); }

int clipmi_row_scores_finish(const float* row_out, int N, const void* class_acc, int C, int n_bins, double* out, void* workspace, size_t workspace_bytes,
                             clipmi_stream_t stream) {
  CLIPMI_REQUIRE(N >= 1 && C >= 1, CLIPMI_ERR_SHAPE, "row_scores_finish: N=%d C=%d (both >= 1)", N, C);
  CLIPMI_REQUIRE(n_bins >= 1 && n_bins <= RS_MAX_BINS, CLIPMI_ERR_ARG, "row_scores_finish: n_bins=%d outside 1..%d", n_bins, RS_MAX_BINS);
  CLIPMI_REQUIRE((int64_t)C * (n_bins + 1) <= 0x7fffffff, CLIPMI_ERR_SHAPE, "row_scores_finish: C=%d x (n_bins=%d + 1) bins exceed 2^31 - 1", C, n_bins);
  CLIPMI_REQUIRE(row_out && class_acc && out && workspace, CLIPMI_ERR_ARG,
                 "row_scores_finish: null pointer (the row scores, the class bins, out and the workspace are required)");
  CLIPMI_REQUIRE(((uintptr_t)row_out | (uintptr_t)class_acc | (uintptr_t)out) % 8 == 0, CLIPMI_ERR_ARG,
                 "row_scores_finish: the row scores, the class bins and out must be 8-byte aligned");
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "row_scores_finish: the workspace must be 256-byte aligned");
  CLIPMI_REQUIRE(workspace_bytes >= finish_bytes(N, C), CLIPMI_ERR_WORKSPACE, "row_scores_finish: workspace of %zu bytes, %zu needed", workspace_bytes,
                 finish_bytes(N, C));
  const int64_t rb = finish_row_blocks(N), cb = finish_class_blocks(C);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(row_scores_partials_kernel, dim3((unsigned)(rb + cb)), dim3(RF_THREADS), 0, s, row_out, N, (const long long*)class_acc, C, n_bins, rb,
                     (double*)workspace);
  if (int rc = check_launch("row_scores_partials_kernel")) return rc;
  hipLaunchKernelGGL(row_scores_reduce_kernel, dim3(1), dim3(64), 0, s, (const double*)workspace, rb, cb, N, C, (double*)out);
  return check_launch("row_scores_reduce_kernel");
}

}  // extern "C"
