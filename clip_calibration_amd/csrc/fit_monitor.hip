// Per-epoch validation of a fit on the device (reference base_learner.py:41-47, Dassl's after_epoch): score cached validation logits into an
// epoch record, compare with the best epoch so far and keep that epoch's parameters -- without a host read.  DESIGN.md "Fit monitor".
//   val_score_rows_kernel     one wave per row, 64 rows per workgroup: max / arg-max (lowest index on a tie), log-sum-exp, nll, confidence and
//                             its digitize bin; the workgroup's rows are then added in ascending row order into ONE partial record
//   val_score_chunk_kernel    the same per-row code (score_row) on a chunk of rows, one 16-byte result per row: {conf, nll, hit, bin}
//   cocoop_val_rows_kernel    CoCoOp: one workgroup per image forms its C per-pair logits in LDS (pair_logit, cocoop_tail.h) and scores them
//   val_score_partials_kernel the 64-row partial records from the row results, in val_score_rows_kernel's order
//   val_score_reduce_kernel   ONE workgroup: one thread per field of the record adds the partial records in ascending workgroup order
//   best_decide_kernel        ONE workgroup: strictly better than the best so far?  updates the best block, writes the decision word
//   best_copy_kernel          grid-stride copy of params into best_params, only when the decision word says "better"
// The record (8-byte aligned, 16 + 16 (n_bins + 1) bytes): {int32 n, int32 correct, float64 nll_sum, bins[n_bins + 1] x {int32 count,
// int32 hits, float64 conf_sum}}; bin b is metrics.digitize_bins' bin b, so bin n_bins -- the last -- holds conf == 1.0 (and a NaN).
// Plain vector code, integer counts and float64 sums added in a fixed order, no atomics: the same inputs give the same bits.  The
// partition into workgroups depends on N alone.
#include <cmath>
#include <cstdint>

#include "cocoop_tail.h"
#include "common.h"

namespace clipmi {
namespace {

constexpr int VS_THREADS = 256;
constexpr int VS_WAVE = 64;
constexpr int VS_WAVES = VS_THREADS / VS_WAVE;
constexpr int VS_ROWS = 64;        // rows per workgroup: the partition of the rows depends on N alone
constexpr int VS_MAX_BINS = 64;
constexpr int COCOOP_VAL_MAX_C = 16384;   // cocoop_val_rows_kernel keeps one image's C fp32 logits in LDS: 64 KiB at most
constexpr int COPY_THREADS = 256;
constexpr int COPY_MAX_BLOCKS = 1024;

struct RecordHead {   // the first 16 bytes of a record
  int32_t n, correct;
  double nll_sum;
};
struct RecordBin {
  int32_t count, hits;
  double conf_sum;
};
struct BestBlock {    // 24 bytes
  int32_t best_epoch, best_correct;
  double best_nll_sum;
  int32_t epochs_seen, pad;
};
static_assert(sizeof(RecordHead) == 16 && sizeof(RecordBin) == 16 && sizeof(BestBlock) == 24, "record layout");

__host__ __device__ inline size_t record_bytes(int n_bins) { return sizeof(RecordHead) + sizeof(RecordBin) * (size_t)(n_bins + 1); }
inline int64_t score_blocks(int N) { return ((int64_t)N + VS_ROWS - 1) / VS_ROWS; }

// numpy.searchsorted(numpy.linspace(0, 1, n_bins + 1), conf, side="right") - 1 for a conf in [0, 1] or a NaN: the edges are i * (1 / n_bins)
// in float64 with the last one exactly 1, as linspace forms them; a NaN sorts behind every edge
__device__ inline double bin_edge(int i, int n_bins, double step) { return i == n_bins ? 1.0 : (double)i * step; }

__device__ inline int conf_bin(float conf, int n_bins) {
  if (!(conf == conf)) return n_bins;
  const double c = (double)conf, step = 1.0 / (double)n_bins;
  int b = (int)(c * (double)n_bins);
  b = b < 0 ? 0 : (b > n_bins ? n_bins : b);
  while (b < n_bins && bin_edge(b + 1, n_bins, step) <= c) ++b;
  while (b > 0 && bin_edge(b, n_bins, step) > c) --b;
  return b;
}

struct RowResult {    // 16 bytes: what clipmi_val_score_rows writes per row
  float conf, nll;
  int32_t hit, bin;
};
static_assert(sizeof(RowResult) == 16, "row result layout");

// One wave scores one row `z` of C logits against the label y; every lane calls it, lane 0's return value is the row's result.
__device__ inline RowResult score_row(const float* __restrict__ z, int64_t y, int C, int n_bins, int lane) {
  // the maximum and its lowest index; a lane walks its columns in ascending order, so `>` keeps the first of equals
  float m = -INFINITY;
  int idx = INT32_MAX, has_nan = 0;
  for (int c = lane; c < C; c += VS_WAVE) {
    const float v = z[c];
    has_nan |= v != v;
    if (v > m || idx == INT32_MAX) {
      m = v;
      idx = c;
    }
  }
  for (int off = 1; off < VS_WAVE; off <<= 1) {
    const float om = __shfl_xor(m, off, VS_WAVE);
    const int oi = __shfl_xor(idx, off, VS_WAVE);
    has_nan |= __shfl_xor(has_nan, off, VS_WAVE);
    if (om > m || (om == m && oi < idx)) {
      m = om;
      idx = oi;
    }
  }
  float sum = 0.f;
  for (int c = lane; c < C; c += VS_WAVE) sum += expf(z[c] - m);
  for (int off = 1; off < VS_WAVE; off <<= 1) sum += __shfl_xor(sum, off, VS_WAVE);   // a + b == b + a: every lane holds the same bits
  RowResult res{0.f, 0.f, 0, 0};
  if (lane == 0) {
    const bool in_range = y >= 0 && y < C;   // a label outside [0, C) is never used as an address
    // lse = m + log(sum), nll = lse - z[y] and conf = exp(m - lse), with the maximum cancelled before the rounding: log(sum) - (z[y] - m), 1 / sum
    const float log_sum = logf(sum);
    float nll = in_range ? log_sum - (z[in_range ? y : 0] - m) : NAN;
    float conf = 1.f / sum;
    int hit = in_range && (int64_t)idx == y;
    if (has_nan) {   // a row that holds a NaN counts as wrong, and its NaN reaches nll_sum
      nll = NAN;
      conf = NAN;
      hit = 0;
    }
    res = RowResult{conf, nll, hit, conf_bin(conf, n_bins)};
  }
  return res;
}

__global__ __launch_bounds__(VS_THREADS) void val_score_rows_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels, int N,
                                                                    int C, int n_bins, char* __restrict__ partials) {
  __shared__ float s_conf[VS_ROWS];
  __shared__ float s_nll[VS_ROWS];
  __shared__ int s_bin[VS_ROWS];   // -1: no such row
  __shared__ int s_hit[VS_ROWS];
  const int wave = threadIdx.x / VS_WAVE, lane = threadIdx.x % VS_WAVE;
  const int64_t row0 = (int64_t)blockIdx.x * VS_ROWS;
  for (int r = wave; r < VS_ROWS; r += VS_WAVES) {
    const int64_t row = row0 + r;
    if (row >= N) {   // the same for every lane of the wave
      if (lane == 0) s_bin[r] = -1;
      continue;
    }
    const RowResult res = score_row(logits + row * ld, lane == 0 ? labels[row] : 0, C, n_bins, lane);
    if (lane == 0) {
      s_conf[r] = res.conf;
      s_nll[r] = res.nll;
      s_hit[r] = res.hit;
      s_bin[r] = res.bin;
    }
  }
  __syncthreads();
  // the workgroup's partial record: thread 0 the head, thread 1 + b bin b, each over the rows in ascending order
  char* out = partials + (size_t)blockIdx.x * record_bytes(n_bins);
  if (threadIdx.x == 0) {
    RecordHead h{0, 0, 0.0};
    for (int r = 0; r < VS_ROWS; ++r) {
      if (s_bin[r] < 0) continue;
      h.n += 1;
      h.correct += s_hit[r];
      h.nll_sum += (double)s_nll[r];
    }
    *(RecordHead*)out = h;
  } else if ((int)threadIdx.x <= n_bins + 1) {
    const int b = (int)threadIdx.x - 1;
    RecordBin q{0, 0, 0.0};
    for (int r = 0; r < VS_ROWS; ++r) {
      if (s_bin[r] != b) continue;
      q.count += 1;
      q.hits += s_hit[r];
      q.conf_sum += (double)s_conf[r];
    }
    ((RecordBin*)(out + sizeof(RecordHead)))[b] = q;
  }
}

// A chunk of rows: one wave per row, VS_WAVES rows per workgroup; each row's result goes out as it is, nothing is added here
__global__ __launch_bounds__(VS_THREADS) void val_score_chunk_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                                     int rows, int C, int n_bins, RowResult* __restrict__ row_results) {
  const int wave = threadIdx.x / VS_WAVE, lane = threadIdx.x % VS_WAVE;
  const int64_t row = (int64_t)blockIdx.x * VS_WAVES + wave;
  if (row >= rows) return;   // the same for every lane of the wave
  const RowResult res = score_row(logits + row * ld, lane == 0 ? labels[row] : 0, C, n_bins, lane);
  if (lane == 0) row_results[row] = res;
}

// CoCoOp's validation rows: one workgroup per image b.  Its C text features txt[b, c, :] (raw tower outputs) are normalised and dotted with the
// image's unit feature by pair_logit, one wave per class, into C fp32 logits in LDS -- per_image_logits_kernel's bits --, and wave 0 scores
// them with score_row; the [Bv, C] logits never go to memory
__global__ __launch_bounds__(VS_THREADS) void cocoop_val_rows_kernel(const float* __restrict__ img_n, const float* __restrict__ txt, float scale,
                                                                     const int64_t* __restrict__ labels, int C, int E, int n_bins,
                                                                     RowResult* __restrict__ row_results) {
  extern __shared__ float s_z[];   // [C]
  const int wave = threadIdx.x / VS_WAVE, lane = threadIdx.x % VS_WAVE;
  const int64_t b = blockIdx.x;
  const float* f = img_n + b * E;
  for (int c = wave; c < C; c += VS_WAVES) {
    float inv;
    const float z = pair_logit(f, txt + (b * C + c) * E, scale, E, lane, &inv);
    if (lane == 0) s_z[c] = z;
  }
  __syncthreads();
  if (wave != 0) return;
  const RowResult res = score_row(s_z, lane == 0 ? labels[b] : 0, C, n_bins, lane);
  if (lane == 0) row_results[b] = res;
}

// The partial record of rows [64 k, 64 k + 64) of the N row results, added as val_score_rows_kernel adds its workgroup's rows: thread 0 the
// head, thread 1 + b bin b, each over the rows in ascending order
__global__ __launch_bounds__(VS_THREADS) void val_score_partials_kernel(const RowResult* __restrict__ row_results, int N, int n_bins,
                                                                        char* __restrict__ partials) {
  __shared__ RowResult s_row[VS_ROWS];
  const int64_t row0 = (int64_t)blockIdx.x * VS_ROWS;
  const int have = (int)((int64_t)N - row0 < VS_ROWS ? (int64_t)N - row0 : VS_ROWS);
  if ((int)threadIdx.x < have) s_row[threadIdx.x] = row_results[row0 + threadIdx.x];
  __syncthreads();
  char* out = partials + (size_t)blockIdx.x * record_bytes(n_bins);
  if (threadIdx.x == 0) {
    RecordHead h{0, 0, 0.0};
    for (int r = 0; r < have; ++r) {
      h.n += 1;
      h.correct += s_row[r].hit;
      h.nll_sum += (double)s_row[r].nll;
    }
    *(RecordHead*)out = h;
  } else if ((int)threadIdx.x <= n_bins + 1) {
    const int b = (int)threadIdx.x - 1;
    RecordBin q{0, 0, 0.0};
    for (int r = 0; r < have; ++r) {
      if (s_row[r].bin != b) continue;
      q.count += 1;
      q.hits += s_row[r].hit;
      q.conf_sum += (double)s_row[r].conf;
    }
    ((RecordBin*)(out + sizeof(RecordHead)))[b] = q;
  }
}

// grid (1): thread 0 adds the heads, thread 1 + b the bins b, over the partial records in ascending workgroup order
__global__ __launch_bounds__(VS_THREADS) void val_score_reduce_kernel(const char* __restrict__ partials, int64_t blocks, int n_bins, char* __restrict__ record) {
  const size_t rb = record_bytes(n_bins);
  if (threadIdx.x == 0) {
    RecordHead h{0, 0, 0.0};
    for (int64_t k = 0; k < blocks; ++k) {
      const RecordHead p = *(const RecordHead*)(partials + k * rb);
      h.n += p.n;
      h.correct += p.correct;
      h.nll_sum += p.nll_sum;
    }
    *(RecordHead*)record = h;
  } else if ((int)threadIdx.x <= n_bins + 1) {
    const int b = (int)threadIdx.x - 1;
    RecordBin q{0, 0, 0.0};
    for (int64_t k = 0; k < blocks; ++k) {
      const RecordBin p = ((const RecordBin*)(partials + k * rb + sizeof(RecordHead)))[b];
      q.count += p.count;
      q.hits += p.hits;
      q.conf_sum += p.conf_sum;
    }
    ((RecordBin*)(record + sizeof(RecordHead)))[b] = q;
  }
}

// grid (1).  Better iff strictly better (Dassl's `curr_result > best_result`): accuracy -- correct > best_correct, which a block that starts at
// -1 grants the first epoch; nll -- a finite nll_sum below best_nll_sum, which starts at +inf, so a non-finite epoch is never taken
__global__ void best_decide_kernel(const char* __restrict__ record, BestBlock* __restrict__ best, int criterion, int epoch, int32_t* __restrict__ decision) {
  if (threadIdx.x != 0) return;
  const RecordHead h = *(const RecordHead*)record;
  const bool better = criterion == 0 ? h.correct > best->best_correct : (isfinite(h.nll_sum) && h.nll_sum < best->best_nll_sum);
  if (better) {
    best->best_epoch = epoch;
    best->best_correct = h.correct;
    best->best_nll_sum = h.nll_sum;
  }
  best->epochs_seen += 1;
  decision[0] = better ? 1 : 0;
}

__global__ __launch_bounds__(COPY_THREADS) void best_copy_kernel(const int32_t* __restrict__ decision, const float* __restrict__ params,
                                                                 float* __restrict__ best_params, int64_t n) {
  if (!decision[0]) return;   // the same for every thread of the launch
  const int64_t stride = (int64_t)gridDim.x * COPY_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * COPY_THREADS + threadIdx.x; i < n; i += stride) best_params[i] = params[i];
}

size_t val_score_bytes(int N, int n_bins) {
  if (N < 1 || n_bins < 1 || n_bins > VS_MAX_BINS) return 0;
  return ((size_t)score_blocks(N) * record_bytes(n_bins) + 255) / 256 * 256;
}

constexpr size_t BEST_SELECT_BYTES = 256;   // the decision word

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

size_t clipmi_val_score_workspace_bytes(int N, int n_bins) { return val_score_bytes(N, n_bins); }

int clipmi_val_score(const float* logits, int64_t ld, const int64_t* labels, int N, int C, int n_bins, void* record, void* workspace, size_t workspace_bytes,
                     clipmi_stream_t stream) {
  CLIPMI_REQUIRE(logits && labels && record && workspace, CLIPMI_ERR_ARG, "val_score: null pointer (logits, labels, the record and the workspace are required)");
  CLIPMI_REQUIRE((uintptr_t)logits % 16 == 0, CLIPMI_ERR_ARG, "val_score: logits must be 16-byte aligned");
  CLIPMI_REQUIRE(((uintptr_t)labels | (uintptr_t)record) % 8 == 0, CLIPMI_ERR_ARG, "val_score: labels and the record must be 8-byte aligned");
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "val_score: the workspace must be 256-byte aligned");
  CLIPMI_REQUIRE(N >= 1 && C >= 1 && ld >= C, CLIPMI_ERR_SHAPE, "val_score: N=%d C=%d ld=%lld (N, C >= 1, ld >= C)", N, C, (long long)ld);
  CLIPMI_REQUIRE(n_bins >= 1 && n_bins <= VS_MAX_BINS, CLIPMI_ERR_ARG, "val_score: n_bins=%d outside 1..%d", n_bins, VS_MAX_BINS);
  CLIPMI_REQUIRE(workspace_bytes >= val_score_bytes(N, n_bins), CLIPMI_ERR_WORKSPACE, "val_score: workspace of %zu bytes, %zu needed", workspace_bytes,
                 val_score_bytes(N, n_bins));
  const int64_t blocks = score_blocks(N);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(val_score_rows_kernel, dim3((unsigned)blocks), dim3(VS_THREADS), 0, s, logits, ld, labels, N, C, n_bins, (char*)workspace);
  if (int rc = check_launch("val_score_rows_kernel")) return rc;
  hipLaunchKernelGGL(val_score_reduce_kernel, dim3(1), dim3(VS_THREADS), 0, s, (const char*)workspace, blocks, n_bins, (char*)record);
  return check_launch("val_score_reduce_kernel");
}

int clipmi_val_score_rows(const float* logits, int64_t ld, const int64_t* labels, int rows, int C, int n_bins, void* row_results, clipmi_stream_t stream) {
  CLIPMI_REQUIRE(logits && labels && row_results, CLIPMI_ERR_ARG, "val_score_rows: null pointer (logits, labels and the row results are required)");
  CLIPMI_REQUIRE(((uintptr_t)logits | (uintptr_t)row_results) % 16 == 0, CLIPMI_ERR_ARG, "val_score_rows: logits and the row results must be 16-byte aligned");
  CLIPMI_REQUIRE((uintptr_t)labels % 8 == 0, CLIPMI_ERR_ARG, "val_score_rows: labels must be 8-byte aligned");
  CLIPMI_REQUIRE(rows >= 1 && C >= 1 && ld >= C, CLIPMI_ERR_SHAPE, "val_score_rows: rows=%d C=%d ld=%lld (rows, C >= 1, ld >= C)", rows, C, (long long)ld);
  CLIPMI_REQUIRE(n_bins >= 1 && n_bins <= VS_MAX_BINS, CLIPMI_ERR_ARG, "val_score_rows: n_bins=%d outside 1..%d", n_bins, VS_MAX_BINS);
  const int64_t blocks = ((int64_t)rows + VS_WAVES - 1) / VS_WAVES;
  hipLaunchKernelGGL(val_score_chunk_kernel, dim3((unsigned)blocks), dim3(VS_THREADS), 0, (hipStream_t)stream, logits, ld, labels, rows, C, n_bins,
                     (RowResult*)row_results);
  return check_launch("val_score_chunk_kernel");
}

int clipmi_cocoop_val_rows(const float* img_n, const float* txt, float scale, const int64_t* labels, int Bv, int C, int E, int n_bins, void* row_results,
                           clipmi_stream_t stream) {
  CLIPMI_REQUIRE(img_n && txt && labels && row_results, CLIPMI_ERR_ARG,
                 "cocoop_val_rows: null pointer (the image features, the text features, labels and the row results are required)");
  CLIPMI_REQUIRE(((uintptr_t)img_n | (uintptr_t)txt) % 4 == 0, CLIPMI_ERR_ARG, "cocoop_val_rows: fp32 arrays must be 4-byte aligned");
  CLIPMI_REQUIRE((uintptr_t)row_results % 16 == 0, CLIPMI_ERR_ARG, "cocoop_val_rows: the row results must be 16-byte aligned");
  CLIPMI_REQUIRE((uintptr_t)labels % 8 == 0, CLIPMI_ERR_ARG, "cocoop_val_rows: labels must be 8-byte aligned");
  CLIPMI_REQUIRE(Bv >= 1 && C >= 1 && C <= COCOOP_VAL_MAX_C && E >= 1, CLIPMI_ERR_SHAPE, "cocoop_val_rows: Bv=%d C=%d E=%d (Bv, E >= 1, C in 1..%d)", Bv, C, E,
                 COCOOP_VAL_MAX_C);
  CLIPMI_REQUIRE(n_bins >= 1 && n_bins <= VS_MAX_BINS, CLIPMI_ERR_ARG, "cocoop_val_rows: n_bins=%d outside 1..%d", n_bins, VS_MAX_BINS);
  CLIPMI_REQUIRE(std::isfinite(scale), CLIPMI_ERR_ARG, "cocoop_val_rows: scale=%g (finite)", scale);
  hipLaunchKernelGGL(cocoop_val_rows_kernel, dim3((unsigned)Bv), dim3(VS_THREADS), (size_t)C * sizeof(float), (hipStream_t)stream, img_n, txt, scale, labels, C,
                     E, n_bins, (RowResult*)row_results);
  return check_launch("cocoop_val_rows_kernel");
}

size_t clipmi_val_score_finish_workspace_bytes(int N, int n_bins) { return val_score_bytes(N, n_bins); }

int clipmi_val_score_finish(const void* row_results, int N, int n_bins, void* record, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  CLIPMI_REQUIRE(row_results && record && workspace, CLIPMI_ERR_ARG,
                 "val_score_finish: null pointer (the row results, the record and the workspace are required)");
  CLIPMI_REQUIRE((uintptr_t)row_results % 16 == 0, CLIPMI_ERR_ARG, "val_score_finish: the row results must be 16-byte aligned");
  CLIPMI_REQUIRE((uintptr_t)record % 8 == 0, CLIPMI_ERR_ARG, "val_score_finish: the record must be 8-byte aligned");
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "val_score_finish: the workspace must be 256-byte aligned");
  CLIPMI_REQUIRE(N >= 1, CLIPMI_ERR_SHAPE, "val_score_finish: N=%d (>= 1)", N);
  CLIPMI_REQUIRE(n_bins >= 1 && n_bins <= VS_MAX_BINS, CLIPMI_ERR_ARG, "val_score_finish: n_bins=%d outside 1..%d", n_bins, VS_MAX_BINS);
  CLIPMI_REQUIRE(workspace_bytes >= val_score_bytes(N, n_bins), CLIPMI_ERR_WORKSPACE, "val_score_finish: workspace of %zu bytes, %zu needed", workspace_bytes,
                 val_score_bytes(N, n_bins));
  const int64_t blocks = score_blocks(N);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(val_score_partials_kernel, dim3((unsigned)blocks), dim3(VS_THREADS), 0, s, (const RowResult*)row_results, N, n_bins, (char*)workspace);
  if (int rc = check_launch("val_score_partials_kernel")) return rc;
  hipLaunchKernelGGL(val_score_reduce_kernel, dim3(1), dim3(VS_THREADS), 0, s, (const char*)workspace, blocks, n_bins, (char*)record);
  return check_launch("val_score_reduce_kernel");
}

size_t clipmi_best_select_workspace_bytes(int64_t n_floats) { return n_floats >= 1 ? BEST_SELECT_BYTES : 0; }

int clipmi_best_select(const void* record, void* best_block, int criterion, int epoch, const float* params, float* best_params, int64_t n_floats,
                       void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  CLIPMI_REQUIRE(record && best_block && params && best_params && workspace, CLIPMI_ERR_ARG,
                 "best_select: null pointer (the record, the best block, params, best_params and the workspace are required)");
  CLIPMI_REQUIRE(((uintptr_t)record | (uintptr_t)best_block) % 8 == 0, CLIPMI_ERR_ARG, "best_select: the record and the best block must be 8-byte aligned");
  CLIPMI_REQUIRE(((uintptr_t)params | (uintptr_t)best_params) % 16 == 0, CLIPMI_ERR_ARG, "best_select: params and best_params must be 16-byte aligned");
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "best_select: the workspace must be 256-byte aligned");
  CLIPMI_REQUIRE(criterion == 0 || criterion == 1, CLIPMI_ERR_ARG, "best_select: criterion=%d (0: accuracy, 1: nll)", criterion);
  CLIPMI_REQUIRE(epoch >= 0, CLIPMI_ERR_ARG, "best_select: epoch=%d (>= 0)", epoch);
  CLIPMI_REQUIRE(n_floats >= 1, CLIPMI_ERR_SHAPE, "best_select: n_floats=%lld (>= 1)", (long long)n_floats);
  CLIPMI_REQUIRE(workspace_bytes >= BEST_SELECT_BYTES, CLIPMI_ERR_WORKSPACE, "best_select: workspace of %zu bytes, %zu needed", workspace_bytes,
                 BEST_SELECT_BYTES);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(best_decide_kernel, dim3(1), dim3(64), 0, s, (const char*)record, (BestBlock*)best_block, criterion, epoch, (int32_t*)workspace);
  if (int rc = check_launch("best_decide_kernel")) return rc;
  const int64_t want = (n_floats + COPY_THREADS - 1) / COPY_THREADS;
  hipLaunchKernelGGL(best_copy_kernel, dim3((unsigned)(want < COPY_MAX_BLOCKS ? want : COPY_MAX_BLOCKS)), dim3(COPY_THREADS), 0, s,
                     (const int32_t*)workspace, params, best_params, n_floats);
  return check_launch("best_copy_kernel");
}

}  // extern "C"
