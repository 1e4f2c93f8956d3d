// The class-sharded CoOp-family fit (DESIGN.md "Class-sharded CoOp fit"): what a rank adds around the unsharded step's kernels when the
// classes are split over G ranks and two all-gathers per step move the text features and the context's partial gradients.
//   shard_compact_kernel        the gathered, padded [G, ceil(C / G), E] block -> the full [C, E] matrix, one launch
//   ctx_partial_kernel          a rank's partial context gradient: its own classes' rows in ascending order (ctx_grad_element)
//   ctx_step_gathered_kernel    the G partials added in rank order, 1 / grad_scale, torch.optim.SGD's rule (sgd_element_fma)
//   shard_prograd_*_kernel      ProGrad on the reduced vectors (generic context) or on a rank's own rows (class-specific context): the
//                               float64 dots of one rank, then the G ranks' dots added in rank order, the decision and the step
//   block_rank_mean_kernel      the batch-sharded block fits' reduction: G gathered blocks -> their rank-ordered mean (VPT, MaPLe, PromptSRC)
//   block_step_gathered_kernel  the same mean, 1 / grad_scale and the SGD rule in one launch: the static SGD route of those fits
// With G = 1 every chain is the unsharded kernel's chain (prompt_train.hip): the same additions in the same order, the same partition of
// the float64 dots, the same rules of train_rules.h -- the same bits.  No float atomics, no workgroup waits for another.
#include <cmath>

#include "common.h"
#include "train_rules.h"

namespace clipmi {
namespace {

constexpr int THREADS = 256;

// one thread per element of out [C, E] (shard_owner: train_rules.h): row c is row c - lo of its owner's block of P = ceil(C / G) rows; the padding rows are never read
__global__ __launch_bounds__(THREADS) void shard_compact_kernel(const float* __restrict__ gathered, float* __restrict__ out, int C, int G, int P, int64_t E) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)C * E) return;
  const int c = (int)(idx / E);
  int lo;
  const int r = shard_owner(c, C, G, &lo);
  out[idx] = gathered[((int64_t)r * P + (c - lo)) * E + idx % E];
}

// one thread per element of the partial [n_ctx, D]: the rank's C own classes added in ascending order, unscaled (times 1.0 is exact)
__global__ __launch_bounds__(THREADS) void ctx_partial_kernel(const float* __restrict__ d_embed, float* __restrict__ partial, int C, int L, int D, int n_ctx) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)n_ctx * D) return;
  partial[idx] = ctx_grad_element(d_embed, idx, C, L, D, n_ctx, 0, 1.f);
}

// element idx of the G partials (rank r's at partials + r * stride) added in rank order
__device__ __forceinline__ float rank_sum(const float* __restrict__ partials, int64_t idx, int G, int64_t stride) {
  float s = partials[idx];
  for (int r = 1; r < G; ++r) s += partials[(int64_t)r * stride + idx];
  return s;
}

__global__ __launch_bounds__(THREADS) void ctx_step_gathered_kernel(const float* __restrict__ partials, int G, int64_t stride, float* __restrict__ ctx,
                                                                    float* __restrict__ buf, float* __restrict__ grad_out, int64_t total, float inv_scale,
                                                                    const float* __restrict__ lr, SgdArgs sgd) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= total) return;
  const float g = rank_sum(partials, idx, G, stride) * inv_scale;
  if (grad_out) grad_out[idx] = g;
  if (ctx) sgd_element_fma(ctx, buf, idx, g, *lr, sgd);
}

// ------------------------------------------------------------------------------------------------------------------------- ProGrad
// workspace: per-workgroup partial sums [3, PROGRAD_DOT_BLOCKS] float64 | a [total] | b [total] fp32 -- clipmi_prograd_step's layout
struct DotsWs {
  double* part;
  float *a, *b;
};
inline size_t dots_bytes(int64_t total) { return align256(3 * PROGRAD_DOT_BLOCKS * sizeof(double)) + 2 * align256((size_t)total * 4); }
inline DotsWs dots_carve(void* ws, int64_t total) {
  char* p = static_cast<char*>(ws);
  DotsWs w;
  w.part = reinterpret_cast<double*>(p);
  w.a = reinterpret_cast<float*>(p + align256(3 * PROGRAD_DOT_BLOCKS * sizeof(double)));
  w.b = reinterpret_cast<float*>(p + align256(3 * PROGRAD_DOT_BLOCKS * sizeof(double)) + align256((size_t)total * 4));
  return w;
}

// a and b of `total` elements, kept in the workspace, and every workgroup's float64 partial sums of a.a, b.b, a.b: prograd_dots_kernel's
// grid and order.  per_class: the rank's own rows of its two d_embed (C its own classes); else the rank-ordered sums of the G gathered partials
__global__ __launch_bounds__(256) void shard_prograd_dots_kernel(const float* __restrict__ src_a, const float* __restrict__ src_b, int G, int64_t stride, int C,
                                                                 int L, int D, int n_ctx, int per_class, float inv_scale, int64_t total, DotsWs w) {
  __shared__ double sl[3][256];
  double d[3] = {0.0, 0.0, 0.0};
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const float a = per_class ? ctx_grad_element(src_a, idx, C, L, D, n_ctx, 1, inv_scale) : rank_sum(src_a, idx, G, stride) * inv_scale;
    const float b = per_class ? ctx_grad_element(src_b, idx, C, L, D, n_ctx, 1, inv_scale) : rank_sum(src_b, idx, G, stride) * inv_scale;
    w.a[idx] = a;
    w.b[idx] = b;
    d[0] += (double)a * (double)a;
    d[1] += (double)b * (double)b;
    d[2] += (double)a * (double)b;
  }
  block_sum_f64(d, sl);
  if (threadIdx.x == 0)
    for (int i = 0; i < 3; ++i) w.part[i * PROGRAD_DOT_BLOCKS + blockIdx.x] = d[i];
}

// one workgroup: the n_part partial sums by the tree prograd_step_kernel adds them with -> this rank's dots [3]
__global__ __launch_bounds__(256) void shard_prograd_finish_kernel(DotsWs w, int n_part, double* __restrict__ dots_rank) {
  __shared__ double sl[3][256];
  const int t = threadIdx.x;
  double d[3];
  for (int i = 0; i < 3; ++i) d[i] = t < n_part ? w.part[i * PROGRAD_DOT_BLOCKS + t] : 0.0;
  block_sum_f64(d, sl);
  if (t == 0)
    for (int i = 0; i < 3; ++i) dots_rank[i] = d[i];
}

// one thread per element: the G ranks' dots [G, 3] added in rank order (every thread of every rank forms the same three sums), the
// decision and the element by train_rules.h's ProGrad rule, the SGD rule
__global__ __launch_bounds__(256) void shard_prograd_apply_kernel(DotsWs w, const double* __restrict__ dots_ranks, int G, float lambda, float* __restrict__ ctx,
                                                                  float* __restrict__ buf, float* __restrict__ grad_out, int* __restrict__ projected,
                                                                  double* __restrict__ dots, int64_t total, const float* __restrict__ lr, SgdArgs sgd) {
#pragma clang fp contract(off)
  double aa = dots_ranks[0], bb = dots_ranks[1], ab = dots_ranks[2];
  for (int r = 1; r < G; ++r) {
    aa += dots_ranks[3 * r];
    bb += dots_ranks[3 * r + 1];
    ab += dots_ranks[3 * r + 2];
  }
  const bool project = prograd_projects(aa, bb, ab);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (projected) *projected = project ? 1 : 0;
    if (dots) { dots[0] = aa; dots[1] = bb; dots[2] = ab; }
  }
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const float g = prograd_element(w.a[idx], w.b[idx], project, lambda, ab, bb);
  if (grad_out) grad_out[idx] = g;
  if (ctx) sgd_element_fma(ctx, buf, idx, g, *lr, sgd);
}

// what the stepping entry points ask of the context and the optimiser, before anything is launched
int check_step(const char* who, const float* ctx, const float* buf, const float* lr, int64_t total, float grad_scale, float momentum, float dampening,
               float weight_decay, int nesterov) {
  CLIPMI_REQUIRE(!ctx || lr, CLIPMI_ERR_ARG, "%s: null pointer (a step needs lr)", who);
  CLIPMI_REQUIRE(total >= 1 && total < (1ll << 31) * THREADS, CLIPMI_ERR_SHAPE, "%s: %lld context elements", who, (long long)total);
  CLIPMI_REQUIRE(std::isfinite(grad_scale) && grad_scale > 0.f, CLIPMI_ERR_ARG, "%s: grad_scale=%g (finite, > 0)", who, grad_scale);
  if (int rc = check_sgd(who, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE(!ctx || momentum == 0.f || buf, CLIPMI_ERR_ARG, "%s: null pointer (a momentum needs the buffer)", who);
  return CLIPMI_OK;
}

inline unsigned blocks_of(int64_t total) { return (unsigned)((total + THREADS - 1) / THREADS); }

// ------------------------------------------------------- the batch-sharded block fits (DESIGN.md "Batch-sharded image-tower fits")
// The G ranks' send blocks [scale * gradient | losses], gathered rank-major, become the block every rank agrees on: the rank-ordered sum
// times inv = (float)(1.0 / G).  A streaming kernel: G reads and one write per element, no reuse.  The middle of the block goes through
// 16-byte loads and stores, a capped grid striding over it; the floats in front of the first 16-byte boundary and behind the last whole
// vector go one by one, and so does the whole block when the rows' bases or the output do not share the first row's alignment.
constexpr int MEAN_MAX_BLOCKS = 2048;

__device__ __forceinline__ float4 rank_sum4(const float* __restrict__ partials, int64_t idx, int G, int64_t stride) {
  float4 s = *reinterpret_cast<const float4*>(partials + idx);
#pragma unroll 4
  for (int r = 1; r < G; ++r) {
    const float4 p = *reinterpret_cast<const float4*>(partials + (int64_t)r * stride + idx);
    s.x += p.x;
    s.y += p.y;
    s.z += p.z;
    s.w += p.w;
  }
  return s;
}

// elements [head, head + 4 nvec) as vectors; [0, head) and [head + 4 nvec, total) as scalars (head == total, nvec == 0: all of them)
__global__ __launch_bounds__(THREADS) void block_rank_mean_kernel(const float* __restrict__ gathered, int G, int64_t stride, int64_t total, int64_t head,
                                                                  int64_t nvec, float inv, float* __restrict__ out) {
  const int64_t tid = (int64_t)blockIdx.x * THREADS + threadIdx.x, step = (int64_t)gridDim.x * THREADS;
  for (int64_t v = tid; v < nvec; v += step) {
    const int64_t idx = head + 4 * v;
    float4 s = rank_sum4(gathered, idx, G, stride);
    s.x *= inv;
    s.y *= inv;
    s.z *= inv;
    s.w *= inv;
    *reinterpret_cast<float4*>(out + idx) = s;
  }
  const int64_t tail = head + 4 * nvec, n_scalar = head + (total - tail);
  for (int64_t k = tid; k < n_scalar; k += step) {
    const int64_t idx = k < head ? k : tail + (k - head);
    out[idx] = rank_sum(gathered, idx, G, stride) * inv;
  }
}

// the static SGD route's step from the gathered blocks: the mean as above, 1 / grad_scale, torch.optim.SGD's rule -- with G = 1 the
// arithmetic of a block's own step entry (maple_step_kernel, promptsrc_step_kernel, vpt_step_kernel) behind its scale * gradient
__global__ __launch_bounds__(THREADS) void block_step_gathered_kernel(const float* __restrict__ gathered, int G, int64_t stride, float* __restrict__ params,
                                                                      float* __restrict__ buf, float* __restrict__ grad_out, int64_t total, float inv,
                                                                      float inv_scale, const float* __restrict__ lr, SgdArgs sgd) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= total) return;
  const float g = (rank_sum(gathered, idx, G, stride) * inv) * inv_scale;
  if (grad_out) grad_out[idx] = g;
  if (params) sgd_element_fma(params, buf, idx, g, *lr, sgd);
}

// what both entry points ask of the gathered blocks and of what they write (`out`: total floats), before anything is launched
int check_gathered(const char* who, const float* gathered, int world, size_t stride, size_t total, const float* out) {
  CLIPMI_REQUIRE(gathered, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE((uintptr_t)gathered % 4 == 0 && (uintptr_t)out % 4 == 0, CLIPMI_ERR_ARG, "%s: a pointer is not 4-byte aligned", who);
  CLIPMI_REQUIRE(world >= 1, CLIPMI_ERR_SHAPE, "%s: world=%d (>= 1)", who, world);
  CLIPMI_REQUIRE(total >= 1 && total < ((size_t)1 << 39), CLIPMI_ERR_SHAPE, "%s: total=%zu (in [1, 2^39))", who, total);
  CLIPMI_REQUIRE(stride >= total && stride < ((size_t)1 << 40), CLIPMI_ERR_SHAPE, "%s: stride=%zu below total=%zu (or 2^40 and more)", who, stride, total);
  if (out) {
    const uintptr_t g0 = (uintptr_t)gathered, g1 = g0 + 4 * ((size_t)(world - 1) * stride + total), o0 = (uintptr_t)out, o1 = o0 + 4 * total;
    CLIPMI_REQUIRE(o1 <= g0 || g1 <= o0, CLIPMI_ERR_ARG, "%s: the output overlaps the gathered blocks", who);
  }
  return CLIPMI_OK;
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

int clipmi_shard_compact(const float* gathered, float* out, int C, int G, int64_t E, clipmi_stream_t stream) {
  CLIPMI_REQUIRE(gathered && out, CLIPMI_ERR_ARG, "shard_compact: null pointer");
  CLIPMI_REQUIRE(G >= 1 && C >= G && E >= 1, CLIPMI_ERR_SHAPE, "shard_compact: C=%d G=%d E=%lld (C >= G >= 1)", C, G, (long long)E);
  CLIPMI_REQUIRE((int64_t)C * E < (1ll << 31) * THREADS, CLIPMI_ERR_SHAPE, "shard_compact: C * E too large");
  hipLaunchKernelGGL(shard_compact_kernel, dim3(blocks_of((int64_t)C * E)), dim3(THREADS), 0, (hipStream_t)stream, gathered, out, C, G, (C + G - 1) / G, E);
  return check_launch("shard_compact_kernel");
}

int clipmi_ctx_partial(const float* d_embed, float* partial, int C, int L, int D, int n_ctx, clipmi_stream_t stream) {
  CLIPMI_REQUIRE(d_embed && partial, CLIPMI_ERR_ARG, "ctx_partial: null pointer");
  CLIPMI_REQUIRE(C >= 1 && D >= 1 && n_ctx >= 1 && 1 + n_ctx <= L, CLIPMI_ERR_SHAPE, "ctx_partial: C=%d L=%d D=%d n_ctx=%d", C, L, D, n_ctx);
  hipLaunchKernelGGL(ctx_partial_kernel, dim3(blocks_of((int64_t)n_ctx * D)), dim3(THREADS), 0, (hipStream_t)stream, d_embed, partial, C, L, D, n_ctx);
  return check_launch("ctx_partial_kernel");
}

int clipmi_ctx_step_gathered(const float* partials, int G, int64_t rank_stride, float* ctx, float* buf, float* grad_out, int D, int n_ctx, float grad_scale,
                             const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, clipmi_stream_t stream) {
  CLIPMI_REQUIRE(partials && (ctx || grad_out), CLIPMI_ERR_ARG, "ctx_step_gathered: null pointer (partials and one of ctx, grad_out are required)");
  CLIPMI_REQUIRE(G >= 1 && D >= 1 && n_ctx >= 1, CLIPMI_ERR_SHAPE, "ctx_step_gathered: G=%d D=%d n_ctx=%d", G, D, n_ctx);
  const int64_t total = (int64_t)n_ctx * D;
  CLIPMI_REQUIRE(rank_stride >= total, CLIPMI_ERR_SHAPE, "ctx_step_gathered: rank_stride=%lld below the partial's %lld elements", (long long)rank_stride,
                 (long long)total);
  if (int rc = check_step("ctx_step_gathered", ctx, buf, lr, total, grad_scale, momentum, dampening, weight_decay, nesterov)) return rc;
  hipLaunchKernelGGL(ctx_step_gathered_kernel, dim3(blocks_of(total)), dim3(THREADS), 0, (hipStream_t)stream, partials, G, rank_stride, ctx, buf, grad_out, total,
                     1.f / grad_scale, lr, make_sgd_args(momentum, dampening, weight_decay, nesterov, first_step));
  return check_launch("ctx_step_gathered_kernel");
}

size_t clipmi_shard_prograd_workspace_bytes(int64_t total) { return total >= 1 && total < (1ll << 31) * 256 ? dots_bytes(total) : 0; }

int clipmi_shard_prograd_dots(const float* src_a, const float* src_b, int G, int64_t rank_stride, int C, int L, int D, int n_ctx, int per_class,
                              float grad_scale, double* dots_rank, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  const char* who = "shard_prograd_dots";
  CLIPMI_REQUIRE(src_a && src_b && dots_rank && workspace, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(C >= 1 && D >= 1 && n_ctx >= 1, CLIPMI_ERR_SHAPE, "%s: C=%d D=%d n_ctx=%d", who, C, D, n_ctx);
  const int64_t total = (int64_t)n_ctx * D * (per_class ? C : 1);
  if (per_class)
    CLIPMI_REQUIRE(1 + n_ctx <= L, CLIPMI_ERR_SHAPE, "%s: L=%d n_ctx=%d", who, L, n_ctx);
  else
    CLIPMI_REQUIRE(G >= 1 && rank_stride >= total, CLIPMI_ERR_SHAPE, "%s: G=%d rank_stride=%lld (partials of %lld elements)", who, G, (long long)rank_stride,
                   (long long)total);
  CLIPMI_REQUIRE(std::isfinite(grad_scale) && grad_scale > 0.f, CLIPMI_ERR_ARG, "%s: grad_scale=%g (finite, > 0)", who, grad_scale);
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 256-byte aligned", who);
  const size_t need = clipmi_shard_prograd_workspace_bytes(total);
  CLIPMI_REQUIRE(need > 0 && workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  const DotsWs w = dots_carve(workspace, total);
  const int64_t blocks = (total + 255) / 256;
  const int n_part = (int)(blocks < PROGRAD_DOT_BLOCKS ? blocks : PROGRAD_DOT_BLOCKS);
  hipLaunchKernelGGL(shard_prograd_dots_kernel, dim3((unsigned)n_part), dim3(256), 0, (hipStream_t)stream, src_a, src_b, G, rank_stride, C, L, D, n_ctx,
                     per_class ? 1 : 0, 1.f / grad_scale, total, w);
  if (int rc = check_launch("shard_prograd_dots_kernel")) return rc;
  hipLaunchKernelGGL(shard_prograd_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, w, n_part, dots_rank);
  return check_launch("shard_prograd_finish_kernel");
}

int clipmi_shard_prograd_apply(const double* dots_ranks, int G, float lambda, float* ctx, float* buf, float* grad_out, int* projected, double* dots,
                               int64_t total, const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov,
                               void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  const char* who = "shard_prograd_apply";
  CLIPMI_REQUIRE(dots_ranks && workspace, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(ctx || grad_out || projected || dots, CLIPMI_ERR_ARG, "%s: null pointer (nothing to write)", who);
  CLIPMI_REQUIRE(G >= 1, CLIPMI_ERR_SHAPE, "%s: G=%d", who, G);
  CLIPMI_REQUIRE(std::isfinite(lambda), CLIPMI_ERR_ARG, "%s: lambda=%g (finite)", who, lambda);
  if (int rc = check_step(who, ctx, buf, lr, total, 1.f, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 256-byte aligned", who);
  const size_t need = clipmi_shard_prograd_workspace_bytes(total);
  CLIPMI_REQUIRE(need > 0 && workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  hipLaunchKernelGGL(shard_prograd_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dots_carve(workspace, total), dots_ranks,
                     G, lambda, ctx, buf, grad_out, projected, dots, total, lr, make_sgd_args(momentum, dampening, weight_decay, nesterov, first_step));
  return check_launch("shard_prograd_apply_kernel");
}

int clipmi_block_rank_mean(const float* gathered, int world, size_t stride, size_t total, float* out, clipmi_stream_t stream) {
  const char* who = "block_rank_mean";
  CLIPMI_REQUIRE(out, CLIPMI_ERR_ARG, "%s: null pointer", who);
  if (int rc = check_gathered(who, gathered, world, stride, total, out)) return rc;
  // the vector path needs every row's base and the output on the first row's 16-byte phase; the head reaches the first boundary
  int64_t head = (int64_t)((16 - (uintptr_t)gathered % 16) % 16 / 4), nvec = 0;
  if (stride % 4 == 0 && (uintptr_t)out % 16 == (uintptr_t)gathered % 16 && (int64_t)total >= head + 4)
    nvec = ((int64_t)total - head) / 4;
  else
    head = (int64_t)total;
  const int64_t n_scalar = (int64_t)total - 4 * nvec, work = nvec > n_scalar ? nvec : n_scalar, blocks = (work + THREADS - 1) / THREADS;
  hipLaunchKernelGGL(block_rank_mean_kernel, dim3((unsigned)(blocks < MEAN_MAX_BLOCKS ? blocks : MEAN_MAX_BLOCKS)), dim3(THREADS), 0, (hipStream_t)stream,
                     gathered, world, (int64_t)stride, (int64_t)total, head, nvec, (float)(1.0 / world), out);
  return check_launch("block_rank_mean_kernel");
}

int clipmi_block_step_gathered(const float* gathered, int world, size_t stride, size_t total, float grad_scale, float* params, float* buf, float* grad_out,
                               const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, clipmi_stream_t stream) {
  const char* who = "block_step_gathered";
  CLIPMI_REQUIRE(params || grad_out, CLIPMI_ERR_ARG, "%s: null pointer (one of params, grad_out is required)", who);
  if (int rc = check_gathered(who, gathered, world, stride, total, params)) return rc;
  if (int rc = check_gathered(who, gathered, world, stride, total, buf)) return rc;
  if (int rc = check_gathered(who, gathered, world, stride, total, grad_out)) return rc;
  if (int rc = check_step(who, params, buf, lr, (int64_t)total, grad_scale, momentum, dampening, weight_decay, nesterov)) return rc;
  hipLaunchKernelGGL(block_step_gathered_kernel, dim3(blocks_of((int64_t)total)), dim3(THREADS), 0, (hipStream_t)stream, gathered, world, (int64_t)stride, params,
                     buf, grad_out, (int64_t)total, (float)(1.0 / world), 1.f / grad_scale, lr,
                     make_sgd_args(momentum, dampening, weight_decay, nesterov, first_step));
  return check_launch("block_step_gathered_kernel");
}

}  // extern "C"
