// The frozen text tower in training mode (reference trainers/classification/coop.py:70-144, 192-222, 282-309): its training forward with a
// stash and its backward down to the input embeddings, which CoOp's, KgCoOp's and ProGrad's steps (prompt_train.hip) put between their loss
// head and their context step.  DESIGN.md "CoOp fit" has the data flow, the stash and the rounding points.
//
// Frozen weights: no weight gradient exists and every Linear's backward is dX = dY W -- the forward's fp16 MFMA GEMM (launch_gemm) on a
// transposed copy of the weight.  New here:
//   ln_backward_kernel         LayerNorm's backward from the saved fp32 rows; adds into the fp32 gradient stream and writes its fp16 copy
//   quickgelu_forward_kernel   QuickGELU of the saved (rounded) c_fc pre-activation
//   quickgelu_backward_kernel  its derivative times the upstream gradient
//   (attention_backward_kernel, causal attention's backward on the matrix cores, lives with the other attention kernels: attention.hip)
//   coop_embed_kernel          prompts with the fp32 context rows in place, plus the positional embedding
//   operand_stats_kernel       zeros, subnormals and the largest magnitude of the fp16 dgrad-GEMM operands
//   deep_splice_kernel         MaPLe's deep text prompts: rows 1 .. n_ctx of every prompt overwritten in the stash, rounded through fp16
// No float atomics and no workgroup waits for another: the same inputs give the same bits.
#include <cmath>

#include "common.h"
#include "model.h"

namespace clipmi {
namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

__device__ __forceinline__ f32x4 load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 load4(const half_t* p) {
  const f16x4 h = *reinterpret_cast<const f16x4*>(p);
  return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}

// ---------------------------------------------------------------------------------------------------------------- LayerNorm backward
// One wave per row, four rows per workgroup; lane l owns the elements 4 l + 256 i .. + 3.  Four passes over the row (it stays in the
// caches): mean, variance about the mean, the two sums of the backward, the result.
template <typename DY>
__global__ __launch_bounds__(THREADS) void ln_backward_kernel(const float* __restrict__ x, int64_t x_stride, const int32_t* __restrict__ row_idx,
                                                              const float* __restrict__ gamma, const DY* __restrict__ dy, float* __restrict__ g,
                                                              half_t* __restrict__ g16, int rows, int D, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * WAVES + wave;
  if (r >= rows) return;   // no barrier below
  const int64_t src = row_idx ? row_idx[r] : r;
  const float* xr = x + src * x_stride;
  const DY* dyr = dy + r * D;
  float* gr = g + src * D;
  const float inv_d = 1.f / (float)D;
  float s = 0.f;
  for (int e = 4 * lane; e < D; e += 256) {
    const f32x4 v = load4(xr + e);
    s += (v[0] + v[1]) + (v[2] + v[3]);
  }
  const float mean = wave_sum(s) * inv_d;
  s = 0.f;
  for (int e = 4 * lane; e < D; e += 256) {
    const f32x4 v = load4(xr + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) s = fmaf(v[j] - mean, v[j] - mean, s);
  }
  const float rstd = rsqrtf(wave_sum(s) * inv_d + eps);
  float s1 = 0.f, s2 = 0.f;
  for (int e = 4 * lane; e < D; e += 256) {
    const f32x4 v = load4(xr + e), gm = load4(gamma + e), d = load4(dyr + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float t = d[j] * gm[j];
      s1 += t;
      s2 = fmaf(t, (v[j] - mean) * rstd, s2);
    }
  }
  const float m1 = wave_sum(s1) * inv_d, m2 = wave_sum(s2) * inv_d;
  for (int e = 4 * lane; e < D; e += 256) {
    const f32x4 v = load4(xr + e), gm = load4(gamma + e), d = load4(dyr + e);
    f32x4 acc = load4(gr + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += rstd * ((d[j] * gm[j] - m1) - (v[j] - mean) * rstd * m2);
    *reinterpret_cast<f32x4*>(gr + e) = acc;
    if (g16) *reinterpret_cast<f16x4*>(g16 + src * D + e) = f16x4{(half_t)acc[0], (half_t)acc[1], (half_t)acc[2], (half_t)acc[3]};
  }
}

}  // namespace

int launch_ln_backward(const float* x, int64_t x_stride, const int32_t* row_idx, const float* gamma, const void* dy, int dy_dtype, float* g,
                       half_t* g16, int64_t rows, int D, float eps, hipStream_t s) {
  if (rows == 0) return CLIPMI_OK;
  const unsigned grid = (unsigned)((rows + WAVES - 1) / WAVES);
  if (dy_dtype == CLIPMI_F32)
    hipLaunchKernelGGL(ln_backward_kernel<float>, dim3(grid), dim3(THREADS), 0, s, x, x_stride, row_idx, gamma, (const float*)dy, g, g16, (int)rows, D, eps);
  else
    hipLaunchKernelGGL(ln_backward_kernel<half_t>, dim3(grid), dim3(THREADS), 0, s, x, x_stride, row_idx, gamma, (const half_t*)dy, g, g16, (int)rows, D, eps);
  return check_launch("ln_backward_kernel");
}

namespace {

// ------------------------------------------------------------------------------------------------------------------------ QuickGELU
__device__ __forceinline__ float sigmoid1702(float h) { return 1.f / (1.f + __expf(-1.702f * h)); }

// a = fp16(h sigmoid(1.702 h)) from the ROUNDED pre-activation h (clip/model.py:162-164); n % 8 == 0 is not required
__global__ __launch_bounds__(THREADS) void quickgelu_forward_kernel(const half_t* __restrict__ h, half_t* __restrict__ a, int64_t n) {
  const int64_t i = ((int64_t)blockIdx.x * THREADS + threadIdx.x) * 8;
  if (i + 8 <= n) {
    const f16x8 v = *reinterpret_cast<const f16x8*>(h + i);
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)((float)v[j] * sigmoid1702((float)v[j]));
    *reinterpret_cast<f16x8*>(a + i) = o;
  } else {
    for (int64_t k = i; k < n; ++k) a[k] = (half_t)((float)h[k] * sigmoid1702((float)h[k]));
  }
}

__device__ __forceinline__ half_t gelu_grad(half_t h16, half_t da16) {
  const float h = (float)h16, s = sigmoid1702(h);
  return (half_t)((float)da16 * (s + 1.702f * h * s * (1.f - s)));
}
__global__ __launch_bounds__(THREADS) void quickgelu_backward_kernel(const half_t* __restrict__ h, const half_t* d_a, half_t* d_h, int64_t n) {
  const int64_t i = ((int64_t)blockIdx.x * THREADS + threadIdx.x) * 8;
  if (i + 8 <= n) {
    const f16x8 v = *reinterpret_cast<const f16x8*>(h + i), d = *reinterpret_cast<const f16x8*>(d_a + i);
    f16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = gelu_grad(v[j], d[j]);
    *reinterpret_cast<f16x8*>(d_h + i) = o;
  } else {
    for (int64_t k = i; k < n; ++k) d_h[k] = gelu_grad(h[k], d_a[k]);
  }
}

inline unsigned grid8(int64_t n) { return (unsigned)((n + 8 * THREADS - 1) / (8 * THREADS)); }

}  // namespace

int launch_quickgelu_forward(const half_t* h, half_t* a, int64_t n, hipStream_t s) {
  if (n == 0) return CLIPMI_OK;
  hipLaunchKernelGGL(quickgelu_forward_kernel, dim3(grid8(n)), dim3(THREADS), 0, s, h, a, n);
  return check_launch("quickgelu_forward_kernel");
}
int launch_quickgelu_backward(const half_t* h, const half_t* d_a, half_t* d_h, int64_t n, hipStream_t s) {
  if (n == 0) return CLIPMI_OK;
  hipLaunchKernelGGL(quickgelu_backward_kernel, dim3(grid8(n)), dim3(THREADS), 0, s, h, d_a, d_h, n);
  return check_launch("quickgelu_backward_kernel");
}

namespace {

// ------------------------------------------------------------------------------------------------------------- embedding, statistics
// xres[c, l, :] = (ctx && 1 <= l <= n_ctx ? ctx[(per_class ? c : 0), l - 1, :] : float(prompts[c, l, :])) + pos[l, :],  l < L of src_L rows
template <typename T>
__global__ __launch_bounds__(THREADS) void coop_embed_kernel(const T* __restrict__ prompts, const float* __restrict__ ctx, const float* __restrict__ pos,
                                                             float* __restrict__ xres, int C, int L, int src_L, int D, int n_ctx, int per_class) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)C * L * D) return;
  const int d = (int)(idx % D), l = (int)((idx / D) % L);
  const int64_t c = idx / ((int64_t)D * L);
  float v;
  if (ctx && l >= 1 && l <= n_ctx) v = ctx[((per_class ? c * n_ctx : 0) + (l - 1)) * D + d];
  else v = (float)prompts[(c * src_L + l) * D + d];
  xres[idx] = v + pos[(int64_t)l * D + d];
}

// x[c, 1 + j, :] = float(half(deep[j, :])) for every prompt c: the reference's .half() of a deep prompt, no positional embedding
// (clip/model.py:313-328).  In place in the stash slab, so the stash holds what the block read.
__global__ __launch_bounds__(THREADS) void deep_splice_kernel(float* __restrict__ x, const float* __restrict__ deep, int C, int L, int D, int n_ctx) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)C * n_ctx * D) return;
  const int d = (int)(idx % D), j = (int)((idx / D) % n_ctx);
  const int64_t c = idx / ((int64_t)D * n_ctx);
  x[(c * L + 1 + j) * D + d] = (float)(half_t)deep[(int64_t)j * D + d];
}

// {elements, exact zeros, fp16 subnormals, largest magnitude (fp16 bits)} of an fp16 operand, added into stats (integer atomics)
__global__ __launch_bounds__(THREADS) void operand_stats_kernel(const uint16_t* __restrict__ x, int64_t n, unsigned long long* __restrict__ stats) {
  __shared__ unsigned long long sz[WAVES], ss[WAVES];
  __shared__ unsigned int sm[WAVES];
  unsigned long long zeros = 0, subs = 0;
  unsigned int mx = 0;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
    const unsigned int a = x[i] & 0x7fffu;
    zeros += a == 0;
    subs += a != 0 && a < 0x0400u;
    if (a <= 0x7c00u && a > mx) mx = a;
    if (a > 0x7c00u) mx = 0x7fffu;   // a NaN reports as the largest pattern
  }
  for (int o = 32; o > 0; o >>= 1) {
    zeros += __shfl_xor(zeros, o);
    subs += __shfl_xor(subs, o);
    const unsigned int om = __shfl_xor(mx, o);
    mx = om > mx ? om : mx;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sz[wave] = zeros; ss[wave] = subs; sm[wave] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < WAVES; ++w) { zeros += sz[w]; subs += ss[w]; mx = sm[w] > mx ? sm[w] : mx; }
    if (blockIdx.x == 0) atomicAdd(&stats[0], (unsigned long long)n);
    atomicAdd(&stats[1], zeros);
    atomicAdd(&stats[2], subs);
    atomicMax(&stats[3], (unsigned long long)mx);
  }
}

}  // namespace

int launch_operand_stats(const half_t* x, int64_t n, unsigned long long* stats, hipStream_t s) {
  if (!stats || n == 0) return CLIPMI_OK;
  const int64_t blocks = (n + THREADS - 1) / THREADS;
  hipLaunchKernelGGL(operand_stats_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(THREADS), 0, s, reinterpret_cast<const uint16_t*>(x), n, stats);
  return check_launch("operand_stats_kernel");
}

int check_train_call(const char* who, const clipmi_model* m, int n_prompts, const void* ws, size_t ws_bytes, const void* stash, size_t stash_bytes,
                     int seq_rows) {
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "%s: null model", who);
  CLIPMI_REQUIRE(m->has_text, CLIPMI_ERR_STATE, "%s: text weights not bound (clipmi_set_text_weights)", who);
  CLIPMI_REQUIRE(n_prompts >= 0, CLIPMI_ERR_SHAPE, "%s: n_prompts=%d", who, n_prompts);
  CLIPMI_REQUIRE((int64_t)n_prompts * m->g.context_length < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: too many prompt tokens", who);
  CLIPMI_REQUIRE(m->g.text_width == 64 * m->g.text_heads && m->g.embed_dim % 64 == 0, CLIPMI_ERR_SHAPE, "%s: text width %d / heads %d / embed dim %d",
                 who, m->g.text_width, m->g.text_heads, m->g.embed_dim);
  if (n_prompts == 0) return CLIPMI_OK;
  size_t need_ws = 0, need_st = 0;
  clipmi_text_train_bytes(m, n_prompts, seq_rows, &need_ws, &need_st);
  CLIPMI_REQUIRE(ws && stash, CLIPMI_ERR_ARG, "%s: null workspace or stash", who);
  CLIPMI_REQUIRE((uintptr_t)ws % 256 == 0 && (uintptr_t)stash % 256 == 0, CLIPMI_ERR_ARG, "%s: workspace and stash must be 256-byte aligned", who);
  CLIPMI_REQUIRE(ws_bytes >= need_ws, CLIPMI_ERR_WORKSPACE, "%s: workspace too small: %zu < %zu", who, ws_bytes, need_ws);
  CLIPMI_REQUIRE(stash_bytes >= need_st, CLIPMI_ERR_WORKSPACE, "%s: stash too small: %zu < %zu", who, stash_bytes, need_st);
  return CLIPMI_OK;
}

namespace {
constexpr auto& gemm = tower_gemm;   // model.h: shared with vision_backward.hip
}  // namespace

int run_train_forward(clipmi_model* m, const void* prompts, int dtype, const float* ctx, int n_ctx, int per_class, const int32_t* eot, int C, int seq_rows,
                      float* out, void* workspace, void* stash_p, hipStream_t s, const float* deep, int n_deep) {
  const int L = live_rows(m, seq_rows), D = m->g.text_width, E = m->g.embed_dim, H = m->g.text_heads, layers = m->g.text_layers;
  const int64_t M = (int64_t)C * L;
  const TrainWs w = carve_ws(workspace, M, C, D, E);
  const Stash st = carve_stash(stash_p, M, D, layers);
  int rc;
  {
    const unsigned grid = (unsigned)((M * D + THREADS - 1) / THREADS);
    if (dtype == CLIPMI_F16)
      hipLaunchKernelGGL(coop_embed_kernel<half_t>, dim3(grid), dim3(THREADS), 0, s, (const half_t*)prompts, ctx, m->tw.positional_embedding, st.x(0), C, L,
                         m->g.context_length, D, n_ctx, per_class);
    else
      hipLaunchKernelGGL(coop_embed_kernel<float>, dim3(grid), dim3(THREADS), 0, s, (const float*)prompts, ctx, m->tw.positional_embedding, st.x(0), C, L,
                         m->g.context_length, D, n_ctx, per_class);
    if ((rc = check_launch("coop_embed_kernel"))) return rc;
  }
  if ((rc = launch_eot_rows(eot, st.idx(), C, L, s))) return rc;
  for (int i = 0; i < layers; ++i) {
    const clipmi_block_weights& b = m->tblocks[i];
    float *x_in = st.x(2 * i), *x_mid = st.x(2 * i + 1), *x_out = st.x(2 * i + 2);
    if (i >= 1 && i <= n_deep) {   // MaPLe: block i reads deep[i - 1] on the rows 1 .. n_ctx, whatever block i - 1 left there
      const int64_t n = (int64_t)C * n_ctx * D;
      hipLaunchKernelGGL(deep_splice_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, x_in, deep + (int64_t)(i - 1) * n_ctx * D, C, L, D,
                         n_ctx);
      if ((rc = check_launch("deep_splice_kernel"))) return rc;
    }
    if ((rc = launch_layernorm(x_in, CLIPMI_F32, D, nullptr, b.ln1_g, b.ln1_b, w.xn, CLIPMI_F16, D, (int)M, D, 1e-5f, s))) return rc;
    if ((rc = gemm(w.xn, D, b.w_qkv, D, b.b_qkv, nullptr, st.qkv(i), 3 * D, CLIPMI_F16, M, 3 * D, D, CLIPMI_EPI_BIAS, s))) return rc;
    if ((rc = launch_attention(st.qkv(i), w.att, C, L, H, 1, s))) return rc;
    if ((rc = gemm(w.att, D, b.w_out, D, b.b_out, x_in, x_mid, D, CLIPMI_F32, M, D, D, CLIPMI_EPI_BIAS_RESIDUAL, s))) return rc;
    if ((rc = launch_layernorm(x_mid, CLIPMI_F32, D, nullptr, b.ln2_g, b.ln2_b, w.xn, CLIPMI_F16, D, (int)M, D, 1e-5f, s))) return rc;
    if ((rc = gemm(w.xn, D, b.w_fc, D, b.b_fc, nullptr, st.h(i), 4 * D, CLIPMI_F16, M, 4 * D, D, CLIPMI_EPI_BIAS, s))) return rc;
    if ((rc = launch_quickgelu_forward(st.h(i), w.hid, M * 4 * D, s))) return rc;
    if ((rc = gemm(w.hid, 4 * D, b.w_proj, 4 * D, b.b_proj, x_mid, x_out, D, CLIPMI_F32, M, D, 4 * D, CLIPMI_EPI_BIAS_RESIDUAL, s))) return rc;
  }
  if ((rc = launch_layernorm(st.x(2 * layers), CLIPMI_F32, D, st.idx(), m->tw.ln_final_g, m->tw.ln_final_b, w.rows16, CLIPMI_F16, D, C, D, 1e-5f, s))) return rc;
  return gemm(w.rows16, D, m->tw.proj_t, D, nullptr, nullptr, out, E, CLIPMI_F32, C, E, D, CLIPMI_EPI_NONE, s);
}

int run_backward(clipmi_model* m, const clipmi_text_dgrad* wt, const float* d_out, int C, int seq_rows, float* g, void* workspace, const void* stash_p,
                 unsigned long long* stats, hipStream_t s, int n_ctx, int n_deep, float* d_deep) {
  const int L = live_rows(m, seq_rows), D = m->g.text_width, E = m->g.embed_dim, H = m->g.text_heads, layers = m->g.text_layers;
  const int64_t M = (int64_t)C * L;
  const TrainWs w = carve_ws(workspace, M, C, D, E);
  const Stash st = carve_stash(const_cast<void*>(stash_p), M, D, layers);
  half_t* g16 = w.xn;
  int rc;
  // tail: d_out text_projection^T, ln_final's backward on the EOT rows, scattered into the zeroed stream
  if ((rc = launch_cast_f32(d_out, w.dfeat16, CLIPMI_F16, (int64_t)C * E, s))) return rc;
  if ((rc = launch_operand_stats(w.dfeat16, (int64_t)C * E, stats, s))) return rc;
  if ((rc = gemm(w.dfeat16, E, wt->proj, E, nullptr, nullptr, w.dxf, D, CLIPMI_F32, C, D, E, CLIPMI_EPI_NONE, s))) return rc;
  if (hipMemsetAsync(g, 0, (size_t)M * D * 4, s) != hipSuccess || hipMemsetAsync(g16, 0, (size_t)M * D * 2, s) != hipSuccess) return check_launch("hipMemsetAsync");
  if ((rc = launch_ln_backward(st.x(2 * layers), D, st.idx(), m->tw.ln_final_g, w.dxf, CLIPMI_F32, g, g16, C, D, 1e-5f, s))) return rc;
  for (int i = layers - 1; i >= 0; --i) {
    const clipmi_block_weights& b = m->tblocks[i];
    const clipmi_block_dgrad& t = wt->blocks[i];
    if ((rc = launch_operand_stats(g16, M * D, stats, s))) return rc;
    if ((rc = gemm(g16, D, t.w_proj_t, D, nullptr, nullptr, w.hid, 4 * D, CLIPMI_F16, M, 4 * D, D, CLIPMI_EPI_NONE, s))) return rc;       // d_a = g W_proj
    if ((rc = launch_quickgelu_backward(st.h(i), w.hid, w.hid, M * 4 * D, s))) return rc;
    if ((rc = launch_operand_stats(w.hid, M * 4 * D, stats, s))) return rc;
    if ((rc = gemm(w.hid, 4 * D, t.w_fc_t, 4 * D, nullptr, nullptr, w.dy, D, CLIPMI_F32, M, D, 4 * D, CLIPMI_EPI_NONE, s))) return rc;    // . W_fc
    if ((rc = launch_ln_backward(st.x(2 * i + 1), D, nullptr, b.ln2_g, w.dy, CLIPMI_F32, g, g16, M, D, 1e-5f, s))) return rc;
    if ((rc = launch_operand_stats(g16, M * D, stats, s))) return rc;
    if ((rc = gemm(g16, D, t.w_out_t, D, nullptr, nullptr, w.att, D, CLIPMI_F16, M, D, D, CLIPMI_EPI_NONE, s))) return rc;                // g W_out
    if ((rc = launch_attention_backward(st.qkv(i), w.att, w.qkv, C, L, H, s))) return rc;
    if ((rc = launch_operand_stats(w.qkv, M * 3 * D, stats, s))) return rc;
    if ((rc = gemm(w.qkv, 3 * D, t.w_qkv_t, 3 * D, nullptr, nullptr, w.dy, D, CLIPMI_F32, M, D, 3 * D, CLIPMI_EPI_NONE, s))) return rc;   // dqkv W_qkv
    if ((rc = launch_ln_backward(st.x(2 * i), D, nullptr, b.ln1_g, w.dy, CLIPMI_F32, g, g16, M, D, 1e-5f, s))) return rc;
    // block i read deep[i - 1] on the rows 1 .. n_ctx: their gradient leaves the stream (block i - 1's outputs there were discarded)
    if (i >= 1 && i <= n_deep && (rc = launch_splice_reduce(g, g16, d_deep + (int64_t)(i - 1) * n_ctx * D, C, L, D, 1, n_ctx, 1, s))) return rc;
  }
  return CLIPMI_OK;
}

// what the _deep entry points ask on top of the plain ones: n_deep prompts [n_ctx, Dt] for the blocks 1 .. n_deep
int check_deep(const char* who, const clipmi_model* m, int n_ctx, int n_deep, const void* deep, int seq_rows) {
  CLIPMI_REQUIRE(n_deep >= 0, CLIPMI_ERR_SHAPE, "%s: n_deep=%d", who, n_deep);
  if (n_deep == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(1 + n_deep <= m->g.text_layers, CLIPMI_ERR_SHAPE, "%s: depth %d for %d text layers", who, 1 + n_deep, m->g.text_layers);
  CLIPMI_REQUIRE(n_ctx >= 1 && 1 + n_ctx <= live_rows(m, seq_rows), CLIPMI_ERR_SHAPE, "%s: n_ctx=%d does not fit the %d token rows that are computed", who,
                 n_ctx, live_rows(m, seq_rows));
  CLIPMI_REQUIRE(deep, CLIPMI_ERR_ARG, "%s: null pointer (n_deep=%d needs the deep prompts)", who, n_deep);
  return CLIPMI_OK;
}

int check_dgrad(const char* who, const clipmi_model* m, const clipmi_text_dgrad* wt) {
  CLIPMI_REQUIRE(wt && wt->proj && wt->blocks, CLIPMI_ERR_ARG, "%s: null transposed weights", who);
  CLIPMI_REQUIRE((uintptr_t)wt->proj % 16 == 0, CLIPMI_ERR_ARG, "%s: transposed weights must be 16-byte aligned", who);
  for (int i = 0; i < m->g.text_layers; ++i) {
    const void* p[] = {wt->blocks[i].w_qkv_t, wt->blocks[i].w_out_t, wt->blocks[i].w_fc_t, wt->blocks[i].w_proj_t};
    for (const void* q : p) CLIPMI_REQUIRE(q && (uintptr_t)q % 16 == 0, CLIPMI_ERR_ARG, "%s: block %d: null or unaligned transposed weight", who, i);
  }
  return CLIPMI_OK;
}

int check_train_inputs(const char* who, const clipmi_model* m, const void* prompts, int dtype, const float* ctx, int n_ctx, const int32_t* eot,
                       int seq_rows, const clipmi_prompt_hook* hook, unsigned flags) {
  CLIPMI_REQUIRE(!(flags & ~(CLIPMI_CALL_STREAM_F32 | CLIPMI_CALL_STREAM_F16)), CLIPMI_ERR_ARG, "%s: bad flags 0x%x", who, flags);
  CLIPMI_REQUIRE(!(flags & CLIPMI_CALL_STREAM_F16), CLIPMI_ERR_STATE, "%s: the training forward runs the fp32 residual stream only", who);
  CLIPMI_REQUIRE(!hook || hook->n_deep == 0, CLIPMI_ERR_ARG, "%s: deep prompts are not supported by the training forward", who);
  CLIPMI_REQUIRE(prompts && eot, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(dtype == CLIPMI_F16 || dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "%s: bad dtype %d", who, dtype);
  CLIPMI_REQUIRE(!ctx || (n_ctx >= 1 && 1 + n_ctx <= live_rows(m, seq_rows)), CLIPMI_ERR_SHAPE, "%s: n_ctx=%d does not fit the %d token rows that are computed",
                 who, n_ctx, live_rows(m, seq_rows));
  return CLIPMI_OK;
}

}  // namespace clipmi

using namespace clipmi;

extern "C" {

int clipmi_layernorm_backward(const float* x, int64_t x_stride, const int32_t* row_idx, const float* gamma, const void* dy, int dy_dtype, float* g,
                              void* g16, int rows, int D, float eps, clipmi_stream_t stream) {
  CLIPMI_REQUIRE(rows >= 0, CLIPMI_ERR_SHAPE, "layernorm_backward: rows=%d", rows);
  CLIPMI_REQUIRE(D >= 4 && D % 4 == 0 && D <= 4096, CLIPMI_ERR_SHAPE, "layernorm_backward: D=%d (a multiple of 4, at most 4096)", D);
  CLIPMI_REQUIRE(x_stride >= D && x_stride % 4 == 0, CLIPMI_ERR_SHAPE, "layernorm_backward: x_stride=%lld", (long long)x_stride);
  CLIPMI_REQUIRE(dy_dtype == CLIPMI_F16 || dy_dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "layernorm_backward: bad dy_dtype %d", dy_dtype);
  if (rows == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(x && gamma && dy && g, CLIPMI_ERR_ARG, "layernorm_backward: null pointer");
  CLIPMI_REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)gamma % 16 == 0 && (uintptr_t)g % 16 == 0 && (uintptr_t)dy % (dy_dtype == CLIPMI_F32 ? 16 : 8) == 0 &&
                     (uintptr_t)g16 % 8 == 0,
                 CLIPMI_ERR_ARG, "layernorm_backward: misaligned pointer");
  return launch_ln_backward(x, x_stride, row_idx, gamma, dy, dy_dtype, g, static_cast<half_t*>(g16), rows, D, eps, (hipStream_t)stream);
}

int clipmi_quickgelu_backward(const void* h, const void* d_a, void* d_h, int64_t n, clipmi_stream_t stream) {
  CLIPMI_REQUIRE(n >= 0, CLIPMI_ERR_SHAPE, "quickgelu_backward: n=%lld", (long long)n);
  if (n == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(h && d_a && d_h, CLIPMI_ERR_ARG, "quickgelu_backward: null pointer");
  CLIPMI_REQUIRE((uintptr_t)h % 16 == 0 && (uintptr_t)d_a % 16 == 0 && (uintptr_t)d_h % 16 == 0, CLIPMI_ERR_ARG, "quickgelu_backward: pointers must be 16-byte aligned");
  return launch_quickgelu_backward(static_cast<const half_t*>(h), static_cast<const half_t*>(d_a), static_cast<half_t*>(d_h), n, (hipStream_t)stream);
}

int clipmi_attention_backward(const void* qkv, const void* d_out, void* dqkv, int N, int L, int H, clipmi_stream_t stream) {
  return launch_attention_backward(static_cast<const half_t*>(qkv), static_cast<const half_t*>(d_out), static_cast<half_t*>(dqkv), N, L, H, (hipStream_t)stream);
}

int clipmi_text_train_bytes(const clipmi_model* m, int n_prompts, int seq_rows, size_t* workspace_bytes, size_t* stash_bytes) {
  if (workspace_bytes) *workspace_bytes = 0;
  if (stash_bytes) *stash_bytes = 0;
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "text_train_bytes: null model");
  CLIPMI_REQUIRE(n_prompts >= 0 && (int64_t)n_prompts * m->g.context_length < (1ll << 31), CLIPMI_ERR_SHAPE, "text_train_bytes: n_prompts=%d", n_prompts);
  const int64_t M = (int64_t)n_prompts * live_rows(m, seq_rows);
  if (workspace_bytes) *workspace_bytes = carve_ws(nullptr, M, n_prompts, m->g.text_width, m->g.embed_dim).bytes;
  if (stash_bytes) *stash_bytes = carve_stash(nullptr, M, m->g.text_width, m->g.text_layers).bytes(n_prompts);
  return CLIPMI_OK;
}

int clipmi_text_encoder_train(clipmi_model* m, const void* prompts, int dtype, const float* ctx, int n_ctx, int ctx_per_class, const int32_t* eot,
                              int n_prompts, int seq_rows, const clipmi_prompt_hook* hook, float* out, void* workspace, size_t workspace_bytes, void* stash,
                              size_t stash_bytes, unsigned flags, clipmi_stream_t stream) {
  if (int rc = check_train_call("text_encoder_train", m, n_prompts, workspace, workspace_bytes, stash, stash_bytes, seq_rows)) return rc;
  if (n_prompts == 0) return CLIPMI_OK;
  if (int rc = check_train_inputs("text_encoder_train", m, prompts, dtype, ctx, n_ctx, eot, seq_rows, hook, flags)) return rc;
  CLIPMI_REQUIRE(out, CLIPMI_ERR_ARG, "text_encoder_train: null pointer");
  return run_train_forward(m, prompts, dtype, ctx, n_ctx, ctx_per_class, eot, n_prompts, seq_rows, out, workspace, stash, (hipStream_t)stream);
}

int clipmi_text_encoder_backward(clipmi_model* m, const clipmi_text_dgrad* wt, const float* d_out, int n_prompts, int seq_rows, float* d_embed,
                                 void* workspace, size_t workspace_bytes, const void* stash, size_t stash_bytes, unsigned long long* operand_stats,
                                 clipmi_stream_t stream) {
  if (int rc = check_train_call("text_encoder_backward", m, n_prompts, workspace, workspace_bytes, stash, stash_bytes, seq_rows)) return rc;
  if (n_prompts == 0) return CLIPMI_OK;
  if (int rc = check_dgrad("text_encoder_backward", m, wt)) return rc;
  CLIPMI_REQUIRE(d_out && d_embed, CLIPMI_ERR_ARG, "text_encoder_backward: null pointer");
  CLIPMI_REQUIRE((uintptr_t)d_embed % 16 == 0, CLIPMI_ERR_ARG, "text_encoder_backward: d_embed must be 16-byte aligned");
  CLIPMI_REQUIRE(live_rows(m, seq_rows) <= AB_MAX_L, CLIPMI_ERR_SHAPE, "text_encoder_backward: %d token rows per prompt (at most %d)", live_rows(m, seq_rows),
                 AB_MAX_L);
  return run_backward(m, wt, d_out, n_prompts, seq_rows, d_embed, workspace, stash, operand_stats, (hipStream_t)stream);
}

int clipmi_text_encoder_train_deep(clipmi_model* m, const void* prompts, int dtype, const float* ctx, int n_ctx, int ctx_per_class, const int32_t* eot,
                                   int n_prompts, int seq_rows, const float* deep, int n_deep, float* out, void* workspace, size_t workspace_bytes,
                                   void* stash, size_t stash_bytes, unsigned flags, clipmi_stream_t stream) {
  const char* who = "text_encoder_train_deep";
  if (int rc = check_train_call(who, m, n_prompts, workspace, workspace_bytes, stash, stash_bytes, seq_rows)) return rc;
  if (int rc = check_deep(who, m, n_ctx, n_deep, deep, seq_rows)) return rc;
  if (n_prompts == 0) return CLIPMI_OK;
  if (int rc = check_train_inputs(who, m, prompts, dtype, ctx, n_ctx, eot, seq_rows, nullptr, flags)) return rc;
  CLIPMI_REQUIRE(out, CLIPMI_ERR_ARG, "%s: null pointer", who);
  return run_train_forward(m, prompts, dtype, ctx, n_ctx, ctx_per_class, eot, n_prompts, seq_rows, out, workspace, stash, (hipStream_t)stream, deep, n_deep);
}

int clipmi_text_encoder_backward_deep(clipmi_model* m, const clipmi_text_dgrad* wt, const float* d_out, int n_prompts, int seq_rows, int n_ctx, int n_deep,
                                      float* d_embed, float* d_deep, void* workspace, size_t workspace_bytes, const void* stash, size_t stash_bytes,
                                      unsigned long long* operand_stats, clipmi_stream_t stream) {
  const char* who = "text_encoder_backward_deep";
  if (int rc = check_train_call(who, m, n_prompts, workspace, workspace_bytes, stash, stash_bytes, seq_rows)) return rc;
  if (int rc = check_deep(who, m, n_ctx, n_deep, d_deep, seq_rows)) return rc;
  if (n_prompts == 0) return CLIPMI_OK;
  if (int rc = check_dgrad(who, m, wt)) return rc;
  CLIPMI_REQUIRE(d_out && d_embed, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE((uintptr_t)d_embed % 16 == 0, CLIPMI_ERR_ARG, "%s: d_embed must be 16-byte aligned", who);
  CLIPMI_REQUIRE(live_rows(m, seq_rows) <= AB_MAX_L, CLIPMI_ERR_SHAPE, "%s: %d token rows per prompt (at most %d)", who, live_rows(m, seq_rows), AB_MAX_L);
  return run_backward(m, wt, d_out, n_prompts, seq_rows, d_embed, workspace, stash, operand_stats, (hipStream_t)stream, n_ctx, n_deep, d_deep);
}

}  // extern "C"
