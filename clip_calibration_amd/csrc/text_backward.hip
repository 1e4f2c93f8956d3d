// CoOp's context trained on the device (reference trainers/classification/coop.py:70-144, 192-222, 282-309): the text tower's training
// forward with a stash, its backward down to the input embeddings with the tower frozen, CoOp's cross-entropy head, and the context's
// gradient with torch.optim.SGD's step.  DESIGN.md "CoOp fit" has the data flow, the stash and the rounding points.
//
// Frozen weights: no weight gradient exists and every Linear's backward is dX = dY W -- the forward's fp16 MFMA GEMM (launch_gemm) on a
// transposed copy of the weight.  New here:
//   ln_backward_kernel         LayerNorm's backward from the saved fp32 rows; adds into the fp32 gradient stream and writes its fp16 copy
//   quickgelu_forward_kernel   QuickGELU of the saved (rounded) c_fc pre-activation
//   quickgelu_backward_kernel  its derivative times the upstream gradient
//   (attention_backward_kernel, causal attention's backward on the matrix cores, lives with the other attention kernels: attention.hip)
//   coop_head_*_kernel         both normalisations, logits, softmax, cross-entropy and the gradient w.r.t. the raw text features
//   prograd_softmax_kernel,    the heads of KgCoOp (cross-entropy + w (1 - mean cosine to the frozen zero-shot features)) and ProGrad (cross-entropy
//   kgcoop_loss_kernel         and the distillation loss against the zero-shot logits, one gradient each) on the same per-class workgroup
//   prograd_dots_kernel,       ProGrad's two context gradients, their three inner products in float64, the projection rule and the SGD step
//   prograd_step_kernel
//   ctx_step_kernel            the context's gradient (a fixed-order sum over the classes) and the SGD rule
//   coop_embed_kernel          prompts with the fp32 context rows in place, plus the positional embedding
// No float atomics and no workgroup waits for another: the same inputs give the same bits.
#include <cmath>

#include "common.h"
#include "model.h"
#include "train_rules.h"

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

// ------------------------------------------------------------------------------------------------------------------------ CoOp head
// workspace of one batch: z [B, C] | dz [B, C] | loss [B] | 1/|f_b| [B] | 1/|t_c| [C], fp32
struct HeadWs {
  float *z, *dz, *loss, *inf, *intx;
};
inline size_t head_floats(int B, int C) { return 2 * (size_t)B * (size_t)C + 2 * (size_t)B + (size_t)C; }
inline HeadWs head_carve(void* ws, int B, int C) {
  HeadWs w;
  w.z = static_cast<float*>(ws);
  w.dz = w.z + (size_t)B * C;
  w.loss = w.dz + (size_t)B * C;
  w.inf = w.loss + B;
  w.intx = w.inf + B;
  return w;
}

// one wave per row of feats (rows 0 .. B), of text (rows B .. B + C) or, with a teacher, of the teacher (rows B + C .. B + 2 C): the
// reciprocal of its L2 norm
__global__ __launch_bounds__(THREADS) void coop_head_norm_kernel(const float* __restrict__ feats, int64_t ld, const float* __restrict__ text, int B, int E, int C,
                                                                 HeadWs ws, const float* __restrict__ teacher, float* __restrict__ inty) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (r >= B + C + (teacher ? C : 0)) return;
  const float* row = r < B ? feats + (int64_t)r * ld : r < B + C ? text + (int64_t)(r - B) * E : teacher + (int64_t)(r - B - C) * E;
  float s = 0.f;
  for (int e = lane; e < E; e += 64) s = fmaf(row[e], row[e], s);
  s = 1.f / sqrtf(wave_sum(s));
  if (lane == 0) (r < B ? ws.inf[r] : r < B + C ? ws.intx[r - B] : inty[r - B - C]) = s;
}

// one wave per (b, c): z = scale (f_b . t_c) / (|f_b| |t_c|), lane-strided fmaf chains and the wave tree
__global__ __launch_bounds__(THREADS) void coop_head_logits_kernel(const float* __restrict__ feats, int64_t ld, const float* __restrict__ text, int B, int E, int C,
                                                                   float scale, HeadWs ws) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (item >= (int64_t)B * C) return;
  const int b = (int)(item / C), c = (int)(item % C);
  const float* f = feats + (int64_t)b * ld;
  const float* tx = text + (int64_t)c * E;
  float s = 0.f;
  for (int e = lane; e < E; e += 64) s = fmaf(f[e], tx[e], s);
  s = wave_sum(s);
  if (lane == 0) ws.z[item] = scale * ((s * ws.inf[b]) * ws.intx[c]);
}

// grid (B): row loss and dz = grad_scale (softmax(z) - onehot(y)) / B of one sample
__global__ __launch_bounds__(THREADS) void coop_head_softmax_kernel(const int64_t* __restrict__ labels, int B, int C, float grad_scale, HeadWs ws) {
#pragma clang fp contract(off)
  __shared__ float swave[2 * WAVES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = blockIdx.x;
  const float* __restrict__ z = ws.z + (size_t)r * C;
  float* __restrict__ dz = ws.dz + (size_t)r * C;
  const int64_t y = labels[r];
  if (y < 0 || y >= C) {      // the same for every thread of the workgroup: nobody waits at a barrier below
    for (int c = t; c < C; c += THREADS) dz[c] = NAN;
    if (t == 0) ws.loss[r] = NAN;
    return;
  }
  float m = -INFINITY;
  for (int c = t; c < C; c += THREADS) m = fmaxf(m, z[c]);
  m = wave_max(m);
  if (lane == 0) swave[wave] = m;
  __syncthreads();
  m = swave[0];
  for (int w = 1; w < WAVES; ++w) m = fmaxf(m, swave[w]);
  float S = 0.f;
  for (int c = t; c < C; c += THREADS) S += __expf(z[c] - m);
  S = wave_sum(S);
  if (lane == 0) swave[WAVES + wave] = S;
  __syncthreads();
  S = swave[WAVES];
  for (int w = 1; w < WAVES; ++w) S += swave[WAVES + w];
  if (t == 0) ws.loss[r] = logf(S) - (z[y] - m);
  const float k = grad_scale / (float)B;
  for (int c = t; c < C; c += THREADS) {
    const float p = __expf(z[c] - m) / S;
    dz[c] = (c == y ? p - 1.f : p) * k;
  }
}

// grid (C): du_c = scale sum_b dz[b, c] x_b (b ascending), q = u_c . du_c, d_text[c] = (du_c - u_c q) / |t_c|.  Workgroup 0 also averages
// the row losses in float64.  KG (KgCoOp): du_c carries the extra term kg o_c, kg = -grad_scale w / C and o_c the normalised teacher row;
// the projection is linear, so its image k ((o_c - u_c (u_c . o_c)) / |t_c|) is added to the cross-entropy's d_text, whose arithmetic is
// CoOp's own (kg = -0 leaves those bits as they are).  u_c . o_c goes to cosv[c] for kgcoop_loss_kernel.
template <bool KG>
__global__ __launch_bounds__(THREADS) void coop_head_grad_kernel(const float* __restrict__ feats, int64_t ld, const float* __restrict__ text, int B, int E, int C,
                                                                 float scale, HeadWs ws, float* __restrict__ d_text, half_t* __restrict__ d_text16,
                                                                 float* __restrict__ loss_out, const float* __restrict__ teacher,
                                                                 const float* __restrict__ inty, float* __restrict__ cosv, float kg) {
  __shared__ float swave[2 * WAVES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, c = blockIdx.x;
  const float* tx = text + (int64_t)c * E;
  const float itn = ws.intx[c];
  float q = 0.f, uo = 0.f;
  for (int e = t; e < E; e += THREADS) {   // pass 1: q
    float du = 0.f;
    for (int b = 0; b < B; ++b) du = fmaf(ws.dz[(size_t)b * C + c], feats[(int64_t)b * ld + e] * ws.inf[b], du);
    q = fmaf(tx[e] * itn, scale * du, q);
    if constexpr (KG) uo = fmaf(tx[e] * itn, teacher[(int64_t)c * E + e] * inty[c], uo);
  }
  q = wave_sum(q);
  if (lane == 0) swave[wave] = q;
  if constexpr (KG) {
    uo = wave_sum(uo);
    if (lane == 0) swave[WAVES + wave] = uo;
  }
  __syncthreads();
  q = swave[0];
  for (int w = 1; w < WAVES; ++w) q += swave[w];
  if constexpr (KG) {
    uo = swave[WAVES];
    for (int w = 1; w < WAVES; ++w) uo += swave[WAVES + w];
    if (t == 0) cosv[c] = uo;
  }
  for (int e = t; e < E; e += THREADS) {   // pass 2: the same du again, then the projection
    float du = 0.f;
    for (int b = 0; b < B; ++b) du = fmaf(ws.dz[(size_t)b * C + c], feats[(int64_t)b * ld + e] * ws.inf[b], du);
    float d = (scale * du - (tx[e] * itn) * q) * itn;
    if constexpr (KG) d = fmaf(kg * itn, fmaf(-(tx[e] * itn), uo, teacher[(int64_t)c * E + e] * inty[c]), d);
    d_text[(int64_t)c * E + e] = d;
    if (d_text16) d_text16[(int64_t)c * E + e] = (half_t)d;
  }
  if (c != 0 || !loss_out) return;   // the same for every thread of the workgroup
  mean_loss_256(ws.loss, B, loss_out);
}

int launch_coop_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale, float grad_scale,
                     float* loss, float* d_text, half_t* d_text16, void* workspace, size_t workspace_bytes, hipStream_t s) {
  CLIPMI_REQUIRE(feats && labels && text && d_text && workspace, CLIPMI_ERR_ARG, "coop_head: null pointer");
  CLIPMI_REQUIRE(std::isfinite(scale) && std::isfinite(grad_scale), CLIPMI_ERR_ARG, "coop_head: scale=%g, grad_scale=%g (both finite)", scale, grad_scale);
  CLIPMI_REQUIRE(B >= 1 && C >= 2 && E >= 1 && ld >= E, CLIPMI_ERR_SHAPE, "coop_head: B=%d C=%d E=%d ld=%lld", B, C, E, (long long)ld);
  CLIPMI_REQUIRE((int64_t)B * C < (1ll << 31), CLIPMI_ERR_SHAPE, "coop_head: B * C too large");
  CLIPMI_REQUIRE((uintptr_t)workspace % 8 == 0, CLIPMI_ERR_ARG, "coop_head: the workspace must be 8-byte aligned");
  CLIPMI_REQUIRE(workspace_bytes >= clipmi_coop_head_workspace_bytes(B, E, C), CLIPMI_ERR_WORKSPACE, "coop_head: workspace of %zu bytes, %zu needed",
                 workspace_bytes, clipmi_coop_head_workspace_bytes(B, E, C));
  const HeadWs ws = head_carve(workspace, B, C);
  hipLaunchKernelGGL(coop_head_norm_kernel, dim3((unsigned)((B + C + WAVES - 1) / WAVES)), dim3(THREADS), 0, s, feats, ld, text, B, E, C, ws,
                     (const float*)nullptr, (float*)nullptr);
  if (int rc = check_launch("coop_head_norm_kernel")) return rc;
  hipLaunchKernelGGL(coop_head_logits_kernel, dim3((unsigned)(((int64_t)B * C + WAVES - 1) / WAVES)), dim3(THREADS), 0, s, feats, ld, text, B, E, C, scale, ws);
  if (int rc = check_launch("coop_head_logits_kernel")) return rc;
  hipLaunchKernelGGL(coop_head_softmax_kernel, dim3((unsigned)B), dim3(THREADS), 0, s, labels, B, C, grad_scale, ws);
  if (int rc = check_launch("coop_head_softmax_kernel")) return rc;
  hipLaunchKernelGGL(coop_head_grad_kernel<false>, dim3((unsigned)C), dim3(THREADS), 0, s, feats, ld, text, B, E, C, scale, ws, d_text, d_text16, loss,
                     (const float*)nullptr, (const float*)nullptr, (float*)nullptr, 0.f);
  return check_launch("coop_head_grad_kernel");
}

// ------------------------------------------------------------------------------------------------------- KgCoOp's and ProGrad's heads
// (reference trainers/classification/kgcoop.py:246-269, prograd.py:291-304).  Both run CoOp's head with a frozen teacher [C, E], the
// zero-shot text features, whose rows are normalised here.  mode: 0 CoOp, 1 KgCoOp, 2 ProGrad (include/clipmi.h).
enum { MODE_COOP = 0, MODE_KGCOOP = 1, MODE_PROGRAD = 2 };

// behind the CoOp head's workspace: 1/|o_c| [C] | u_c . o_c [C] | and for ProGrad z_tea [B, C] | dz_kl [B, C] | kl row loss [B], fp32
struct TeacherWs {
  float *inty, *cosv, *z_tea, *dz_kl, *loss_kl;
};
inline size_t prompt_head_floats(int B, int C, int mode) {
  size_t n = head_floats(B, C);
  if (mode != MODE_COOP) n += 2 * (size_t)C;
  if (mode == MODE_PROGRAD) n += 2 * (size_t)B * (size_t)C + (size_t)B;
  return n;
}
inline TeacherWs teacher_carve(void* ws, int B, int C) {
  TeacherWs w;
  w.inty = static_cast<float*>(ws) + head_floats(B, C);
  w.cosv = w.inty + C;
  w.z_tea = w.cosv + C;
  w.dz_kl = w.z_tea + (size_t)B * C;
  w.loss_kl = w.dz_kl + (size_t)B * C;
  return w;
}

// the 256 threads' sum / maximum: the wave tree, then the waves in ascending order -- the order of coop_head_softmax_kernel.  sw: WAVES
// floats of LDS; every thread of the workgroup calls it.
__device__ __forceinline__ float block_sum(float v, float* sw) {
#pragma clang fp contract(off)
  v = wave_sum(v);
  __syncthreads();   // the readers of the previous use are done
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
  __syncthreads();
  v = sw[0];
  for (int w = 1; w < WAVES; ++w) v += sw[w];
  return v;
}
__device__ __forceinline__ float block_max(float v, float* sw) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
  __syncthreads();
  v = sw[0];
  for (int w = 1; w < WAVES; ++w) v = fmaxf(v, sw[w]);
  return v;
}

// grid (B), ProGrad: the cross-entropy's row loss and dz exactly as coop_head_softmax_kernel forms them, and beside them the distillation
// term at the temperature T = 1 / inv_t: p = softmax(z / T), p_tea = softmax(z_tea / T), kl row loss = T^2 sum_c p_tea (log S - (z - m) / T),
// dz_kl = grad_scale T (p - p_tea) / B.  The label reaches the cross-entropy only.  Student and teacher go through the same expressions:
// equal logits give dz_kl = 0 exactly.
__global__ __launch_bounds__(THREADS) void prograd_softmax_kernel(const int64_t* __restrict__ labels, int B, int C, float grad_scale, float T, float inv_t,
                                                                  HeadWs ws, TeacherWs tw) {
#pragma clang fp contract(off)
  __shared__ float sw[WAVES];
  const int t = threadIdx.x, r = blockIdx.x;
  const float* __restrict__ z = ws.z + (size_t)r * C;
  const float* __restrict__ zt = tw.z_tea + (size_t)r * C;
  float* __restrict__ dz = ws.dz + (size_t)r * C;
  float* __restrict__ dzk = tw.dz_kl + (size_t)r * C;
  const int64_t y = labels[r];
  const bool bad = y < 0 || y >= C;      // the same for every thread of the workgroup
  float m = -INFINITY, mt = -INFINITY;
  for (int c = t; c < C; c += THREADS) {
    m = fmaxf(m, z[c]);
    mt = fmaxf(mt, zt[c]);
  }
  m = block_max(m, sw);
  mt = block_max(mt, sw);
  float S = 0.f, Ss = 0.f, St = 0.f;
  for (int c = t; c < C; c += THREADS) {
    S += __expf(z[c] - m);
    Ss += __expf((z[c] - m) * inv_t);
    St += __expf((zt[c] - mt) * inv_t);
  }
  S = block_sum(S, sw);
  Ss = block_sum(Ss, sw);
  St = block_sum(St, sw);
  const float k = grad_scale / (float)B, kt = k * T, log_ss = logf(Ss);
  float kl = 0.f;
  for (int c = t; c < C; c += THREADS) {
    const float p = __expf(z[c] - m) / S;
    dz[c] = bad ? NAN : (c == y ? p - 1.f : p) * k;
    const float ps = __expf((z[c] - m) * inv_t) / Ss, pt = __expf((zt[c] - mt) * inv_t) / St;
    dzk[c] = (ps - pt) * kt;
    kl += pt * (log_ss - (z[c] - m) * inv_t);
  }
  kl = block_sum(kl, sw);
  if (t == 0) {
    ws.loss[r] = bad ? NAN : logf(S) - (z[bad ? 0 : y] - m);
    tw.loss_kl[r] = kl * (T * T);
  }
}

// one workgroup, KgCoOp: losses = [ce + w score, ce, score], ce the float64 mean of the row losses and score = 1 - the float64 mean of
// u_c . o_c, both in mean_loss_256's order
__global__ __launch_bounds__(256) void kgcoop_loss_kernel(HeadWs ws, TeacherWs tw, int B, int C, float w, float* __restrict__ losses) {
#pragma clang fp contract(off)
  __shared__ double sl[256];
  const int t = threadIdx.x;
  mean_loss_256(ws.loss, B, losses + 1);
  double s = 0.0;
  for (int c = t; c < C; c += 256) s += (double)tw.cosv[c];
  sl[t] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) sl[t] += sl[t + h];
    __syncthreads();
  }
  if (t == 0) {
    const float score = (float)(1.0 - sl[0] / (double)C);
    losses[2] = score;
    losses[0] = losses[1] + w * score;
  }
}

int launch_prompt_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale, float grad_scale, int mode,
                       const float* teacher, float w, float T, float* losses, float* d_text, half_t* d_text16, float* d_text_kl, void* workspace,
                       size_t workspace_bytes, hipStream_t s) {
  CLIPMI_REQUIRE(mode == MODE_COOP || mode == MODE_KGCOOP || mode == MODE_PROGRAD, CLIPMI_ERR_ARG, "prompt_head: bad mode %d", mode);
  CLIPMI_REQUIRE(feats && labels && text && d_text && workspace && losses, CLIPMI_ERR_ARG, "prompt_head: null pointer");
  CLIPMI_REQUIRE(mode == MODE_COOP || teacher, CLIPMI_ERR_ARG, "prompt_head: null pointer (KgCoOp and ProGrad need the teacher)");
  CLIPMI_REQUIRE(mode != MODE_PROGRAD || d_text_kl, CLIPMI_ERR_ARG, "prompt_head: null pointer (ProGrad writes two gradients)");
  CLIPMI_REQUIRE(std::isfinite(scale) && std::isfinite(grad_scale), CLIPMI_ERR_ARG, "prompt_head: scale=%g, grad_scale=%g (both finite)", scale, grad_scale);
  CLIPMI_REQUIRE(mode != MODE_KGCOOP || (std::isfinite(w) && w >= 0.f), CLIPMI_ERR_ARG, "prompt_head: w=%g (finite, >= 0)", w);
  CLIPMI_REQUIRE(mode != MODE_PROGRAD || (std::isfinite(T) && T > 0.f), CLIPMI_ERR_ARG, "prompt_head: T=%g (finite, > 0)", T);
  CLIPMI_REQUIRE(B >= 1 && C >= 2 && E >= 1 && ld >= E, CLIPMI_ERR_SHAPE, "prompt_head: B=%d C=%d E=%d ld=%lld", B, C, E, (long long)ld);
  CLIPMI_REQUIRE((int64_t)B * C < (1ll << 31), CLIPMI_ERR_SHAPE, "prompt_head: B * C too large");
  CLIPMI_REQUIRE((uintptr_t)workspace % 8 == 0, CLIPMI_ERR_ARG, "prompt_head: the workspace must be 8-byte aligned");
  const size_t need = clipmi_prompt_head_workspace_bytes(B, E, C, mode);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "prompt_head: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  if (mode == MODE_COOP) {
    if (int rc = launch_coop_head(feats, ld, labels, text, B, E, C, scale, grad_scale, losses, d_text, d_text16, workspace, workspace_bytes, s)) return rc;
    return CLIPMI_OK;
  }
  const HeadWs ws = head_carve(workspace, B, C);
  const TeacherWs tw = teacher_carve(workspace, B, C);
  const dim3 threads(THREADS), per_bc((unsigned)(((int64_t)B * C + WAVES - 1) / WAVES));
  hipLaunchKernelGGL(coop_head_norm_kernel, dim3((unsigned)((B + 2 * C + WAVES - 1) / WAVES)), threads, 0, s, feats, ld, text, B, E, C, ws, teacher, tw.inty);
  if (int rc = check_launch("coop_head_norm_kernel")) return rc;
  hipLaunchKernelGGL(coop_head_logits_kernel, per_bc, threads, 0, s, feats, ld, text, B, E, C, scale, ws);
  if (int rc = check_launch("coop_head_logits_kernel")) return rc;
  if (mode == MODE_KGCOOP) {
    hipLaunchKernelGGL(coop_head_softmax_kernel, dim3((unsigned)B), threads, 0, s, labels, B, C, grad_scale, ws);
    if (int rc = check_launch("coop_head_softmax_kernel")) return rc;
    hipLaunchKernelGGL(coop_head_grad_kernel<true>, dim3((unsigned)C), threads, 0, s, feats, ld, text, B, E, C, scale, ws, d_text, d_text16,
                       (float*)nullptr, teacher, (const float*)tw.inty, tw.cosv, -(grad_scale * w / (float)C));
    if (int rc = check_launch("coop_head_grad_kernel")) return rc;
    hipLaunchKernelGGL(kgcoop_loss_kernel, dim3(1), dim3(256), 0, s, ws, tw, B, C, w, losses);
    return check_launch("kgcoop_loss_kernel");
  }
  HeadWs wt = ws, wk = ws;   // the teacher's logits with the teacher's norms; the distillation term's dz and row losses
  wt.z = tw.z_tea;
  wt.intx = tw.inty;
  wk.dz = tw.dz_kl;
  wk.loss = tw.loss_kl;
  hipLaunchKernelGGL(coop_head_logits_kernel, per_bc, threads, 0, s, feats, ld, teacher, B, E, C, scale, wt);
  if (int rc = check_launch("coop_head_logits_kernel")) return rc;
  hipLaunchKernelGGL(prograd_softmax_kernel, dim3((unsigned)B), threads, 0, s, labels, B, C, grad_scale, T, 1.f / T, ws, tw);
  if (int rc = check_launch("prograd_softmax_kernel")) return rc;
  hipLaunchKernelGGL(coop_head_grad_kernel<false>, dim3((unsigned)C), threads, 0, s, feats, ld, text, B, E, C, scale, ws, d_text, d_text16, losses,
                     (const float*)nullptr, (const float*)nullptr, (float*)nullptr, 0.f);
  if (int rc = check_launch("coop_head_grad_kernel")) return rc;
  hipLaunchKernelGGL(coop_head_grad_kernel<false>, dim3((unsigned)C), threads, 0, s, feats, ld, text, B, E, C, scale, wk, d_text_kl, (half_t*)nullptr,
                     losses + 1, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, 0.f);
  return check_launch("coop_head_grad_kernel");
}

// --------------------------------------------------------------------------------------------------------------------- context step
// one thread per element of ctx: the classes' rows added in ascending order (generic context), 1 / grad_scale, torch.optim.SGD's rule as
// torch's GPU kernels round it (sgd_element_fma, train_rules.h)
__device__ __forceinline__ float ctx_grad_element(const float* __restrict__ d_embed, int64_t idx, int C, int L, int D, int n_ctx, int per_class,
                                                  float inv_scale) {
  const int64_t per = (int64_t)n_ctx * D;
  const int d = (int)(idx % D), j = (int)((idx / D) % n_ctx);
  float g = 0.f;
  if (per_class) {
    const int64_t c = idx / per;
    g = d_embed[((c * L) + 1 + j) * D + d];
  } else {
    for (int64_t c = 0; c < C; ++c) g += d_embed[((c * L) + 1 + j) * D + d];
  }
  return g * inv_scale;
}

__global__ __launch_bounds__(THREADS) void ctx_step_kernel(const float* __restrict__ d_embed, float* __restrict__ ctx, float* __restrict__ buf,
                                                           float* __restrict__ grad_out, int C, int L, int D, int n_ctx, int per_class, float inv_scale,
                                                           const float* __restrict__ lr, SgdArgs sgd) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const int64_t per = (int64_t)n_ctx * D, total = per_class ? per * C : per;
  if (idx >= total) return;
  const float g = ctx_grad_element(d_embed, idx, C, L, D, n_ctx, per_class, inv_scale);
  if (grad_out) grad_out[idx] = g;
  if (ctx) sgd_element_fma(ctx, buf, idx, g, *lr, sgd);
}

int launch_ctx_step(const float* d_embed, float* ctx, float* buf, float* grad_out, int C, int L, int D, int n_ctx, int per_class, float grad_scale,
                    const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, hipStream_t s) {
  CLIPMI_REQUIRE(d_embed && (ctx || grad_out), CLIPMI_ERR_ARG, "ctx_step: null pointer (d_embed and one of ctx, grad_out are required)");
  CLIPMI_REQUIRE(!ctx || lr, CLIPMI_ERR_ARG, "ctx_step: null pointer (a step needs lr)");
  CLIPMI_REQUIRE(C >= 1 && D >= 1 && n_ctx >= 1 && 1 + n_ctx <= L, CLIPMI_ERR_SHAPE, "ctx_step: C=%d L=%d D=%d n_ctx=%d", C, L, D, n_ctx);
  CLIPMI_REQUIRE(std::isfinite(grad_scale) && grad_scale > 0.f, CLIPMI_ERR_ARG, "ctx_step: grad_scale=%g (finite, > 0)", grad_scale);
  CLIPMI_REQUIRE(momentum >= 0.f && momentum < 1.f && dampening >= 0.f && dampening < 1.f, CLIPMI_ERR_ARG,
                 "ctx_step: momentum=%g, dampening=%g (both in [0, 1))", momentum, dampening);
  CLIPMI_REQUIRE(weight_decay >= 0.f && std::isfinite(weight_decay), CLIPMI_ERR_ARG, "ctx_step: weight_decay=%g (finite, >= 0)", weight_decay);
  CLIPMI_REQUIRE(!nesterov || (momentum > 0.f && dampening == 0.f), CLIPMI_ERR_ARG, "ctx_step: nesterov needs a momentum and zero dampening");
  CLIPMI_REQUIRE(!ctx || momentum == 0.f || buf, CLIPMI_ERR_ARG, "ctx_step: null pointer (a momentum needs the buffer)");
  const int64_t total = (int64_t)n_ctx * D * (per_class ? C : 1);
  CLIPMI_REQUIRE(total < (1ll << 31) * THREADS, CLIPMI_ERR_SHAPE, "ctx_step: context too large");
  const SgdArgs sgd{momentum, (float)(1.0 - (double)dampening), weight_decay, nesterov ? 1 : 0, first_step ? 1 : 0};
  hipLaunchKernelGGL(ctx_step_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, d_embed, ctx, buf, grad_out, C, L, D, n_ctx,
                     per_class ? 1 : 0, 1.f / grad_scale, lr, sgd);
  return check_launch("ctx_step_kernel");
}

// ------------------------------------------------------------------------------------------------------------------ ProGrad's step
// (reference prograd.py:371-409).  a and b are the context gradients of the cross-entropy and of the distillation loss, each formed as
// ctx_step_kernel forms its gradient.  Two launches: the first keeps a and b and writes every workgroup's partial sums of a.a, b.b and a.b
// in float64 (a grid of at most DOT_BLOCKS workgroups, a function of the context's size alone); the second adds the partials in a fixed
// order in every workgroup, decides, and steps.  The reference compares dot(a / |a|, b / |b|) with 0: that is a.b < 0 unless a norm is
// zero or something is not finite, where the reference's comparison is false and the plain a is applied.
constexpr int DOT_BLOCKS = 256;

// workspace: partial sums [3, DOT_BLOCKS] float64 | a [total] | b [total] fp32
struct ProgradWs {
  double* part;
  float *a, *b;
};
inline size_t prograd_step_bytes(int64_t total) { return align256(3 * DOT_BLOCKS * sizeof(double)) + 2 * align256((size_t)total * 4); }
inline ProgradWs prograd_carve(void* ws, int64_t total) {
  ProgradWs w;
  char* p = static_cast<char*>(ws);
  w.part = reinterpret_cast<double*>(p);
  w.a = reinterpret_cast<float*>(p + align256(3 * DOT_BLOCKS * sizeof(double)));
  w.b = reinterpret_cast<float*>(p + align256(3 * DOT_BLOCKS * sizeof(double)) + align256((size_t)total * 4));
  return w;
}

// the 256 threads' three float64 sums by a binary tree over LDS; the result is valid in every thread
__device__ __forceinline__ void block_sum3_f64(double& x, double& y, double& z, double (*sl)[256]) {
  const int t = threadIdx.x;
  sl[0][t] = x; sl[1][t] = y; sl[2][t] = z;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
      sl[0][t] += sl[0][t + h];
      sl[1][t] += sl[1][t + h];
      sl[2][t] += sl[2][t + h];
    }
    __syncthreads();
  }
  x = sl[0][0]; y = sl[1][0]; z = sl[2][0];
}

__global__ __launch_bounds__(256) void prograd_dots_kernel(const float* __restrict__ d_embed_a, const float* __restrict__ d_embed_b, int C, int L, int D,
                                                           int n_ctx, int per_class, float inv_scale, int64_t total, ProgradWs w) {
  __shared__ double sl[3][256];
  double aa = 0.0, bb = 0.0, ab = 0.0;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const float a = ctx_grad_element(d_embed_a, idx, C, L, D, n_ctx, per_class, inv_scale);
    const float b = ctx_grad_element(d_embed_b, idx, C, L, D, n_ctx, per_class, inv_scale);
    w.a[idx] = a;
    w.b[idx] = b;
    aa += (double)a * (double)a;
    bb += (double)b * (double)b;
    ab += (double)a * (double)b;
  }
  block_sum3_f64(aa, bb, ab, sl);
  if (threadIdx.x == 0) {
    w.part[blockIdx.x] = aa;
    w.part[DOT_BLOCKS + blockIdx.x] = bb;
    w.part[2 * DOT_BLOCKS + blockIdx.x] = ab;
  }
}

// one thread per element of ctx; n_part: the first launch's grid.  g = a - lambda (a.b / b.b) b when a.b < 0, else a; then the SGD rule
__global__ __launch_bounds__(256) void prograd_step_kernel(ProgradWs w, int n_part, float lambda, float* __restrict__ ctx, float* __restrict__ buf,
                                                           float* __restrict__ grad_out, int* __restrict__ projected, double* __restrict__ dots,
                                                           int64_t total, const float* __restrict__ lr, SgdArgs sgd) {
#pragma clang fp contract(off)
  __shared__ double sl[3][256];
  const int t = threadIdx.x;
  double aa = t < n_part ? w.part[t] : 0.0, bb = t < n_part ? w.part[DOT_BLOCKS + t] : 0.0, ab = t < n_part ? w.part[2 * DOT_BLOCKS + t] : 0.0;
  block_sum3_f64(aa, bb, ab, sl);
  const bool finite = isfinite(aa) && isfinite(bb) && isfinite(ab);
  const bool project = finite && ab < 0.0 && aa > 0.0 && bb > 0.0;
  if (blockIdx.x == 0 && t == 0) {
    if (projected) *projected = project ? 1 : 0;
    if (dots) { dots[0] = aa; dots[1] = bb; dots[2] = ab; }
  }
  const int64_t idx = (int64_t)blockIdx.x * 256 + t;
  if (idx >= total) return;
  float g = w.a[idx];
  if (project) {
    const float k = (float)((double)lambda * (ab / bb));
    g = g - k * w.b[idx];
  }
  if (grad_out) grad_out[idx] = g;
  if (ctx) sgd_element_fma(ctx, buf, idx, g, *lr, sgd);
}

int launch_prograd_step(const float* d_embed_xe, const float* d_embed_kl, float* ctx, float* buf, float* grad_out, int* projected, double* dots, int C, int L,
                        int D, int n_ctx, int per_class, float grad_scale, float lambda, const float* lr, int first_step, float momentum, float dampening,
                        float weight_decay, int nesterov, void* workspace, size_t workspace_bytes, hipStream_t s) {
  CLIPMI_REQUIRE(d_embed_xe && d_embed_kl && workspace, CLIPMI_ERR_ARG, "prograd_step: null pointer (both d_embed and the workspace are required)");
  CLIPMI_REQUIRE(ctx || grad_out || projected || dots, CLIPMI_ERR_ARG, "prograd_step: null pointer (nothing to write)");
  CLIPMI_REQUIRE(!ctx || lr, CLIPMI_ERR_ARG, "prograd_step: null pointer (a step needs lr)");
  CLIPMI_REQUIRE(C >= 1 && D >= 1 && n_ctx >= 1 && 1 + n_ctx <= L, CLIPMI_ERR_SHAPE, "prograd_step: C=%d L=%d D=%d n_ctx=%d", C, L, D, n_ctx);
  CLIPMI_REQUIRE(std::isfinite(grad_scale) && grad_scale > 0.f, CLIPMI_ERR_ARG, "prograd_step: grad_scale=%g (finite, > 0)", grad_scale);
  CLIPMI_REQUIRE(std::isfinite(lambda), CLIPMI_ERR_ARG, "prograd_step: lambda=%g (finite)", lambda);
  CLIPMI_REQUIRE(momentum >= 0.f && momentum < 1.f && dampening >= 0.f && dampening < 1.f, CLIPMI_ERR_ARG,
                 "prograd_step: momentum=%g, dampening=%g (both in [0, 1))", momentum, dampening);
  CLIPMI_REQUIRE(weight_decay >= 0.f && std::isfinite(weight_decay), CLIPMI_ERR_ARG, "prograd_step: weight_decay=%g (finite, >= 0)", weight_decay);
  CLIPMI_REQUIRE(!nesterov || (momentum > 0.f && dampening == 0.f), CLIPMI_ERR_ARG, "prograd_step: nesterov needs a momentum and zero dampening");
  CLIPMI_REQUIRE(!ctx || momentum == 0.f || buf, CLIPMI_ERR_ARG, "prograd_step: null pointer (a momentum needs the buffer)");
  const int64_t total = (int64_t)n_ctx * D * (per_class ? C : 1);
  CLIPMI_REQUIRE(total < (1ll << 31) * 256, CLIPMI_ERR_SHAPE, "prograd_step: context too large");
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "prograd_step: the workspace must be 256-byte aligned");
  CLIPMI_REQUIRE(workspace_bytes >= prograd_step_bytes(total), CLIPMI_ERR_WORKSPACE, "prograd_step: workspace of %zu bytes, %zu needed", workspace_bytes,
                 prograd_step_bytes(total));
  const ProgradWs w = prograd_carve(workspace, total);
  const int64_t blocks = (total + 255) / 256;
  const int n_part = (int)(blocks < DOT_BLOCKS ? blocks : DOT_BLOCKS);
  const SgdArgs sgd{momentum, (float)(1.0 - (double)dampening), weight_decay, nesterov ? 1 : 0, first_step ? 1 : 0};
  hipLaunchKernelGGL(prograd_dots_kernel, dim3((unsigned)n_part), dim3(256), 0, s, d_embed_xe, d_embed_kl, C, L, D, n_ctx, per_class ? 1 : 0, 1.f / grad_scale,
                     total, w);
  if (int rc = check_launch("prograd_dots_kernel")) return rc;
  hipLaunchKernelGGL(prograd_step_kernel, dim3((unsigned)blocks), dim3(256), 0, s, w, n_part, lambda, ctx, buf, grad_out, projected, dots, total, lr, sgd);
  return check_launch("prograd_step_kernel");
}

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

int launch_operand_stats(const half_t* x, int64_t n, unsigned long long* stats, hipStream_t s) {
  if (!stats || n == 0) return CLIPMI_OK;
  const int64_t blocks = (n + THREADS - 1) / THREADS;
  hipLaunchKernelGGL(operand_stats_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(THREADS), 0, s, reinterpret_cast<const uint16_t*>(x), n, stats);
  return check_launch("operand_stats_kernel");
}

// ----------------------------------------------------------------------------------------------------------------- the tower drivers
int live_rows(const clipmi_model* m, int seq_rows) { return seq_rows > 0 && seq_rows < m->g.context_length ? seq_rows : m->g.context_length; }

struct Carver {
  char* base; size_t off = 0;
  explicit Carver(void* p) : base(static_cast<char*>(p)) {}
  template <typename T> T* take(size_t bytes) {
    T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align256(bytes);
    return r;
  }
};

// workspace shared by the training forward and the backward over M = C * L token rows
struct TrainWs {
  half_t* xn;      // [M, D]   LayerNorm output (forward) / fp16 copy of the gradient stream (backward)
  half_t* att;     // [M, D]   attention output / its gradient
  half_t* hid;     // [M, 4D]  QuickGELU output / the gradient of c_fc's output
  half_t* qkv;     // [M, 3D]  backward: dqkv
  float* dy;       // [M, D]   backward: the fp32 output of the dgrad GEMM in front of a LayerNorm backward
  half_t* rows16;  // [C, D]   ln_final's output rows
  half_t* dfeat16; // [C, E]
  float* dxf;      // [C, D]   d_out text_projection^T
  size_t bytes;
};
TrainWs carve_ws(void* p, int64_t M, int64_t C, int D, int E) {
  Carver c(p);
  TrainWs w;
  w.xn = c.take<half_t>((size_t)M * D * 2);
  w.att = c.take<half_t>((size_t)M * D * 2);
  w.hid = c.take<half_t>((size_t)M * D * 8);
  w.qkv = c.take<half_t>((size_t)M * D * 6);
  w.dy = c.take<float>((size_t)M * D * 4);
  w.rows16 = c.take<half_t>((size_t)C * D * 2);
  w.dfeat16 = c.take<half_t>((size_t)C * E * 2);
  w.dxf = c.take<float>((size_t)C * D * 4);
  w.bytes = c.off;
  return w;
}

// the stash: x[2 i] = block i's input rows, x[2 i + 1] = its rows before ln_2, x[2 layers] = ln_final's input; per block qkv and h
struct Stash {
  char* base; int64_t M; int D, layers; size_t x_bytes, qkv_bytes, h_bytes;
  float* x(int k) const { return reinterpret_cast<float*>(base + (size_t)k * x_bytes); }
  half_t* qkv(int i) const { return reinterpret_cast<half_t*>(base + (size_t)(2 * layers + 1) * x_bytes + (size_t)i * qkv_bytes); }
  half_t* h(int i) const { return reinterpret_cast<half_t*>(base + (size_t)(2 * layers + 1) * x_bytes + (size_t)layers * qkv_bytes + (size_t)i * h_bytes); }
  int32_t* idx() const { return reinterpret_cast<int32_t*>(base + (size_t)(2 * layers + 1) * x_bytes + (size_t)layers * (qkv_bytes + h_bytes)); }
  size_t bytes(int64_t C) const { return (size_t)(2 * layers + 1) * x_bytes + (size_t)layers * (qkv_bytes + h_bytes) + align256((size_t)C * 8); }
};
Stash carve_stash(void* p, int64_t M, int D, int layers) {
  Stash st;
  st.base = static_cast<char*>(p); st.M = M; st.D = D; st.layers = layers;
  st.x_bytes = align256((size_t)M * D * 4);
  st.qkv_bytes = align256((size_t)M * D * 6);
  st.h_bytes = align256((size_t)M * D * 8);
  return st;
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

int gemm(const half_t* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* residual, void* out, int64_t ldo, int out_dtype,
         int64_t M, int N, int K, int epilogue, hipStream_t s) {
  GemmArgs a{};
  a.A = A; a.lda = lda; a.W = static_cast<const half_t*>(W); a.ldw = ldw; a.bias = bias; a.residual = residual; a.out = out; a.ldo = ldo;
  a.out_dtype = out_dtype; a.M = (int)M; a.N = N; a.K = K; a.epilogue = epilogue;
  return launch_gemm(a, s);
}

int run_train_forward(clipmi_model* m, const void* prompts, int dtype, const float* ctx, int n_ctx, int per_class, const int32_t* eot, int C, int seq_rows,
                      float* out, void* workspace, void* stash_p, hipStream_t s) {
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
                 unsigned long long* stats, hipStream_t s) {
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
  }
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

}  // namespace
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

size_t clipmi_coop_head_workspace_bytes(int B, int E, int C) {
  if (B < 1 || E < 1 || C < 2) return 0;
  return align256(head_floats(B, C) * sizeof(float));
}

int clipmi_coop_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale, float grad_scale,
                     float* loss, float* d_text, void* d_text16, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  return launch_coop_head(feats, ld, labels, text, B, E, C, scale, grad_scale, loss, d_text, static_cast<half_t*>(d_text16), workspace, workspace_bytes,
                          (hipStream_t)stream);
}

int clipmi_ctx_step(const float* d_embed, float* ctx, float* buf, float* grad_out, int C, int L, int D, int n_ctx, int per_class, float grad_scale,
                    const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, clipmi_stream_t stream) {
  return launch_ctx_step(d_embed, ctx, buf, grad_out, C, L, D, n_ctx, per_class, grad_scale, lr, first_step, momentum, dampening, weight_decay, nesterov,
                         (hipStream_t)stream);
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

// workspace of the one-call step: the tower's workspace | text features [C, E] | their gradient [C, E] | d_embed [M, D] | the head's workspace
size_t clipmi_coop_train_step_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B) {
  size_t ws = 0;
  if (!m || n_prompts < 2 || B < 1 || clipmi_text_train_bytes(m, n_prompts, seq_rows, &ws, nullptr) != CLIPMI_OK) return 0;
  const size_t feat = align256((size_t)n_prompts * m->g.embed_dim * 4);
  return ws + 2 * feat + align256((size_t)n_prompts * live_rows(m, seq_rows) * m->g.text_width * 4) +
         clipmi_coop_head_workspace_bytes(B, m->g.embed_dim, n_prompts);
}

int clipmi_coop_train_step(clipmi_model* m, const clipmi_text_dgrad* wt, const void* prompts, int dtype, float* ctx, float* buf, int n_ctx,
                           int ctx_per_class, const int32_t* eot, int n_prompts, int seq_rows, const float* feats, int64_t ld, const int64_t* labels, int B,
                           float scale, float grad_scale, const float* lr, int first_step, float momentum, float dampening, float weight_decay,
                           int nesterov, float* loss, float* grad_out, void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes,
                           clipmi_stream_t stream) {
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "coop_train_step: null model");
  CLIPMI_REQUIRE(n_prompts >= 2 && B >= 1, CLIPMI_ERR_SHAPE, "coop_train_step: n_prompts=%d (>= 2), B=%d (>= 1)", n_prompts, B);
  CLIPMI_REQUIRE(ctx && lr, CLIPMI_ERR_ARG, "coop_train_step: null pointer (ctx and lr are required)");
  const size_t need = clipmi_coop_train_step_bytes(m, n_prompts, seq_rows, B);
  CLIPMI_REQUIRE(need > 0 && workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "coop_train_step: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  size_t tower = 0;
  clipmi_text_train_bytes(m, n_prompts, seq_rows, &tower, nullptr);
  if (int rc = check_train_call("coop_train_step", m, n_prompts, workspace, tower, stash, stash_bytes, seq_rows)) return rc;
  if (int rc = check_train_inputs("coop_train_step", m, prompts, dtype, ctx, n_ctx, eot, seq_rows, nullptr, 0)) return rc;
  if (int rc = check_dgrad("coop_train_step", m, wt)) return rc;
  const int L = live_rows(m, seq_rows), D = m->g.text_width, E = m->g.embed_dim;
  CLIPMI_REQUIRE(L <= AB_MAX_L, CLIPMI_ERR_SHAPE, "coop_train_step: %d token rows per prompt (at most %d)", L, AB_MAX_L);
  Carver c(static_cast<char*>(workspace) + tower);
  float* text = c.take<float>((size_t)n_prompts * E * 4);
  float* d_text = c.take<float>((size_t)n_prompts * E * 4);
  float* d_embed = c.take<float>((size_t)n_prompts * L * D * 4);
  void* head_ws = c.take<char>(clipmi_coop_head_workspace_bytes(B, E, n_prompts));
  hipStream_t s = (hipStream_t)stream;
  if (int rc = run_train_forward(m, prompts, dtype, ctx, n_ctx, ctx_per_class, eot, n_prompts, seq_rows, text, workspace, stash, s)) return rc;
  if (int rc = launch_coop_head(feats, ld, labels, text, B, E, n_prompts, scale, grad_scale, loss, d_text, nullptr, head_ws,
                                clipmi_coop_head_workspace_bytes(B, E, n_prompts), s))
    return rc;
  if (int rc = run_backward(m, wt, d_text, n_prompts, seq_rows, d_embed, workspace, stash, nullptr, s)) return rc;
  return launch_ctx_step(d_embed, ctx, buf, grad_out, n_prompts, L, D, n_ctx, ctx_per_class, grad_scale, lr, first_step, momentum, dampening, weight_decay,
                         nesterov, s);
}

size_t clipmi_prompt_head_workspace_bytes(int B, int E, int C, int mode) {
  if (B < 1 || E < 1 || C < 2 || mode < MODE_COOP || mode > MODE_PROGRAD) return 0;
  return align256(prompt_head_floats(B, C, mode) * sizeof(float));
}

int clipmi_prompt_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale, float grad_scale,
                       int mode, const float* teacher, float w, float T, float* losses, float* d_text, void* d_text16, float* d_text_kl,
                       void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  return launch_prompt_head(feats, ld, labels, text, B, E, C, scale, grad_scale, mode, teacher, w, T, losses, d_text, static_cast<half_t*>(d_text16),
                            d_text_kl, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t clipmi_prograd_step_workspace_bytes(int C, int D, int n_ctx, int per_class) {
  if (C < 1 || D < 1 || n_ctx < 1) return 0;
  return prograd_step_bytes((int64_t)n_ctx * D * (per_class ? C : 1));
}

int clipmi_prograd_step(const float* d_embed_xe, const float* d_embed_kl, float* ctx, float* buf, float* grad_out, int* projected, double* dots, int C,
                        int L, int D, int n_ctx, int per_class, float grad_scale, float lambda, const float* lr, int first_step, float momentum,
                        float dampening, float weight_decay, int nesterov, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  return launch_prograd_step(d_embed_xe, d_embed_kl, ctx, buf, grad_out, projected, dots, C, L, D, n_ctx, per_class, grad_scale, lambda, lr, first_step,
                             momentum, dampening, weight_decay, nesterov, workspace, workspace_bytes, (hipStream_t)stream);
}

// workspace of the one-call step: the tower's workspace | text features [C, E] | their gradient [C, E] | d_embed [M, D] | the head's workspace
// and, for ProGrad, | the second gradient [C, E] | the second d_embed [M, D] | clipmi_prograd_step's workspace
size_t clipmi_prompt_train_step_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int mode, int n_ctx, int ctx_per_class) {
  size_t ws = 0;
  if (!m || n_prompts < 2 || B < 1 || n_ctx < 1 || mode < MODE_COOP || mode > MODE_PROGRAD ||
      clipmi_text_train_bytes(m, n_prompts, seq_rows, &ws, nullptr) != CLIPMI_OK)
    return 0;
  const size_t feat = align256((size_t)n_prompts * m->g.embed_dim * 4);
  const size_t embed = align256((size_t)n_prompts * live_rows(m, seq_rows) * m->g.text_width * 4);
  size_t n = ws + 2 * feat + embed + clipmi_prompt_head_workspace_bytes(B, m->g.embed_dim, n_prompts, mode);
  if (mode == MODE_PROGRAD) n += feat + embed + clipmi_prograd_step_workspace_bytes(n_prompts, m->g.text_width, n_ctx, ctx_per_class);
  return n;
}

int clipmi_prompt_train_step(clipmi_model* m, const clipmi_text_dgrad* wt, const void* prompts, int dtype, float* ctx, float* buf, int n_ctx,
                             int ctx_per_class, const int32_t* eot, int n_prompts, int seq_rows, const float* feats, int64_t ld, const int64_t* labels,
                             int B, float scale, float grad_scale, int mode, const float* teacher, float w, float T, float lambda, const float* lr,
                             int first_step, float momentum, float dampening, float weight_decay, int nesterov, float* losses, float* grad_out,
                             int* projected, double* dots, void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes,
                             clipmi_stream_t stream) {
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "prompt_train_step: null model");
  CLIPMI_REQUIRE(mode == MODE_COOP || mode == MODE_KGCOOP || mode == MODE_PROGRAD, CLIPMI_ERR_ARG, "prompt_train_step: bad mode %d", mode);
  CLIPMI_REQUIRE(n_prompts >= 2 && B >= 1, CLIPMI_ERR_SHAPE, "prompt_train_step: n_prompts=%d (>= 2), B=%d (>= 1)", n_prompts, B);
  CLIPMI_REQUIRE(ctx && lr && losses, CLIPMI_ERR_ARG, "prompt_train_step: null pointer (ctx, lr and losses are required)");
  const size_t need = clipmi_prompt_train_step_bytes(m, n_prompts, seq_rows, B, mode, n_ctx, ctx_per_class);
  CLIPMI_REQUIRE(need > 0 && workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "prompt_train_step: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  size_t tower = 0;
  clipmi_text_train_bytes(m, n_prompts, seq_rows, &tower, nullptr);
  if (int rc = check_train_call("prompt_train_step", m, n_prompts, workspace, tower, stash, stash_bytes, seq_rows)) return rc;
  if (int rc = check_train_inputs("prompt_train_step", m, prompts, dtype, ctx, n_ctx, eot, seq_rows, nullptr, 0)) return rc;
  if (int rc = check_dgrad("prompt_train_step", m, wt)) return rc;
  const int L = live_rows(m, seq_rows), D = m->g.text_width, E = m->g.embed_dim;
  CLIPMI_REQUIRE(L <= AB_MAX_L, CLIPMI_ERR_SHAPE, "prompt_train_step: %d token rows per prompt (at most %d)", L, AB_MAX_L);
  const size_t head_bytes = clipmi_prompt_head_workspace_bytes(B, E, n_prompts, mode);
  Carver c(static_cast<char*>(workspace) + tower);
  float* text = c.take<float>((size_t)n_prompts * E * 4);
  float* d_text = c.take<float>((size_t)n_prompts * E * 4);
  float* d_embed = c.take<float>((size_t)n_prompts * L * D * 4);
  void* head_ws = c.take<char>(head_bytes);
  float *d_text_kl = nullptr, *d_embed_kl = nullptr;
  void* step_ws = nullptr;
  const size_t step_bytes = clipmi_prograd_step_workspace_bytes(n_prompts, D, n_ctx, ctx_per_class);
  if (mode == MODE_PROGRAD) {
    d_text_kl = c.take<float>((size_t)n_prompts * E * 4);
    d_embed_kl = c.take<float>((size_t)n_prompts * L * D * 4);
    step_ws = c.take<char>(step_bytes);
  }
  hipStream_t s = (hipStream_t)stream;
  if (int rc = run_train_forward(m, prompts, dtype, ctx, n_ctx, ctx_per_class, eot, n_prompts, seq_rows, text, workspace, stash, s)) return rc;
  if (int rc = launch_prompt_head(feats, ld, labels, text, B, E, n_prompts, scale, grad_scale, mode, teacher, w, T, losses, d_text, nullptr, d_text_kl, head_ws,
                                  head_bytes, s))
    return rc;
  if (int rc = run_backward(m, wt, d_text, n_prompts, seq_rows, d_embed, workspace, stash, nullptr, s)) return rc;
  if (mode != MODE_PROGRAD)
    return launch_ctx_step(d_embed, ctx, buf, grad_out, n_prompts, L, D, n_ctx, ctx_per_class, grad_scale, lr, first_step, momentum, dampening, weight_decay,
                           nesterov, s);
  // the stash is read-only in the backward; the tower's workspace is reused, so the second backward follows the first on the stream
  if (int rc = run_backward(m, wt, d_text_kl, n_prompts, seq_rows, d_embed_kl, workspace, stash, nullptr, s)) return rc;
  return launch_prograd_step(d_embed, d_embed_kl, ctx, buf, grad_out, projected, dots, n_prompts, L, D, n_ctx, ctx_per_class, grad_scale, lambda, lr,
                             first_step, momentum, dampening, weight_decay, nesterov, step_ws, step_bytes, s);
}

}  // extern "C"
