// CoCoOp's context and meta-net trained on the device (reference trainers/classification/cocoop.py:153-202, 259-278): the meta-net's
// forward with what its backward needs kept, the per-image prompt assembly in fp32, the per-pair loss head with its backward, the reduce of
// the tower's d_embed into the five gradients, one SGD launch over one parameter block, and the one-call step that puts the frozen text
// tower's training forward and backward (text_backward.hip) between them.  DESIGN.md "CoCoOp fit" has the data flow and the rounding points.
//   cocoop_meta_kernel         x_b = f_b / |f_b|, hid_b = relu(W1 x_b + b1), pi_b = W2 hid_b + b2
//   cocoop_embed_kernel        the B C prompts (image-major) as fp32 embeddings: context rows ctx_j + pi_b, every other row the widened base
//   cocoop_norm_kernel,        reciprocal norms, z[b, c] = s x_b . u_{b,c} by one wave per pair, the cross-entropy row of one image (xent_row),
//   cocoop_logits_kernel,      d_text of one pair through the normalisation's projection; workgroup 0 of the last also forms the batch loss
//   cocoop_softmax_kernel,
//   cocoop_dtext_kernel
//   cocoop_dcs_kernel          dcs[b, j, :] = (1 / grad_scale) sum_c d_embed[(b C + c) L + 1 + j, :], c ascending
//   cocoop_dw2_kernel          dctx, dpi, db2, dW2
//   cocoop_dhid_kernel         dhid[b, h] = [hid > 0] sum_d W2[d, h] dpi[b, d]
//   cocoop_dw1_kernel          db1, dW1
//   cocoop_step_kernel         sgd_element_fma over the parameter block [ctx | W1 | b1 | W2 | b2]
//   cocoop_shard_compact_kernel, cocoop_shard_rows_kernel, cocoop_dcs_partial_kernel, cocoop_dcs_gathered_kernel
//                              the class-sharded step's copies and sums (below, "the class-sharded step")
// Notation: N = B C prompts, prompt b C + c is image b with class c; H the meta-net's hidden width.  No float atomics and no workgroup waits
// for another: the same inputs give the same bits.
#include <cmath>

#include "common.h"
#include "model.h"
#include "train_rules.h"

namespace clipmi {
namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_H = 4096;

// the parameter block, its momentum block and its gradient block share one layout, in floats: ctx [n_ctx, D] | W1 [H, E] | b1 [H] | W2 [D, H] | b2 [D]
struct Block {
  int64_t w1, b1, w2, b2, total;
};
inline Block block_of(int n_ctx, int D, int E, int H) {
  Block k;
  k.w1 = (int64_t)n_ctx * D;
  k.b1 = k.w1 + (int64_t)H * E;
  k.w2 = k.b1 + H;
  k.b2 = k.w2 + (int64_t)D * H;
  k.total = k.b2 + D;
  return k;
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ld4(const half_t* p) {
  const f16x4 h = *reinterpret_cast<const f16x4*>(p);
  return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}

// -------------------------------------------------------------------------------------------------------------------- the meta-net
// grid (B), the shape of cocoop_ctx_kernel: the norm over the workgroup, then each wave owns hidden units wave, wave + 4, ..., then one
// thread per output element with the hidden units ascending.  hid is kept as the ReLU wrote it: its zeros are the backward's mask.
__global__ __launch_bounds__(THREADS) void cocoop_meta_kernel(const float* __restrict__ feats, int64_t ld, const float* __restrict__ w1,
                                                              const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                              float* __restrict__ x_n, float* __restrict__ hid, float* __restrict__ pi, int E, int H, int D) {
  extern __shared__ float sh[];   // [H]
  __shared__ float sw[WAVES];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* f = feats + (int64_t)b * ld;
  float s = 0.f;
  for (int e = t; e < E; e += THREADS) s = fmaf(f[e], f[e], s);
  const float inv = 1.f / sqrtf(block_sum<WAVES>(s, sw));
  for (int e = t; e < E; e += THREADS) x_n[(int64_t)b * E + e] = f[e] * inv;
  for (int h = wave; h < H; h += WAVES) {
    float a = 0.f;
    for (int e = lane; e < E; e += 64) a = fmaf(w1[(int64_t)h * E + e], f[e] * inv, a);
    a = wave_sum(a);
    if (lane == 0) {
      const float v = fmaxf(a + b1[h], 0.f);
      sh[h] = v;
      hid[(int64_t)b * H + h] = v;
    }
  }
  __syncthreads();
  for (int d = t; d < D; d += THREADS) {
    float a = b2[d];
    for (int h = 0; h < H; ++h) a = fmaf(w2[(int64_t)d * H + h], sh[h], a);
    pi[(int64_t)b * D + d] = a;
  }
}

int check_meta(const char* who, const float* feats, int64_t ld, const float* w1, const float* b1, const float* w2, const float* b2, const float* x_n,
               const float* hid, const float* pi, int B, int E, int H, int D) {
  CLIPMI_REQUIRE(feats && w1 && b1 && w2 && b2 && x_n && hid && pi, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(B >= 1 && E >= 1 && ld >= E && D >= 1, CLIPMI_ERR_SHAPE, "%s: B=%d E=%d ld=%lld D=%d", who, B, E, (long long)ld, D);
  CLIPMI_REQUIRE(H >= 1 && H <= MAX_H, CLIPMI_ERR_SHAPE, "%s: H=%d (1 .. %d)", who, H, MAX_H);
  return CLIPMI_OK;
}

int enqueue_meta(const float* feats, int64_t ld, const float* w1, const float* b1, const float* w2, const float* b2, float* x_n, float* hid, float* pi, int B,
                 int E, int H, int D, hipStream_t s) {
  hipLaunchKernelGGL(cocoop_meta_kernel, dim3((unsigned)B), dim3(THREADS), (size_t)H * sizeof(float), s, feats, ld, w1, b1, w2, b2, x_n, hid, pi, E, H, D);
  return check_launch("cocoop_meta_kernel");
}

// ------------------------------------------------------------------------------------------------------------------- the assembly
// one thread per four elements of the live rows: out[n, l, 4 i ..] of the prompt buffer [N, Lc, D], n = b C + c.  A context row is the one
// fp32 addition ctx[j] + pi[b]; every other row is widened from the base embedding of class c.  Rows behind the L live ones are not written.
template <typename T>
__global__ __launch_bounds__(THREADS) void cocoop_embed_kernel(const T* __restrict__ base, const float* __restrict__ ctx, const float* __restrict__ pi,
                                                               const int32_t* __restrict__ cls_eot, float* __restrict__ out, int32_t* __restrict__ eot, int B,
                                                               int C, int L, int Lc, int D, int n_ctx) {
  const int D4 = D / 4;
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const int64_t N = (int64_t)B * C;
  if (idx >= N * L * D4) return;
  const int d = (int)(idx % D4) * 4, l = (int)((idx / D4) % L);
  const int64_t n = idx / ((int64_t)D4 * L);
  const int c = (int)(n % C);
  const int64_t b = n / C;
  f32x4 v;
  if (l >= 1 && l <= n_ctx) {
    const f32x4 a = ld4(ctx + (int64_t)(l - 1) * D + d), p = ld4(pi + b * D + d);
    v = f32x4{a[0] + p[0], a[1] + p[1], a[2] + p[2], a[3] + p[3]};
  } else {
    v = ld4(base + ((int64_t)c * Lc + l) * D + d);
  }
  *reinterpret_cast<f32x4*>(out + (n * Lc + l) * D + d) = v;
  if (l == 0 && d == 0) eot[n] = cls_eot[c];
}

int check_embed(const char* who, const void* base, int dtype, const float* ctx, const float* pi, const int32_t* cls_eot, const float* out, const int32_t* eot,
                int B, int C, int L, int Lc, int D, int n_ctx, int min_c = 2) {
  CLIPMI_REQUIRE(base && ctx && pi && cls_eot && out && eot, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(dtype == CLIPMI_F16 || dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "%s: bad dtype %d", who, dtype);
  CLIPMI_REQUIRE(B >= 1 && C >= min_c, CLIPMI_ERR_SHAPE, "%s: B=%d (>= 1), C=%d (>= %d)", who, B, C, min_c);
  CLIPMI_REQUIRE(D >= 4 && D % 4 == 0, CLIPMI_ERR_SHAPE, "%s: D=%d (a multiple of 4)", who, D);
  CLIPMI_REQUIRE(L >= 1 && L <= Lc && n_ctx >= 1 && 1 + n_ctx <= L, CLIPMI_ERR_SHAPE, "%s: n_ctx=%d, L=%d of Lc=%d rows (SOS and the context must fit the live rows)",
                 who, n_ctx, L, Lc);
  CLIPMI_REQUIRE((int64_t)B * C * Lc < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: too many prompt tokens (B * C * Lc = %lld)", who, (long long)B * C * Lc);
  CLIPMI_REQUIRE((uintptr_t)base % 16 == 0 && (uintptr_t)ctx % 16 == 0 && (uintptr_t)pi % 16 == 0 && (uintptr_t)out % 16 == 0, CLIPMI_ERR_ARG,
                 "%s: base, ctx, pi and the prompt buffer must be 16-byte aligned", who);
  return CLIPMI_OK;
}

int enqueue_embed(const void* base, int dtype, const float* ctx, const float* pi, const int32_t* cls_eot, float* out, int32_t* eot, int B, int C, int L, int Lc,
                  int D, int n_ctx, hipStream_t s) {
  const int64_t total = (int64_t)B * C * L * (D / 4);
  const dim3 grid((unsigned)((total + THREADS - 1) / THREADS)), threads(THREADS);
  if (dtype == CLIPMI_F16)
    hipLaunchKernelGGL(cocoop_embed_kernel<half_t>, grid, threads, 0, s, (const half_t*)base, ctx, pi, cls_eot, out, eot, B, C, L, Lc, D, n_ctx);
  else
    hipLaunchKernelGGL(cocoop_embed_kernel<float>, grid, threads, 0, s, (const float*)base, ctx, pi, cls_eot, out, eot, B, C, L, Lc, D, n_ctx);
  return check_launch("cocoop_embed_kernel");
}

// --------------------------------------------------------------------------------------------------------------------------- the head
// (reference cocoop.py:186-202).  workspace of one batch, fp32: 1/|f_b| [B] | 1/|t_n| [N] | z [B, C] | dz [B, C] | row loss [B]
struct HeadWs {
  float *inf, *intx, *z, *dz, *loss;
};
inline size_t head_floats(int B, int C) { return 2 * (size_t)B + 3 * (size_t)B * C; }
inline HeadWs head_carve(void* ws, int B, int C) {
  HeadWs w;
  w.inf = static_cast<float*>(ws);
  w.intx = w.inf + B;
  w.z = w.intx + (size_t)B * C;
  w.dz = w.z + (size_t)B * C;
  w.loss = w.dz + (size_t)B * C;
  return w;
}

// one wave per row of feats (rows 0 .. B) or of text (rows B .. B + N): the reciprocal of its L2 norm
__global__ __launch_bounds__(THREADS) void cocoop_norm_kernel(const float* __restrict__ feats, int64_t ld, const float* __restrict__ text, int B, int E, int N,
                                                              HeadWs ws) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (r >= (int64_t)B + N) return;
  const float* row = r < B ? feats + r * ld : text + (r - B) * E;
  float s = 0.f;
  for (int e = lane; e < E; e += 64) s = fmaf(row[e], row[e], s);
  s = 1.f / sqrtf(wave_sum(s));
  if (lane == 0) (r < B ? ws.inf[r] : ws.intx[r - B]) = s;
}

// one wave per pair n = b C + c: z = scale (f_b . t_n) / (|f_b| |t_n|)
__global__ __launch_bounds__(THREADS) void cocoop_logits_kernel(const float* __restrict__ feats, int64_t ld, const float* __restrict__ text, int B, int E, int C,
                                                                float scale, HeadWs ws) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (n >= (int64_t)B * C) return;
  const float* f = feats + (n / C) * ld;
  const float* tx = text + n * E;
  float s = 0.f;
  for (int e = lane; e < E; e += 64) s = fmaf(f[e], tx[e], s);
  s = wave_sum(s);
  if (lane == 0) ws.z[n] = scale * ((s * ws.inf[n / C]) * ws.intx[n]);
}

// grid (B): row loss and dz = grad_scale (softmax(z) - onehot(y)) / B of one image.  A label outside [0, C) makes both NaN.
__global__ __launch_bounds__(THREADS) void cocoop_softmax_kernel(const int64_t* __restrict__ labels, int B, int C, float grad_scale, HeadWs ws) {
#pragma clang fp contract(off)
  __shared__ float sw[2 * WAVES];   // the maximum's, the sum's
  const int t = threadIdx.x, r = blockIdx.x;
  const float* z = ws.z + (size_t)r * C;
  float* dz = ws.dz + (size_t)r * C;
  const int64_t y = labels[r];
  if (y < 0 || y >= C) {      // the same for every thread of the workgroup: nobody waits at a barrier below
    for (int c = t; c < C; c += THREADS) dz[c] = NAN;
    if (t == 0) ws.loss[r] = NAN;
    return;
  }
  float m = -INFINITY;
  for (int c = t; c < C; c += THREADS) m = fmaxf(m, z[c]);
  m = block_max<WAVES>(m, sw);
  xent_row<WAVES>(z, dz, C, m, y, grad_scale / (float)B, sw + WAVES, ws.loss + r);
}

// one wave per pair n: du = scale dz[n] x_b (no sum over the images: every pair has its own text row), q = u_n . du,
// d_text[n] = (du - u_n q) / |t_n|.  Workgroup 0 then averages the row losses in float64; no wave leaves before that.
__global__ __launch_bounds__(THREADS) void cocoop_dtext_kernel(const float* __restrict__ feats, int64_t ld, const float* __restrict__ text, int B, int E, int C,
                                                               float scale, HeadWs ws, float* __restrict__ d_text, float* __restrict__ row_losses,
                                                               float* __restrict__ loss_out) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (n < (int64_t)B * C) {    // the same for every lane of the wave
    const int64_t b = n / C;
    const float* f = feats + b * ld;
    const float* tx = text + n * E;
    const float inf = ws.inf[b], itn = ws.intx[n], k = scale * ws.dz[n];
    float q = 0.f;
    for (int e = lane; e < E; e += 64) q = fmaf(tx[e] * itn, k * (f[e] * inf), q);
    q = wave_sum(q);
    for (int e = lane; e < E; e += 64) d_text[n * E + e] = (k * (f[e] * inf) - (tx[e] * itn) * q) * itn;
  }
  if (blockIdx.x != 0) return;   // the same for every thread of the workgroup
  if (row_losses)
    for (int r = threadIdx.x; r < B; r += THREADS) row_losses[r] = ws.loss[r];
  mean_loss_256(ws.loss, B, loss_out);
}

int check_head(const char* who, const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale, float grad_scale,
               const float* loss, const float* d_text, const void* workspace, size_t workspace_bytes) {
  CLIPMI_REQUIRE(feats && labels && text && loss && d_text && workspace, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(std::isfinite(scale), CLIPMI_ERR_ARG, "%s: scale=%g (finite)", who, scale);
  CLIPMI_REQUIRE(std::isfinite(grad_scale) && grad_scale > 0.f, CLIPMI_ERR_ARG, "%s: grad_scale=%g (finite, > 0)", who, grad_scale);
  CLIPMI_REQUIRE(B >= 1 && C >= 2 && E >= 1 && ld >= E, CLIPMI_ERR_SHAPE, "%s: B=%d C=%d E=%d ld=%lld", who, B, C, E, (long long)ld);
  CLIPMI_REQUIRE((int64_t)B * C < (1ll << 31) / E, CLIPMI_ERR_SHAPE, "%s: B * C * E too large", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 8 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 8-byte aligned", who);
  const size_t need = clipmi_cocoop_head_workspace_bytes(B, C);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  return CLIPMI_OK;
}

// the four launches alone: the caller has passed check_head
int enqueue_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale, float grad_scale, float* loss,
                 float* row_losses, float* d_text, void* workspace, hipStream_t s) {
  const HeadWs ws = head_carve(workspace, B, C);
  const int64_t N = (int64_t)B * C;
  const dim3 threads(THREADS);
  auto waves = [](int64_t items) { return dim3((unsigned)((items + WAVES - 1) / WAVES)); };
  hipLaunchKernelGGL(cocoop_norm_kernel, waves((int64_t)B + N), threads, 0, s, feats, ld, text, B, E, (int)N, ws);
  if (int rc = check_launch("cocoop_norm_kernel")) return rc;
  hipLaunchKernelGGL(cocoop_logits_kernel, waves(N), threads, 0, s, feats, ld, text, B, E, C, scale, ws);
  if (int rc = check_launch("cocoop_logits_kernel")) return rc;
  hipLaunchKernelGGL(cocoop_softmax_kernel, dim3((unsigned)B), threads, 0, s, labels, B, C, grad_scale, ws);
  if (int rc = check_launch("cocoop_softmax_kernel")) return rc;
  hipLaunchKernelGGL(cocoop_dtext_kernel, waves(N), threads, 0, s, feats, ld, text, B, E, C, scale, ws, d_text, row_losses, loss);
  return check_launch("cocoop_dtext_kernel");
}

// ------------------------------------------------------------------------------------------------------------------------- the reduce
// workspace, fp32: dcs [B, n_ctx, D] | dpi [B, D] | dhid [B, H]
struct ReduceWs {
  float *dcs, *dpi, *dhid;
};
inline size_t reduce_floats(int B, int n_ctx, int D, int H) { return (size_t)B * n_ctx * D + (size_t)B * D + (size_t)B * H; }
inline ReduceWs reduce_carve(void* ws, int B, int n_ctx, int D, int H) {
  ReduceWs w;
  w.dcs = static_cast<float*>(ws);
  w.dpi = w.dcs + (size_t)B * n_ctx * D;
  w.dhid = w.dpi + (size_t)B * D;
  return w;
}

// one thread per (b, j, d): the C prompts of image b, c ascending; 1 / grad_scale is applied here and nowhere else
__global__ __launch_bounds__(THREADS) void cocoop_dcs_kernel(const float* __restrict__ d_embed, ReduceWs ws, int B, int C, int L, int D, int n_ctx, float inv_scale) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)B * n_ctx * D) return;
  const int d = (int)(idx % D), j = (int)((idx / D) % n_ctx);
  const int64_t b = idx / ((int64_t)n_ctx * D);
  float g = 0.f;
  for (int64_t c = 0; c < C; ++c) g += d_embed[((b * C + c) * L + 1 + j) * D + d];
  ws.dcs[idx] = g * inv_scale;
}

// one thread per (d, h): dW2[d, h] = sum_b dpi[b, d] hid[b, h], b ascending, with dpi[b, d] = sum_j dcs[b, j, d], j ascending, formed by the
// same expression in every thread of a row d.  The thread of h = 0 also writes dpi[:, d], db2[d] = sum_b dpi[b, d] and dctx[j, d] = sum_b dcs[b, j, d].
__global__ __launch_bounds__(THREADS) void cocoop_dw2_kernel(ReduceWs ws, const float* __restrict__ hid, float* __restrict__ grad, Block k, int B, int D, int H,
                                                             int n_ctx) {
#pragma clang fp contract(off)
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)D * H) return;
  const int h = (int)(idx % H), d = (int)(idx / H);
  float w = 0.f, bias = 0.f;
  for (int b = 0; b < B; ++b) {
    float p = 0.f;
    for (int j = 0; j < n_ctx; ++j) p += ws.dcs[((int64_t)b * n_ctx + j) * D + d];
    w = fmaf(p, hid[(int64_t)b * H + h], w);
    if (h == 0) {
      ws.dpi[(int64_t)b * D + d] = p;
      bias += p;
    }
  }
  grad[k.w2 + idx] = w;
  if (h != 0) return;
  grad[k.b2 + d] = bias;
  for (int j = 0; j < n_ctx; ++j) {
    float g = 0.f;
    for (int b = 0; b < B; ++b) g += ws.dcs[((int64_t)b * n_ctx + j) * D + d];
    grad[(int64_t)j * D + d] = g;
  }
}

// grid (B), one wave per hidden unit in turn: dhid[b, h] = [hid[b, h] > 0] sum_d W2[d, h] dpi[b, d], lane-strided and the wave tree --
// torch's relu backward: zero where the OUTPUT is zero
__global__ __launch_bounds__(THREADS) void cocoop_dhid_kernel(ReduceWs ws, const float* __restrict__ hid, const float* __restrict__ w2, int D, int H) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int h = wave; h < H; h += WAVES) {
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s = fmaf(w2[(int64_t)d * H + h], ws.dpi[(int64_t)b * D + d], s);
    s = wave_sum(s);
    if (lane == 0) ws.dhid[(int64_t)b * H + h] = hid[(int64_t)b * H + h] > 0.f ? s : 0.f;
  }
}

// one thread per (h, e): dW1[h, e] = sum_b dhid[b, h] x[b, e], b ascending; the thread of e = 0 also writes db1[h] = sum_b dhid[b, h]
__global__ __launch_bounds__(THREADS) void cocoop_dw1_kernel(ReduceWs ws, const float* __restrict__ x_n, float* __restrict__ grad, Block k, int B, int E, int H) {
#pragma clang fp contract(off)
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)H * E) return;
  const int e = (int)(idx % E), h = (int)(idx / E);
  float w = 0.f, bias = 0.f;
  for (int b = 0; b < B; ++b) {
    const float g = ws.dhid[(int64_t)b * H + h];
    w = fmaf(g, x_n[(int64_t)b * E + e], w);
    bias += g;
  }
  grad[k.w1 + idx] = w;
  if (e == 0) grad[k.b1 + h] = bias;
}

int check_reduce(const char* who, const float* d_embed, const float* x_n, const float* hid, const float* w2, const float* grad, int B, int C, int L, int D, int E,
                 int H, int n_ctx, float grad_scale, const void* workspace, size_t workspace_bytes) {
  CLIPMI_REQUIRE(d_embed && x_n && hid && w2 && grad && workspace, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(B >= 1 && C >= 2 && D >= 1 && E >= 1, CLIPMI_ERR_SHAPE, "%s: B=%d C=%d D=%d E=%d", who, B, C, D, E);
  CLIPMI_REQUIRE(H >= 1 && H <= MAX_H, CLIPMI_ERR_SHAPE, "%s: H=%d (1 .. %d)", who, H, MAX_H);
  CLIPMI_REQUIRE(n_ctx >= 1 && 1 + n_ctx <= L, CLIPMI_ERR_SHAPE, "%s: n_ctx=%d, L=%d (SOS and the context must fit the live rows)", who, n_ctx, L);
  CLIPMI_REQUIRE(std::isfinite(grad_scale) && grad_scale > 0.f, CLIPMI_ERR_ARG, "%s: grad_scale=%g (finite, > 0)", who, grad_scale);
  CLIPMI_REQUIRE((int64_t)B * C * L < (1ll << 31) && block_of(n_ctx, D, E, H).total < (1ll << 31) && (int64_t)B * n_ctx * D < (1ll << 31), CLIPMI_ERR_SHAPE,
                 "%s: prompt set or parameter block too large", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 4 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 4-byte aligned", who);
  const size_t need = clipmi_cocoop_reduce_workspace_bytes(B, n_ctx, D, H);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  return CLIPMI_OK;
}

// the four launches alone: the caller has passed check_reduce
int enqueue_reduce(const float* d_embed, const float* x_n, const float* hid, const float* w2, float* grad, int B, int C, int L, int D, int E, int H, int n_ctx,
                   float grad_scale, void* workspace, hipStream_t s) {
  const ReduceWs ws = reduce_carve(workspace, B, n_ctx, D, H);
  const Block k = block_of(n_ctx, D, E, H);
  const dim3 threads(THREADS);
  auto per = [](int64_t items) { return dim3((unsigned)((items + THREADS - 1) / THREADS)); };
  hipLaunchKernelGGL(cocoop_dcs_kernel, per((int64_t)B * n_ctx * D), threads, 0, s, d_embed, ws, B, C, L, D, n_ctx, 1.f / grad_scale);
  if (int rc = check_launch("cocoop_dcs_kernel")) return rc;
  hipLaunchKernelGGL(cocoop_dw2_kernel, per((int64_t)D * H), threads, 0, s, ws, hid, grad, k, B, D, H, n_ctx);
  if (int rc = check_launch("cocoop_dw2_kernel")) return rc;
  hipLaunchKernelGGL(cocoop_dhid_kernel, dim3((unsigned)B), threads, 0, s, ws, hid, w2, D, H);
  if (int rc = check_launch("cocoop_dhid_kernel")) return rc;
  hipLaunchKernelGGL(cocoop_dw1_kernel, per((int64_t)H * E), threads, 0, s, ws, x_n, grad, k, B, E, H);
  return check_launch("cocoop_dw1_kernel");
}

// --------------------------------------------------------------------------------------------------------------------------- the step
// one thread per element of the parameter block: torch.optim.SGD's rule as torch's GPU kernels round it (sgd_element_fma), the same
// hyper-parameters for the five tensors -- the reference hands the whole prompt learner to one optimiser, so weight decay falls on the biases too
__global__ __launch_bounds__(THREADS) void cocoop_step_kernel(const float* __restrict__ grad, float* __restrict__ params, float* __restrict__ buf, int64_t total,
                                                              const float* __restrict__ lr, SgdArgs sgd) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= total) return;
  sgd_element_fma(params, buf, idx, grad[idx], *lr, sgd);
}

int check_step(const char* who, const float* grad, const float* params, const float* buf, const float* lr, int n_ctx, int D, int E, int H, float momentum,
               float dampening, float weight_decay, int nesterov) {
  CLIPMI_REQUIRE(grad && params && lr, CLIPMI_ERR_ARG, "%s: null pointer (grad, params and lr are required)", who);
  CLIPMI_REQUIRE(n_ctx >= 1 && D >= 1 && E >= 1, CLIPMI_ERR_SHAPE, "%s: n_ctx=%d D=%d E=%d", who, n_ctx, D, E);
  CLIPMI_REQUIRE(H >= 1 && H <= MAX_H, CLIPMI_ERR_SHAPE, "%s: H=%d (1 .. %d)", who, H, MAX_H);
  if (int rc = check_sgd(who, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE(momentum == 0.f || buf, CLIPMI_ERR_ARG, "%s: null pointer (a momentum needs the buffer)", who);
  CLIPMI_REQUIRE(block_of(n_ctx, D, E, H).total < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: parameter block too large", who);
  return CLIPMI_OK;
}

int enqueue_step(const float* grad, float* params, float* buf, int n_ctx, int D, int E, int H, const float* lr, int first_step, float momentum, float dampening,
                 float weight_decay, int nesterov, hipStream_t s) {
  const int64_t total = block_of(n_ctx, D, E, H).total;
  hipLaunchKernelGGL(cocoop_step_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, grad, params, buf, total, lr,
                     make_sgd_args(momentum, dampening, weight_decay, nesterov, first_step));
  return check_launch("cocoop_step_kernel");
}

// ------------------------------------------------------------------------------ the class-sharded step (DESIGN.md "Class-sharded CoCoOp fit")
// Rank r of G owns the classes [lo, hi) the balanced split gives it (shard_owner, train_rules.h) and runs the tower over its B C_r prompts,
// image-major: prompt b C_r + (c - lo) is image b with class c.  Its rows are no contiguous range of the unsharded [B, C, .], hence the copies.
//   cocoop_shard_compact_kernel   the gathered text features [G, >= B ceil(C / G), E] -> [B, C, E]
//   cocoop_shard_rows_kernel      rows {b C + c : lo <= c < hi} of d_text [B, C, E] -> [B C_r, E]
//   cocoop_dcs_partial_kernel     cocoop_dcs_kernel's sum over the rank's own classes, c ascending from 0.f, unscaled
//   cocoop_dcs_gathered_kernel    the G partials added in rank order from 0.f, times 1 / grad_scale once, into the reduce workspace's dcs
// With G = 1 the chain is cocoop_dcs_kernel's: (0 + the classes ascending) = p, 0.f + p = p (p is never -0: it started from +0), p * inv_scale.
// V = 4: 16-byte accesses; V = 1: scalar.
template <int V>
__device__ __forceinline__ void ldv(const float* __restrict__ p, float (&x)[V]) {
  if constexpr (V == 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3];
  } else {
    x[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void stv(float* __restrict__ p, const float (&x)[V]) {
  if constexpr (V == 4)
    *reinterpret_cast<f32x4*>(p) = f32x4{x[0], x[1], x[2], x[3]};
  else
    *p = x[0];
}
inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

// one thread per V elements of out [B, C, E]: block r of gathered (at r stride) holds rank r's [B, C_r, E] as its tower left it; the rows
// behind them and the elements behind B ceil(C / G) E of a block are never read
template <int V>
__global__ __launch_bounds__(THREADS) void cocoop_shard_compact_kernel(const float* __restrict__ gathered, float* __restrict__ out, int B, int C, int G,
                                                                       int E, int64_t stride) {
  const int EV = E / V;
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)B * C * EV) return;
  const int e = (int)(idx % EV) * V, c = (int)((idx / EV) % C);
  const int64_t b = idx / ((int64_t)EV * C);
  int lo;
  const int r = shard_owner(c, C, G, &lo);
  const int Cr = C / G + (r < C % G ? 1 : 0);
  float x[V];
  ldv<V>(gathered + (int64_t)r * stride + (b * Cr + (c - lo)) * E + e, x);
  stv<V>(out + (b * C + c) * E + e, x);
}

// one thread per V elements of out [B, C_r, E], C_r = hi - lo: out[b, c] = d_text[b, lo + c]
template <int V>
__global__ __launch_bounds__(THREADS) void cocoop_shard_rows_kernel(const float* __restrict__ d_text, float* __restrict__ out, int B, int C, int lo, int Cr,
                                                                    int E) {
  const int EV = E / V;
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)B * Cr * EV) return;
  const int e = (int)(idx % EV) * V, c = (int)((idx / EV) % Cr);
  const int64_t b = idx / ((int64_t)EV * Cr);
  float x[V];
  ldv<V>(d_text + (b * C + lo + c) * E + e, x);
  stv<V>(out + (b * Cr + c) * E + e, x);
}

// one thread per V elements of partial [B, n_ctx, D]: the C (the rank's own) prompts of image b, c ascending from 0.f; no scale
template <int V>
__global__ __launch_bounds__(THREADS) void cocoop_dcs_partial_kernel(const float* __restrict__ d_embed, float* __restrict__ partial, int B, int C, int L, int D,
                                                                     int n_ctx) {
  const int DV = D / V;
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)B * n_ctx * DV) return;
  const int d = (int)(idx % DV) * V, j = (int)((idx / DV) % n_ctx);
  const int64_t b = idx / ((int64_t)DV * n_ctx);
  float g[V];
#pragma unroll
  for (int v = 0; v < V; ++v) g[v] = 0.f;
  for (int64_t c = 0; c < C; ++c) {
    float x[V];
    ldv<V>(d_embed + ((b * C + c) * L + 1 + j) * D + d, x);
#pragma unroll
    for (int v = 0; v < V; ++v) g[v] += x[v];
  }
  stv<V>(partial + (b * n_ctx + j) * D + d, g);
}

// one thread per V elements of dcs [B n_ctx D]: the G partials (rank r's at partials + r stride) in rank order from 0.f, then 1 / grad_scale
template <int V>
__global__ __launch_bounds__(THREADS) void cocoop_dcs_gathered_kernel(const float* __restrict__ partials, int G, int64_t stride, float* __restrict__ dcs,
                                                                      int64_t total, float inv_scale) {
  const int64_t idx = ((int64_t)blockIdx.x * THREADS + threadIdx.x) * V;
  if (idx >= total) return;
  float g[V], x[V];
#pragma unroll
  for (int v = 0; v < V; ++v) g[v] = 0.f;
  for (int r = 0; r < G; ++r) {
    ldv<V>(partials + (int64_t)r * stride + idx, x);
#pragma unroll
    for (int v = 0; v < V; ++v) g[v] += x[v];
  }
#pragma unroll
  for (int v = 0; v < V; ++v) g[v] *= inv_scale;
  stv<V>(dcs + idx, g);
}

int check_reduce_gathered(const char* who, const float* partials, int G, int64_t rank_stride, const float* x_n, const float* hid, const float* w2,
                          const float* grad, int B, int D, int E, int H, int n_ctx, float grad_scale, const void* workspace, size_t workspace_bytes) {
  CLIPMI_REQUIRE(partials && x_n && hid && w2 && grad && workspace, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(G >= 1 && B >= 1 && D >= 1 && E >= 1 && n_ctx >= 1, CLIPMI_ERR_SHAPE, "%s: G=%d B=%d D=%d E=%d n_ctx=%d", who, G, B, D, E, n_ctx);
  CLIPMI_REQUIRE(H >= 1 && H <= MAX_H, CLIPMI_ERR_SHAPE, "%s: H=%d (1 .. %d)", who, H, MAX_H);
  CLIPMI_REQUIRE(std::isfinite(grad_scale) && grad_scale > 0.f, CLIPMI_ERR_ARG, "%s: grad_scale=%g (finite, > 0)", who, grad_scale);
  CLIPMI_REQUIRE(block_of(n_ctx, D, E, H).total < (1ll << 31) && (int64_t)B * n_ctx * D < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: parameter block too large", who);
  const int64_t block = (int64_t)B * n_ctx * D;
  CLIPMI_REQUIRE(rank_stride >= block && rank_stride < (1ll << 40), CLIPMI_ERR_SHAPE, "%s: rank_stride=%lld below a rank's block of %lld elements", who,
                 (long long)rank_stride, (long long)block);
  CLIPMI_REQUIRE((uintptr_t)workspace % 4 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 4-byte aligned", who);
  const size_t need = clipmi_cocoop_reduce_workspace_bytes(B, n_ctx, D, H);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  return CLIPMI_OK;
}

// the rank-ordered sum, then cocoop_reduce's last three launches as they are: the caller has passed check_reduce_gathered
int enqueue_reduce_gathered(const float* partials, int G, int64_t rank_stride, const float* x_n, const float* hid, const float* w2, float* grad, int B, int D,
                            int E, int H, int n_ctx, float grad_scale, void* workspace, hipStream_t s) {
  const ReduceWs ws = reduce_carve(workspace, B, n_ctx, D, H);
  const Block k = block_of(n_ctx, D, E, H);
  const dim3 threads(THREADS);
  auto per = [](int64_t items) { return dim3((unsigned)((items + THREADS - 1) / THREADS)); };
  const int64_t total = (int64_t)B * n_ctx * D;
  if (total % 4 == 0 && rank_stride % 4 == 0 && aligned16(partials) && aligned16(ws.dcs))
    hipLaunchKernelGGL(cocoop_dcs_gathered_kernel<4>, per(total / 4), threads, 0, s, partials, G, rank_stride, ws.dcs, total, 1.f / grad_scale);
  else
    hipLaunchKernelGGL(cocoop_dcs_gathered_kernel<1>, per(total), threads, 0, s, partials, G, rank_stride, ws.dcs, total, 1.f / grad_scale);
  if (int rc = check_launch("cocoop_dcs_gathered_kernel")) return rc;
  hipLaunchKernelGGL(cocoop_dw2_kernel, per((int64_t)D * H), threads, 0, s, ws, hid, grad, k, B, D, H, n_ctx);
  if (int rc = check_launch("cocoop_dw2_kernel")) return rc;
  hipLaunchKernelGGL(cocoop_dhid_kernel, dim3((unsigned)B), threads, 0, s, ws, hid, w2, D, H);
  if (int rc = check_launch("cocoop_dhid_kernel")) return rc;
  hipLaunchKernelGGL(cocoop_dw1_kernel, per((int64_t)H * E), threads, 0, s, ws, x_n, grad, k, B, E, H);
  return check_launch("cocoop_dw1_kernel");
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

size_t clipmi_cocoop_block_floats(int n_ctx, int D, int E, int H) {
  if (n_ctx < 1 || D < 1 || E < 1 || H < 1 || H > MAX_H) return 0;
  return (size_t)block_of(n_ctx, D, E, H).total;
}

int clipmi_cocoop_meta(const float* feats, int64_t ld, const float* w1, const float* b1, const float* w2, const float* b2, float* x_n, float* hid, float* pi,
                       int B, int E, int H, int D, clipmi_stream_t stream) {
  if (int rc = check_meta("cocoop_meta", feats, ld, w1, b1, w2, b2, x_n, hid, pi, B, E, H, D)) return rc;
  return enqueue_meta(feats, ld, w1, b1, w2, b2, x_n, hid, pi, B, E, H, D, (hipStream_t)stream);
}

int clipmi_cocoop_embed(const void* base, int dtype, const float* ctx, const float* pi, const int32_t* cls_eot, float* prompts, int32_t* eot, int B, int C,
                        int L, int Lc, int D, int n_ctx, clipmi_stream_t stream) {
  if (int rc = check_embed("cocoop_embed", base, dtype, ctx, pi, cls_eot, prompts, eot, B, C, L, Lc, D, n_ctx)) return rc;
  return enqueue_embed(base, dtype, ctx, pi, cls_eot, prompts, eot, B, C, L, Lc, D, n_ctx, (hipStream_t)stream);
}

size_t clipmi_cocoop_head_workspace_bytes(int B, int C) {
  if (B < 1 || C < 2) return 0;
  return align256(head_floats(B, C) * sizeof(float));
}

int clipmi_cocoop_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale, float grad_scale,
                       float* loss, float* row_losses, float* d_text, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  if (int rc = check_head("cocoop_head", feats, ld, labels, text, B, E, C, scale, grad_scale, loss, d_text, workspace, workspace_bytes)) return rc;
  return enqueue_head(feats, ld, labels, text, B, E, C, scale, grad_scale, loss, row_losses, d_text, workspace, (hipStream_t)stream);
}

size_t clipmi_cocoop_reduce_workspace_bytes(int B, int n_ctx, int D, int H) {
  if (B < 1 || n_ctx < 1 || D < 1 || H < 1 || H > MAX_H) return 0;
  return align256(reduce_floats(B, n_ctx, D, H) * sizeof(float));
}

int clipmi_cocoop_reduce(const float* d_embed, const float* x_n, const float* hid, const float* w2, float* grad, int B, int C, int L, int D, int E, int H,
                         int n_ctx, float grad_scale, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  if (int rc = check_reduce("cocoop_reduce", d_embed, x_n, hid, w2, grad, B, C, L, D, E, H, n_ctx, grad_scale, workspace, workspace_bytes)) return rc;
  return enqueue_reduce(d_embed, x_n, hid, w2, grad, B, C, L, D, E, H, n_ctx, grad_scale, workspace, (hipStream_t)stream);
}

int clipmi_cocoop_step(const float* grad, float* params, float* buf, int n_ctx, int D, int E, int H, const float* lr, int first_step, float momentum,
                       float dampening, float weight_decay, int nesterov, clipmi_stream_t stream) {
  if (int rc = check_step("cocoop_step", grad, params, buf, lr, n_ctx, D, E, H, momentum, dampening, weight_decay, nesterov)) return rc;
  return enqueue_step(grad, params, buf, n_ctx, D, E, H, lr, first_step, momentum, dampening, weight_decay, nesterov, (hipStream_t)stream);
}

// ---- the class-sharded step's entry points (include/clipmi.h; DESIGN.md "Class-sharded CoCoOp fit")

int clipmi_cocoop_embed_classes(const void* base, int dtype, const float* ctx, const float* pi, const int32_t* cls_eot, float* prompts, int32_t* eot, int B,
                                int C, int lo, int hi, int L, int Lc, int D, int n_ctx, clipmi_stream_t stream) {
  const char* who = "cocoop_embed_classes";
  CLIPMI_REQUIRE(base && cls_eot, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(dtype == CLIPMI_F16 || dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "%s: bad dtype %d", who, dtype);
  CLIPMI_REQUIRE(C >= 1 && lo >= 0 && lo < hi && hi <= C, CLIPMI_ERR_SHAPE, "%s: classes [%d, %d) of C=%d (a non-empty range)", who, lo, hi, C);
  CLIPMI_REQUIRE(Lc >= 1 && D >= 1 && (int64_t)C * Lc < (1ll << 31) / D, CLIPMI_ERR_SHAPE, "%s: C=%d Lc=%d D=%d", who, C, Lc, D);
  const void* own = static_cast<const char*>(base) + (size_t)lo * Lc * D * (dtype == CLIPMI_F16 ? 2 : 4);
  if (int rc = check_embed(who, own, dtype, ctx, pi, cls_eot + lo, prompts, eot, B, hi - lo, L, Lc, D, n_ctx, 1)) return rc;
  return enqueue_embed(own, dtype, ctx, pi, cls_eot + lo, prompts, eot, B, hi - lo, L, Lc, D, n_ctx, (hipStream_t)stream);
}

int clipmi_cocoop_shard_compact(const float* gathered, float* out, int B, int C, int G, int E, int64_t rank_stride, clipmi_stream_t stream) {
  const char* who = "cocoop_shard_compact";
  CLIPMI_REQUIRE(gathered && out, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(G >= 1 && C >= G && B >= 1 && E >= 1, CLIPMI_ERR_SHAPE, "%s: B=%d C=%d G=%d E=%d (C >= G >= 1)", who, B, C, G, E);
  const int64_t block = (int64_t)B * ((C + G - 1) / G) * E;
  CLIPMI_REQUIRE((int64_t)B * C < (1ll << 31) / E, CLIPMI_ERR_SHAPE, "%s: B * C * E too large", who);
  CLIPMI_REQUIRE(rank_stride >= block && rank_stride < (1ll << 40), CLIPMI_ERR_SHAPE, "%s: rank_stride=%lld below a rank's block of %lld elements", who,
                 (long long)rank_stride, (long long)block);
  const bool vec = E % 4 == 0 && rank_stride % 4 == 0 && aligned16(gathered) && aligned16(out);
  const int64_t total = (int64_t)B * C * (vec ? E / 4 : E);
  const dim3 grid((unsigned)((total + THREADS - 1) / THREADS)), threads(THREADS);
  if (vec)
    hipLaunchKernelGGL(cocoop_shard_compact_kernel<4>, grid, threads, 0, (hipStream_t)stream, gathered, out, B, C, G, E, rank_stride);
  else
    hipLaunchKernelGGL(cocoop_shard_compact_kernel<1>, grid, threads, 0, (hipStream_t)stream, gathered, out, B, C, G, E, rank_stride);
  return check_launch("cocoop_shard_compact_kernel");
}

int clipmi_cocoop_shard_rows(const float* d_text, float* out, int B, int C, int lo, int hi, int E, clipmi_stream_t stream) {
  const char* who = "cocoop_shard_rows";
  CLIPMI_REQUIRE(d_text && out, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(B >= 1 && C >= 1 && E >= 1 && lo >= 0 && lo < hi && hi <= C, CLIPMI_ERR_SHAPE, "%s: B=%d E=%d, classes [%d, %d) of C=%d (a non-empty range)", who,
                 B, E, lo, hi, C);
  CLIPMI_REQUIRE((int64_t)B * C < (1ll << 31) / E, CLIPMI_ERR_SHAPE, "%s: B * C * E too large", who);
  const bool vec = E % 4 == 0 && aligned16(d_text) && aligned16(out);
  const int64_t total = (int64_t)B * (hi - lo) * (vec ? E / 4 : E);
  const dim3 grid((unsigned)((total + THREADS - 1) / THREADS)), threads(THREADS);
  if (vec)
    hipLaunchKernelGGL(cocoop_shard_rows_kernel<4>, grid, threads, 0, (hipStream_t)stream, d_text, out, B, C, lo, hi - lo, E);
  else
    hipLaunchKernelGGL(cocoop_shard_rows_kernel<1>, grid, threads, 0, (hipStream_t)stream, d_text, out, B, C, lo, hi - lo, E);
  return check_launch("cocoop_shard_rows_kernel");
}

int clipmi_cocoop_dcs_partial(const float* d_embed, float* partial, int B, int C, int L, int D, int n_ctx, clipmi_stream_t stream) {
  const char* who = "cocoop_dcs_partial";
  CLIPMI_REQUIRE(d_embed && partial, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(B >= 1 && C >= 1 && D >= 1, CLIPMI_ERR_SHAPE, "%s: B=%d C=%d D=%d (all >= 1)", who, B, C, D);
  CLIPMI_REQUIRE(n_ctx >= 1 && 1 + n_ctx <= L, CLIPMI_ERR_SHAPE, "%s: n_ctx=%d, L=%d (SOS and the context must fit the live rows)", who, n_ctx, L);
  CLIPMI_REQUIRE((int64_t)B * C * L < (1ll << 31) && (int64_t)B * n_ctx * D < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: prompt set or block too large", who);
  const bool vec = D % 4 == 0 && aligned16(d_embed) && aligned16(partial);
  const int64_t total = (int64_t)B * n_ctx * (vec ? D / 4 : D);
  const dim3 grid((unsigned)((total + THREADS - 1) / THREADS)), threads(THREADS);
  if (vec)
    hipLaunchKernelGGL(cocoop_dcs_partial_kernel<4>, grid, threads, 0, (hipStream_t)stream, d_embed, partial, B, C, L, D, n_ctx);
  else
    hipLaunchKernelGGL(cocoop_dcs_partial_kernel<1>, grid, threads, 0, (hipStream_t)stream, d_embed, partial, B, C, L, D, n_ctx);
  return check_launch("cocoop_dcs_partial_kernel");
}

int clipmi_cocoop_reduce_gathered(const float* partials, int G, int64_t rank_stride, const float* x_n, const float* hid, const float* w2, float* grad, int B,
                                  int D, int E, int H, int n_ctx, float grad_scale, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  if (int rc = check_reduce_gathered("cocoop_reduce_gathered", partials, G, rank_stride, x_n, hid, w2, grad, B, D, E, H, n_ctx, grad_scale, workspace,
                                     workspace_bytes))
    return rc;
  return enqueue_reduce_gathered(partials, G, rank_stride, x_n, hid, w2, grad, B, D, E, H, n_ctx, grad_scale, workspace, (hipStream_t)stream);
}

// workspace: the tower's workspace (N prompts) | x_n [B, E] | hid [B, H] | pi [B, D] | prompts fp32 [N, Lc, D] | EOT int32 [N] | text features
// [N, E] | their gradient [N, E] | d_embed [N L, D] | the gradient block | the head's workspace | the reduce's workspace
size_t clipmi_cocoop_train_step_bytes(const clipmi_model* m, int C, int seq_rows, int B, int H, int n_ctx) {
  size_t ws = 0;
  if (!m || C < 2 || B < 1 || H < 1 || H > MAX_H || n_ctx < 1 || (int64_t)B * C >= (1ll << 31) / m->g.context_length) return 0;
  const int N = B * C, D = m->g.text_width, E = m->g.embed_dim;
  if (clipmi_text_train_bytes(m, N, seq_rows, &ws, nullptr) != CLIPMI_OK) return 0;
  const size_t feat = align256((size_t)N * E * 4);
  return ws + align256((size_t)B * E * 4) + align256((size_t)B * H * 4) + align256((size_t)B * D * 4) + align256((size_t)N * m->g.context_length * D * 4) +
         align256((size_t)N * 4) + 2 * feat + align256((size_t)N * live_rows(m, seq_rows) * D * 4) + align256((size_t)block_of(n_ctx, D, E, H).total * 4) +
         clipmi_cocoop_head_workspace_bytes(B, C) + clipmi_cocoop_reduce_workspace_bytes(B, n_ctx, D, H);
}

size_t clipmi_cocoop_train_step_scaled_bytes(const clipmi_model* m, int C, int seq_rows, int B, int H, int n_ctx) {
  const size_t base = clipmi_cocoop_train_step_bytes(m, C, seq_rows, B, H, n_ctx);
  return base ? base + block_step_scaled_bytes(block_of(n_ctx, m->g.text_width, m->g.embed_dim, H).total) : 0;
}

}  // extern "C"

// the one-call step, static (sc == NULL: grad_scale and first_step as given) or under the dynamic loss scale (sc: the head and the reduce run at
// grad_scale = 1, d_text is multiplied by the block's scale in between, and the block step divides, decides and applies)
static int cocoop_train_step(const char* who, const ScalerCall* sc, size_t need, clipmi_model* m, const clipmi_text_dgrad* wt, const void* base, int dtype,
                             float* params, float* buf, int n_ctx, int H, const int32_t* cls_eot, int C, int seq_rows, const float* feats, int64_t ld,
                             const int64_t* labels, int B, float scale, float grad_scale, const float* lr, int first_step, float momentum, float dampening,
                             float weight_decay, int nesterov, float* loss, float* grad_out, void* workspace, size_t workspace_bytes, void* stash,
                             size_t stash_bytes, hipStream_t s) {
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "%s: null model", who);
  CLIPMI_REQUIRE(params && lr && loss, CLIPMI_ERR_ARG, "%s: null pointer (params, lr and loss are required)", who);
  CLIPMI_REQUIRE(H >= 1 && H <= MAX_H, CLIPMI_ERR_SHAPE, "%s: H=%d (1 .. %d)", who, H, MAX_H);
  CLIPMI_REQUIRE(n_ctx >= 1, CLIPMI_ERR_SHAPE, "%s: n_ctx=%d (>= 1)", who, n_ctx);
  CLIPMI_REQUIRE(C >= 2 && B >= 1, CLIPMI_ERR_SHAPE, "%s: C=%d (>= 2), B=%d (>= 1)", who, C, B);
  CLIPMI_REQUIRE((int64_t)B * C < (1ll << 31) / m->g.context_length, CLIPMI_ERR_SHAPE, "%s: too many prompt tokens (B * C = %lld prompts)", who, (long long)B * C);
  CLIPMI_REQUIRE(need > 0, CLIPMI_ERR_SHAPE, "%s: B * C = %d prompts of %d rows are more than the tower takes", who, B * C, seq_rows);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  const int N = B * C;
  size_t tower = 0;
  clipmi_text_train_bytes(m, N, seq_rows, &tower, nullptr);
  if (int rc = check_train_call(who, m, N, workspace, tower, stash, stash_bytes, seq_rows)) return rc;
  if (int rc = check_dgrad(who, m, wt)) return rc;
  const int Lc = m->g.context_length, L = live_rows(m, seq_rows), D = m->g.text_width, E = m->g.embed_dim;
  CLIPMI_REQUIRE(L <= AB_MAX_L, CLIPMI_ERR_SHAPE, "%s: %d token rows per prompt (at most %d)", who, L, AB_MAX_L);
  const Block k = block_of(n_ctx, D, E, H);
  const size_t head_bytes = clipmi_cocoop_head_workspace_bytes(B, C), reduce_bytes = clipmi_cocoop_reduce_workspace_bytes(B, n_ctx, D, H);
  Carver c(static_cast<char*>(workspace) + tower);
  float* x_n = c.take<float>((size_t)B * E * 4);
  float* hid = c.take<float>((size_t)B * H * 4);
  float* pi = c.take<float>((size_t)B * D * 4);
  float* prompts = c.take<float>((size_t)N * Lc * D * 4);
  int32_t* eot = c.take<int32_t>((size_t)N * 4);
  float* text = c.take<float>((size_t)N * E * 4);
  float* d_text = c.take<float>((size_t)N * E * 4);
  float* d_embed = c.take<float>((size_t)N * L * D * 4);
  float* grad_ws = c.take<float>((size_t)k.total * 4);
  void* head_ws = c.take<char>(head_bytes);
  void* reduce_ws = c.take<char>(reduce_bytes);
  const size_t scaled_bytes = sc ? block_step_scaled_bytes(k.total) : 0;
  void* scaled_ws = c.take<char>(scaled_bytes);
  float* grad = grad_out && !sc ? grad_out : grad_ws;   // under the scaler the reduce's block is scale * gradient: grad_out gets the block step's
  if (sc) grad_scale = 1.f;
  const float *w1 = params + k.w1, *b1 = params + k.b1, *w2 = params + k.w2, *b2 = params + k.b2;
  // every refusal of the seven stages comes before the first launch: a refused call enqueues nothing
  if (int rc = check_meta(who, feats, ld, w1, b1, w2, b2, x_n, hid, pi, B, E, H, D)) return rc;
  if (int rc = check_embed(who, base, dtype, params, pi, cls_eot, prompts, eot, B, C, L, Lc, D, n_ctx)) return rc;
  if (int rc = check_train_inputs(who, m, prompts, CLIPMI_F32, nullptr, 0, eot, seq_rows, nullptr, 0)) return rc;
  if (int rc = check_head(who, feats, ld, labels, text, B, E, C, scale, grad_scale, loss, d_text, head_ws, head_bytes)) return rc;
  if (int rc = check_reduce(who, d_embed, x_n, hid, w2, grad, B, C, L, D, E, H, n_ctx, grad_scale, reduce_ws, reduce_bytes)) return rc;
  if (sc) {
    if (int rc = check_block_step_scaled(who, grad, params, buf, grad_out, lr, k.total, *sc, momentum, dampening,
                                         weight_decay, nesterov, scaled_ws, scaled_bytes))
      return rc;
  } else if (int rc = check_step(who, grad, params, buf, lr, n_ctx, D, E, H, momentum, dampening, weight_decay, nesterov)) {
    return rc;
  }
  if (int rc = enqueue_meta(feats, ld, w1, b1, w2, b2, x_n, hid, pi, B, E, H, D, s)) return rc;
  if (int rc = enqueue_embed(base, dtype, params, pi, cls_eot, prompts, eot, B, C, L, Lc, D, n_ctx, s)) return rc;
  if (int rc = run_train_forward(m, prompts, CLIPMI_F32, nullptr, 0, 0, eot, N, seq_rows, text, workspace, stash, s)) return rc;
  if (int rc = enqueue_head(feats, ld, labels, text, B, E, C, scale, grad_scale, loss, nullptr, d_text, head_ws, s)) return rc;
  if (sc)
    if (int rc = launch_grad_scale_rows(who, d_text, N, E, sc->state, s)) return rc;
  if (int rc = run_backward(m, wt, d_text, N, seq_rows, d_embed, workspace, stash, nullptr, s)) return rc;
  if (int rc = enqueue_reduce(d_embed, x_n, hid, w2, grad, B, C, L, D, E, H, n_ctx, grad_scale, reduce_ws, s)) return rc;
  if (sc)
    return launch_block_step_scaled(grad, params, buf, grad_out, k.total, *sc, lr, momentum, dampening,
                                    weight_decay, nesterov, scaled_ws, s);
  return enqueue_step(grad, params, buf, n_ctx, D, E, H, lr, first_step, momentum, dampening, weight_decay, nesterov, s);
}

extern "C" {

int clipmi_cocoop_train_step(clipmi_model* m, const clipmi_text_dgrad* wt, const void* base, int dtype, float* params, float* buf, int n_ctx, int H,
                             const int32_t* cls_eot, int C, int seq_rows, const float* feats, int64_t ld, const int64_t* labels, int B, float scale,
                             float grad_scale, const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, float* loss,
                             float* grad_out, void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes, clipmi_stream_t stream) {
  return cocoop_train_step("cocoop_train_step", nullptr, clipmi_cocoop_train_step_bytes(m, C, seq_rows, B, H, n_ctx), m, wt, base, dtype, params, buf, n_ctx, H,
                           cls_eot, C, seq_rows, feats, ld, labels, B, scale, grad_scale, lr, first_step, momentum, dampening, weight_decay, nesterov, loss,
                           grad_out, workspace, workspace_bytes, stash, stash_bytes, (hipStream_t)stream);
}

int clipmi_cocoop_train_step_scaled(clipmi_model* m, const clipmi_text_dgrad* wt, const void* base, int dtype, float* params, float* buf, int n_ctx, int H,
                                    const int32_t* cls_eot, int C, int seq_rows, const float* feats, int64_t ld, const int64_t* labels, int B, float scale,
                                    clipmi_scaler_state* state, float growth_factor, float backoff_factor, int growth_interval, const float* lr,
                                    float momentum, float dampening, float weight_decay, int nesterov, float* loss, float* grad_out, void* workspace,
                                    size_t workspace_bytes, void* stash, size_t stash_bytes, clipmi_stream_t stream) {
  const ScalerCall sc{state, growth_factor, backoff_factor, growth_interval};
  return cocoop_train_step("cocoop_train_step_scaled", &sc, clipmi_cocoop_train_step_scaled_bytes(m, C, seq_rows, B, H, n_ctx), m, wt, base, dtype, params, buf,
                           n_ctx, H, cls_eot, C, seq_rows, feats, ld, labels, B, scale, 1.f, lr, 0, momentum, dampening, weight_decay, nesterov, loss, grad_out,
                           workspace, workspace_bytes, stash, stash_bytes, (hipStream_t)stream);
}

// ---- one chunk of Bv validation images (DESIGN.md "Fit monitor", "CoCoOp and ProDA"): the launches of the inference forward (cocoop.py:186-199) --
// clipmi_cocoop_ctx, clipmi_cocoop_prompts, clipmi_text_encoder over the Bv C prompts -- and the fused per-pair tail and row score
// (clipmi_cocoop_val_rows).  workspace: the tower's (Bv C prompts) | ctx_shifted fp32 [Bv, n_ctx, D] | prompts fp16 [Bv C, Lc, D] | text fp32
// [Bv C, E], each part 256-byte aligned
size_t clipmi_cocoop_val_chunk_bytes(const clipmi_model* m, int C, int seq_rows, int Bv, int n_ctx) {
  if (!m || C < 1 || Bv < 1 || n_ctx < 1 || (int64_t)Bv * C >= (1ll << 31) / m->g.context_length) return 0;
  const size_t N = (size_t)Bv * C, D = m->g.text_width;
  return align256(clipmi_text_workspace_bytes(m, (int)N, seq_rows)) + align256((size_t)Bv * n_ctx * D * 4) + align256(N * m->g.context_length * D * 2) +
         align256(N * m->g.embed_dim * 4);
}

int clipmi_cocoop_val_chunk(clipmi_model* m, const void* base, int dtype, const float* params, int n_ctx, int H, const int32_t* eot, int C, int seq_rows,
                            const float* img_n, int Bv, float scale, const int64_t* labels, int n_bins, void* row_results, unsigned flags, void* workspace,
                            size_t workspace_bytes, clipmi_stream_t stream) {
  const char* who = "cocoop_val_chunk";
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "%s: null model", who);
  CLIPMI_REQUIRE(base && params && eot && img_n && labels && row_results && workspace, CLIPMI_ERR_ARG,
                 "%s: null pointer (base, params, eot, the image features, labels, the row results and the workspace are required)", who);
  CLIPMI_REQUIRE(dtype == CLIPMI_F16 || dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "%s: bad dtype %d", who, dtype);
  CLIPMI_REQUIRE(H >= 1 && H <= MAX_H, CLIPMI_ERR_SHAPE, "%s: H=%d (1 .. %d)", who, H, MAX_H);
  const int Lc = m->g.context_length, D = m->g.text_width, E = m->g.embed_dim;
  CLIPMI_REQUIRE(n_ctx >= 1 && n_ctx < Lc - 1 && D % 8 == 0, CLIPMI_ERR_SHAPE, "%s: n_ctx=%d (1 .. %d), D=%d (a multiple of 8)", who, n_ctx, Lc - 2, D);
  CLIPMI_REQUIRE(C >= 1 && Bv >= 1, CLIPMI_ERR_SHAPE, "%s: C=%d Bv=%d (both >= 1)", who, C, Bv);
  CLIPMI_REQUIRE((int64_t)Bv * C < (1ll << 31) / Lc, CLIPMI_ERR_SHAPE, "%s: too many prompt tokens (Bv * C = %lld prompts)", who, (long long)Bv * C);
  CLIPMI_REQUIRE(((uintptr_t)params | (uintptr_t)img_n | (uintptr_t)eot) % 4 == 0, CLIPMI_ERR_ARG, "%s: fp32 and int32 arrays must be 4-byte aligned", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 256-byte aligned", who);
  const size_t need = clipmi_cocoop_val_chunk_bytes(m, C, seq_rows, Bv, n_ctx);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  const int N = Bv * C;
  const size_t tower = align256(clipmi_text_workspace_bytes(m, N, seq_rows));
  Carver c(static_cast<char*>(workspace) + tower);
  float* ctx_shifted = c.take<float>((size_t)Bv * n_ctx * D * 4);
  half_t* prompts = c.take<half_t>((size_t)N * Lc * D * 2);
  float* text = c.take<float>((size_t)N * E * 4);
  // the tower's own refusals (unbound weights, the flags) through a call of no prompts, which launches nothing; the tail's through a look at its arguments
  if (int rc = clipmi_text_encoder(m, nullptr, CLIPMI_F16, nullptr, 0, seq_rows, nullptr, nullptr, workspace, tower, flags, stream)) return rc;
  CLIPMI_REQUIRE((uintptr_t)row_results % 16 == 0 && (uintptr_t)labels % 8 == 0, CLIPMI_ERR_ARG,
                 "%s: the row results must be 16-byte aligned, labels 8-byte aligned", who);
  CLIPMI_REQUIRE(C <= 16384, CLIPMI_ERR_SHAPE, "%s: C=%d (at most 16384: the row kernel keeps an image's logits in LDS)", who, C);
  CLIPMI_REQUIRE(n_bins >= 1 && n_bins <= 64, CLIPMI_ERR_ARG, "%s: n_bins=%d outside 1..64", who, n_bins);
  CLIPMI_REQUIRE(std::isfinite(scale), CLIPMI_ERR_ARG, "%s: scale=%g (finite)", who, scale);
  const Block k = block_of(n_ctx, D, E, H);
  if (int rc = clipmi_cocoop_ctx(img_n, params + k.w1, params + k.b1, params + k.w2, params + k.b2, params, ctx_shifted, Bv, E, H, D, n_ctx, stream)) return rc;
  if (int rc = clipmi_cocoop_prompts(base, dtype, ctx_shifted, prompts, Bv, C, Lc, D, n_ctx, stream)) return rc;
  if (int rc = clipmi_text_encoder(m, prompts, CLIPMI_F16, eot, N, seq_rows, nullptr, text, workspace, tower, flags, stream)) return rc;
  return clipmi_cocoop_val_rows(img_n, text, scale, labels, Bv, C, E, n_bins, row_results, stream);
}

}  // extern "C"
