// ProDA's collection of contexts trained on the device (reference trainers/classification/proda.py:146-228, 258-304): the prompt assembly
// at the three class-token positions, the prompt-distribution loss head with its backward, the gather-reduce of the tower's d_embed back
// into ctx [P, n_ctx, D] with torch.optim.SGD's step, and the one-call step that puts the frozen text tower's training forward and backward
// (text_backward.hip) between them.  DESIGN.md "ProDA fit" has the data flow, the formulas and the rounding points.
//   proda_embed_kernel         the C Pb class prompts (class-major, the selected contexts in the caller's end | middle | front order) and the
//                              P no-class prompts as fp32 embeddings, with the EOT index of each
//   proda_norm_kernel          reciprocal norms of feats, of the C Pb + P text rows
//   proda_mean_kernel          m_c = mean_q u_{c,q}
//   proda_logits_kernel        z[b, c] = s x_b . m_c + 0.5 s^2 sigma[b, c], sigma in the difference form (never the [E, C, C] covariance)
//   proda_softmax_kernel       row loss and dz of one sample (xent_row)
//   proda_gram_kernel,         the no-class term: G = n n^T, then alpha / (P (P - 1)) sum_{p != q} |G_pq| and its gradient through the norm
//   proda_nc_grad_kernel
//   proda_grad_kernel          d_text of one class's Pb rows; workgroup 0 also forms the three losses
//   proda_ctx_step_kernel      the context's gradient (classes ascending, the no-class row last) and the SGD rule
//   proda_scaled_grad_kernel   the same gradient under the dynamic loss scale: divided by the device scale, into the scaled step's workspace with
//                              one found-non-finite flag per workgroup; grad_scaler.hip's decision and step launches follow it
//   proda_shard_compact_kernel, proda_ctx_partial_kernel, proda_ctx_step_gathered_kernel, proda_gathered_scaled_grad_kernel
//                              the class-sharded step (one process per GPU, two all-gathers): described where they stand
// Notation: N = C Pb + P text rows; row c Pb + q is class c with the q-th selected context, row C Pb + p the no-class prompt of context p.
// No float atomics and no workgroup waits for another: the same inputs give the same bits.
#include <cmath>

#include "common.h"
#include "fit_monitor.h"
#include "l2norm.h"
#include "model.h"
#include "train_rules.h"

namespace clipmi {
namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int VAL_MAX_P = 4096;   // proda_val_mean_kernel keeps a class's P reciprocal norms in LDS
enum { POS_FRONT = 0, POS_MIDDLE = 1, POS_END = 2 };

// a class's name length as every kernel here reads it: inside [0, L - 3 - n_ctx], so that no row index computed from it leaves the L live
// rows (the callers check the values on the host; a bad one on the device moves tokens, it is never an address out of bounds)
__device__ __forceinline__ int clamp_name_len(int nl, int L, int n_ctx) { return min(max(nl, 0), L - 3 - n_ctx); }

// the token row of context vector j in a prompt of the position `ps` whose class name is nl tokens long (h = n_ctx / 2)
__device__ __forceinline__ int ctx_row(int ps, int j, int nl, int h) {
  if (ps == POS_FRONT) return 1 + nl + j;
  if (ps == POS_MIDDLE) return j < h ? 1 + j : 1 + nl + j;
  return 1 + j;
}

// ---------------------------------------------------------------------------------------------------------------------- the assembly
// token row l of a class prompt of the position `ps` whose name is nl tokens long: *j >= 0 -- context vector *j; *j < 0 -- the returned row of
// the class's base embedding (the row itself outside 1 .. n_ctx + nl, else name token t = base row 1 + n_ctx + t).  The training assembly and
// the validation's share it.
__device__ __forceinline__ int class_row_source(int l, int ps, int nl, int n_ctx, int* j) {
  const int r = l - 1, h = n_ctx / 2;
  *j = -1;
  if (r < 0 || r >= n_ctx + nl) return l;
  int t;
  if (ps == POS_FRONT) { *j = r < nl ? -1 : r - nl; t = r; }
  else if (ps == POS_MIDDLE) { *j = r < h ? r : r < h + nl ? -1 : r - nl; t = r - h; }
  else { *j = r < n_ctx ? r : -1; t = r - n_ctx; }
  return 1 + n_ctx + t;
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ld4(const half_t* p) {
  const f16x4 h = *reinterpret_cast<const f16x4*>(p);
  return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}

// one thread per four elements of the live rows: out[n, l, 4 i ..] of the prompt buffer [N, Lc, D].  A context row is copied from the fp32
// master as it is; a base row is widened.  Row l of a class prompt holds, with r = l - 1 < n_ctx + nl:
//   end     r < n_ctx: ctx[r], else the name token r - n_ctx
//   front   r < nl: the name token r, else ctx[r - nl]
//   middle  r < h: ctx[r];  r < h + nl: the name token r - h;  else ctx[r - nl]
// and the base row l everywhere else (SOS; '.', EOT and the padding from 1 + n_ctx + nl on).  Name token t is base row 1 + n_ctx + t.
// The EOT row of a class prompt is the class's own, cls_eot[c], whatever the position and the name length.
// The no-class prompts written are those of the contexts p0 .. p0 + Pn - 1 (all P of them but for a rank of the class-sharded fit, which
// owns a range); the class arrays then start at the rank's first class.
template <typename T>
__global__ __launch_bounds__(THREADS) void proda_embed_kernel(const T* __restrict__ base, const T* __restrict__ nc_base, const float* __restrict__ ctx,
                                                              const int32_t* __restrict__ sel, const int32_t* __restrict__ pos,
                                                              const int32_t* __restrict__ name_lens, const int32_t* __restrict__ cls_eot, float* __restrict__ out,
                                                              int32_t* __restrict__ eot, int C, int Pb, int P, int p0, int Pn, int L, int Lc, int D, int n_ctx) {
  const int D4 = D / 4;
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const int64_t N = (int64_t)C * Pb + Pn;
  if (idx >= N * L * D4) return;
  const int d = (int)(idx % D4) * 4, l = (int)((idx / D4) % L);
  const int64_t n = idx / ((int64_t)D4 * L);
  float* dst = out + (n * Lc + l) * D + d;
  f32x4 v;
  if (n >= (int64_t)C * Pb) {                       // [SOS | ctx_p | '.' EOT pad]
    const int p = p0 + (int)(n - (int64_t)C * Pb);
    v = (l >= 1 && l <= n_ctx) ? ld4(ctx + ((int64_t)p * n_ctx + (l - 1)) * D + d) : ld4(nc_base + (int64_t)l * D + d);
    if (l == 0 && d == 0) eot[n] = n_ctx + 2;
  } else {
    const int c = (int)(n / Pb), q = (int)(n % Pb);
    const int p = sel[q], nl = clamp_name_len(name_lens[c], L, n_ctx);
    if (l == 0 && d == 0) eot[n] = cls_eot[c];
    const T* cls = base + (int64_t)c * Lc * D + d;
    if (p < 0 || p >= P) {                          // a selection outside the collection is never an address: the prompt is poisoned
      v = f32x4{NAN, NAN, NAN, NAN};
    } else {
      int j;
      const int src = class_row_source(l, pos[p], nl, n_ctx, &j);
      v = j >= 0 ? ld4(ctx + ((int64_t)p * n_ctx + j) * D + d) : ld4(cls + (int64_t)src * D);
    }
  }
  *reinterpret_cast<f32x4*>(dst) = v;
}

// The validation's assembly (proda.py:146-222 with infer = True): the P prompts of the classes c0 .. c0 + cc - 1, class-major, a class's prompts in the
// order of `order` [P] (the caller's end | middle | front order of ALL contexts), in the MODEL's type T as the inference forward assembles them: a
// context row is the fp32 master rounded to T (what loading it into the module's parameter does), a base row is copied.  Only the L live rows are
// written.  One thread per four elements.  No no-class prompts.  eot[n] is the class's own EOT row.
template <typename T>
__global__ __launch_bounds__(THREADS) void proda_val_embed_kernel(const T* __restrict__ base, const float* __restrict__ ctx, const int32_t* __restrict__ order,
                                                                  const int32_t* __restrict__ pos, const int32_t* __restrict__ name_lens,
                                                                  const int32_t* __restrict__ cls_eot, T* __restrict__ out, int32_t* __restrict__ eot, int c0,
                                                                  int cc, int P, int L, int Lc, int D, int n_ctx) {
  const int D4 = D / 4;
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)cc * P * L * D4) return;
  const int d = (int)(idx % D4) * 4, l = (int)((idx / D4) % L);
  const int64_t n = idx / ((int64_t)D4 * L);
  const int c = c0 + (int)(n / P), q = (int)(n % P);
  const int p = order[q], nl = clamp_name_len(name_lens[c], L, n_ctx);
  if (l == 0 && d == 0) eot[n] = cls_eot[c];
  const T* cls = base + (int64_t)c * Lc * D + d;
  f32x4 v;
  if (p < 0 || p >= P) {
    v = f32x4{NAN, NAN, NAN, NAN};
  } else {
    int j;
    const int src = class_row_source(l, pos[p], nl, n_ctx, &j);
    v = j >= 0 ? ld4(ctx + ((int64_t)p * n_ctx + j) * D + d) : ld4(cls + (int64_t)src * D);
  }
  T* dst = out + (n * Lc + l) * D + d;
#pragma unroll
  for (int e = 0; e < 4; ++e) dst[e] = (T)v[e];
}

// The validation's classifier (proda.py:324-331): grid (cc), one workgroup per class.  Each of the class's P raw text features is normalised --
// its reciprocal norm by one wave in l2norm_kernel's order (row_sumsq), the product rounded to fp32 as that kernel stores it -- and the P unit
// features are added in ascending row order, then divided by P (group_mean_kernel's order): the bits of clipmi_l2_normalize followed by
// clipmi_group_mean, without the [cc P, E] normalised copy.  The mean is not renormalised.
__global__ __launch_bounds__(THREADS) void proda_val_mean_kernel(const float* __restrict__ text, float* __restrict__ mean, int P, int E, int vec8) {
  extern __shared__ float s_inv[];   // [P]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* rows = text + (int64_t)blockIdx.x * P * E;
  for (int p = wave; p < P; p += WAVES) {
    const float ss = row_sumsq(rows + (int64_t)p * E, E, vec8, lane);
    if (lane == 0) s_inv[p] = 1.0f / sqrtf(ss);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += THREADS) {
#pragma clang fp contract(off)   // the product and the sum round separately, as the two kernels round them: never one fma
    float s = 0.f;
    for (int p = 0; p < P; ++p) {
      const float unit = rows[(int64_t)p * E + e] * s_inv[p];
      s = s + unit;
    }
    mean[(int64_t)blockIdx.x * E + e] = s / (float)P;
  }
}

int check_embed(const char* who, const void* base, const void* nc_base, int dtype, const float* ctx, const int32_t* sel, const int32_t* pos,
                const int32_t* name_lens, const int32_t* cls_eot, const float* out, const int32_t* eot, int C, int Pb, int P, int L, int Lc, int D, int n_ctx,
                int min_C = 2) {
  CLIPMI_REQUIRE(base && nc_base && ctx && sel && pos && name_lens && cls_eot && out && eot, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(dtype == CLIPMI_F16 || dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "%s: bad dtype %d", who, dtype);
  CLIPMI_REQUIRE(C >= min_C && P >= 2 && Pb >= 1 && Pb <= P, CLIPMI_ERR_SHAPE, "%s: C=%d (>= %d), P=%d (>= 2), Pb=%d (1 .. P)", who, C, min_C, P, Pb);
  CLIPMI_REQUIRE(D >= 4 && D % 4 == 0 && n_ctx >= 1 && L <= Lc && n_ctx + 3 <= L, CLIPMI_ERR_SHAPE,
                 "%s: D=%d (a multiple of 4), n_ctx=%d, L=%d of Lc=%d rows (SOS, the context, '.' and EOT must fit)", who, D, n_ctx, L, Lc);
  CLIPMI_REQUIRE(((int64_t)C * Pb + P) * Lc < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: too many prompt tokens", who);
  CLIPMI_REQUIRE((uintptr_t)base % 16 == 0 && (uintptr_t)nc_base % 16 == 0 && (uintptr_t)ctx % 16 == 0 && (uintptr_t)out % 16 == 0, CLIPMI_ERR_ARG,
                 "%s: base, nc_base, ctx and the prompt buffer must be 16-byte aligned", who);
  return CLIPMI_OK;
}

// the launch alone: the caller has passed check_embed
int enqueue_embed(const void* base, const void* nc_base, int dtype, const float* ctx, const int32_t* sel, const int32_t* pos, const int32_t* name_lens,
                  const int32_t* cls_eot, float* out, int32_t* eot, int C, int Pb, int P, int L, int Lc, int D, int n_ctx, hipStream_t s, int p0 = 0,
                  int Pn = -1) {
  if (Pn < 0) Pn = P;   // every context's no-class prompt: the unsharded step
  const int64_t total = ((int64_t)C * Pb + Pn) * L * (D / 4);
  const dim3 grid((unsigned)((total + THREADS - 1) / THREADS)), threads(THREADS);
  if (dtype == CLIPMI_F16)
    hipLaunchKernelGGL(proda_embed_kernel<half_t>, grid, threads, 0, s, (const half_t*)base, (const half_t*)nc_base, ctx, sel, pos, name_lens, cls_eot, out,
                       eot, C, Pb, P, p0, Pn, L, Lc, D, n_ctx);
  else
    hipLaunchKernelGGL(proda_embed_kernel<float>, grid, threads, 0, s, (const float*)base, (const float*)nc_base, ctx, sel, pos, name_lens, cls_eot, out, eot,
                       C, Pb, P, p0, Pn, L, Lc, D, n_ctx);
  return check_launch("proda_embed_kernel");
}

// --------------------------------------------------------------------------------------------------------------------------- the head
// (reference proda.py:272-302).  workspace of one batch, fp32: 1/|f_b| [B] | 1/|text_n| [N] | m [C, E] | z [B, C] | dz [B, C] | row loss [B] |
// G [P, P]
struct ProdaWs {
  float *inf, *intx, *m, *z, *dz, *loss, *G;
};
inline size_t proda_head_floats(int B, int E, int C, int Pb, int P) {
  return 2 * (size_t)B + (size_t)C * Pb + P + (size_t)C * E + 2 * (size_t)B * C + (size_t)P * P;
}
inline ProdaWs proda_carve(void* ws, int B, int E, int C, int Pb, int P) {
  ProdaWs w;
  w.inf = static_cast<float*>(ws);
  w.intx = w.inf + B;
  w.m = w.intx + ((size_t)C * Pb + P);
  w.z = w.m + (size_t)C * E;
  w.dz = w.z + (size_t)B * C;
  w.loss = w.dz + (size_t)B * C;
  w.G = w.loss + B;
  return w;
}

// one wave per row of feats (rows 0 .. B) or of text (rows B .. B + N): the reciprocal of its L2 norm
__global__ __launch_bounds__(THREADS) void proda_norm_kernel(const float* __restrict__ feats, int64_t ld, const float* __restrict__ text, int B, int E, int N,
                                                             ProdaWs ws) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (r >= (int64_t)B + N) return;
  const float* row = r < B ? feats + r * ld : text + (r - B) * E;
  float s = 0.f;
  for (int e = lane; e < E; e += 64) s = fmaf(row[e], row[e], s);
  s = 1.f / sqrtf(wave_sum(s));
  if (lane == 0) (r < B ? ws.inf[r] : ws.intx[r - B]) = s;
}

// one thread per (c, e): m_c = (sum_q u_{c,q}) / Pb, q ascending
__global__ __launch_bounds__(THREADS) void proda_mean_kernel(const float* __restrict__ text, int E, int C, int Pb, ProdaWs ws) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)C * E) return;
  const int e = (int)(idx % E);
  const int64_t c = idx / E;
  float s = 0.f;
  for (int q = 0; q < Pb; ++q) s += text[(c * Pb + q) * E + e] * ws.intx[c * Pb + q];
  ws.m[idx] = s / (float)Pb;
}

// v_{c,q,e} = u_{c,q,e} - m_{c,e}
__device__ __forceinline__ float vdev(const float* __restrict__ text, const ProdaWs& ws, int64_t c, int q, int Pb, int E, int e) {
  return text[(c * Pb + q) * E + e] * ws.intx[c * Pb + q] - ws.m[c * E + e];
}

// one wave per (b, c): z = s x_b . m_c + 0.5 s^2 / (Pb + 1) sum_q sum_e x_be^2 (v_{y_b,q,e} - v_{c,q,e})^2 -- the second term is a sum of
// squares, and exactly zero at c = y_b and at Pb = 1.  A label outside [0, C) makes the row NaN and is not used as an address.
__global__ __launch_bounds__(THREADS) void proda_logits_kernel(const float* __restrict__ feats, int64_t ld, const int64_t* __restrict__ labels,
                                                               const float* __restrict__ text, int B, int E, int C, int Pb, float scale, ProdaWs ws) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (item >= (int64_t)B * C) return;
  const int b = (int)(item / C), c = (int)(item % C);
  const int64_t y = labels[b];
  if (y < 0 || y >= C) {
    if (lane == 0) ws.z[item] = NAN;
    return;
  }
  const float* f = feats + (int64_t)b * ld;
  const float inf = ws.inf[b];
  float dot = 0.f, sig = 0.f;
  for (int e = lane; e < E; e += 64) {
    const float x = f[e] * inf;
    dot = fmaf(x, ws.m[(int64_t)c * E + e], dot);
    float sq = 0.f;
    for (int q = 0; q < Pb; ++q) {
      const float d = vdev(text, ws, y, q, Pb, E, e) - vdev(text, ws, c, q, Pb, E, e);
      sq = fmaf(d, d, sq);
    }
    sig = fmaf(x * x, sq, sig);
  }
  dot = wave_sum(dot);
  sig = wave_sum(sig);
  if (lane == 0) ws.z[item] = fmaf(0.5f * scale * scale, sig / (float)(Pb + 1), scale * dot);
}

// grid (B): row loss and dz = grad_scale (softmax(z) - onehot(y)) / B of one sample
__global__ __launch_bounds__(THREADS) void proda_softmax_kernel(const int64_t* __restrict__ labels, int B, int C, float grad_scale, ProdaWs ws) {
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

// one wave per (p, q): G_pq = n_p . n_q of the normalised no-class rows (text rows C Pb ..)
__global__ __launch_bounds__(THREADS) void proda_gram_kernel(const float* __restrict__ nc, const float* __restrict__ inn, int E, int P, ProdaWs ws) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (item >= (int64_t)P * P) return;
  const int p = (int)(item / P), q = (int)(item % P);
  const float *a = nc + (int64_t)p * E, *b = nc + (int64_t)q * E;
  const float ia = inn[p], ib = inn[q];
  float s = 0.f;
  for (int e = lane; e < E; e += 64) s = fmaf(a[e] * ia, b[e] * ib, s);
  s = wave_sum(s);
  if (lane == 0) ws.G[item] = s;
}

__device__ __forceinline__ float sign_of(float g) { return g != g ? g : (float)((g > 0.f) - (g < 0.f)); }

// grid (P): dn_p = k sum_{q != p} sign(G_pq) n_q (q ascending; k = grad_scale 2 alpha / (P (P - 1)): G is symmetric and every pair counts
// twice in the mean), then d_text = (dn_p - n_p (n_p . dn_p)) / |nc_p|
__global__ __launch_bounds__(THREADS) void proda_nc_grad_kernel(const float* __restrict__ nc, const float* __restrict__ inn, int E, int P, float k, ProdaWs ws,
                                                                float* __restrict__ d_nc) {
  __shared__ float sw[WAVES];
  const int t = threadIdx.x, p = blockIdx.x;
  const float* G = ws.G + (size_t)p * P;
  const float ip = inn[p];
  float dot = 0.f;
  for (int e = t; e < E; e += THREADS) {   // pass 1: n_p . dn_p
    float dn = 0.f;
    for (int q = 0; q < P; ++q)
      if (q != p) dn = fmaf(sign_of(G[q]), nc[(int64_t)q * E + e] * inn[q], dn);
    dot = fmaf(nc[(int64_t)p * E + e] * ip, k * dn, dot);
  }
  dot = block_sum<WAVES>(dot, sw);
  for (int e = t; e < E; e += THREADS) {   // pass 2: the same dn again, then the projection
    float dn = 0.f;
    for (int q = 0; q < P; ++q)
      if (q != p) dn = fmaf(sign_of(G[q]), nc[(int64_t)q * E + e] * inn[q], dn);
    d_nc[(int64_t)p * E + e] = (k * dn - (nc[(int64_t)p * E + e] * ip) * dot) * ip;
  }
}

// grid (C): the Pb rows of class k.  With w[b, c] = 0.5 s^2 dz[b, c] and b, c ascending:
//   dm_k = s sum_b dz[b, k] x_b
//   dv_{k,q,e} = 2 / (Pb + 1) [ sum_b w[b, k] x_be^2 (v_kqe - v_{y_b,q,e}) + sum_{b: y_b = k} sum_c w[b, c] x_be^2 (v_kqe - v_cqe) ]
//   du_{k,q} = dv_{k,q} - mean_q' dv_{k,q'} + dm_k / Pb;   d_text_{k,q} = (du - u (u . du)) / |text_{k,q}|
// Phase 1 leaves du in d_text (every thread reads back only what it wrote itself); phase 2 projects row by row, its reductions alternating
// between two halves of sw so that one barrier per row is enough.  Workgroup 0 then forms losses = [upper + alpha m, upper, m]: upper the
// float64 mean of the row losses, m the float64 mean of |G_pq| over p != q in a fixed order.
__global__ __launch_bounds__(THREADS) void proda_grad_kernel(const float* __restrict__ feats, int64_t ld, const int64_t* __restrict__ labels,
                                                             const float* __restrict__ text, int B, int E, int C, int Pb, int P, float scale, float alpha,
                                                             ProdaWs ws, float* __restrict__ d_text, float* __restrict__ losses) {
  __shared__ float sw[2][WAVES];
  __shared__ double sl[1][256];
  const int t = threadIdx.x, k = blockIdx.x;
  const float half_s2 = 0.5f * scale * scale, inv_pb = 1.f / (float)Pb, two_over = 2.f / (float)(Pb + 1);
  for (int e = t; e < E; e += THREADS) {
    float dm = 0.f;
    for (int b = 0; b < B; ++b) dm = fmaf(ws.dz[(size_t)b * C + k], feats[(int64_t)b * ld + e] * ws.inf[b], dm);
    dm *= scale;
    float mean = 0.f;
    for (int q = 0; q < Pb; ++q) {
      const float vk = vdev(text, ws, k, q, Pb, E, e);
      float a = 0.f;
      for (int b = 0; b < B; ++b) {
        const int64_t y = labels[b];
        const float x = feats[(int64_t)b * ld + e] * ws.inf[b], x2 = x * x;
        const float vy = (y < 0 || y >= C) ? NAN : vdev(text, ws, y, q, Pb, E, e);
        a = fmaf(half_s2 * ws.dz[(size_t)b * C + k] * x2, vk - vy, a);
        if (y == k)
          for (int c = 0; c < C; ++c) a = fmaf(half_s2 * ws.dz[(size_t)b * C + c] * x2, vk - vdev(text, ws, c, q, Pb, E, e), a);
      }
      a *= two_over;
      d_text[((int64_t)k * Pb + q) * E + e] = a;
      mean += a;
    }
    mean *= inv_pb;
    for (int q = 0; q < Pb; ++q) {
      float* p = d_text + ((int64_t)k * Pb + q) * E + e;
      *p = (*p - mean) + dm * inv_pb;
    }
  }
  for (int q = 0; q < Pb; ++q) {
    const float* tx = text + ((int64_t)k * Pb + q) * E;
    float* dt = d_text + ((int64_t)k * Pb + q) * E;
    const float itn = ws.intx[(int64_t)k * Pb + q];
    float dot = 0.f;
    for (int e = t; e < E; e += THREADS) dot = fmaf(tx[e] * itn, dt[e], dot);
    dot = block_sum<WAVES>(dot, sw[q & 1]);
    for (int e = t; e < E; e += THREADS) dt[e] = (dt[e] - (tx[e] * itn) * dot) * itn;
  }
  if (k != 0) return;   // the same for every thread of the workgroup
  mean_loss_256(ws.loss, B, losses + 1);
  double s[1] = {0.0};
  for (int i = t; i < P * P; i += 256)
    if (i / P != i % P) s[0] += (double)fabsf(ws.G[i]);
  block_sum_f64(s, sl);
  if (t == 0) {
#pragma clang fp contract(off)
    const float lm = (float)(s[0] / ((double)P * (double)(P - 1)));
    losses[2] = lm;
    losses[0] = losses[1] + alpha * lm;
  }
}

int check_head(const char* who, const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, int Pb, int P, float scale,
                float grad_scale, float alpha, const float* losses, const float* d_text, const void* workspace, size_t workspace_bytes) {
  CLIPMI_REQUIRE(feats && labels && text && losses && d_text && workspace, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(std::isfinite(scale) && std::isfinite(grad_scale), CLIPMI_ERR_ARG, "%s: scale=%g, grad_scale=%g (both finite)", who, scale, grad_scale);
  CLIPMI_REQUIRE(std::isfinite(alpha) && alpha >= 0.f, CLIPMI_ERR_ARG, "%s: alpha=%g (finite, >= 0)", who, alpha);
  CLIPMI_REQUIRE(B >= 1 && C >= 2 && E >= 1 && ld >= E && P >= 2 && Pb >= 1 && Pb <= P, CLIPMI_ERR_SHAPE, "%s: B=%d C=%d E=%d ld=%lld Pb=%d P=%d", who, B, C, E,
                 (long long)ld, Pb, P);
  CLIPMI_REQUIRE((int64_t)B * C < (1ll << 31) && (int64_t)C * Pb + P < (1ll << 31) / E && (int64_t)P * P < (1ll << 31), CLIPMI_ERR_SHAPE,
                 "%s: B * C, (C * Pb + P) * E or P * P too large", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 8 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 8-byte aligned", who);
  const size_t need = clipmi_proda_head_workspace_bytes(B, E, C, Pb, P);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  return CLIPMI_OK;
}

// the seven launches alone: the caller has passed check_head
int enqueue_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, int Pb, int P, float scale, float grad_scale,
                 float alpha, float* losses, float* d_text, void* workspace, hipStream_t s) {
  const ProdaWs ws = proda_carve(workspace, B, E, C, Pb, P);
  const int N = C * Pb + P;
  const float* nc = text + (int64_t)C * Pb * E;
  const float* inn = ws.intx + (int64_t)C * Pb;
  const dim3 threads(THREADS);
  auto waves = [](int64_t items) { return dim3((unsigned)((items + WAVES - 1) / WAVES)); };
  hipLaunchKernelGGL(proda_norm_kernel, waves((int64_t)B + N), threads, 0, s, feats, ld, text, B, E, N, ws);
  if (int rc = check_launch("proda_norm_kernel")) return rc;
  hipLaunchKernelGGL(proda_mean_kernel, dim3((unsigned)(((int64_t)C * E + THREADS - 1) / THREADS)), threads, 0, s, text, E, C, Pb, ws);
  if (int rc = check_launch("proda_mean_kernel")) return rc;
  hipLaunchKernelGGL(proda_logits_kernel, waves((int64_t)B * C), threads, 0, s, feats, ld, labels, text, B, E, C, Pb, scale, ws);
  if (int rc = check_launch("proda_logits_kernel")) return rc;
  hipLaunchKernelGGL(proda_softmax_kernel, dim3((unsigned)B), threads, 0, s, labels, B, C, grad_scale, ws);
  if (int rc = check_launch("proda_softmax_kernel")) return rc;
  hipLaunchKernelGGL(proda_gram_kernel, waves((int64_t)P * P), threads, 0, s, nc, inn, E, P, ws);
  if (int rc = check_launch("proda_gram_kernel")) return rc;
  const float k = (float)((double)grad_scale * 2.0 * (double)alpha / ((double)P * (double)(P - 1)));
  hipLaunchKernelGGL(proda_nc_grad_kernel, dim3((unsigned)P), threads, 0, s, nc, inn, E, P, k, ws, d_text + (int64_t)C * Pb * E);
  if (int rc = check_launch("proda_nc_grad_kernel")) return rc;
  hipLaunchKernelGGL(proda_grad_kernel, dim3((unsigned)C), threads, 0, s, feats, ld, labels, text, B, E, C, Pb, P, scale, alpha, ws, d_text, losses);
  return check_launch("proda_grad_kernel");
}

// ------------------------------------------------------------------------------------------------------------------- the context step
// one thread per element (p, j, d) of ctx [P, n_ctx, D].  If p is selected at slot q: the rows of the C class prompts that hold context
// vector j, c ascending; then, always, the no-class prompt's row 1 + j, added last; 1 / grad_scale; torch.optim.SGD's rule as torch's GPU
// kernels round it (sgd_element_fma).  A context outside the selection still moves by the no-class term, weight decay and momentum.
__device__ __forceinline__ float proda_grad_element(const float* __restrict__ d_embed, int64_t idx, const int32_t* __restrict__ sel,
                                                    const int32_t* __restrict__ pos, const int32_t* __restrict__ name_lens, int C, int Pb, int L, int D,
                                                    int n_ctx, float inv_scale) {
  const int d = (int)(idx % D), j = (int)((idx / D) % n_ctx), p = (int)(idx / ((int64_t)n_ctx * D));
  int slot = -1;
  for (int q = 0; q < Pb; ++q)
    if (sel[q] == p && slot < 0) slot = q;
  float g = 0.f;
  if (slot >= 0) {
    const int ps = pos[p], h = n_ctx / 2;
    for (int64_t c = 0; c < C; ++c) {
      const int row = ctx_row(ps, j, clamp_name_len(name_lens[c], L, n_ctx), h);
      g += d_embed[((c * Pb + slot) * L + row) * D + d];
    }
  }
  g += d_embed[(((int64_t)C * Pb + p) * L + 1 + j) * D + d];
  return g * inv_scale;
}

__global__ __launch_bounds__(THREADS) void proda_ctx_step_kernel(const float* __restrict__ d_embed, float* __restrict__ ctx, float* __restrict__ buf,
                                                                 float* __restrict__ grad_out, const int32_t* __restrict__ sel, const int32_t* __restrict__ pos,
                                                                 const int32_t* __restrict__ name_lens, int C, int Pb, int P, int L, int D, int n_ctx,
                                                                 float inv_scale, const float* __restrict__ lr, SgdArgs sgd) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)P * n_ctx * D) return;
  const float g = proda_grad_element(d_embed, idx, sel, pos, name_lens, C, Pb, L, D, n_ctx, inv_scale);
  if (grad_out) grad_out[idx] = g;
  if (ctx) sgd_element_fma(ctx, buf, idx, g, *lr, sgd);
}

// The same gradient under the dynamic loss scale (grad_scaler.hip, model.h): 1 / state->scale read on the device, the unscaled gradient into
// the step's workspace and into grad_out, and the workgroup's flag set when any element it produced is an inf or a NaN.  Every context
// takes part: an unselected one is its no-class row.  A row of d_embed that no context vector sits on is never read.
static_assert(THREADS == SCALED_THREADS, "one found-non-finite flag per workgroup of the gradient launch");
__global__ __launch_bounds__(THREADS) void proda_scaled_grad_kernel(const float* __restrict__ d_embed, float* __restrict__ grad_out,
                                                                    const int32_t* __restrict__ sel, const int32_t* __restrict__ pos,
                                                                    const int32_t* __restrict__ name_lens, int C, int Pb, int P, int L, int D, int n_ctx,
                                                                    const clipmi_scaler_state* __restrict__ st, ScaledWs w) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  int bad = 0;
  if (idx < (int64_t)P * n_ctx * D) {
    const float g = proda_grad_element(d_embed, idx, sel, pos, name_lens, C, Pb, L, D, n_ctx, 1.f / st->scale);
    w.grad[idx] = g;
    if (grad_out) grad_out[idx] = g;
    bad = !isfinite(g);
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) w.flags[blockIdx.x] = bad ? 1 : 0;
}

int check_ctx_step(const char* who, const float* d_embed, float* ctx, float* buf, float* grad_out, const int32_t* sel, const int32_t* pos,
                    const int32_t* name_lens, int C, int Pb, int P, int L, int D, int n_ctx, float grad_scale, const float* lr, int first_step, float momentum,
                    float dampening, float weight_decay, int nesterov) {
  CLIPMI_REQUIRE(d_embed && sel && pos && name_lens && (ctx || grad_out), CLIPMI_ERR_ARG,
                 "%s: null pointer (d_embed, sel, pos, name_lens and one of ctx, grad_out are required)", who);
  CLIPMI_REQUIRE(!ctx || lr, CLIPMI_ERR_ARG, "%s: null pointer (a step needs lr)", who);
  CLIPMI_REQUIRE(C >= 2 && P >= 2 && Pb >= 1 && Pb <= P && D >= 1 && n_ctx >= 1 && n_ctx + 3 <= L, CLIPMI_ERR_SHAPE, "%s: C=%d Pb=%d P=%d L=%d D=%d n_ctx=%d", who,
                 C, Pb, P, L, D, n_ctx);
  CLIPMI_REQUIRE(std::isfinite(grad_scale) && grad_scale > 0.f, CLIPMI_ERR_ARG, "%s: grad_scale=%g (finite, > 0)", who, grad_scale);
  if (int rc = check_sgd(who, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE(!ctx || momentum == 0.f || buf, CLIPMI_ERR_ARG, "%s: null pointer (a momentum needs the buffer)", who);
  const int64_t total = (int64_t)P * n_ctx * D;
  CLIPMI_REQUIRE(total < (1ll << 31) && ((int64_t)C * Pb + P) * L < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: context or prompt set too large", who);
  return CLIPMI_OK;
}

// the launch alone: the caller has passed check_ctx_step
int enqueue_ctx_step(const float* d_embed, float* ctx, float* buf, float* grad_out, const int32_t* sel, const int32_t* pos, const int32_t* name_lens, int C,
                     int Pb, int P, int L, int D, int n_ctx, float grad_scale, const float* lr, int first_step, float momentum, float dampening,
                     float weight_decay, int nesterov, hipStream_t s) {
  const int64_t total = (int64_t)P * n_ctx * D;
  hipLaunchKernelGGL(proda_ctx_step_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, d_embed, ctx, buf, grad_out, sel, pos,
                     name_lens, C, Pb, P, L, D, n_ctx, 1.f / grad_scale, lr, make_sgd_args(momentum, dampening, weight_decay, nesterov, first_step));
  return check_launch("proda_ctx_step_kernel");
}

// everything clipmi_proda_ctx_step_scaled refuses, before anything is launched: clipmi_proda_ctx_step's refusals (at a scale of 1: the
// real one lives on the device) together with clipmi_ctx_step_scaled's
int check_ctx_step_scaled(const char* who, const float* d_embed, float* ctx, float* buf, float* grad_out, const int32_t* sel, const int32_t* pos,
                          const int32_t* name_lens, int C, int Pb, int P, int L, int D, int n_ctx, const ScalerCall& sc, const float* lr, float momentum,
                          float dampening, float weight_decay, int nesterov, const void* workspace, size_t workspace_bytes) {
  CLIPMI_REQUIRE(ctx && lr && workspace, CLIPMI_ERR_ARG, "%s: null pointer (ctx, lr and the workspace are required)", who);
  if (int rc = check_scaler(who, sc)) return rc;
  if (int rc = check_ctx_step(who, d_embed, ctx, buf, grad_out, sel, pos, name_lens, C, Pb, P, L, D, n_ctx, 1.f, lr, 0, momentum, dampening, weight_decay,
                              nesterov))
    return rc;
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 256-byte aligned", who);
  const size_t need = scaled_step_bytes((int64_t)P * n_ctx * D);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  return CLIPMI_OK;
}

// the three launches: the caller has passed check_ctx_step_scaled
int enqueue_ctx_step_scaled(const float* d_embed, float* ctx, float* buf, float* grad_out, const int32_t* sel, const int32_t* pos, const int32_t* name_lens,
                            int C, int Pb, int P, int L, int D, int n_ctx, const ScalerCall& sc, const float* lr, float momentum, float dampening,
                            float weight_decay, int nesterov, void* workspace, hipStream_t s) {
  const int64_t total = (int64_t)P * n_ctx * D;
  const ScaledWs w = scaled_carve(workspace, total);
  hipLaunchKernelGGL(proda_scaled_grad_kernel, dim3((unsigned)scaled_grad_blocks(total)), dim3(THREADS), 0, s, d_embed, grad_out, sel, pos, name_lens, C, Pb, P,
                     L, D, n_ctx, (const clipmi_scaler_state*)sc.state, w);
  if (int rc = check_launch("proda_scaled_grad_kernel")) return rc;
  return launch_scaled_decide_apply(w, total, ctx, buf, sc, lr, momentum, dampening, weight_decay, nesterov, s);
}

// ---------------------------------------------------------------------------------- the class-sharded step (DESIGN.md "Class-sharded ProDA fit")
// Rank r of G owns the classes the balanced split gives it (shard_owner, train_rules.h), with all Pb prompts of each, and the no-class
// prompts of the contexts the same split of P gives it.  Its tower runs over C_r Pb + P_r prompts, the class prompts first.
//   proda_shard_compact_kernel        the gathered text features [G, RB, E], RB = ceil(C / G) Pb + ceil(P / G) -> [C Pb + P, E] in the unsharded order
//   proda_ctx_partial_kernel          a rank's send block: [Pb, n_ctx, D] class sums of its own classes | its own no-class rows [P_r, n_ctx, D]
//   proda_ctx_step_gathered_kernel    the G class sums added in rank order, the owner's no-class row last, 1 / grad_scale, the SGD rule
//   proda_gathered_scaled_grad_kernel the same sum under the dynamic loss scale, in proda_scaled_grad_kernel's shape
// With G = 1 every chain is proda_grad_element's: 0 + the classes ascending + the no-class row.  V = 4: 16-byte accesses; V = 1: scalar.
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

// one thread per element of out [C Pb + P, E].  Block r of the gathered rows is rank r's tower output as it lies -- its C_r Pb class rows, then
// its P_r no-class rows -- with padding behind them up to RB rows that is never read
__global__ __launch_bounds__(THREADS) void proda_shard_compact_kernel(const float* __restrict__ gathered, float* __restrict__ out, int C, int Pb, int P, int G,
                                                                      int RB, int64_t E) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  const int64_t n_cls = (int64_t)C * Pb;
  if (idx >= (n_cls + P) * E) return;
  const int64_t n = idx / E;
  int lo, r;
  int64_t row;
  if (n < n_cls) {
    const int c = (int)(n / Pb);
    r = shard_owner(c, C, G, &lo);
    row = (int64_t)(c - lo) * Pb + n % Pb;
  } else {
    const int p = (int)(n - n_cls);
    r = shard_owner(p, P, G, &lo);
    row = (int64_t)(C / G + (r < C % G ? 1 : 0)) * Pb + (p - lo);
  }
  out[idx] = gathered[((int64_t)r * RB + row) * E + idx % E];
}

// one thread per V elements of the send block [(Pb + Pn), n_ctx, D] from the rank's own d_embed [(C Pb + Pn) L, D] (C its own classes, Pn its
// own no-class prompts; name_lens its own classes').  Slot q < Pb: the rows of the C prompts c Pb + q that hold context vector j of context
// sel[q], c ascending from 0.f, unscaled (a selection outside [0, P) is never an index: its sums are zero and no context reads them).
// Slot Pb + i: row 1 + j of the rank's i-th no-class prompt, copied.
template <int V>
__global__ __launch_bounds__(THREADS) void proda_ctx_partial_kernel(const float* __restrict__ d_embed, float* __restrict__ partial,
                                                                    const int32_t* __restrict__ sel, const int32_t* __restrict__ pos,
                                                                    const int32_t* __restrict__ name_lens, int C, int Pb, int P, int Pn, int L, int D, int n_ctx) {
  const int DV = D / V;
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)(Pb + Pn) * n_ctx * DV) return;
  const int d = (int)(idx % DV) * V, j = (int)((idx / DV) % n_ctx), s = (int)(idx / ((int64_t)DV * n_ctx));
  float g[V];
  if (s < Pb) {
#pragma unroll
    for (int v = 0; v < V; ++v) g[v] = 0.f;
    const int p = sel[s];
    if (p >= 0 && p < P) {
      const int ps = pos[p], h = n_ctx / 2;
      for (int64_t c = 0; c < C; ++c) {
        const int row = ctx_row(ps, j, clamp_name_len(name_lens[c], L, n_ctx), h);
        float x[V];
        ldv<V>(d_embed + ((c * Pb + s) * L + row) * D + d, x);
#pragma unroll
        for (int v = 0; v < V; ++v) g[v] += x[v];
      }
    }
  } else {
    ldv<V>(d_embed + (((int64_t)C * Pb + (s - Pb)) * L + 1 + j) * D + d, g);
  }
  stv<V>(partial + ((int64_t)s * n_ctx + j) * D + d, g);
}

// V elements e .. e + V - 1 (e = j D + d) of context p's gradient from the G gathered send blocks (rank r's at gathered + r stride): if p is
// selected at slot q the G class sums of slot q added in RANK order from 0.f; then, always and last, the no-class row of the rank that owns p
template <int V>
__device__ __forceinline__ void proda_gathered_elements(const float* __restrict__ gathered, int G, int64_t stride, int p, int64_t e,
                                                        const int32_t* __restrict__ sel, int Pb, int P, int64_t nD, float inv_scale, float (&g)[V]) {
  int slot = -1;
  for (int q = 0; q < Pb; ++q)
    if (sel[q] == p && slot < 0) slot = q;
#pragma unroll
  for (int v = 0; v < V; ++v) g[v] = 0.f;
  float x[V];
  if (slot >= 0) {
    for (int r = 0; r < G; ++r) {
      ldv<V>(gathered + (int64_t)r * stride + slot * nD + e, x);
#pragma unroll
      for (int v = 0; v < V; ++v) g[v] += x[v];
    }
  }
  int lo;
  const int r = shard_owner(p, P, G, &lo);
  ldv<V>(gathered + (int64_t)r * stride + (Pb + (p - lo)) * nD + e, x);
#pragma unroll
  for (int v = 0; v < V; ++v) g[v] = (g[v] + x[v]) * inv_scale;
}

// one thread per V elements of ctx [P, n_ctx D]; the SGD rule on registers, ctx and buf read and written once
template <int V>
__global__ __launch_bounds__(THREADS) void proda_ctx_step_gathered_kernel(const float* __restrict__ gathered, int G, int64_t stride, float* __restrict__ ctx,
                                                                          float* __restrict__ buf, float* __restrict__ grad_out,
                                                                          const int32_t* __restrict__ sel, int Pb, int P, int64_t nD, float inv_scale,
                                                                          const float* __restrict__ lr, SgdArgs sgd) {
  const int64_t nV = nD / V, idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= P * nV) return;
  const int p = (int)(idx / nV);
  const int64_t e = (idx % nV) * V, o = p * nD + e;
  float g[V];
  proda_gathered_elements<V>(gathered, G, stride, p, e, sel, Pb, P, nD, inv_scale, g);
  if (grad_out) stv<V>(grad_out + o, g);
  if (!ctx) return;
  const bool with_buf = sgd.momentum != 0.f;
  float w[V], b[V];
  ldv<V>(ctx + o, w);
  if (with_buf) ldv<V>(buf + o, b);
  const float rate = *lr;
#pragma unroll
  for (int v = 0; v < V; ++v) sgd_element_fma(w, b, v, g[v], rate, sgd);
  stv<V>(ctx + o, w);
  if (with_buf) stv<V>(buf + o, b);
}

// The same sum under the dynamic loss scale, one thread per element as proda_scaled_grad_kernel: times 1 / state->scale into the step's
// workspace and into grad_out, the workgroup's flag set when any element it produced is an inf or a NaN
__global__ __launch_bounds__(THREADS) void proda_gathered_scaled_grad_kernel(const float* __restrict__ gathered, int G, int64_t stride, float* __restrict__ grad_out,
                                                                             const int32_t* __restrict__ sel, int Pb, int P, int64_t nD,
                                                                             const clipmi_scaler_state* __restrict__ st, ScaledWs w) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  int bad = 0;
  if (idx < P * nD) {
    float g[1];
    proda_gathered_elements<1>(gathered, G, stride, (int)(idx / nD), idx % nD, sel, Pb, P, nD, 1.f / st->scale, g);
    w.grad[idx] = g[0];
    if (grad_out) grad_out[idx] = g[0];
    bad = !isfinite(g[0]);
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) w.flags[blockIdx.x] = bad ? 1 : 0;
}

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

// what both gathered steps ask of the send blocks: rank r's block of (Pb + ceil(P / G)) n_ctx D floats at gathered + r rank_stride
int check_gathered_step(const char* who, const float* gathered, int G, int64_t rank_stride, const int32_t* sel, int Pb, int P, int D, int n_ctx) {
  CLIPMI_REQUIRE(gathered && sel, CLIPMI_ERR_ARG, "%s: null pointer (the gathered blocks and sel are required)", who);
  CLIPMI_REQUIRE(G >= 1 && P >= 2 && P >= G && Pb >= 1 && Pb <= P && D >= 1 && n_ctx >= 1, CLIPMI_ERR_SHAPE, "%s: G=%d P=%d (>= 2, >= G) Pb=%d (1 .. P) D=%d n_ctx=%d",
                 who, G, P, Pb, D, n_ctx);
  CLIPMI_REQUIRE((int64_t)P * n_ctx * D < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: context set too large", who);
  const int64_t block = (int64_t)(Pb + (P + G - 1) / G) * n_ctx * D;
  CLIPMI_REQUIRE(rank_stride >= block && rank_stride < (1ll << 40), CLIPMI_ERR_SHAPE, "%s: rank_stride=%lld below a rank's block of %lld elements", who,
                 (long long)rank_stride, (long long)block);
  return CLIPMI_OK;
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

int clipmi_proda_embed_shard(const void* base, const void* nc_base, int dtype, const float* ctx, const int32_t* sel, const int32_t* pos,
                             const int32_t* name_lens, const int32_t* cls_eot, float* prompts, int32_t* eot, int C, int Pb, int P, int p0, int Pn, int L,
                             int Lc, int D, int n_ctx, clipmi_stream_t stream) {
  const char* who = "proda_embed_shard";
  if (int rc = check_embed(who, base, nc_base, dtype, ctx, sel, pos, name_lens, cls_eot, prompts, eot, C, Pb, P, L, Lc, D, n_ctx, 1)) return rc;
  CLIPMI_REQUIRE(p0 >= 0 && Pn >= 1 && p0 <= P - Pn, CLIPMI_ERR_SHAPE, "%s: the no-class prompts [%d, %d + %d) leave the P=%d contexts", who, p0, p0, Pn, P);
  return enqueue_embed(base, nc_base, dtype, ctx, sel, pos, name_lens, cls_eot, prompts, eot, C, Pb, P, L, Lc, D, n_ctx, (hipStream_t)stream, p0, Pn);
}

int clipmi_proda_shard_compact(const float* gathered, float* out, int C, int Pb, int P, int G, int64_t E, clipmi_stream_t stream) {
  const char* who = "proda_shard_compact";
  CLIPMI_REQUIRE(gathered && out, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(G >= 1 && C >= G && P >= G && Pb >= 1 && E >= 1, CLIPMI_ERR_SHAPE, "%s: C=%d P=%d G=%d Pb=%d E=%lld (C >= G, P >= G, G >= 1)", who, C, P, G, Pb,
                 (long long)E);
  const int64_t RB = (int64_t)((C + G - 1) / G) * Pb + (P + G - 1) / G, rows = (int64_t)C * Pb + P;
  CLIPMI_REQUIRE(RB < (1ll << 31) && E < (1ll << 31) && rows * E < (1ll << 31) * THREADS && G * RB * E < (1ll << 40), CLIPMI_ERR_SHAPE, "%s: too many rows", who);
  hipLaunchKernelGGL(proda_shard_compact_kernel, dim3((unsigned)((rows * E + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, gathered, out, C,
                     Pb, P, G, (int)RB, E);
  return check_launch("proda_shard_compact_kernel");
}

int clipmi_proda_ctx_partial(const float* d_embed, float* partial, const int32_t* sel, const int32_t* pos, const int32_t* name_lens, int C, int Pb, int P,
                             int Pn, int L, int D, int n_ctx, clipmi_stream_t stream) {
  const char* who = "proda_ctx_partial";
  CLIPMI_REQUIRE(d_embed && partial && sel && pos && name_lens, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(C >= 1 && P >= 2 && Pb >= 1 && Pb <= P && Pn >= 1 && Pn <= P && D >= 1 && n_ctx >= 1 && n_ctx + 3 <= L, CLIPMI_ERR_SHAPE,
                 "%s: C=%d Pb=%d P=%d Pn=%d L=%d D=%d n_ctx=%d", who, C, Pb, P, Pn, L, D, n_ctx);
  CLIPMI_REQUIRE(((int64_t)C * Pb + Pn) * L < (1ll << 31) && (int64_t)(Pb + Pn) * n_ctx * D < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: prompt set or block too large", who);
  const bool vec = D % 4 == 0 && aligned16(d_embed) && aligned16(partial);
  const int64_t total = (int64_t)(Pb + Pn) * n_ctx * (vec ? D / 4 : D);
  const dim3 grid((unsigned)((total + THREADS - 1) / THREADS)), threads(THREADS);
  if (vec)
    hipLaunchKernelGGL(proda_ctx_partial_kernel<4>, grid, threads, 0, (hipStream_t)stream, d_embed, partial, sel, pos, name_lens, C, Pb, P, Pn, L, D, n_ctx);
  else
    hipLaunchKernelGGL(proda_ctx_partial_kernel<1>, grid, threads, 0, (hipStream_t)stream, d_embed, partial, sel, pos, name_lens, C, Pb, P, Pn, L, D, n_ctx);
  return check_launch("proda_ctx_partial_kernel");
}

int clipmi_proda_ctx_step_gathered(const float* gathered, int G, int64_t rank_stride, float* ctx, float* buf, float* grad_out, const int32_t* sel, int Pb, int P,
                                   int D, int n_ctx, float grad_scale, const float* lr, int first_step, float momentum, float dampening, float weight_decay,
                                   int nesterov, clipmi_stream_t stream) {
  const char* who = "proda_ctx_step_gathered";
  CLIPMI_REQUIRE(ctx || grad_out, CLIPMI_ERR_ARG, "%s: null pointer (one of ctx, grad_out is required)", who);
  CLIPMI_REQUIRE(!ctx || lr, CLIPMI_ERR_ARG, "%s: null pointer (a step needs lr)", who);
  if (int rc = check_gathered_step(who, gathered, G, rank_stride, sel, Pb, P, D, n_ctx)) return rc;
  CLIPMI_REQUIRE(std::isfinite(grad_scale) && grad_scale > 0.f, CLIPMI_ERR_ARG, "%s: grad_scale=%g (finite, > 0)", who, grad_scale);
  if (int rc = check_sgd(who, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE(!ctx || momentum == 0.f || buf, CLIPMI_ERR_ARG, "%s: null pointer (a momentum needs the buffer)", who);
  const int64_t nD = (int64_t)n_ctx * D;
  // 16-byte accesses need every block of n_ctx D floats of the three streams on one 16-byte phase
  const bool vec = nD % 4 == 0 && rank_stride % 4 == 0 && aligned16(gathered) && aligned16(ctx) && aligned16(buf) && aligned16(grad_out);
  const int64_t total = P * (vec ? nD / 4 : nD);
  const dim3 grid((unsigned)((total + THREADS - 1) / THREADS)), threads(THREADS);
  const SgdArgs sgd = make_sgd_args(momentum, dampening, weight_decay, nesterov, first_step);
  if (vec)
    hipLaunchKernelGGL(proda_ctx_step_gathered_kernel<4>, grid, threads, 0, (hipStream_t)stream, gathered, G, rank_stride, ctx, buf, grad_out, sel, Pb, P, nD,
                       1.f / grad_scale, lr, sgd);
  else
    hipLaunchKernelGGL(proda_ctx_step_gathered_kernel<1>, grid, threads, 0, (hipStream_t)stream, gathered, G, rank_stride, ctx, buf, grad_out, sel, Pb, P, nD,
                       1.f / grad_scale, lr, sgd);
  return check_launch("proda_ctx_step_gathered_kernel");
}

int clipmi_proda_ctx_reduce_gathered_scaled(const float* gathered, int G, int64_t rank_stride, float* ctx, float* buf, float* grad_out, const int32_t* sel,
                                            int Pb, int P, int D, int n_ctx, clipmi_scaler_state* state, float growth_factor, float backoff_factor,
                                            int growth_interval, const float* lr, float momentum, float dampening, float weight_decay, int nesterov,
                                            void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  const char* who = "proda_ctx_reduce_gathered_scaled";
  const ScalerCall sc{state, growth_factor, backoff_factor, growth_interval};
  CLIPMI_REQUIRE(ctx && lr && workspace, CLIPMI_ERR_ARG, "%s: null pointer (ctx, lr and the workspace are required)", who);
  if (int rc = check_scaler(who, sc)) return rc;
  if (int rc = check_gathered_step(who, gathered, G, rank_stride, sel, Pb, P, D, n_ctx)) return rc;
  if (int rc = check_sgd(who, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE(momentum == 0.f || buf, CLIPMI_ERR_ARG, "%s: null pointer (a momentum needs the buffer)", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 256-byte aligned", who);
  const int64_t nD = (int64_t)n_ctx * D, total = P * nD;
  const size_t need = scaled_step_bytes(total);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  const ScaledWs w = scaled_carve(workspace, total);
  hipLaunchKernelGGL(proda_gathered_scaled_grad_kernel, dim3((unsigned)scaled_grad_blocks(total)), dim3(THREADS), 0, (hipStream_t)stream, gathered, G, rank_stride,
                     grad_out, sel, Pb, P, nD, (const clipmi_scaler_state*)state, w);
  if (int rc = check_launch("proda_gathered_scaled_grad_kernel")) return rc;
  return launch_scaled_decide_apply(w, total, ctx, buf, sc, lr, momentum, dampening, weight_decay, nesterov, (hipStream_t)stream);
}

int clipmi_proda_embed(const void* base, const void* nc_base, int dtype, const float* ctx, const int32_t* sel, const int32_t* pos, const int32_t* name_lens,
                       const int32_t* cls_eot, float* prompts, int32_t* eot, int C, int Pb, int P, int L, int Lc, int D, int n_ctx, clipmi_stream_t stream) {
  if (int rc = check_embed("proda_embed", base, nc_base, dtype, ctx, sel, pos, name_lens, cls_eot, prompts, eot, C, Pb, P, L, Lc, D, n_ctx)) return rc;
  return enqueue_embed(base, nc_base, dtype, ctx, sel, pos, name_lens, cls_eot, prompts, eot, C, Pb, P, L, Lc, D, n_ctx, (hipStream_t)stream);
}

size_t clipmi_proda_head_workspace_bytes(int B, int E, int C, int Pb, int P) {
  if (B < 1 || E < 1 || C < 2 || P < 2 || Pb < 1 || Pb > P) return 0;
  return align256(proda_head_floats(B, E, C, Pb, P) * sizeof(float));
}

int clipmi_proda_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, int Pb, int P, float scale,
                      float grad_scale, float alpha, float* losses, float* d_text, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  if (int rc = check_head("proda_head", feats, ld, labels, text, B, E, C, Pb, P, scale, grad_scale, alpha, losses, d_text, workspace, workspace_bytes)) return rc;
  return enqueue_head(feats, ld, labels, text, B, E, C, Pb, P, scale, grad_scale, alpha, losses, d_text, workspace, (hipStream_t)stream);
}

int clipmi_proda_ctx_step(const float* d_embed, float* ctx, float* buf, float* grad_out, const int32_t* sel, const int32_t* pos, const int32_t* name_lens,
                          int C, int Pb, int P, int L, int D, int n_ctx, float grad_scale, const float* lr, int first_step, float momentum,
                          float dampening, float weight_decay, int nesterov, clipmi_stream_t stream) {
  if (int rc = check_ctx_step("proda_ctx_step", d_embed, ctx, buf, grad_out, sel, pos, name_lens, C, Pb, P, L, D, n_ctx, grad_scale, lr, first_step, momentum,
                              dampening, weight_decay, nesterov))
    return rc;
  return enqueue_ctx_step(d_embed, ctx, buf, grad_out, sel, pos, name_lens, C, Pb, P, L, D, n_ctx, grad_scale, lr, first_step, momentum, dampening,
                          weight_decay, nesterov, (hipStream_t)stream);
}

size_t clipmi_proda_ctx_step_scaled_workspace_bytes(int P, int D, int n_ctx) {
  if (P < 2 || D < 1 || n_ctx < 1 || (int64_t)P * n_ctx * D >= (1ll << 31)) return 0;
  return scaled_step_bytes((int64_t)P * n_ctx * D);
}

int clipmi_proda_ctx_step_scaled(const float* d_embed, float* ctx, float* buf, float* grad_out, const int32_t* sel, const int32_t* pos,
                                 const int32_t* name_lens, int C, int Pb, int P, int L, int D, int n_ctx, clipmi_scaler_state* state, float growth_factor,
                                 float backoff_factor, int growth_interval, const float* lr, float momentum, float dampening, float weight_decay,
                                 int nesterov, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  const ScalerCall sc{state, growth_factor, backoff_factor, growth_interval};
  if (int rc = check_ctx_step_scaled("proda_ctx_step_scaled", d_embed, ctx, buf, grad_out, sel, pos, name_lens, C, Pb, P, L, D, n_ctx, sc, lr, momentum,
                                     dampening, weight_decay, nesterov, workspace, workspace_bytes))
    return rc;
  return enqueue_ctx_step_scaled(d_embed, ctx, buf, grad_out, sel, pos, name_lens, C, Pb, P, L, D, n_ctx, sc, lr, momentum, dampening, weight_decay, nesterov,
                                 workspace, (hipStream_t)stream);
}

// workspace: the tower's workspace (N prompts) | prompts fp32 [N, Lc, D] | EOT int32 [N] | text features [N, E] | their gradient [N, E] |
// d_embed [N L, D] | the head's workspace; the scaled step's own behind them
size_t clipmi_proda_train_step_bytes(const clipmi_model* m, int C, int Pb, int P, int seq_rows, int B) {
  size_t ws = 0;
  if (!m || C < 2 || P < 2 || Pb < 1 || Pb > P || B < 1 || (int64_t)C * Pb + P >= (1ll << 31) / m->g.context_length) return 0;
  const int N = C * Pb + P;
  if (clipmi_text_train_bytes(m, N, seq_rows, &ws, nullptr) != CLIPMI_OK) return 0;
  const size_t feat = align256((size_t)N * m->g.embed_dim * 4);
  return ws + align256((size_t)N * m->g.context_length * m->g.text_width * 4) + align256((size_t)N * 4) + 2 * feat +
         align256((size_t)N * live_rows(m, seq_rows) * m->g.text_width * 4) + clipmi_proda_head_workspace_bytes(B, m->g.embed_dim, C, Pb, P);
}

size_t clipmi_proda_train_step_scaled_bytes(const clipmi_model* m, int C, int Pb, int P, int seq_rows, int B, int n_ctx) {
  const size_t base = clipmi_proda_train_step_bytes(m, C, Pb, P, seq_rows, B);
  const size_t step = m ? clipmi_proda_ctx_step_scaled_workspace_bytes(P, m->g.text_width, n_ctx) : 0;
  return base && step ? base + step : 0;
}

}  // extern "C"

namespace clipmi {
namespace {

// both one-call steps.  sc == nullptr: the static one at grad_scale.  Otherwise the head runs at grad_scale = 1, its d_text is multiplied
// by the device scale before the backward rounds it to fp16, and the step is the scaled one (grad_scale and first_step are not used)
int train_step(const char* who, clipmi_model* m, const clipmi_text_dgrad* wt, const void* base, const void* nc_base, int dtype, float* ctx, float* buf,
               int n_ctx, const int32_t* sel, const int32_t* pos, const int32_t* name_lens, const int32_t* cls_eot, int C, int Pb, int P, int seq_rows,
               const float* feats, int64_t ld, const int64_t* labels, int B, float scale, float grad_scale, const ScalerCall* sc, float alpha,
               const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, float* losses, float* grad_out,
               void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes, hipStream_t s) {
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "%s: null model", who);
  CLIPMI_REQUIRE(ctx && lr && losses, CLIPMI_ERR_ARG, "%s: null pointer (ctx, lr and losses are required)", who);
  const size_t need = sc ? clipmi_proda_train_step_scaled_bytes(m, C, Pb, P, seq_rows, B, n_ctx) : clipmi_proda_train_step_bytes(m, C, Pb, P, seq_rows, B);
  CLIPMI_REQUIRE(need > 0, CLIPMI_ERR_SHAPE, "%s: C=%d (>= 2), Pb=%d (1 .. P), P=%d (>= 2), B=%d (>= 1)%s", who, C, Pb, P, B, sc ? ", n_ctx >= 1" : "");
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  const int N = C * Pb + P;
  size_t tower = 0;
  clipmi_text_train_bytes(m, N, seq_rows, &tower, nullptr);
  if (int rc = check_train_call(who, m, N, workspace, tower, stash, stash_bytes, seq_rows)) return rc;
  if (int rc = check_dgrad(who, m, wt)) return rc;
  const int Lc = m->g.context_length, L = live_rows(m, seq_rows), D = m->g.text_width, E = m->g.embed_dim;
  CLIPMI_REQUIRE(L <= AB_MAX_L, CLIPMI_ERR_SHAPE, "%s: %d token rows per prompt (at most %d)", who, L, AB_MAX_L);
  const size_t head_bytes = clipmi_proda_head_workspace_bytes(B, E, C, Pb, P);
  const size_t step_bytes = sc ? clipmi_proda_ctx_step_scaled_workspace_bytes(P, D, n_ctx) : 0;
  Carver c(static_cast<char*>(workspace) + tower);
  float* prompts = c.take<float>((size_t)N * Lc * D * 4);
  int32_t* eot = c.take<int32_t>((size_t)N * 4);
  float* text = c.take<float>((size_t)N * E * 4);
  float* d_text = c.take<float>((size_t)N * E * 4);
  float* d_embed = c.take<float>((size_t)N * L * D * 4);
  void* head_ws = c.take<char>(head_bytes);
  void* step_ws = sc ? c.take<char>(step_bytes) : nullptr;
  const float head_scale = sc ? 1.f : grad_scale;
  // every refusal of every stage comes before the first launch: a refused call enqueues nothing
  if (int rc = check_embed(who, base, nc_base, dtype, ctx, sel, pos, name_lens, cls_eot, prompts, eot, C, Pb, P, L, Lc, D, n_ctx)) return rc;
  if (int rc = check_train_inputs(who, m, prompts, CLIPMI_F32, nullptr, 0, eot, seq_rows, nullptr, 0)) return rc;
  if (int rc = check_head(who, feats, ld, labels, text, B, E, C, Pb, P, scale, head_scale, alpha, losses, d_text, head_ws, head_bytes)) return rc;
  if (sc) {
    if (int rc = check_ctx_step_scaled(who, d_embed, ctx, buf, grad_out, sel, pos, name_lens, C, Pb, P, L, D, n_ctx, *sc, lr, momentum, dampening,
                                       weight_decay, nesterov, step_ws, step_bytes))
      return rc;
  } else if (int rc = check_ctx_step(who, d_embed, ctx, buf, grad_out, sel, pos, name_lens, C, Pb, P, L, D, n_ctx, grad_scale, lr, first_step, momentum,
                                     dampening, weight_decay, nesterov)) {
    return rc;
  }
  if (int rc = enqueue_embed(base, nc_base, dtype, ctx, sel, pos, name_lens, cls_eot, prompts, eot, C, Pb, P, L, Lc, D, n_ctx, s)) return rc;
  if (int rc = run_train_forward(m, prompts, CLIPMI_F32, nullptr, 0, 0, eot, N, seq_rows, text, workspace, stash, s)) return rc;
  if (int rc = enqueue_head(feats, ld, labels, text, B, E, C, Pb, P, scale, head_scale, alpha, losses, d_text, head_ws, s)) return rc;
  if (sc) {
    if (int rc = launch_grad_scale_rows(who, d_text, N, E, sc->state, s)) return rc;
  }
  if (int rc = run_backward(m, wt, d_text, N, seq_rows, d_embed, workspace, stash, nullptr, s)) return rc;
  if (sc)
    return enqueue_ctx_step_scaled(d_embed, ctx, buf, grad_out, sel, pos, name_lens, C, Pb, P, L, D, n_ctx, *sc, lr, momentum, dampening, weight_decay, nesterov,
                                   step_ws, s);
  return enqueue_ctx_step(d_embed, ctx, buf, grad_out, sel, pos, name_lens, C, Pb, P, L, D, n_ctx, grad_scale, lr, first_step, momentum, dampening, weight_decay,
                          nesterov, s);
}

}  // namespace
}  // namespace clipmi

extern "C" {

int clipmi_proda_train_step(clipmi_model* m, const clipmi_text_dgrad* wt, const void* base, const void* nc_base, int dtype, float* ctx, float* buf, int n_ctx,
                            const int32_t* sel, const int32_t* pos, const int32_t* name_lens, const int32_t* cls_eot, int C, int Pb, int P, int seq_rows,
                            const float* feats, int64_t ld, const int64_t* labels, int B, float scale, float grad_scale, float alpha, const float* lr, int first_step,
                            float momentum, float dampening, float weight_decay, int nesterov, float* losses, float* grad_out, void* workspace,
                            size_t workspace_bytes, void* stash, size_t stash_bytes, clipmi_stream_t stream) {
  return train_step("proda_train_step", m, wt, base, nc_base, dtype, ctx, buf, n_ctx, sel, pos, name_lens, cls_eot, C, Pb, P, seq_rows, feats, ld, labels, B, scale,
                    grad_scale, nullptr, alpha, lr, first_step, momentum, dampening, weight_decay, nesterov, losses, grad_out, workspace, workspace_bytes, stash,
                    stash_bytes, (hipStream_t)stream);
}

int clipmi_proda_train_step_scaled(clipmi_model* m, const clipmi_text_dgrad* wt, const void* base, const void* nc_base, int dtype, float* ctx, float* buf,
                                   int n_ctx, const int32_t* sel, const int32_t* pos, const int32_t* name_lens, const int32_t* cls_eot, int C, int Pb, int P,
                                   int seq_rows, const float* feats, int64_t ld, const int64_t* labels, int B, float scale, clipmi_scaler_state* state,
                                   float growth_factor, float backoff_factor, int growth_interval, float alpha, const float* lr, float momentum,
                                   float dampening, float weight_decay, int nesterov, float* losses, float* grad_out, void* workspace, size_t workspace_bytes,
                                   void* stash, size_t stash_bytes, clipmi_stream_t stream) {
  const ScalerCall sc{state, growth_factor, backoff_factor, growth_interval};
  if (int rc = check_scaler("proda_train_step_scaled", sc)) return rc;
  return train_step("proda_train_step_scaled", m, wt, base, nc_base, dtype, ctx, buf, n_ctx, sel, pos, name_lens, cls_eot, C, Pb, P, seq_rows, feats, ld, labels, B,
                    scale, 1.f, &sc, alpha, lr, 0, momentum, dampening, weight_decay, nesterov, losses, grad_out, workspace, workspace_bytes, stash, stash_bytes,
                    (hipStream_t)stream);
}

// ---- one validation (DESIGN.md "Fit monitor", "CoCoOp and ProDA"): set_classifier and forward of the inference mirror (proda.py:316-331, 304-313).
int clipmi_proda_val_mean(const float* text, float* mean, int G, int P, int E, clipmi_stream_t stream) {
  CLIPMI_REQUIRE(text && mean, CLIPMI_ERR_ARG, "proda_val_mean: null pointer");
  CLIPMI_REQUIRE(((uintptr_t)text | (uintptr_t)mean) % 4 == 0, CLIPMI_ERR_ARG, "proda_val_mean: fp32 arrays must be 4-byte aligned");
  CLIPMI_REQUIRE(G >= 1 && P >= 1 && P <= VAL_MAX_P && E >= 1, CLIPMI_ERR_SHAPE, "proda_val_mean: G=%d P=%d E=%d (G, E >= 1, P in 1..%d)", G, P, E, VAL_MAX_P);
  const int vec8 = (E % 8 == 0 && (uintptr_t)text % 16 == 0) ? 1 : 0;   // clipmi_l2_normalize's rule
  hipLaunchKernelGGL(proda_val_mean_kernel, dim3((unsigned)G), dim3(THREADS), (size_t)P * sizeof(float), (hipStream_t)stream, text, mean, P, E, vec8);
  return check_launch("proda_val_mean_kernel");
}

size_t clipmi_proda_val_monitor_bytes(int n_val, int C, int n_bins) { return fit_monitor_bytes(n_val, C, n_bins); }

// workspace: the tower's (cc P prompts, cc = min(class_chunk, C)) | prompts in the model's type [cc P, Lc, D] (sized for fp32) | EOT int32 [cc P] | text
// fp32 [cc P, E] | mean fp32 [C, E] | normalised validation features fp32 [n_val, E] | clipmi_fused_tail's workspace
size_t clipmi_proda_val_logits_bytes(const clipmi_model* m, int C, int P, int seq_rows, int class_chunk, int n_val) {
  if (!m || C < 2 || P < 1 || P > VAL_MAX_P || class_chunk < 1 || n_val < 1 || n_val > 262144) return 0;
  const int cc = class_chunk < C ? class_chunk : C;
  if ((int64_t)cc * P >= (1ll << 31) / m->g.context_length) return 0;
  const size_t N = (size_t)cc * P, E = m->g.embed_dim;
  return align256(clipmi_text_workspace_bytes(m, (int)N, seq_rows)) + align256(N * m->g.context_length * m->g.text_width * 4) + align256(N * 4) +
         align256(N * E * 4) + align256((size_t)C * E * 4) + align256((size_t)n_val * E * 4) + align256(clipmi_fused_tail_workspace_bytes(n_val, C));
}

int clipmi_proda_val_logits(clipmi_model* m, const void* base, int dtype, const float* ctx, const int32_t* order, const int32_t* pos, const int32_t* name_lens,
                            const int32_t* cls_eot, int C, int P, int n_ctx, int seq_rows, int class_chunk, float scale, unsigned flags, int epoch,
                            const float* val_feats, int64_t val_ld, const int64_t* val_labels, int n_val, int n_bins, void* records, int criterion,
                            void* best_block, float* best_params, void* monitor_workspace, size_t monitor_workspace_bytes, void* workspace,
                            size_t workspace_bytes, clipmi_stream_t stream) {
  const char* who = "proda_val_logits";
  hipStream_t s = (hipStream_t)stream;
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "%s: null model", who);
  CLIPMI_REQUIRE(base && ctx && order && pos && name_lens && cls_eot && workspace, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(dtype == CLIPMI_F16 || dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "%s: bad dtype %d", who, dtype);
  const int Lc = m->g.context_length, L = live_rows(m, seq_rows), D = m->g.text_width, E = m->g.embed_dim;
  CLIPMI_REQUIRE(C >= 2 && P >= 1 && P <= VAL_MAX_P && class_chunk >= 1, CLIPMI_ERR_SHAPE, "%s: C=%d (>= 2), P=%d (1 .. %d), class_chunk=%d (>= 1)", who, C, P,
                 VAL_MAX_P, class_chunk);
  CLIPMI_REQUIRE(D >= 4 && D % 4 == 0 && n_ctx >= 1 && n_ctx + 3 <= L, CLIPMI_ERR_SHAPE,
                 "%s: D=%d (a multiple of 4), n_ctx=%d, L=%d rows (SOS, the context, '.' and EOT must fit)", who, D, n_ctx, L);
  CLIPMI_REQUIRE(E % 16 == 0, CLIPMI_ERR_SHAPE, "%s: E=%d (a multiple of 16, clipmi_fused_tail's)", who, E);
  const int cc = class_chunk < C ? class_chunk : C;
  CLIPMI_REQUIRE((int64_t)cc * P < (1ll << 31) / Lc, CLIPMI_ERR_SHAPE, "%s: too many prompt tokens (%lld prompts per tower call)", who, (long long)cc * P);
  CLIPMI_REQUIRE(((uintptr_t)base | (uintptr_t)ctx) % 16 == 0, CLIPMI_ERR_ARG, "%s: base and ctx must be 16-byte aligned", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 256-byte aligned", who);
  CLIPMI_REQUIRE(std::isfinite(scale), CLIPMI_ERR_ARG, "%s: scale=%g (finite)", who, scale);
  CLIPMI_REQUIRE(epoch >= 0, CLIPMI_ERR_ARG, "%s: epoch=%d (>= 0)", who, epoch);
  const FitMonitor mon{val_feats, val_ld, val_labels, n_val, n_bins, records, criterion, best_block, best_params, monitor_workspace, monitor_workspace_bytes};
  if (int rc = check_fit_monitor(who, mon, E, C)) return rc;
  CLIPMI_REQUIRE(val_ld == E && (uintptr_t)val_feats % 16 == 0, CLIPMI_ERR_ARG, "%s: the validation features must be contiguous (ld == E = %d) and 16-byte aligned",
                 who, E);
  CLIPMI_REQUIRE(n_val <= 262144 && (int64_t)n_val * C * 4 < 0xFFFFFFF0ll && (C + 63) / 64 <= 65535, CLIPMI_ERR_SHAPE,
                 "%s: N_val=%d x C=%d is more than clipmi_fused_tail takes in one call", who, n_val, C);
  const size_t need = clipmi_proda_val_logits_bytes(m, C, P, seq_rows, class_chunk, n_val);
  CLIPMI_REQUIRE(need > 0 && workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  const int N = cc * P;
  const size_t tower = align256(clipmi_text_workspace_bytes(m, N, seq_rows)), tail_bytes = align256(clipmi_fused_tail_workspace_bytes(n_val, C));
  // the tower's own refusals (unbound weights, the flags) through a call of no prompts, which launches nothing
  if (int rc = clipmi_text_encoder(m, nullptr, dtype, nullptr, 0, seq_rows, nullptr, nullptr, workspace, tower, flags, stream)) return rc;
  Carver c(static_cast<char*>(workspace) + tower);
  void* prompts = c.take<char>((size_t)N * Lc * D * 4);
  int32_t* eot = c.take<int32_t>((size_t)N * 4);
  float* text = c.take<float>((size_t)N * E * 4);
  float* mean = c.take<float>((size_t)C * E * 4);
  float* img_n = c.take<float>((size_t)n_val * E * 4);
  void* tail_ws = c.take<char>(tail_bytes);
  for (int c0 = 0; c0 < C; c0 += cc) {
    const int n = C - c0 < cc ? C - c0 : cc;
    const int64_t total = (int64_t)n * P * L * (D / 4);
    const dim3 grid((unsigned)((total + THREADS - 1) / THREADS)), threads(THREADS);
    if (dtype == CLIPMI_F16)
      hipLaunchKernelGGL(proda_val_embed_kernel<half_t>, grid, threads, 0, s, (const half_t*)base, ctx, order, pos, name_lens, cls_eot, (half_t*)prompts, eot, c0, n,
                         P, L, Lc, D, n_ctx);
    else
      hipLaunchKernelGGL(proda_val_embed_kernel<float>, grid, threads, 0, s, (const float*)base, ctx, order, pos, name_lens, cls_eot, (float*)prompts, eot, c0, n, P,
                         L, Lc, D, n_ctx);
    if (int rc = check_launch("proda_val_embed_kernel")) return rc;
    if (int rc = clipmi_text_encoder(m, prompts, dtype, eot, n * P, seq_rows, nullptr, text, workspace, tower, flags, stream)) return rc;
    if (int rc = clipmi_proda_val_mean(text, mean + (size_t)c0 * E, n, P, E, stream)) return rc;
  }
  // clipmi_fused_tail's ticket counters start from zero (and are left so)
  if (hipMemsetAsync(tail_ws, 0, 64 * 1024, s) != hipSuccess) return check_launch("hipMemsetAsync");
  if (int rc = clipmi_fused_tail(val_feats, CLIPMI_F32, 1, mean, scale, nullptr, fit_monitor_logits(mon), img_n, nullptr, nullptr, nullptr, nullptr, 0, tail_ws,
                                 tail_bytes, n_val, C, E, stream))
    return rc;
  return fit_monitor_score(mon, epoch, C, ctx, (int64_t)P * n_ctx * D, stream);
}

}  // extern "C"
