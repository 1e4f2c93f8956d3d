// CoOp's, KgCoOp's and ProGrad's context trained on the device (reference trainers/classification/coop.py:192-222, 282-309,
// kgcoop.py:246-269, prograd.py:291-304, 371-409): the loss heads on the raw text features, the context's gradient with torch.optim.SGD's
// step, ProGrad's projection, and the one-call step that puts the frozen text tower's training forward and backward (text_backward.hip)
// between them.  DESIGN.md "CoOp fit" and "KgCoOp / ProGrad fit" have the data flow and the rounding points.
//   coop_head_*_kernel         both normalisations, logits, softmax, cross-entropy and the gradient w.r.t. the raw text features
//   prograd_softmax_kernel,    the heads of KgCoOp (cross-entropy + w (1 - mean cosine to the frozen zero-shot features)) and ProGrad (cross-entropy
//   kgcoop_loss_kernel         and the distillation loss against the zero-shot logits, one gradient each) on the same per-class workgroup
//   ctx_step_kernel            the context's gradient (a fixed-order sum over the classes) and the SGD rule
//   prograd_dots_kernel,       ProGrad's two context gradients, their three inner products in float64, the projection rule and the SGD step
//   prograd_step_kernel
//   (MaPLe's joint head, launch_maple_head, is these kernels: CoOp's and VPT's gradient kernels behind one softmax; maple_train.hip drives it)
//   promptsrc_*_kernel         PromptSRC's additions to that joint head: the logit KL rows, the two L1 terms, the five losses (promptsrc_train.hip drives it)
// The cross-entropy row, the workgroup reductions and the optimiser's rules are train_rules.h's.  No float atomics and no workgroup waits
// for another: the same inputs give the same bits.
#include <cmath>

#include "common.h"
#include "model.h"
#include "train_rules.h"

namespace clipmi {
namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

// ------------------------------------------------------------------------------------------------------------------------ the heads
// (reference coop.py:205-222, kgcoop.py:246-269, prograd.py:291-304).  mode: 0 CoOp, 1 KgCoOp, 2 ProGrad (include/clipmi.h); the latter two
// take a frozen teacher [C, E], the zero-shot text features, whose rows are normalised here.
enum { MODE_COOP = 0, MODE_KGCOOP = 1, MODE_PROGRAD = 2 };

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

// grid (C): du_c = scale sum_b dz[b, c] x_b (b ascending), q = u_c . du_c, d_text[c] = (du_c - u_c q) / |t_c|.  Workgroup 0 also averages
// the row losses in float64.  KG (KgCoOp): du_c carries the extra term kg o_c, kg = -grad_scale w / C and o_c the normalised teacher row;
// the projection is linear, so its image k ((o_c - u_c (u_c . o_c)) / |t_c|) is added to the cross-entropy's d_text, whose arithmetic is
// CoOp's own (kg = -0 leaves those bits as they are).  u_c . o_c goes to cosv[c] for kgcoop_loss_kernel.
template <bool KG>
__global__ __launch_bounds__(THREADS) void coop_head_grad_kernel(const float* __restrict__ feats, int64_t ld, const float* __restrict__ text, int B, int E, int C,
                                                                 float scale, HeadWs ws, float* __restrict__ d_text, half_t* __restrict__ d_text16,
                                                                 float* __restrict__ loss_out, const float* __restrict__ teacher,
                                                                 const float* __restrict__ inty, float* __restrict__ cosv, float kg) {
  __shared__ float sw[2 * WAVES];
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
  q = wave_sum(q);               // q and, for KgCoOp, u_c . o_c in block_sum's order, under one barrier
  if (lane == 0) sw[wave] = q;
  if constexpr (KG) {
    uo = wave_sum(uo);
    if (lane == 0) sw[WAVES + wave] = uo;
  }
  __syncthreads();
  q = sw[0];
  for (int w = 1; w < WAVES; ++w) q += sw[w];
  if constexpr (KG) {
    uo = sw[WAVES];
    for (int w = 1; w < WAVES; ++w) uo += sw[WAVES + w];
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

// grid (B), ProGrad: the cross-entropy's row loss and dz by the function coop_head_softmax_kernel forms them with, and beside them the
// distillation term at the temperature T = 1 / inv_t: p = softmax(z / T), p_tea = softmax(z_tea / T), kl row loss = T^2 sum_c p_tea (log S - (z - m) / T),
// dz_kl = grad_scale T (p - p_tea) / B.  The label reaches the cross-entropy only: a bad one makes that half NaN and leaves the other.
// Student and teacher go through the same expressions: equal logits give dz_kl = 0 exactly.
__global__ __launch_bounds__(THREADS) void prograd_softmax_kernel(const int64_t* __restrict__ labels, int B, int C, float grad_scale, float T, float inv_t,
                                                                  HeadWs ws, TeacherWs tw) {
#pragma clang fp contract(off)
  __shared__ float sw[6][WAVES];   // one row per reduction: none waits for the readers of another
  const int t = threadIdx.x, r = blockIdx.x;
  const float* z = ws.z + (size_t)r * C;
  const float* __restrict__ zt = tw.z_tea + (size_t)r * C;
  float* dz = ws.dz + (size_t)r * C;
  float* __restrict__ dzk = tw.dz_kl + (size_t)r * C;
  const int64_t y = labels[r];
  const bool bad = y < 0 || y >= C;      // the same for every thread of the workgroup
  float m = -INFINITY, mt = -INFINITY;
  for (int c = t; c < C; c += THREADS) {
    m = fmaxf(m, z[c]);
    mt = fmaxf(mt, zt[c]);
  }
  m = block_max<WAVES>(m, sw[0]);
  mt = block_max<WAVES>(mt, sw[1]);
  const float k = grad_scale / (float)B, kt = k * T;
  xent_row<WAVES>(z, dz, C, m, bad ? 0 : y, k, sw[2], ws.loss + r);
  if (bad) {                             // each thread over the elements it has just written
    for (int c = t; c < C; c += THREADS) dz[c] = NAN;
    if (t == 0) ws.loss[r] = NAN;
  }
  float Ss = 0.f, St = 0.f;
  for (int c = t; c < C; c += THREADS) {
    Ss += __expf((z[c] - m) * inv_t);
    St += __expf((zt[c] - mt) * inv_t);
  }
  Ss = block_sum<WAVES>(Ss, sw[3]);
  St = block_sum<WAVES>(St, sw[4]);
  const float log_ss = logf(Ss);
  float kl = 0.f;
  for (int c = t; c < C; c += THREADS) {
    const float ps = __expf((z[c] - m) * inv_t) / Ss, pt = __expf((zt[c] - mt) * inv_t) / St;
    dzk[c] = (ps - pt) * kt;
    kl += pt * (log_ss - (z[c] - m) * inv_t);
  }
  kl = block_sum<WAVES>(kl, sw[5]);
  if (t == 0) tw.loss_kl[r] = kl * (T * T);
}

// one workgroup, KgCoOp: losses = [ce + w score, ce, score], ce the float64 mean of the row losses and score = 1 - the float64 mean of
// u_c . o_c, both in mean_loss_256's order
__global__ __launch_bounds__(256) void kgcoop_loss_kernel(HeadWs ws, TeacherWs tw, int B, int C, float w, float* __restrict__ losses) {
#pragma clang fp contract(off)
  __shared__ double sl[1][256];
  mean_loss_256(ws.loss, B, losses + 1);
  const double s = sum_f64_256(tw.cosv, C, sl);
  if (threadIdx.x == 0) {
    const float score = (float)(1.0 - s / (double)C);
    losses[2] = score;
    losses[0] = losses[1] + w * score;
  }
}

// The head of every mode.  losses: [3] for KgCoOp and ProGrad; CoOp writes losses[0] alone and, where the caller allows it, takes none.
// Everything the head refuses, before anything is launched
int check_head(const char* who, bool need_losses, const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale,
               float grad_scale, int mode, const float* teacher, float w, float T, const float* losses, const float* d_text, const float* d_text_kl,
               const void* workspace, size_t workspace_bytes) {
  CLIPMI_REQUIRE(mode == MODE_COOP || mode == MODE_KGCOOP || mode == MODE_PROGRAD, CLIPMI_ERR_ARG, "%s: bad mode %d", who, mode);
  CLIPMI_REQUIRE(feats && labels && text && d_text && workspace && (losses || (mode == MODE_COOP && !need_losses)), CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(mode == MODE_COOP || teacher, CLIPMI_ERR_ARG, "%s: null pointer (KgCoOp and ProGrad need the teacher)", who);
  CLIPMI_REQUIRE(mode != MODE_PROGRAD || d_text_kl, CLIPMI_ERR_ARG, "%s: null pointer (ProGrad writes two gradients)", who);
  CLIPMI_REQUIRE(std::isfinite(scale) && std::isfinite(grad_scale), CLIPMI_ERR_ARG, "%s: scale=%g, grad_scale=%g (both finite)", who, scale, grad_scale);
  CLIPMI_REQUIRE(mode != MODE_KGCOOP || (std::isfinite(w) && w >= 0.f), CLIPMI_ERR_ARG, "%s: w=%g (finite, >= 0)", who, w);
  CLIPMI_REQUIRE(mode != MODE_PROGRAD || (std::isfinite(T) && T > 0.f), CLIPMI_ERR_ARG, "%s: T=%g (finite, > 0)", who, T);
  CLIPMI_REQUIRE(B >= 1 && C >= 2 && E >= 1 && ld >= E, CLIPMI_ERR_SHAPE, "%s: B=%d C=%d E=%d ld=%lld", who, B, C, E, (long long)ld);
  CLIPMI_REQUIRE((int64_t)B * C < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: B * C too large", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 8 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 8-byte aligned", who);
  const size_t need = clipmi_prompt_head_workspace_bytes(B, E, C, mode);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  return CLIPMI_OK;
}

// the launches alone: the caller has passed check_head
int enqueue_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale, float grad_scale, int mode,
                 const float* teacher, float w, float T, float* losses, float* d_text, half_t* d_text16, float* d_text_kl, void* workspace, hipStream_t s) {
  const HeadWs ws = head_carve(workspace, B, C);
  const TeacherWs tw = mode == MODE_COOP ? TeacherWs{} : teacher_carve(workspace, B, C);
  if (mode == MODE_COOP) teacher = nullptr;   // CoOp's head has none: a pointer passed anyway is not read
  const dim3 threads(THREADS), per_bc((unsigned)(((int64_t)B * C + WAVES - 1) / WAVES)), per_c((unsigned)C);
  const float *no_tea = nullptr, *no_inty = nullptr;
  float* none = nullptr;
  hipLaunchKernelGGL(coop_head_norm_kernel, dim3((unsigned)((B + (teacher ? 2 : 1) * C + WAVES - 1) / WAVES)), threads, 0, s, feats, ld, text, B, E, C, ws,
                     teacher, tw.inty);
  if (int rc = check_launch("coop_head_norm_kernel")) return rc;
  hipLaunchKernelGGL(coop_head_logits_kernel, per_bc, threads, 0, s, feats, ld, text, B, E, C, scale, ws);
  if (int rc = check_launch("coop_head_logits_kernel")) return rc;
  if (mode != MODE_PROGRAD) {
    hipLaunchKernelGGL(coop_head_softmax_kernel, dim3((unsigned)B), threads, 0, s, labels, B, C, grad_scale, ws);
    if (int rc = check_launch("coop_head_softmax_kernel")) return rc;
    if (mode == MODE_COOP) {
      hipLaunchKernelGGL(coop_head_grad_kernel<false>, per_c, threads, 0, s, feats, ld, text, B, E, C, scale, ws, d_text, d_text16, losses, no_tea, no_inty,
                         none, 0.f);
      return check_launch("coop_head_grad_kernel");
    }
    hipLaunchKernelGGL(coop_head_grad_kernel<true>, per_c, threads, 0, s, feats, ld, text, B, E, C, scale, ws, d_text, d_text16, none, teacher,
                       (const float*)tw.inty, tw.cosv, -(grad_scale * w / (float)C));
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
  hipLaunchKernelGGL(coop_head_grad_kernel<false>, per_c, threads, 0, s, feats, ld, text, B, E, C, scale, ws, d_text, d_text16, losses, no_tea, no_inty, none,
                     0.f);
  if (int rc = check_launch("coop_head_grad_kernel")) return rc;
  hipLaunchKernelGGL(coop_head_grad_kernel<false>, per_c, threads, 0, s, feats, ld, text, B, E, C, scale, wk, d_text_kl, (half_t*)nullptr, losses + 1, no_tea,
                     no_inty, none, 0.f);
  return check_launch("coop_head_grad_kernel");
}

// --------------------------------------------------------------------------------------------------------------------- context step
// one thread per element of ctx: the classes' rows added in ascending order (generic context), 1 / grad_scale, torch.optim.SGD's rule as
// torch's GPU kernels round it (ctx_grad_element, sgd_element_fma: train_rules.h)
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

// what clipmi_ctx_step and clipmi_prograd_step ask of the context and the optimiser alike; *total: the elements of ctx
int check_ctx_step(const char* who, const float* ctx, const float* buf, const float* lr, int C, int L, int D, int n_ctx, int per_class, float grad_scale,
                   float momentum, float dampening, float weight_decay, int nesterov, int64_t* total) {
  CLIPMI_REQUIRE(!ctx || lr, CLIPMI_ERR_ARG, "%s: null pointer (a step needs lr)", who);
  CLIPMI_REQUIRE(C >= 1 && D >= 1 && n_ctx >= 1 && 1 + n_ctx <= L, CLIPMI_ERR_SHAPE, "%s: C=%d L=%d D=%d n_ctx=%d", who, C, L, D, n_ctx);
  CLIPMI_REQUIRE(std::isfinite(grad_scale) && grad_scale > 0.f, CLIPMI_ERR_ARG, "%s: grad_scale=%g (finite, > 0)", who, grad_scale);
  if (int rc = check_sgd(who, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE(!ctx || momentum == 0.f || buf, CLIPMI_ERR_ARG, "%s: null pointer (a momentum needs the buffer)", who);
  *total = (int64_t)n_ctx * D * (per_class ? C : 1);
  CLIPMI_REQUIRE(*total < (1ll << 31) * THREADS, CLIPMI_ERR_SHAPE, "%s: context too large", who);
  return CLIPMI_OK;
}

// the launch alone: the caller has passed check_ctx_step
int enqueue_ctx_step(const float* d_embed, float* ctx, float* buf, float* grad_out, int C, int L, int D, int n_ctx, int per_class, int64_t total, float grad_scale,
                     const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, hipStream_t s) {
  hipLaunchKernelGGL(ctx_step_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, d_embed, ctx, buf, grad_out, C, L, D, n_ctx,
                     per_class ? 1 : 0, 1.f / grad_scale, lr, make_sgd_args(momentum, dampening, weight_decay, nesterov, first_step));
  return check_launch("ctx_step_kernel");
}

// ------------------------------------------------------------------------------------------------------------------ ProGrad's step
// (reference prograd.py:371-409).  a and b are the context gradients of the cross-entropy and of the distillation loss, each formed as
// ctx_step_kernel forms its gradient.  Two launches: the first keeps a and b and writes every workgroup's partial sums of a.a, b.b and a.b
// in float64 (a grid of at most DOT_BLOCKS workgroups, a function of the context's size alone); the second adds the partials in a fixed
// order in every workgroup, decides, and steps by train_rules.h's ProGrad rule (shard_train.hip's class-sharded step shares it).
constexpr int DOT_BLOCKS = PROGRAD_DOT_BLOCKS;

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

__global__ __launch_bounds__(256) void prograd_dots_kernel(const float* __restrict__ d_embed_a, const float* __restrict__ d_embed_b, int C, int L, int D,
                                                           int n_ctx, int per_class, float inv_scale, int64_t total, ProgradWs w) {
  __shared__ double sl[3][256];
  double d[3] = {0.0, 0.0, 0.0};   // a.a, b.b, a.b
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const float a = ctx_grad_element(d_embed_a, idx, C, L, D, n_ctx, per_class, inv_scale);
    const float b = ctx_grad_element(d_embed_b, idx, C, L, D, n_ctx, per_class, inv_scale);
    w.a[idx] = a;
    w.b[idx] = b;
    d[0] += (double)a * (double)a;
    d[1] += (double)b * (double)b;
    d[2] += (double)a * (double)b;
  }
  block_sum_f64(d, sl);
  if (threadIdx.x == 0)
    for (int i = 0; i < 3; ++i) w.part[i * DOT_BLOCKS + blockIdx.x] = d[i];
}

// one thread per element of ctx; n_part: the first launch's grid.  g = a - lambda (a.b / b.b) b when a.b < 0, else a; then the SGD rule
__global__ __launch_bounds__(256) void prograd_step_kernel(ProgradWs w, int n_part, float lambda, float* __restrict__ ctx, float* __restrict__ buf,
                                                           float* __restrict__ grad_out, int* __restrict__ projected, double* __restrict__ dots,
                                                           int64_t total, const float* __restrict__ lr, SgdArgs sgd) {
#pragma clang fp contract(off)
  __shared__ double sl[3][256];
  const int t = threadIdx.x;
  double d[3];
  for (int i = 0; i < 3; ++i) d[i] = t < n_part ? w.part[i * DOT_BLOCKS + t] : 0.0;
  block_sum_f64(d, sl);
  const double aa = d[0], bb = d[1], ab = d[2];
  const bool project = prograd_projects(aa, bb, ab);
  if (blockIdx.x == 0 && t == 0) {
    if (projected) *projected = project ? 1 : 0;
    if (dots) { dots[0] = aa; dots[1] = bb; dots[2] = ab; }
  }
  const int64_t idx = (int64_t)blockIdx.x * 256 + t;
  if (idx >= total) return;
  const float g = prograd_element(w.a[idx], w.b[idx], project, lambda, ab, bb);
  if (grad_out) grad_out[idx] = g;
  if (ctx) sgd_element_fma(ctx, buf, idx, g, *lr, sgd);
}

// everything clipmi_prograd_step refuses, before anything is launched; *total: the elements of ctx
int check_prograd_step(const char* who, const float* d_embed_xe, const float* d_embed_kl, const float* ctx, const float* buf, const float* grad_out,
                       const int* projected, const double* dots, int C, int L, int D, int n_ctx, int per_class, float grad_scale, float lambda, const float* lr,
                       float momentum, float dampening, float weight_decay, int nesterov, const void* workspace, size_t workspace_bytes, int64_t* total) {
  CLIPMI_REQUIRE(d_embed_xe && d_embed_kl && workspace, CLIPMI_ERR_ARG, "%s: null pointer (both d_embed and the workspace are required)", who);
  CLIPMI_REQUIRE(ctx || grad_out || projected || dots, CLIPMI_ERR_ARG, "%s: null pointer (nothing to write)", who);
  CLIPMI_REQUIRE(std::isfinite(lambda), CLIPMI_ERR_ARG, "%s: lambda=%g (finite)", who, lambda);
  if (int rc = check_ctx_step(who, ctx, buf, lr, C, L, D, n_ctx, per_class, grad_scale, momentum, dampening, weight_decay, nesterov, total)) return rc;
  CLIPMI_REQUIRE((uintptr_t)workspace % 256 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 256-byte aligned", who);
  CLIPMI_REQUIRE(workspace_bytes >= prograd_step_bytes(*total), CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes,
                 prograd_step_bytes(*total));
  return CLIPMI_OK;
}

// the two launches: the caller has passed check_prograd_step
int enqueue_prograd_step(const float* d_embed_xe, const float* d_embed_kl, float* ctx, float* buf, float* grad_out, int* projected, double* dots, int C, int L,
                         int D, int n_ctx, int per_class, int64_t total, float grad_scale, float lambda, const float* lr, int first_step, float momentum,
                         float dampening, float weight_decay, int nesterov, void* workspace, hipStream_t s) {
  const ProgradWs w = prograd_carve(workspace, total);
  const int64_t blocks = (total + 255) / 256;
  const int n_part = (int)(blocks < DOT_BLOCKS ? blocks : DOT_BLOCKS);
  hipLaunchKernelGGL(prograd_dots_kernel, dim3((unsigned)n_part), dim3(256), 0, s, d_embed_xe, d_embed_kl, C, L, D, n_ctx, per_class ? 1 : 0, 1.f / grad_scale,
                     total, w);
  if (int rc = check_launch("prograd_dots_kernel")) return rc;
  hipLaunchKernelGGL(prograd_step_kernel, dim3((unsigned)blocks), dim3(256), 0, s, w, n_part, lambda, ctx, buf, grad_out, projected, dots, total, lr,
                     make_sgd_args(momentum, dampening, weight_decay, nesterov, first_step));
  return check_launch("prograd_step_kernel");
}

// ------------------------------------------------------------------------------------------------------------------ the one-call step
// The tower's training forward, the head, the backward (twice for ProGrad: the stash is read-only in it and the tower's workspace is reused, so
// the second follows the first on the stream) and the step: one body behind clipmi_prompt_train_step, clipmi_coop_train_step and their
// _scaled, _placed and _scaled_placed variants (model.h).  workspace: the tower's workspace | text features [C, E] | their gradient [C, E] |
// d_embed [M, D] | the head's workspace | the step's: clipmi_ctx_step_scaled's under a dynamic scale, for ProGrad the second gradient [C, E] |
// the second d_embed [M, D] | clipmi_prograd_step's workspace.  Behind all that, at the offset the unplaced sizer reports, a placed step keeps
// the placed prompts fp32 [C, Lc, D] | the compact gradient [C (1 + n_ctx), D] and, for ProGrad, | the second one.
struct StepWs {
  float *text, *d_text, *d_embed, *d_text_kl, *d_embed_kl, *prompts, *compact, *compact_kl;
  void *head, *step;
  size_t head_bytes, step_bytes;
};
StepWs step_carve(void* workspace, size_t tower, size_t unplaced, const clipmi_model* m, int C, int L, int B, int mode, int n_ctx, int per_class, bool scaled,
                  bool placed) {
  const int D = m->g.text_width, E = m->g.embed_dim;
  StepWs w{};
  w.head_bytes = clipmi_prompt_head_workspace_bytes(B, E, C, mode);
  Carver c(static_cast<char*>(workspace) + tower);
  w.text = c.take<float>((size_t)C * E * 4);
  w.d_text = c.take<float>((size_t)C * E * 4);
  w.d_embed = c.take<float>((size_t)C * L * D * 4);
  w.head = c.take<char>(w.head_bytes);
  if (scaled) {
    w.step_bytes = clipmi_ctx_step_scaled_workspace_bytes(C, D, n_ctx, per_class);
    w.step = c.take<char>(w.step_bytes);
  } else if (mode == MODE_PROGRAD) {
    w.d_text_kl = c.take<float>((size_t)C * E * 4);
    w.d_embed_kl = c.take<float>((size_t)C * L * D * 4);
    w.step_bytes = clipmi_prograd_step_workspace_bytes(C, D, n_ctx, per_class);
    w.step = c.take<char>(w.step_bytes);
  }
  if (!placed) return w;
  Carver x(static_cast<char*>(workspace) + unplaced);
  w.prompts = x.take<float>((size_t)C * m->g.context_length * D * 4);
  w.compact = x.take<float>((size_t)C * (1 + n_ctx) * D * 4);
  if (mode == MODE_PROGRAD) w.compact_kl = x.take<float>((size_t)C * (1 + n_ctx) * D * 4);
  return w;
}

}  // namespace

int prompt_train_step(const char* who, bool need_losses, size_t need, const ScalerCall* sc, const PromptPlacement* pl, clipmi_model* m,
                      const clipmi_text_dgrad* wt, const void* prompts, int dtype, float* ctx, float* buf, int n_ctx, int per_class, const int32_t* eot, int C,
                      int seq_rows, const float* feats, int64_t ld, const int64_t* labels, int B, float scale, float grad_scale, int mode, const float* teacher,
                      float w, float T, float lambda, const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov,
                      float* losses, float* grad_out, int* projected, double* dots, void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes,
                      hipStream_t s) {
  // every refusal of every stage comes before the first launch: a refused call enqueues nothing.  The text weights are looked at last
  CLIPMI_REQUIRE(!sc || mode != MODE_PROGRAD, CLIPMI_ERR_ARG, "%s: ProGrad's mode has no dynamic loss scale (its two gradients share one step)", who);
  CLIPMI_REQUIRE(mode == MODE_COOP || mode == MODE_KGCOOP || mode == MODE_PROGRAD, CLIPMI_ERR_ARG, "%s: bad mode %d", who, mode);
  if (sc)
    if (int rc = check_scaler(who, *sc)) return rc;
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "%s: null model", who);
  CLIPMI_REQUIRE(C >= 2 && B >= 1, CLIPMI_ERR_SHAPE, "%s: n_prompts=%d (>= 2), B=%d (>= 1)", who, C, B);
  CLIPMI_REQUIRE(ctx && lr && (losses || !need_losses), CLIPMI_ERR_ARG, "%s: null pointer (ctx and lr%s are required)", who, need_losses ? " and losses" : "");
  const int L = live_rows(m, seq_rows), Lc = m->g.context_length, D = m->g.text_width, E = m->g.embed_dim;
  const int R = pl ? 1 + n_ctx : L;   // the rows per class of the gradient stream the step reads
  if (pl)   // the prompt buffer lies a multiple of 256 bytes behind the workspace's start
    if (int rc = check_place(who, prompts, dtype, ctx, pl->position, pl->name_lens, static_cast<const float*>(workspace), C, L, Lc, D, n_ctx)) return rc;
  CLIPMI_REQUIRE(need > 0 && workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  size_t tower = 0;
  clipmi_text_train_bytes(m, C, seq_rows, &tower, nullptr);
  const size_t unplaced = !pl ? 0
                          : sc ? clipmi_prompt_train_step_scaled_bytes(m, C, seq_rows, B, mode, n_ctx, per_class)
                               : clipmi_prompt_train_step_bytes(m, C, seq_rows, B, mode, n_ctx, per_class);
  const StepWs p = step_carve(workspace, tower, unplaced, m, C, L, B, mode, n_ctx, per_class, sc != nullptr, pl != nullptr);
  if (int rc = check_head(who, need_losses, feats, ld, labels, p.text, B, E, C, scale, grad_scale, mode, teacher, w, T, losses, p.d_text, p.d_text_kl, p.head,
                          p.head_bytes))
    return rc;
  const float *g = pl ? p.compact : p.d_embed, *g_kl = pl ? p.compact_kl : p.d_embed_kl;
  int64_t total;
  if (sc) {
    if (int rc = check_ctx_step_scaled(who, g, ctx, buf, lr, C, R, D, n_ctx, per_class, *sc, momentum, dampening, weight_decay, nesterov, p.step, p.step_bytes,
                                       &total))
      return rc;
  } else if (mode != MODE_PROGRAD) {
    if (int rc = check_ctx_step(who, ctx, buf, lr, C, R, D, n_ctx, per_class, grad_scale, momentum, dampening, weight_decay, nesterov, &total)) return rc;
  } else if (int rc = check_prograd_step(who, g, g_kl, ctx, buf, grad_out, projected, dots, C, R, D, n_ctx, per_class, grad_scale, lambda, lr, momentum,
                                         dampening, weight_decay, nesterov, p.step, p.step_bytes, &total)) {
    return rc;
  }
  if (int rc = check_train_inputs(who, m, prompts, dtype, ctx, n_ctx, eot, seq_rows, nullptr, 0)) return rc;
  if (int rc = check_train_call(who, m, C, workspace, tower, stash, stash_bytes, seq_rows)) return rc;
  if (int rc = check_dgrad(who, m, wt)) return rc;
  CLIPMI_REQUIRE(L <= AB_MAX_L, CLIPMI_ERR_SHAPE, "%s: %d token rows per prompt (at most %d)", who, L, AB_MAX_L);
  if (pl) {   // the context already lies on its rows of the fp32 prompts: the tower splices nothing
    if (int rc = enqueue_place(prompts, dtype, ctx, per_class, pl->position, pl->name_lens, p.prompts, C, L, Lc, D, n_ctx, s)) return rc;
    if (int rc = run_train_forward(m, p.prompts, CLIPMI_F32, nullptr, 0, 0, eot, C, seq_rows, p.text, workspace, stash, s)) return rc;
  } else if (int rc = run_train_forward(m, prompts, dtype, ctx, n_ctx, per_class, eot, C, seq_rows, p.text, workspace, stash, s)) {
    return rc;
  }
  if (int rc = enqueue_head(feats, ld, labels, p.text, B, E, C, scale, grad_scale, mode, teacher, w, T, losses, p.d_text, nullptr, p.d_text_kl, p.head, s)) return rc;
  if (sc)
    if (int rc = launch_grad_scale_rows(who, p.d_text, C, E, sc->state, s)) return rc;
  if (int rc = run_backward(m, wt, p.d_text, C, seq_rows, p.d_embed, workspace, stash, nullptr, s)) return rc;
  if (mode == MODE_PROGRAD)
    if (int rc = run_backward(m, wt, p.d_text_kl, C, seq_rows, p.d_embed_kl, workspace, stash, nullptr, s)) return rc;
  if (pl) {
    if (int rc = enqueue_unplace(p.d_embed, pl->position, pl->name_lens, p.compact, C, L, D, n_ctx, s)) return rc;
    if (mode == MODE_PROGRAD)
      if (int rc = enqueue_unplace(p.d_embed_kl, pl->position, pl->name_lens, p.compact_kl, C, L, D, n_ctx, s)) return rc;
  }
  if (sc)
    return launch_ctx_step_scaled(g, ctx, buf, grad_out, C, R, D, n_ctx, per_class, total, *sc, lr, momentum, dampening, weight_decay, nesterov, p.step, s);
  if (mode != MODE_PROGRAD)
    return enqueue_ctx_step(g, ctx, buf, grad_out, C, R, D, n_ctx, per_class, total, grad_scale, lr, first_step, momentum, dampening, weight_decay, nesterov, s);
  return enqueue_prograd_step(g, g_kl, ctx, buf, grad_out, projected, dots, C, R, D, n_ctx, per_class, total, grad_scale, lambda, lr, first_step, momentum,
                              dampening, weight_decay, nesterov, p.step, s);
}

namespace {

// ------------------------------------------------------------------------------------------------------------------------------ VPT
// (reference trainers/classification/vpt.py: the text features are fixed, the image features carry the gradient).  The head is CoOp's
// with the two sides exchanged: the same norms, logits and cross-entropy rows, then one workgroup per IMAGE.
// grid (B): dx_b = scale sum_c dz[b, c] u_c (c ascending), q = x_b . dx_b, d_feats[b] = (dx_b - x_b q) / |f_b|.  Workgroup 0 also averages
// the row losses in float64.
__global__ __launch_bounds__(THREADS) void vpt_head_grad_kernel(const float* __restrict__ feats, int64_t ld, const float* __restrict__ text, int B, int E, int C,
                                                                float scale, HeadWs ws, float* __restrict__ d_feats, float* __restrict__ loss_out) {
  __shared__ float sw[WAVES];
  const int t = threadIdx.x, b = blockIdx.x;
  const float* f = feats + (int64_t)b * ld;
  const float ifn = ws.inf[b];
  const float* dz = ws.dz + (size_t)b * C;
  float q = 0.f;
  for (int e = t; e < E; e += THREADS) {   // pass 1: q
    float dx = 0.f;
    for (int c = 0; c < C; ++c) dx = fmaf(dz[c], text[(int64_t)c * E + e] * ws.intx[c], dx);
    q = fmaf(f[e] * ifn, scale * dx, q);
  }
  q = block_sum<WAVES>(q, sw);
  for (int e = t; e < E; e += THREADS) {   // pass 2: the same dx again, then the projection
    float dx = 0.f;
    for (int c = 0; c < C; ++c) dx = fmaf(dz[c], text[(int64_t)c * E + e] * ws.intx[c], dx);
    d_feats[(int64_t)b * E + e] = (scale * dx - (f[e] * ifn) * q) * ifn;
  }
  if (b != 0 || !loss_out) return;   // the same for every thread of the workgroup
  mean_loss_256(ws.loss, B, loss_out);
}

int launch_vpt_head(const char* who, const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale,
                    float grad_scale, float* loss, float* d_feats, void* workspace, size_t workspace_bytes, hipStream_t s) {
  CLIPMI_REQUIRE(feats && labels && text && d_feats && workspace, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(std::isfinite(scale) && std::isfinite(grad_scale), CLIPMI_ERR_ARG, "%s: scale=%g, grad_scale=%g (both finite)", who, scale, grad_scale);
  CLIPMI_REQUIRE(B >= 1 && C >= 2 && E >= 1 && ld >= E, CLIPMI_ERR_SHAPE, "%s: B=%d C=%d E=%d ld=%lld", who, B, C, E, (long long)ld);
  CLIPMI_REQUIRE((int64_t)B * C < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: B * C too large", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 8 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 8-byte aligned", who);
  const size_t need = clipmi_vpt_head_workspace_bytes(B, E, C);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  const HeadWs ws = head_carve(workspace, B, C);
  const dim3 threads(THREADS);
  const float* no_tea = nullptr;
  float* none = nullptr;
  hipLaunchKernelGGL(coop_head_norm_kernel, dim3((unsigned)((B + C + WAVES - 1) / WAVES)), threads, 0, s, feats, ld, text, B, E, C, ws, no_tea, none);
  if (int rc = check_launch("coop_head_norm_kernel")) return rc;
  hipLaunchKernelGGL(coop_head_logits_kernel, dim3((unsigned)(((int64_t)B * C + WAVES - 1) / WAVES)), threads, 0, s, feats, ld, text, B, E, C, scale, ws);
  if (int rc = check_launch("coop_head_logits_kernel")) return rc;
  hipLaunchKernelGGL(coop_head_softmax_kernel, dim3((unsigned)B), threads, 0, s, labels, B, C, grad_scale, ws);
  if (int rc = check_launch("coop_head_softmax_kernel")) return rc;
  hipLaunchKernelGGL(vpt_head_grad_kernel, dim3((unsigned)B), threads, 0, s, feats, ld, text, B, E, C, scale, ws, d_feats, loss);
  return check_launch("vpt_head_grad_kernel");
}

// one thread per element of the [depth, n_ctx, D] master block: 1 / grad_scale, torch.optim.SGD's rule as torch's GPU kernels round it
__global__ __launch_bounds__(THREADS) void vpt_step_kernel(const float* __restrict__ d_prompts, float* __restrict__ prompts, float* __restrict__ buf,
                                                           float* __restrict__ grad_out, int64_t total, float inv_scale, const float* __restrict__ lr,
                                                           SgdArgs sgd) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= total) return;
  const float g = d_prompts[idx] * inv_scale;
  if (grad_out) grad_out[idx] = g;
  if (prompts) sgd_element_fma(prompts, buf, idx, g, *lr, sgd);
}

int launch_vpt_step(const char* who, const float* d_prompts, float* prompts, float* buf, float* grad_out, int depth, int n_ctx, int D, float grad_scale,
                    const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, hipStream_t s) {
  CLIPMI_REQUIRE(d_prompts && (prompts || grad_out), CLIPMI_ERR_ARG, "%s: null pointer (d_prompts and one of prompts, grad_out are required)", who);
  CLIPMI_REQUIRE(!prompts || lr, CLIPMI_ERR_ARG, "%s: null pointer (a step needs lr)", who);
  CLIPMI_REQUIRE(depth >= 1 && n_ctx >= 1 && D >= 1, CLIPMI_ERR_SHAPE, "%s: depth=%d n_ctx=%d D=%d", who, depth, n_ctx, D);
  CLIPMI_REQUIRE(std::isfinite(grad_scale) && grad_scale > 0.f, CLIPMI_ERR_ARG, "%s: grad_scale=%g (finite, > 0)", who, grad_scale);
  if (int rc = check_sgd(who, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE(!prompts || momentum == 0.f || buf, CLIPMI_ERR_ARG, "%s: null pointer (a momentum needs the buffer)", who);
  const int64_t total = (int64_t)depth * n_ctx * D;
  CLIPMI_REQUIRE(total < (1ll << 31) * THREADS, CLIPMI_ERR_SHAPE, "%s: prompts too large", who);
  hipLaunchKernelGGL(vpt_step_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, d_prompts, prompts, buf, grad_out, total,
                     1.f / grad_scale, lr, make_sgd_args(momentum, dampening, weight_decay, nesterov, first_step));
  return check_launch("vpt_step_kernel");
}

// ------------------------------------------------------------------------------------------------------------------------ PromptSRC
// (reference trainers/classification/promptsrc.py:186-210, 298-317).  The joint head's launches and, beside them, the three
// self-regularising terms against a frozen teacher: the second logits matrix zz = s Y O^T by coop_head_logits_kernel on the teacher's
// norms, the KL rows in the softmax launch, and the two L1 terms added to the joint head's d_text and d_feats by a launch of their own
// (the projection is linear, as for KgCoOp: the cross-entropy's arithmetic stays CoOp's and VPT's own).
// behind the CoOp head's workspace: 1/|o_c| [C] | 1/|y_b| [B] | zz [B, C] | kl row [B] | l1 row [C + B] (text rows, then image rows), fp32
struct SrcWs {
  float *inty, *inzs, *zz, *kl, *l1;
};
inline size_t promptsrc_head_floats(int B, int C) { return head_floats(B, C) + (size_t)B * (size_t)C + 2 * ((size_t)B + (size_t)C) + (size_t)B; }
inline SrcWs src_carve(void* ws, int B, int C) {
  SrcWs w;
  w.inty = static_cast<float*>(ws) + head_floats(B, C);
  w.inzs = w.inty + C;
  w.zz = w.inzs + B;
  w.kl = w.zz + (size_t)B * C;
  w.l1 = w.kl + B;
  return w;
}

// grid (B): coop_head_softmax_kernel's row loss and dz by the same function, and beside them the logit term: p = softmax(z), q = softmax(zz),
// kl row = sum_c q (log q - log p), dz += kk (p - q) with kk = grad_scale w_logit / (B C).  The label reaches the cross-entropy only.
// Student and teacher go through the same expressions: equal logits give p - q = 0 exactly.
__global__ __launch_bounds__(THREADS) void promptsrc_softmax_kernel(const int64_t* __restrict__ labels, int B, int C, float grad_scale, float kk, HeadWs ws,
                                                                    SrcWs sw_) {
#pragma clang fp contract(off)
  __shared__ float sw[6][WAVES];   // one row per reduction: none waits for the readers of another
  const int t = threadIdx.x, r = blockIdx.x;
  const float* z = ws.z + (size_t)r * C;
  const float* __restrict__ zt = sw_.zz + (size_t)r * C;
  float* dz = ws.dz + (size_t)r * C;
  const int64_t y = labels[r];
  const bool bad = y < 0 || y >= C;      // the same for every thread of the workgroup
  float m = -INFINITY, mt = -INFINITY;
  for (int c = t; c < C; c += THREADS) {
    m = fmaxf(m, z[c]);
    mt = fmaxf(mt, zt[c]);
  }
  m = block_max<WAVES>(m, sw[0]);
  mt = block_max<WAVES>(mt, sw[1]);
  xent_row<WAVES>(z, dz, C, m, bad ? 0 : y, grad_scale / (float)B, sw[2], ws.loss + r);
  if (bad) {                             // each thread over the elements it has just written
    for (int c = t; c < C; c += THREADS) dz[c] = NAN;
    if (t == 0) ws.loss[r] = NAN;
  }
  float Ss = 0.f, St = 0.f;
  for (int c = t; c < C; c += THREADS) {
    Ss += __expf(z[c] - m);
    St += __expf(zt[c] - mt);
  }
  Ss = block_sum<WAVES>(Ss, sw[3]);
  St = block_sum<WAVES>(St, sw[4]);
  const float log_ss = logf(Ss), log_st = logf(St);
  float kl = 0.f;
  for (int c = t; c < C; c += THREADS) {
    const float ps = __expf(z[c] - m) / Ss, pt = __expf(zt[c] - mt) / St;
    dz[c] = dz[c] + (ps - pt) * kk;
    kl += pt * (((zt[c] - mt) - log_st) - ((z[c] - m) - log_ss));
  }
  kl = block_sum<WAVES>(kl, sw[5]);
  if (t == 0) sw_.kl[r] = kl;
}

// sign with sign(0) = 0; a NaN stays a NaN
__device__ __forceinline__ float sign_or_nan(float d) { return d > 0.f ? 1.f : d < 0.f ? -1.f : d; }

// grid (C + B): workgroup r < C is the text row c = r (a = u_c, o = the normalised teacher row, k = grad_scale w_text / (C E)), the others
// the image row b = r - C (a = x_b, o = the normalised frozen feature, k = grad_scale w_image / (B E)).  s = sign(a - o), the row's
// sum |a - o| to l1[r], and k (s - a (a . s)) / |raw row| added to the joint head's gradient row (and rounded again into the fp16 copy).
// An addend of exactly 0 is not added: a row that equals its teacher leaves the cross-entropy's bits.  k == 0: the side is skipped.
__global__ __launch_bounds__(THREADS) void promptsrc_l1_kernel(const float* __restrict__ feats, int64_t ld, const float* __restrict__ zs,
                                                               const float* __restrict__ text, const float* __restrict__ teacher, int E, int C, HeadWs ws,
                                                               SrcWs sw_, float kt, float ki, float* __restrict__ d_text, half_t* __restrict__ d_text16,
                                                               float* __restrict__ d_feats) {
#pragma clang fp contract(off)
  __shared__ float sw[2][WAVES];
  const int t = threadIdx.x, r = blockIdx.x;
  const bool text_side = r < C;          // the same for every thread of the workgroup, as is k
  const float k = text_side ? kt : ki;
  if (k == 0.f) return;
  const int b = r - C;
  const float* a = text_side ? text + (int64_t)r * E : feats + (int64_t)b * ld;
  const float* o = text_side ? teacher + (int64_t)r * E : zs + (int64_t)b * E;
  const float ia = text_side ? ws.intx[r] : ws.inf[b], io = text_side ? sw_.inty[r] : sw_.inzs[b];
  float* out = text_side ? d_text + (int64_t)r * E : d_feats + (int64_t)b * E;
  half_t* out16 = text_side && d_text16 ? d_text16 + (int64_t)r * E : nullptr;
  float l1 = 0.f, qs = 0.f;
  for (int e = t; e < E; e += THREADS) {
    const float u = a[e] * ia, d = u - o[e] * io;
    l1 += fabsf(d);
    qs += u * sign_or_nan(d);
  }
  l1 = block_sum<WAVES>(l1, sw[0]);
  qs = block_sum<WAVES>(qs, sw[1]);
  if (t == 0) sw_.l1[r] = l1;
  const float kia = k * ia;
  for (int e = t; e < E; e += THREADS) {
    const float u = a[e] * ia;
    const float add = kia * (sign_or_nan(u - o[e] * io) - u * qs);
    if (add != 0.f) {
      const float v = out[e] + add;
      out[e] = v;
      if (out16) out16[e] = (half_t)v;
    }
  }
}

// one workgroup: losses = [total, CE, text L1, image L1, logit KL], each the float64 mean of its fp32 rows in sum_f64_256's order and each
// unweighted but the total; a term whose weight is 0 was skipped and reads 0
__global__ __launch_bounds__(256) void promptsrc_loss_kernel(HeadWs ws, SrcWs sw_, int B, int E, int C, float w_text, float w_image, float w_logit,
                                                             float* __restrict__ losses) {
#pragma clang fp contract(off)
  __shared__ double sl[4][256];
  const double ce = sum_f64_256(ws.loss, B, sl) / (double)B;
  double total = ce, lt = 0.0, li = 0.0, kl = 0.0;
  if (w_text != 0.f) {
    lt = sum_f64_256(sw_.l1, C, sl + 1) / ((double)C * (double)E);
    total += (double)w_text * lt;
  }
  if (w_image != 0.f) {
    li = sum_f64_256(sw_.l1 + C, B, sl + 2) / ((double)B * (double)E);
    total += (double)w_image * li;
  }
  if (w_logit != 0.f) {
    kl = sum_f64_256(sw_.kl, B, sl + 3) / ((double)B * (double)C);
    total += (double)w_logit * kl;
  }
  if (threadIdx.x == 0) {
    losses[0] = (float)total;
    losses[1] = (float)ce;
    losses[2] = (float)lt;
    losses[3] = (float)li;
    losses[4] = (float)kl;
  }
}

}  // namespace

// --------------------------------------------------------------------------------------------------------------------------- MaPLe
// (reference trainers/classification/maple.py:190-216: both sides of the logits carry a gradient).  CoOp's norms, logits and cross-entropy
// rows once, then CoOp's gradient kernel for the text side and VPT's for the image side on the same dz: each side's bits are its own head's.
int launch_maple_head(const char* who, const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale,
                      float grad_scale, float* loss, float* d_feats, float* d_text, half_t* d_text16, void* workspace, size_t workspace_bytes, hipStream_t s) {
  CLIPMI_REQUIRE(feats && labels && text && d_feats && d_text && workspace, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(std::isfinite(scale) && std::isfinite(grad_scale), CLIPMI_ERR_ARG, "%s: scale=%g, grad_scale=%g (both finite)", who, scale, grad_scale);
  CLIPMI_REQUIRE(B >= 1 && C >= 2 && E >= 1 && ld >= E, CLIPMI_ERR_SHAPE, "%s: B=%d C=%d E=%d ld=%lld", who, B, C, E, (long long)ld);
  CLIPMI_REQUIRE((int64_t)B * C < (1ll << 31), CLIPMI_ERR_SHAPE, "%s: B * C too large", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 8 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 8-byte aligned", who);
  const size_t need = clipmi_prompt_head_workspace_bytes(B, E, C, MODE_COOP);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  const HeadWs ws = head_carve(workspace, B, C);
  const dim3 threads(THREADS);
  const float *no_tea = nullptr, *no_inty = nullptr;
  float* none = nullptr;
  hipLaunchKernelGGL(coop_head_norm_kernel, dim3((unsigned)((B + C + WAVES - 1) / WAVES)), threads, 0, s, feats, ld, text, B, E, C, ws, no_tea, none);
  if (int rc = check_launch("coop_head_norm_kernel")) return rc;
  hipLaunchKernelGGL(coop_head_logits_kernel, dim3((unsigned)(((int64_t)B * C + WAVES - 1) / WAVES)), threads, 0, s, feats, ld, text, B, E, C, scale, ws);
  if (int rc = check_launch("coop_head_logits_kernel")) return rc;
  hipLaunchKernelGGL(coop_head_softmax_kernel, dim3((unsigned)B), threads, 0, s, labels, B, C, grad_scale, ws);
  if (int rc = check_launch("coop_head_softmax_kernel")) return rc;
  hipLaunchKernelGGL(coop_head_grad_kernel<false>, dim3((unsigned)C), threads, 0, s, feats, ld, text, B, E, C, scale, ws, d_text, d_text16, loss, no_tea, no_inty,
                     none, 0.f);
  if (int rc = check_launch("coop_head_grad_kernel")) return rc;
  hipLaunchKernelGGL(vpt_head_grad_kernel, dim3((unsigned)B), threads, 0, s, feats, ld, text, B, E, C, scale, ws, d_feats, none);
  return check_launch("vpt_head_grad_kernel");
}

// --------------------------------------------------------------------------------------------------------------------- PromptSRC
// The joint head's five launches on the cross-entropy (with all three weights 0 they are all but the loss: the same bits), the teacher's
// norms and logits, the KL rows inside the softmax launch, the L1 launch and the losses.  A zero-weight term is skipped, not multiplied in.
size_t promptsrc_head_bytes(int B, int E, int C) {
  if (B < 1 || E < 1 || C < 2) return 0;
  return align256(promptsrc_head_floats(B, C) * sizeof(float));
}

int check_promptsrc_head(const char* who, const float* feats, int64_t ld, const float* zs_feats, const int64_t* labels, const float* text, const float* teacher,
                         int B, int E, int C, float scale, float grad_scale, float w_text, float w_image, float w_logit, const float* losses,
                         const float* d_feats, const float* d_text, const void* workspace, size_t workspace_bytes) {
  CLIPMI_REQUIRE(feats && zs_feats && labels && text && teacher && losses && d_feats && d_text && workspace, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(std::isfinite(scale) && std::isfinite(grad_scale), CLIPMI_ERR_ARG, "%s: scale=%g, grad_scale=%g (both finite)", who, scale, grad_scale);
  CLIPMI_REQUIRE(std::isfinite(w_text) && w_text >= 0.f && std::isfinite(w_image) && w_image >= 0.f && std::isfinite(w_logit) && w_logit >= 0.f, CLIPMI_ERR_ARG,
                 "%s: w_text=%g, w_image=%g, w_logit=%g (each finite, >= 0)", who, w_text, w_image, w_logit);
  CLIPMI_REQUIRE(B >= 1 && C >= 2 && E >= 1 && ld >= E, CLIPMI_ERR_SHAPE, "%s: B=%d C=%d E=%d ld=%lld", who, B, C, E, (long long)ld);
  CLIPMI_REQUIRE((int64_t)B * C < (1ll << 31) && B + C < (1 << 30), CLIPMI_ERR_SHAPE, "%s: B * C too large", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 8 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 8-byte aligned", who);
  const size_t need = promptsrc_head_bytes(B, E, C);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  return CLIPMI_OK;
}

int launch_promptsrc_head(const char* who, const float* feats, int64_t ld, const float* zs_feats, const int64_t* labels, const float* text,
                          const float* teacher, int B, int E, int C, float scale, float grad_scale, float w_text, float w_image, float w_logit,
                          float* losses, float* d_feats, float* d_text, half_t* d_text16, void* workspace, size_t workspace_bytes, hipStream_t s) {
  if (int rc = check_promptsrc_head(who, feats, ld, zs_feats, labels, text, teacher, B, E, C, scale, grad_scale, w_text, w_image, w_logit, losses, d_feats,
                                    d_text, workspace, workspace_bytes))
    return rc;
  const HeadWs ws = head_carve(workspace, B, C);
  const SrcWs sw = src_carve(workspace, B, C);
  const dim3 threads(THREADS), per_bc((unsigned)(((int64_t)B * C + WAVES - 1) / WAVES)), per_row((unsigned)((B + C + WAVES - 1) / WAVES));
  const float *no_tea = nullptr, *no_inty = nullptr;
  float* none = nullptr;
  const bool regularised = w_text != 0.f || w_image != 0.f || w_logit != 0.f;
  hipLaunchKernelGGL(coop_head_norm_kernel, per_row, threads, 0, s, feats, ld, text, B, E, C, ws, no_tea, none);
  if (int rc = check_launch("coop_head_norm_kernel")) return rc;
  if (regularised) {   // the teacher's side by the same kernel: 1/|y_b| and 1/|o_c|
    HeadWs wn = ws;
    wn.inf = sw.inzs;
    wn.intx = sw.inty;
    hipLaunchKernelGGL(coop_head_norm_kernel, per_row, threads, 0, s, zs_feats, (int64_t)E, teacher, B, E, C, wn, no_tea, none);
    if (int rc = check_launch("coop_head_norm_kernel")) return rc;
  }
  hipLaunchKernelGGL(coop_head_logits_kernel, per_bc, threads, 0, s, feats, ld, text, B, E, C, scale, ws);
  if (int rc = check_launch("coop_head_logits_kernel")) return rc;
  if (w_logit != 0.f) {
    HeadWs wt = ws;   // the teacher's logits with the teacher's norms
    wt.z = sw.zz;
    wt.inf = sw.inzs;
    wt.intx = sw.inty;
    hipLaunchKernelGGL(coop_head_logits_kernel, per_bc, threads, 0, s, zs_feats, (int64_t)E, teacher, B, E, C, scale, wt);
    if (int rc = check_launch("coop_head_logits_kernel")) return rc;
    hipLaunchKernelGGL(promptsrc_softmax_kernel, dim3((unsigned)B), threads, 0, s, labels, B, C, grad_scale, grad_scale * w_logit / ((float)B * (float)C), ws, sw);
    if (int rc = check_launch("promptsrc_softmax_kernel")) return rc;
  } else {
    hipLaunchKernelGGL(coop_head_softmax_kernel, dim3((unsigned)B), threads, 0, s, labels, B, C, grad_scale, ws);
    if (int rc = check_launch("coop_head_softmax_kernel")) return rc;
  }
  hipLaunchKernelGGL(coop_head_grad_kernel<false>, dim3((unsigned)C), threads, 0, s, feats, ld, text, B, E, C, scale, ws, d_text, d_text16, none, no_tea, no_inty,
                     none, 0.f);
  if (int rc = check_launch("coop_head_grad_kernel")) return rc;
  hipLaunchKernelGGL(vpt_head_grad_kernel, dim3((unsigned)B), threads, 0, s, feats, ld, text, B, E, C, scale, ws, d_feats, none);
  if (int rc = check_launch("vpt_head_grad_kernel")) return rc;
  if (w_text != 0.f || w_image != 0.f) {
    hipLaunchKernelGGL(promptsrc_l1_kernel, dim3((unsigned)(C + B)), threads, 0, s, feats, ld, zs_feats, text, teacher, E, C, ws, sw,
                       grad_scale * w_text / ((float)C * (float)E), grad_scale * w_image / ((float)B * (float)E), d_text, d_text16, d_feats);
    if (int rc = check_launch("promptsrc_l1_kernel")) return rc;
  }
  hipLaunchKernelGGL(promptsrc_loss_kernel, dim3(1), dim3(256), 0, s, ws, sw, B, E, C, w_text, w_image, w_logit, losses);
  return check_launch("promptsrc_loss_kernel");
}

}  // namespace clipmi

using namespace clipmi;

extern "C" {

size_t clipmi_maple_head_workspace_bytes(int B, int E, int C) { return clipmi_prompt_head_workspace_bytes(B, E, C, MODE_COOP); }

int clipmi_maple_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale, float grad_scale,
                      float* loss, float* d_feats, float* d_text, void* d_text16, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  return launch_maple_head("maple_head", feats, ld, labels, text, B, E, C, scale, grad_scale, loss, d_feats, d_text, static_cast<half_t*>(d_text16), workspace,
                           workspace_bytes, (hipStream_t)stream);
}

size_t clipmi_prompt_head_workspace_bytes(int B, int E, int C, int mode) {
  if (B < 1 || E < 1 || C < 2 || mode < MODE_COOP || mode > MODE_PROGRAD) return 0;
  return align256(prompt_head_floats(B, C, mode) * sizeof(float));
}

int clipmi_prompt_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale, float grad_scale,
                       int mode, const float* teacher, float w, float T, float* losses, float* d_text, void* d_text16, float* d_text_kl,
                       void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  if (int rc = check_head("prompt_head", true, feats, ld, labels, text, B, E, C, scale, grad_scale, mode, teacher, w, T, losses, d_text, d_text_kl, workspace,
                          workspace_bytes))
    return rc;
  return enqueue_head(feats, ld, labels, text, B, E, C, scale, grad_scale, mode, teacher, w, T, losses, d_text, static_cast<half_t*>(d_text16), d_text_kl,
                      workspace, (hipStream_t)stream);
}

// CoOp's own symbols: mode 0 of the above, except that the loss may be NULL
size_t clipmi_coop_head_workspace_bytes(int B, int E, int C) { return clipmi_prompt_head_workspace_bytes(B, E, C, MODE_COOP); }

int clipmi_coop_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale, float grad_scale,
                     float* loss, float* d_text, void* d_text16, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  if (int rc = check_head("coop_head", false, feats, ld, labels, text, B, E, C, scale, grad_scale, MODE_COOP, nullptr, 0.f, 0.f, loss, d_text, nullptr, workspace,
                          workspace_bytes))
    return rc;
  return enqueue_head(feats, ld, labels, text, B, E, C, scale, grad_scale, MODE_COOP, nullptr, 0.f, 0.f, loss, d_text, static_cast<half_t*>(d_text16), nullptr,
                      workspace, (hipStream_t)stream);
}

int clipmi_ctx_step(const float* d_embed, float* ctx, float* buf, float* grad_out, int C, int L, int D, int n_ctx, int per_class, float grad_scale,
                    const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, clipmi_stream_t stream) {
  CLIPMI_REQUIRE(d_embed && (ctx || grad_out), CLIPMI_ERR_ARG, "ctx_step: null pointer (d_embed and one of ctx, grad_out are required)");
  int64_t total;
  if (int rc = check_ctx_step("ctx_step", ctx, buf, lr, C, L, D, n_ctx, per_class, grad_scale, momentum, dampening, weight_decay, nesterov, &total)) return rc;
  return enqueue_ctx_step(d_embed, ctx, buf, grad_out, C, L, D, n_ctx, per_class, total, grad_scale, lr, first_step, momentum, dampening, weight_decay, nesterov,
                          (hipStream_t)stream);
}

size_t clipmi_prograd_step_workspace_bytes(int C, int D, int n_ctx, int per_class) {
  if (C < 1 || D < 1 || n_ctx < 1) return 0;
  return prograd_step_bytes((int64_t)n_ctx * D * (per_class ? C : 1));
}

int clipmi_prograd_step(const float* d_embed_xe, const float* d_embed_kl, float* ctx, float* buf, float* grad_out, int* projected, double* dots, int C,
                        int L, int D, int n_ctx, int per_class, float grad_scale, float lambda, const float* lr, int first_step, float momentum,
                        float dampening, float weight_decay, int nesterov, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  int64_t total;
  if (int rc = check_prograd_step("prograd_step", d_embed_xe, d_embed_kl, ctx, buf, grad_out, projected, dots, C, L, D, n_ctx, per_class, grad_scale, lambda, lr,
                                  momentum, dampening, weight_decay, nesterov, workspace, workspace_bytes, &total))
    return rc;
  return enqueue_prograd_step(d_embed_xe, d_embed_kl, ctx, buf, grad_out, projected, dots, C, L, D, n_ctx, per_class, total, grad_scale, lambda, lr, first_step,
                              momentum, dampening, weight_decay, nesterov, workspace, (hipStream_t)stream);
}

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
  return prompt_train_step("prompt_train_step", true, clipmi_prompt_train_step_bytes(m, n_prompts, seq_rows, B, mode, n_ctx, ctx_per_class), nullptr, nullptr, m,
                           wt, prompts, dtype, ctx, buf, n_ctx, ctx_per_class, eot, n_prompts, seq_rows, feats, ld, labels, B, scale, grad_scale, mode, teacher, w, T,
                           lambda, lr, first_step, momentum, dampening, weight_decay, nesterov, losses, grad_out, projected, dots, workspace, workspace_bytes,
                           stash, stash_bytes, (hipStream_t)stream);
}

// CoOp's own symbols: mode 0 of the above (whose size does not depend on the context), except that the loss may be NULL
size_t clipmi_coop_train_step_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B) {
  return clipmi_prompt_train_step_bytes(m, n_prompts, seq_rows, B, MODE_COOP, 1, 0);
}

int clipmi_coop_train_step(clipmi_model* m, const clipmi_text_dgrad* wt, const void* prompts, int dtype, float* ctx, float* buf, int n_ctx,
                           int ctx_per_class, const int32_t* eot, int n_prompts, int seq_rows, const float* feats, int64_t ld, const int64_t* labels, int B,
                           float scale, float grad_scale, const float* lr, int first_step, float momentum, float dampening, float weight_decay,
                           int nesterov, float* loss, float* grad_out, void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes,
                           clipmi_stream_t stream) {
  return prompt_train_step("coop_train_step", false, clipmi_coop_train_step_bytes(m, n_prompts, seq_rows, B), nullptr, nullptr, m, wt, prompts, dtype, ctx, buf,
                           n_ctx, ctx_per_class, eot, n_prompts, seq_rows, feats, ld, labels, B, scale, grad_scale, MODE_COOP, nullptr, 0.f, 0.f, 0.f, lr,
                           first_step, momentum, dampening, weight_decay, nesterov, loss, grad_out, nullptr, nullptr, workspace, workspace_bytes, stash,
                           stash_bytes, (hipStream_t)stream);
}

// ---- VPT
size_t clipmi_vpt_head_workspace_bytes(int B, int E, int C) { return clipmi_prompt_head_workspace_bytes(B, E, C, MODE_COOP); }

int clipmi_vpt_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale, float grad_scale,
                    float* loss, float* d_feats, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  return launch_vpt_head("vpt_head", feats, ld, labels, text, B, E, C, scale, grad_scale, loss, d_feats, workspace, workspace_bytes, (hipStream_t)stream);
}

int clipmi_vpt_step(const float* d_prompts, float* prompts, float* buf, float* grad_out, int depth, int n_ctx, int D, float grad_scale, const float* lr,
                    int first_step, float momentum, float dampening, float weight_decay, int nesterov, clipmi_stream_t stream) {
  return launch_vpt_step("vpt_step", d_prompts, prompts, buf, grad_out, depth, n_ctx, D, grad_scale, lr, first_step, momentum, dampening, weight_decay,
                         nesterov, (hipStream_t)stream);
}

size_t clipmi_vpt_train_step_bytes(const clipmi_model* m, int B, int n_ctx, int C) {
  size_t ws = 0;
  if (!m || B < 1 || C < 2 || clipmi_vision_train_bytes(m, B, n_ctx, &ws, nullptr) != CLIPMI_OK) return 0;
  return ws + 2 * align256((size_t)B * m->g.embed_dim * 4) + align256((size_t)m->g.vision_layers * n_ctx * m->g.vision_width * 4) +
         clipmi_vpt_head_workspace_bytes(B, m->g.embed_dim, C);
}

size_t clipmi_vpt_train_step_scaled_bytes(const clipmi_model* m, int B, int n_ctx, int depth, int C) {
  const size_t base = clipmi_vpt_train_step_bytes(m, B, n_ctx, C);
  const size_t step = base && depth >= 1 && depth <= m->g.vision_layers ? block_step_scaled_bytes((int64_t)depth * n_ctx * m->g.vision_width) : 0;
  return base && step ? base + step : 0;
}

}  // extern "C"

// VPT's one-call step, static (sc == NULL) or under the dynamic loss scale (sc: the head at grad_scale = 1, d_feats times the block's scale, the
// backward, and the block step on d_prompts, which is scale * gradient as it stands)
static int vpt_train_step(const char* who, const ScalerCall* sc, size_t need, clipmi_model* m, const clipmi_vision_dgrad* wt, const void* image, int image_dtype,
                          int B, float* prompts, float* buf, int n_ctx, int depth, const float* text, int C, const int64_t* labels, float scale,
                          float grad_scale, const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, float* loss,
                          float* grad_out, void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes, hipStream_t s) {
  CLIPMI_REQUIRE(B >= 1 && C >= 2, CLIPMI_ERR_SHAPE, "%s: B=%d C=%d", who, B, C);
  size_t tower = 0;
  if (int rc = clipmi_vision_train_bytes(m, B, n_ctx, &tower, nullptr)) return rc;
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  if (int rc = check_vision_train_call(who, m, B, n_ctx, depth, workspace, tower, stash, stash_bytes)) return rc;
  if (int rc = check_vision_dgrad(who, m, wt)) return rc;
  CLIPMI_REQUIRE(image && prompts && text && labels, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(image_dtype == CLIPMI_F16 || image_dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "%s: image dtype %d", who, image_dtype);
  const int E = m->g.embed_dim, D = m->g.vision_width;
  const size_t head_bytes = clipmi_vpt_head_workspace_bytes(B, E, C);
  Carver c(static_cast<char*>(workspace) + tower);
  float* feats = c.take<float>((size_t)B * E * 4);
  float* d_feats = c.take<float>((size_t)B * E * 4);
  float* d_prompts = c.take<float>((size_t)m->g.vision_layers * n_ctx * D * 4);
  void* head_ws = c.take<char>(head_bytes);
  const int64_t total = (int64_t)depth * n_ctx * D;
  const size_t scaled_bytes = sc ? block_step_scaled_bytes(total) : 0;
  void* scaled_ws = c.take<char>(scaled_bytes);
  if (sc) {   // the scaler's and the optimiser's refusals come ahead of the first launch
    CLIPMI_REQUIRE(need > 0, CLIPMI_ERR_SHAPE, "%s: B=%d n_ctx=%d depth=%d C=%d", who, B, n_ctx, depth, C);
    CLIPMI_REQUIRE(std::isfinite(scale), CLIPMI_ERR_ARG, "%s: scale=%g (finite)", who, scale);
    if (int rc = check_block_step_scaled(who, d_prompts, prompts, buf, grad_out, lr, total, *sc, momentum, dampening, weight_decay, nesterov, scaled_ws,
                                         scaled_bytes))
      return rc;
  }
  if (int rc = run_vision_train_forward(m, image, image_dtype, B, prompts, n_ctx, depth, feats, workspace, stash, s)) return rc;
  if (int rc = launch_vpt_head(who, feats, E, labels, text, B, E, C, scale, grad_scale, loss, d_feats, head_ws, head_bytes, s)) return rc;
  if (sc)
    if (int rc = launch_grad_scale_rows(who, d_feats, B, E, sc->state, s)) return rc;
  if (int rc = run_vision_backward(m, wt, d_feats, B, n_ctx, depth, d_prompts, workspace, stash, nullptr, s)) return rc;
  if (sc)
    return launch_block_step_scaled(d_prompts, prompts, buf, grad_out, total, *sc, lr, momentum, dampening, weight_decay, nesterov, scaled_ws, s);
  return launch_vpt_step(who, d_prompts, prompts, buf, grad_out, depth, n_ctx, D, grad_scale, lr, first_step, momentum, dampening, weight_decay, nesterov, s);
}

extern "C" {

int clipmi_vpt_train_step(clipmi_model* m, const clipmi_vision_dgrad* wt, const void* image, int image_dtype, int B, float* prompts, float* buf, int n_ctx,
                          int depth, const float* text, int C, const int64_t* labels, float scale, float grad_scale, const float* lr, int first_step,
                          float momentum, float dampening, float weight_decay, int nesterov, float* loss, float* grad_out, void* workspace,
                          size_t workspace_bytes, void* stash, size_t stash_bytes, clipmi_stream_t stream) {
  return vpt_train_step("vpt_train_step", nullptr, clipmi_vpt_train_step_bytes(m, B, n_ctx, C), m, wt, image, image_dtype, B, prompts, buf, n_ctx, depth, text, C,
                        labels, scale, grad_scale, lr, first_step, momentum, dampening, weight_decay, nesterov, loss, grad_out, workspace, workspace_bytes, stash,
                        stash_bytes, (hipStream_t)stream);
}

int clipmi_vpt_train_step_scaled(clipmi_model* m, const clipmi_vision_dgrad* wt, const void* image, int image_dtype, int B, float* prompts, float* buf,
                                 int n_ctx, int depth, const float* text, int C, const int64_t* labels, float scale, clipmi_scaler_state* state,
                                 float growth_factor, float backoff_factor, int growth_interval, const float* lr, float momentum, float dampening,
                                 float weight_decay, int nesterov, float* loss, float* grad_out, void* workspace, size_t workspace_bytes, void* stash,
                                 size_t stash_bytes, clipmi_stream_t stream) {
  const ScalerCall sc{state, growth_factor, backoff_factor, growth_interval};
  return vpt_train_step("vpt_train_step_scaled", &sc, clipmi_vpt_train_step_scaled_bytes(m, B, n_ctx, depth, C), m, wt, image, image_dtype, B, prompts, buf, n_ctx,
                        depth, text, C, labels, scale, 1.f, lr, 0, momentum, dampening, weight_decay, nesterov, loss, grad_out, workspace, workspace_bytes, stash,
                        stash_bytes, (hipStream_t)stream);
}

// ---- one chunk of validation images (DESIGN.md "Fit monitor", "The image-tower fits"): the training forward at `prompts`, clipmi_l2_normalize,
// clipmi_logits against the normalised text features and clipmi_val_score_rows, the four calls enqueued by one.  Workspace: the tower's | features
// fp32 [B, E] | normalised features fp32 [B, E] | logits fp32 [B, C], each part 256-byte aligned
size_t clipmi_vision_val_chunk_bytes(const clipmi_model* m, int B, int n_ctx, int C) {
  size_t ws = 0;
  if (!m || B < 1 || C < 1 || clipmi_vision_train_bytes(m, B, n_ctx, &ws, nullptr) != CLIPMI_OK) return 0;
  return ws + 2 * align256((size_t)B * m->g.embed_dim * 4) + align256((size_t)B * C * 4);
}

int clipmi_vision_val_chunk(clipmi_model* m, const void* image, int image_dtype, int B, const float* prompts, int n_ctx, int depth, const float* text_n, int C,
                            float scale, const int64_t* labels, int n_bins, void* row_results, void* workspace, size_t workspace_bytes, void* stash,
                            size_t stash_bytes, clipmi_stream_t stream) {
  const char* who = "vision_val_chunk";
  hipStream_t s = (hipStream_t)stream;
  CLIPMI_REQUIRE(B >= 1 && C >= 1, CLIPMI_ERR_SHAPE, "%s: B=%d C=%d (both >= 1)", who, B, C);
  size_t tower = 0;
  if (int rc = clipmi_vision_train_bytes(m, B, n_ctx, &tower, nullptr)) return rc;
  const size_t need = clipmi_vision_val_chunk_bytes(m, B, n_ctx, C);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
  if (int rc = check_vision_train_call(who, m, B, n_ctx, depth, workspace, tower, stash, stash_bytes)) return rc;
  CLIPMI_REQUIRE(image && prompts && text_n && labels && row_results, CLIPMI_ERR_ARG, "%s: null pointer", who);
  CLIPMI_REQUIRE(image_dtype == CLIPMI_F16 || image_dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "%s: image dtype %d", who, image_dtype);
  CLIPMI_REQUIRE(((uintptr_t)text_n | (uintptr_t)row_results) % 16 == 0, CLIPMI_ERR_ARG, "%s: the text features and the row results must be 16-byte aligned", who);
  CLIPMI_REQUIRE((uintptr_t)labels % 8 == 0, CLIPMI_ERR_ARG, "%s: labels must be 8-byte aligned", who);
  CLIPMI_REQUIRE(n_bins >= 1 && n_bins <= 64, CLIPMI_ERR_ARG, "%s: n_bins=%d outside 1..64", who, n_bins);
  CLIPMI_REQUIRE(std::isfinite(scale), CLIPMI_ERR_ARG, "%s: scale=%g (finite)", who, scale);
  const int E = m->g.embed_dim;
  Carver c(static_cast<char*>(workspace) + tower);
  float* feats = c.take<float>((size_t)B * E * 4);
  float* feats_n = c.take<float>((size_t)B * E * 4);
  float* logits = c.take<float>((size_t)B * C * 4);
  if (int rc = run_vision_train_forward(m, image, image_dtype, B, prompts, n_ctx, depth, feats, workspace, stash, s)) return rc;
  if (int rc = launch_l2_normalize(feats, CLIPMI_F32, feats_n, B, E, s)) return rc;
  if (int rc = clipmi_logits(feats_n, text_n, scale, nullptr, logits, nullptr, nullptr, B, C, E, stream)) return rc;
  return clipmi_val_score_rows(logits, C, labels, B, C, n_bins, row_results, stream);
}

}  // extern "C"
