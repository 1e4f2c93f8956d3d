// TaskRes' text residuals trained on the device (reference trainers/classification/taskres.py:96-210): both towers and logit_scale are
// frozen and the base text features are computed once, so a step is a function of the raw image features f [B, E], the labels, the base
// text features [C, E], alpha and the optimiser state.  The learned tensor r [C, E] IS the classifier.  With s = exp(logit_scale):
//   x_b = f_b / |f_b|;  t_c = base_c + alpha r_c;  n_c = |t_c|;  u_c = t_c / n_c;  z = s X U^T;  loss = mean_b CE(z_b, y_b)
//   dz = (softmax(z) - onehot(y)) / B;  du_c = s sum_b dz[b, c] x_b;  dr_c = alpha (du_c - u_c (u_c . du_c)) / n_c
// followed by torch.optim.SGD's or torch.optim.Adam's rule on r.  All fp32 with fp32 master values.
//
// Three launches per step, ordered by the stream alone (DESIGN.md "TaskRes fit"):
//   taskres_logits_kernel   z, 64 x 64 tiles over (b, c), depth E.  The tile streams whole rows of f and of t = base + alpha r through
//                           LDS, so it sums their squares on the way (a fixed order per row, the same in every tile) and divides the
//                           raw dot by both norms at the end: z = s ((f_b . t_c) / |f_b|) / n_c.  The first tile column / row leaves
//                           |f_b| / n_c in the workspace for the third launch.
//   taskres_softmax_kernel  one workgroup per sample: row maximum, sum, row loss, dz (beside z, which the third launch reads again).
//   taskres_update_kernel   dU, 64 x 64 tiles over (c, e), depth B, with x_b = f_b / |f_b| formed by the loader; then in the tile's
//                           epilogue u . du as sum_b dz[b, c] z[b, c] (the same number: z[b, c] = s x_b . u_c; a tile holds 64 of a
//                           row's E columns, the column sums of dz * z need none of them), dr, and the optimiser's rule in place
//                           on r and its state.  Tile (0, 0) also averages the row losses in float64.
// Both products are plain LDS-tiled fp32 vector kernels: every output element is ONE chain of fmaf in depth order, which is also what
// the fp32-input matrix instruction of gfx950 computes -- DESIGN.md says why the vector form shipped.
// No float atomics, no workgroup waits for another, the same inputs give the same bits.  A sample index outside [0, N) or a label
// outside [0, C) is never used as an address: the row's loss and gradient terms are NaN (the host checks both before it launches).
#include <cmath>

#include "common.h"
#include "fit_monitor.h"
#include "train_rules.h"

namespace clipmi {
namespace {

constexpr int TILE = 64;          // output tile edge; 256 threads hold 4 x 4 elements each
constexpr int TK = 16;            // depth of one LDS stage
constexpr int LDT = TILE + 4;     // row pitch of a stage in floats: 16-byte aligned rows, the loaders' stores fall on distinct banks
constexpr int THREADS = 256;
constexpr int MAX_DIM = 65535 * TILE;   // rows and C: a grid's y extent

enum { OPT_SGD = 0, OPT_ADAM = 1 };   // the `optimizer` argument of the entry points (include/clipmi.h)
struct OptArgs {
  int kind;
  SgdArgs sgd;
  AdamArgs adam;
};

// the batch: sample of row b is order[b] (or first + b) of the N cached rows
struct Batch {
  const float* feats; int64_t ld; const int64_t* labels; const int32_t* order;
  int first, rows, N;
};
__device__ __forceinline__ int sample_of(const Batch& bt, int row) {   // -1: not a sample
  const int i = bt.order ? bt.order[row] : bt.first + row;
  return i >= 0 && i < bt.N ? i : -1;
}

// workspace of one batch of `rows`: z [rows, C] | dz [rows, C] | loss [rows] | |f_b| [rows] | n_c [C], fp32
struct Workspace {
  float *z, *dz, *loss, *nf, *nt;
};
inline size_t workspace_floats(int rows, int C) { return 2 * (size_t)rows * (size_t)C + 2 * (size_t)rows + (size_t)C; }
inline Workspace carve(void* workspace, int rows, int C) {
  float* p = static_cast<float*>(workspace);
  Workspace w;
  w.z = p;
  w.dz = w.z + (size_t)rows * C;
  w.loss = w.dz + (size_t)rows * C;
  w.nf = w.loss + rows;
  w.nt = w.nf + rows;
  return w;
}

// acc[i][j] += sum_k sa[k][4 tm + i] * sb[k][4 tn + j] over one stage, k ascending: one fmaf chain per element
__device__ __forceinline__ void stage_fma(const float (*sa)[LDT], const float (*sb)[LDT], int tm, int tn, float (&acc)[4][4]) {
#pragma unroll
  for (int k = 0; k < TK; ++k) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(&sa[k][4 * tm]);
    const f32x4 b = *reinterpret_cast<const f32x4*>(&sb[k][4 * tn]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
  }
}

// the sum over the 16 lanes of a DPP row (lanes 16 q .. 16 q + 15), by the same tree in every lane
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  v += dpp_f<0x140>(v);
  return v;
}

// grid (ceil(C / 64), ceil(rows / 64)).  Both operands are depth-contiguous: thread t loads column t % 16 of the stage for the rows
// t / 16 + 16 j, j < 4, of either operand -- and so meets every 16th element of each of its rows, whose squares it sums.
// The validation logits (clipmi_taskres_val_logits) are this kernel on the validation rows with ws.z the caller's [N_val, C] and no place for
// the norms (ws.nf == ws.nt == null): one code, so validation sees the logits a step on those rows would see.  A tile column normalises its 64
// classifier rows once for the 64 validation rows it meets, on the way, not once per row.
__global__ __launch_bounds__(THREADS) void taskres_logits_kernel(Batch bt, const float* __restrict__ base, const float* __restrict__ res, int E, int C,
                                                                 float alpha, float scale, Workspace ws) {
#pragma clang fp contract(off)   // t = base + alpha r is rounded as the update kernel rounds it
  __shared__ __attribute__((aligned(16))) float sa[TK][LDT];
  __shared__ __attribute__((aligned(16))) float sb[TK][LDT];
  __shared__ float sna[TILE], snb[TILE];
  const int t = threadIdx.x, lk = t & 15, lr = t >> 4, tm = t >> 4, tn = t & 15;
  const int b0 = blockIdx.y * TILE, c0 = blockIdx.x * TILE;
  const float* pf[4];       // the sample's features, or null with `fill` in their place: 0 behind the batch, NaN for no sample
  float fill[4];
  int64_t tc[4];            // the class's offset into base and res, -1 behind C
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = b0 + lr + 16 * j, c = c0 + lr + 16 * j;
    const int i = row < bt.rows ? sample_of(bt, row) : -1;
    pf[j] = i >= 0 ? bt.feats + (int64_t)i * bt.ld : nullptr;
    fill[j] = row < bt.rows ? NAN : 0.f;
    tc[j] = c < C ? (int64_t)c * E : -1;
  }
  float ra[4], rb[4], ssa[4] = {0.f, 0.f, 0.f, 0.f}, ssb[4] = {0.f, 0.f, 0.f, 0.f};
  auto load = [&](int kc) {
    const int e = kc + lk;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ra[j] = e < E ? (pf[j] ? pf[j][e] : fill[j]) : 0.f;
      rb[j] = e < E && tc[j] >= 0 ? base[tc[j] + e] + alpha * res[tc[j] + e] : 0.f;
    }
  };
  float acc[4][4] = {};
  load(0);
  for (int kc = 0; kc < E; kc += TK) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sa[lk][lr + 16 * j] = ra[j];
      sb[lk][lr + 16 * j] = rb[j];
      ssa[j] = fmaf(ra[j], ra[j], ssa[j]);
      ssb[j] = fmaf(rb[j], rb[j], ssb[j]);
    }
    __syncthreads();
    if (kc + TK < E) load(kc + TK);
    stage_fma(sa, sb, tm, tn, acc);
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float na = sqrtf(row16_sum(ssa[j])), nb = sqrtf(row16_sum(ssb[j]));
    if (lk == 0) {
      const int row = b0 + lr + 16 * j, c = c0 + lr + 16 * j;
      sna[lr + 16 * j] = na;
      snb[lr + 16 * j] = nb;
      if (ws.nf && blockIdx.x == 0 && row < bt.rows) ws.nf[row] = na;
      if (ws.nt && blockIdx.y == 0 && c < C) ws.nt[c] = nb;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = b0 + 4 * tm + i;
    if (row >= bt.rows) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + 4 * tn + j;
      if (c < C) ws.z[(size_t)row * C + c] = scale * ((acc[i][j] / sna[4 * tm + i]) / snb[4 * tn + j]);
    }
  }
}

// grid (rows): row loss and dz = (softmax(z) - onehot(y)) / B of one sample
__global__ __launch_bounds__(THREADS) void taskres_softmax_kernel(Batch bt, int C, Workspace ws) {
#pragma clang fp contract(off)
  constexpr int WAVES = THREADS / 64;
  __shared__ float swave[2 * WAVES];   // the maximum's, the sum's
  const int t = threadIdx.x, r = blockIdx.x;
  const float* z = ws.z + (size_t)r * C;
  float* dz = ws.dz + (size_t)r * C;
  const int i = sample_of(bt, r);
  const int64_t y = i >= 0 ? bt.labels[i] : -1;
  if (y < 0 || y >= C) {      // the same for every thread of the workgroup: nobody waits at a barrier below
    for (int c = t; c < C; c += THREADS) dz[c] = NAN;
    if (t == 0) ws.loss[r] = NAN;
    return;
  }
  float m = -INFINITY;
  for (int c = t; c < C; c += THREADS) m = fmaxf(m, z[c]);
  m = block_max<WAVES>(m, swave);
  xent_row<WAVES>(z, dz, C, m, y, 1.f / (float)bt.rows, swave + WAVES, ws.loss + r);
}

// grid (ceil(E / 64), ceil(C / 64)).  Both operands are depth-strided (dz [b, c] along c, x [b, e] along e): thread t loads element
// t % 64 of the stage's rows t / 64 + 4 j, j < 4.  Every element of r, and of its state, is read and written by one thread of one
// workgroup; the norms and the logits this launch reads are final before it starts, and it is final before the next step's first launch
// starts: the stream orders them.
__global__ __launch_bounds__(THREADS) void taskres_update_kernel(Batch bt, const float* __restrict__ base, float* __restrict__ res,
                                                                 float* __restrict__ state1, float* __restrict__ state2, int E, int C, float alpha,
                                                                 float scale, Workspace ws, const float* __restrict__ lr, OptArgs opt,
                                                                 float* __restrict__ loss_out) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float sa[TK][LDT];
  __shared__ __attribute__((aligned(16))) float sb[TK][LDT];
  __shared__ float sparts[4][TILE], sq[TILE];
  const int t = threadIdx.x, lm = t & 63, lk = t >> 6, tm = t >> 4, tn = t & 15;
  const int c0 = blockIdx.y * TILE, e0 = blockIdx.x * TILE;
  const int rows = bt.rows;
  {   // q_c = sum_b dz[b, c] z[b, c] = u_c . du_c: the rows in four consecutive ranges, summed serially and then added in range order
    const int c = c0 + lm, span = (rows + 3) / 4;
    const int k0 = lk * span, k1 = k0 + span < rows ? k0 + span : rows;
    float s = 0.f;
    if (c < C)
      for (int b = k0; b < k1; ++b) s = fmaf(ws.dz[(size_t)b * C + c], ws.z[(size_t)b * C + c], s);
    sparts[lk][lm] = s;
    __syncthreads();
    if (t < TILE) sq[t] = ((sparts[0][t] + sparts[1][t]) + sparts[2][t]) + sparts[3][t];
    __syncthreads();
  }
  const int c = c0 + lm, e = e0 + lm;
  float ra[4], rb[4];
  auto load = [&](int kb) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int b = kb + lk + 4 * j;
      ra[j] = b < rows && c < C ? ws.dz[(size_t)b * C + c] : 0.f;
      float x = 0.f;
      if (b < rows && e < E) {
        const int i = sample_of(bt, b);
        x = i >= 0 ? bt.feats[(int64_t)i * bt.ld + e] / ws.nf[b] : NAN;
      }
      rb[j] = x;
    }
  };
  float acc[4][4] = {};
  load(0);
  for (int kb = 0; kb < rows; kb += TK) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sa[lk + 4 * j][lm] = ra[j];
      sb[lk + 4 * j][lm] = rb[j];
    }
    __syncthreads();
    if (kb + TK < rows) load(kb + TK);
    stage_fma(sa, sb, tm, tn, acc);
    __syncthreads();
  }
  const float rate = *lr;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int cc = c0 + 4 * tm + i;
    if (cc >= C) continue;
    const float n = ws.nt[cc], q = sq[4 * tm + i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ee = e0 + 4 * tn + j;
      if (ee >= E) continue;
      const int64_t idx = (int64_t)cc * E + ee;
      const float u = (base[idx] + alpha * res[idx]) / n;
      const float du = scale * acc[i][j];
      const float g = alpha * ((du - u * q) / n);
      if (opt.kind == OPT_ADAM) adam_element(res, state1, state2, idx, g, rate, opt.adam);
      else sgd_element(res, state1, idx, g, rate, opt.sgd);
    }
  }
  if (blockIdx.x != 0 || blockIdx.y != 0 || !loss_out) return;   // the same for every thread of the workgroup
  mean_loss_256(ws.loss, rows, loss_out);
}

struct Problem {
  const float* feats; int64_t ld; const int64_t* labels; const float* base;
  float *res, *state1, *state2;
  int n, E, C;
  float alpha, scale;
};
struct Optimiser {
  int kind; int64_t steps_done;
  float weight_decay, momentum, dampening; int nesterov;
  double beta1, beta2, eps;
};

bool aligned(const void* p, size_t a) { return (uintptr_t)p % a == 0; }

int check_problem(const char* who, const Problem& p, const float* lr, const Optimiser& o) {
  CLIPMI_REQUIRE(p.feats && p.labels && p.base && p.res && lr, CLIPMI_ERR_ARG,
                 "%s: null pointer (feats, labels, base, residuals and lr are required)", who);
  CLIPMI_REQUIRE(o.kind == OPT_SGD || o.kind == OPT_ADAM, CLIPMI_ERR_ARG, "%s: optimizer=%d (0 = SGD, 1 = Adam)", who, o.kind);
  CLIPMI_REQUIRE(o.steps_done >= 0, CLIPMI_ERR_ARG, "%s: steps_done=%lld (>= 0)", who, (long long)o.steps_done);
  if (o.kind == OPT_SGD) {
    if (int rc = check_sgd(who, o.momentum, o.dampening, o.weight_decay, o.nesterov)) return rc;
    CLIPMI_REQUIRE(o.momentum == 0.f || p.state1, CLIPMI_ERR_ARG, "%s: null pointer (a momentum needs the buffer state1)", who);
  } else {
    CLIPMI_REQUIRE(o.weight_decay >= 0.f && std::isfinite(o.weight_decay), CLIPMI_ERR_ARG, "%s: weight_decay=%g (finite, >= 0)", who, o.weight_decay);
    CLIPMI_REQUIRE(o.beta1 >= 0.0 && o.beta1 < 1.0, CLIPMI_ERR_ARG, "%s: beta1=%g (in [0, 1))", who, o.beta1);
    CLIPMI_REQUIRE(o.beta2 >= 0.0 && o.beta2 < 1.0, CLIPMI_ERR_ARG, "%s: beta2=%g (in [0, 1))", who, o.beta2);
    CLIPMI_REQUIRE(o.eps >= 0.0 && std::isfinite(o.eps), CLIPMI_ERR_ARG, "%s: eps=%g (finite, >= 0)", who, o.eps);
    CLIPMI_REQUIRE(p.state1 && p.state2, CLIPMI_ERR_ARG, "%s: null pointer (Adam needs the buffers state1 and state2)", who);
  }
  CLIPMI_REQUIRE(aligned(p.feats, 4) && aligned(p.base, 4) && aligned(p.res, 4) && aligned(p.state1, 4) && aligned(p.state2, 4) && aligned(lr, 4) &&
                     aligned(p.labels, 8),
                 CLIPMI_ERR_ARG, "%s: fp32 arrays must be 4-byte aligned, the labels 8-byte aligned", who);
  CLIPMI_REQUIRE(std::isfinite(p.alpha) && std::isfinite(p.scale), CLIPMI_ERR_ARG, "%s: alpha=%g, scale=%g (both finite)", who, p.alpha, p.scale);
  CLIPMI_REQUIRE(p.n >= 1, CLIPMI_ERR_SHAPE, "%s: n=%d (>= 1)", who, p.n);
  CLIPMI_REQUIRE(p.C >= 2 && p.C <= MAX_DIM, CLIPMI_ERR_SHAPE, "%s: C=%d (2 .. %d classes)", who, p.C, MAX_DIM);
  CLIPMI_REQUIRE(p.E >= 1, CLIPMI_ERR_SHAPE, "%s: E=%d (>= 1)", who, p.E);
  CLIPMI_REQUIRE(p.ld >= p.E, CLIPMI_ERR_SHAPE, "%s: ld=%lld < E=%d", who, (long long)p.ld, p.E);
  return CLIPMI_OK;
}

int check_workspace(const char* who, const void* workspace, size_t bytes, int rows, const Problem& p) {
  CLIPMI_REQUIRE(rows <= MAX_DIM, CLIPMI_ERR_SHAPE, "%s: a batch of %d rows (%d at most)", who, rows, MAX_DIM);
  CLIPMI_REQUIRE(workspace, CLIPMI_ERR_ARG, "%s: null workspace", who);
  CLIPMI_REQUIRE(aligned(workspace, 8), CLIPMI_ERR_ARG, "%s: the workspace must be 8-byte aligned", who);
  const size_t need = clipmi_taskres_train_workspace_bytes(rows, p.E, p.C);
  CLIPMI_REQUIRE(bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, bytes, need);
  return CLIPMI_OK;
}

// the kernels' constants of step number t (1-based), as torch's single-tensor paths form them
OptArgs opt_args(const Optimiser& o, int64_t t) {
  OptArgs a{};
  a.kind = o.kind;
  a.sgd = make_sgd_args(o.momentum, o.dampening, o.weight_decay, o.nesterov, t == 1);
  a.adam = AdamArgs{(float)(1.0 - o.beta1), (float)o.beta2, (float)(1.0 - o.beta2), (float)o.eps, o.weight_decay,
                    1.0 - std::pow(o.beta1, (double)t), std::sqrt(1.0 - std::pow(o.beta2, (double)t))};
  return a;
}

// one step on the samples order[0 .. rows) (or first .. first + rows - 1) of the n cached rows
int launch_step(const Problem& p, const int32_t* order, int first, int rows, const float* lr, const OptArgs& a, float* loss_out, void* workspace,
                hipStream_t s) {
  const Workspace ws = carve(workspace, rows, p.C);
  const Batch bt{p.feats, p.ld, p.labels, order, first, rows, p.n};
  const unsigned tb = (unsigned)((rows + TILE - 1) / TILE), tc = (unsigned)((p.C + TILE - 1) / TILE), te = (unsigned)((p.E + TILE - 1) / TILE);
  hipLaunchKernelGGL(taskres_logits_kernel, dim3(tc, tb), dim3(THREADS), 0, s, bt, p.base, p.res, p.E, p.C, p.alpha, p.scale, ws);
  if (int rc = check_launch("taskres_logits_kernel")) return rc;
  hipLaunchKernelGGL(taskres_softmax_kernel, dim3((unsigned)rows), dim3(THREADS), 0, s, bt, p.C, ws);
  if (int rc = check_launch("taskres_softmax_kernel")) return rc;
  hipLaunchKernelGGL(taskres_update_kernel, dim3(te, tc), dim3(THREADS), 0, s, bt, p.base, p.res, p.state1, p.state2, p.E, p.C, p.alpha, p.scale, ws,
                     lr, a, loss_out);
  return check_launch("taskres_update_kernel");
}

// the validation logits: what clipmi_taskres_val_logits refuses, in the vocabulary of check_problem
int check_val(const char* who, const float* feats, int64_t ld, const float* base, const float* res, int n_val, int E, int C, float alpha, float scale,
              const float* logits) {
  CLIPMI_REQUIRE(feats && base && res && logits, CLIPMI_ERR_ARG, "%s: null pointer (feats, base, residuals and the logits are required)", who);
  CLIPMI_REQUIRE(aligned(feats, 4) && aligned(base, 4) && aligned(res, 4), CLIPMI_ERR_ARG, "%s: fp32 arrays must be 4-byte aligned", who);
  CLIPMI_REQUIRE(aligned(logits, 16), CLIPMI_ERR_ARG, "%s: the logits must be 16-byte aligned (clipmi_val_score reads them)", who);
  CLIPMI_REQUIRE(std::isfinite(alpha) && std::isfinite(scale), CLIPMI_ERR_ARG, "%s: alpha=%g, scale=%g (both finite)", who, alpha, scale);
  CLIPMI_REQUIRE(n_val >= 1 && n_val <= MAX_DIM, CLIPMI_ERR_SHAPE, "%s: N_val=%d (1 .. %d)", who, n_val, MAX_DIM);
  CLIPMI_REQUIRE(C >= 2 && C <= MAX_DIM, CLIPMI_ERR_SHAPE, "%s: C=%d (2 .. %d classes)", who, C, MAX_DIM);
  CLIPMI_REQUIRE(E >= 1, CLIPMI_ERR_SHAPE, "%s: E=%d (>= 1)", who, E);
  CLIPMI_REQUIRE(ld >= E, CLIPMI_ERR_SHAPE, "%s: ld=%lld < E=%d", who, (long long)ld, E);
  return CLIPMI_OK;
}

// the training step's first launch on the validation rows: z goes to `logits` [n_val, C], the norms are not kept
int launch_val(const float* feats, int64_t ld, const float* base, const float* res, int n_val, int E, int C, float alpha, float scale, float* logits,
               hipStream_t s) {
  const Workspace ws{logits, nullptr, nullptr, nullptr, nullptr};
  const Batch bt{feats, ld, nullptr, nullptr, 0, n_val, n_val};
  const unsigned tb = (unsigned)((n_val + TILE - 1) / TILE), tc = (unsigned)((C + TILE - 1) / TILE);
  hipLaunchKernelGGL(taskres_logits_kernel, dim3(tc, tb), dim3(THREADS), 0, s, bt, base, res, E, C, alpha, scale, ws);
  return check_launch("taskres_logits_kernel");
}

// The one body of clipmi_taskres_fit and clipmi_taskres_fit_monitored.  Without a monitor the steps are enqueued and nothing else; with one,
// behind the last step of every epoch: the validation logits of the residuals as they are, the epoch record and, with a best slot, the
// selection of the residual matrix (the optimiser's state is not part of it).
int run_fit(const char* who, const Problem& p, const Optimiser& o, const int32_t* order, int batch, int epochs, int drop_last, const float* lr,
            float* losses, void* workspace, size_t workspace_bytes, const FitMonitor* mon, hipStream_t stream) {
  if (int rc = check_problem(who, p, lr, o)) return rc;
  CLIPMI_REQUIRE(batch >= 1, CLIPMI_ERR_SHAPE, "%s: batch=%d (>= 1)", who, batch);
  CLIPMI_REQUIRE(epochs >= 0, CLIPMI_ERR_ARG, "%s: epochs=%d (>= 0)", who, epochs);
  const int width = batch < p.n ? batch : p.n;   // the widest batch of the run
  if (int rc = check_workspace(who, workspace, workspace_bytes, width, p)) return rc;
  if (mon) {
    if (int rc = check_fit_monitor(who, *mon, p.E, p.C)) return rc;
    CLIPMI_REQUIRE(mon->n_val <= MAX_DIM, CLIPMI_ERR_SHAPE, "%s: N_val=%d (%d at most)", who, mon->n_val, MAX_DIM);
    CLIPMI_REQUIRE(!mon->best_block || aligned(p.res, 16), CLIPMI_ERR_ARG, "%s: a best slot needs the residuals 16-byte aligned", who);
  }
  const int per_epoch = drop_last ? p.n / batch : (int)(((int64_t)p.n + batch - 1) / batch);
  int64_t step = 0;
  for (int e = 0; e < epochs; ++e) {
    const int32_t* epoch_order = order ? order + (int64_t)e * p.n : nullptr;
    for (int k = 0; k < per_epoch; ++k, ++step) {
      const int first = k * batch;   // k < per_epoch <= n: no overflow
      const int rows = p.n - first < batch ? p.n - first : batch;
      if (int rc = launch_step(p, epoch_order ? epoch_order + first : nullptr, first, rows, lr + step, opt_args(o, o.steps_done + step + 1),
                               losses ? losses + step : nullptr, workspace, stream))
        return rc;
    }
    if (!mon) continue;
    if (int rc = launch_val(mon->val_feats, mon->val_ld, p.base, p.res, mon->n_val, p.E, p.C, p.alpha, p.scale, fit_monitor_logits(*mon), stream))
      return rc;
    if (int rc = fit_monitor_score(*mon, e, p.C, p.res, (int64_t)p.C * p.E, (clipmi_stream_t)stream)) return rc;
  }
  return CLIPMI_OK;
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

size_t clipmi_taskres_train_workspace_bytes(int rows, int E, int C) {
  if (rows < 1 || E < 1 || C < 2) return 0;
  return align256(workspace_floats(rows, C) * sizeof(float));
}

int clipmi_taskres_train_step(const float* feats, int64_t ld, const int64_t* labels, const float* base, float* residuals, float* state1,
                              float* state2, int rows, int E, int C, float alpha, float scale, const float* lr, int optimizer,
                              int64_t steps_done, float weight_decay, float momentum, float dampening, int nesterov, double beta1, double beta2,
                              double eps, float* loss, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  const Problem p{feats, ld, labels, base, residuals, state1, state2, rows, E, C, alpha, scale};
  const Optimiser o{optimizer, steps_done, weight_decay, momentum, dampening, nesterov, beta1, beta2, eps};
  if (int rc = check_problem("taskres_train_step", p, lr, o)) return rc;
  if (int rc = check_workspace("taskres_train_step", workspace, workspace_bytes, rows, p)) return rc;
  return launch_step(p, nullptr, 0, rows, lr, opt_args(o, steps_done + 1), loss, workspace, (hipStream_t)stream);
}

int clipmi_taskres_fit(const float* feats, int64_t ld, const int64_t* labels, const int32_t* order, const float* base, float* residuals,
                       float* state1, float* state2, int n, int E, int C, int batch, int epochs, int drop_last, float alpha, float scale,
                       const float* lr, int optimizer, int64_t steps_done, float weight_decay, float momentum, float dampening, int nesterov,
                       double beta1, double beta2, double eps, float* losses, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  const Problem p{feats, ld, labels, base, residuals, state1, state2, n, E, C, alpha, scale};
  const Optimiser o{optimizer, steps_done, weight_decay, momentum, dampening, nesterov, beta1, beta2, eps};
  return run_fit("taskres_fit", p, o, order, batch, epochs, drop_last, lr, losses, workspace, workspace_bytes, nullptr, (hipStream_t)stream);
}

size_t clipmi_taskres_fit_monitored_workspace_bytes(int n_val, int C, int n_bins) {
  return C >= 2 && C <= MAX_DIM && n_val <= MAX_DIM ? fit_monitor_bytes(n_val, C, n_bins) : 0;
}

int clipmi_taskres_fit_monitored(const float* feats, int64_t ld, const int64_t* labels, const int32_t* order, const float* base, float* residuals,
                                 float* state1, float* state2, int n, int E, int C, int batch, int epochs, int drop_last, float alpha, float scale,
                                 const float* lr, int optimizer, int64_t steps_done, float weight_decay, float momentum, float dampening,
                                 int nesterov, double beta1, double beta2, double eps, float* losses, void* workspace, size_t workspace_bytes,
                                 const float* val_feats, int64_t val_ld, const int64_t* val_labels, int n_val, int n_bins, void* records,
                                 int criterion, void* best_block, float* best_params, void* monitor_workspace, size_t monitor_workspace_bytes,
                                 clipmi_stream_t stream) {
  const Problem p{feats, ld, labels, base, residuals, state1, state2, n, E, C, alpha, scale};
  const Optimiser o{optimizer, steps_done, weight_decay, momentum, dampening, nesterov, beta1, beta2, eps};
  const FitMonitor mon{val_feats, val_ld, val_labels, n_val, n_bins, records, criterion, best_block, best_params, monitor_workspace,
                       monitor_workspace_bytes};
  return run_fit("taskres_fit_monitored", p, o, order, batch, epochs, drop_last, lr, losses, workspace, workspace_bytes, &mon, (hipStream_t)stream);
}

int clipmi_taskres_val_logits(const float* feats, int64_t ld, const float* base, const float* residuals, int n_val, int E, int C, float alpha,
                              float scale, float* logits, clipmi_stream_t stream) {
  if (int rc = check_val("taskres_val_logits", feats, ld, base, residuals, n_val, E, C, alpha, scale, logits)) return rc;
  return launch_val(feats, ld, base, residuals, n_val, E, C, alpha, scale, logits, (hipStream_t)stream);
}

}  // extern "C"
