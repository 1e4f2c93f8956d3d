// CLIP-Adapter's bottleneck trained on the device (reference trainers/classification/clip_adapter.py:138-187): both towers are frozen and,
// with the shipped config, so is the context, so a step is a function of the raw image features f [B, E], the labels, the frozen
// L2-normalised text features T [C, E] and the two bias-free matrices W1 [H, E], W2 [E, H].  With r = ratio, s = exp(logit_scale):
//   p1 = f W1^T, h = relu(p1);  p2 = h W2^T, a = relu(p2);  g = r a + (1 - r) f;  n = |g|, u = g / n;  z = s u T^T;  loss = mean CE(z, y)
//   dz = (softmax(z) - onehot(y)) / B;  du = s dz T;  dg = (du - u (u . du)) / n;  da = r dg [p2 > 0];  dW2 = da^T h;
//   dh = (da W2) [p1 > 0];  dW1 = dh^T f                                                  (relu'(0) = 0, as torch has it)
// followed by torch.optim.SGD's rule on both matrices.  All fp32, fp32 master weights, plain vector arithmetic: a step is a few tens of
// MFLOP and latency-bound, so what counts is the number of launches and that nothing returns to the host.
//
// Two launches per step, ordered by the stream alone (DESIGN.md "CLIP-Adapter fit"):
//   adapter_rows_kernel    one workgroup per sample.  Every product is a dot over one wave's lanes (lane-strided fp32 partial sums, then the
//                          wave tree of common.h) or a serial sum over the rows of T / W2 with the columns across the threads, split in
//                          a fixed number of consecutive parts that are then added in order.  T is read twice per sample from L2.
//                          Writes h, da, dh and the row loss to the workspace; the logits of the row live in the workspace in between.
//   adapter_update_kernel  one thread per element of W2 and of W1: the element's gradient summed over the batch rows in row order, then
//                          the SGD rule in place on the weight and its momentum buffer; workgroup 0 also averages the row losses in
//                          float64 in a fixed order into the loss history.  The learning rate is read from a device array.
// No float atomics, no workgroup waits for another, the same inputs give the same bits.  A sample index outside [0, N) or a label outside
// [0, C) is never used as an address: the row's loss and gradient terms are NaN (the host checks both before it launches anything).
#include <cmath>

#include "common.h"
#include "fit_monitor.h"
#include "train_rules.h"   // SgdArgs, check_sgd, sgd_element, waves_max, xent_row, mean_loss_256

namespace clipmi {
namespace {

constexpr int ROWS_THREADS = 1024;            // 16 waves per sample: the 2 C dots over E are the long pole
constexpr int ROWS_WAVES = ROWS_THREADS / 64;
constexpr size_t ROWS_LDS_MAX = 64 * 1024;    // what a launch gets without raising the kernel's dynamic LDS attribute

// workspace of one batch of `rows`: h [rows, H] | da [rows, E] | dh [rows, H] | z [rows, C] | loss [rows], fp32
struct Workspace {
  float *h, *da, *dh, *z, *loss;
};
__host__ __device__ inline size_t workspace_floats(int rows, int E, int H, int C) { return (size_t)rows * ((size_t)E + 2 * (size_t)H + (size_t)C + 1); }
inline Workspace carve(void* workspace, int rows, int E, int H, int C) {
  float* p = static_cast<float*>(workspace);
  Workspace w;
  w.h = p;
  w.da = w.h + (size_t)rows * H;
  w.dh = w.da + (size_t)rows * E;
  w.z = w.dh + (size_t)rows * H;
  w.loss = w.z + (size_t)rows * C;
  return w;
}
// LDS of the rows kernel: f, u, a, d [E] each, h, dh [H] each, parts [ROWS_THREADS], wave scratch [2 * ROWS_WAVES]
inline size_t rows_lds_bytes(int E, int H) { return (4 * (size_t)E + 2 * (size_t)H + ROWS_THREADS + 2 * ROWS_WAVES) * sizeof(float); }

// sum_k row[k] * vec[k], k < n, over the lanes of one wave: lane-strided partial sums, then the tree; every lane holds the result
__device__ __forceinline__ float wave_dot(const float* __restrict__ row, const float* vec, int n, int lane) {
  float s = 0.f;
  for (int k = lane; k < n; k += 64) s += row[k] * vec[k];
  return wave_sum(s);
}

// out[j] = sum_k coef[k] * mat[k * ld + j] for j < cols, k < depth: the columns across the threads (coalesced rows of mat), the depth
// split in `parts` consecutive ranges that are summed serially and then added in range order.  parts * cols <= ROWS_THREADS or parts == 1.
// out[] (LDS, cols floats) overlaps neither coef nor parts_lds; ends with the result in out[] behind a barrier.
__device__ __forceinline__ void columns_sum(const float* __restrict__ mat, int64_t ld, const float* coef, int depth, int cols, float* parts_lds,
                                            float* out) {
  const int parts = cols < ROWS_THREADS ? ROWS_THREADS / cols : 1;
  const int span = (depth + parts - 1) / parts;
  if (parts == 1) {
    for (int j = threadIdx.x; j < cols; j += ROWS_THREADS) {
      float s = 0.f;
      for (int k = 0; k < depth; ++k) s += coef[k] * mat[(int64_t)k * ld + j];
      out[j] = s;
    }
    __syncthreads();
    return;
  }
  const int t = threadIdx.x;
  if (t < parts * cols) {
    const int j = t % cols, p = t / cols;
    const int k0 = p * span, k1 = k0 + span < depth ? k0 + span : depth;
    float s = 0.f;
    for (int k = k0; k < k1; ++k) s += coef[k] * mat[(int64_t)k * ld + j];
    parts_lds[t] = s;
  }
  __syncthreads();
  if (t < cols) {
    float s = parts_lds[t];
    for (int p = 1; p < parts; ++p) s += parts_lds[p * cols + t];
    out[t] = s;
  }
  __syncthreads();
}

// The LDS of one sample, carved the same way by every kernel that runs the forward
struct RowLds {
  float *sf, *su, *sa, *sd, *sh, *sdh, *sparts, *swave;
};
__device__ __forceinline__ RowLds carve_lds(float* lds, int E, int H) {
  RowLds s;
  s.sf = lds;               // f, the raw features of the sample
  s.su = s.sf + E;          // g, then u
  s.sa = s.su + E;          // a = relu(p2): the second mask
  s.sd = s.sa + E;          // du, then da
  s.sh = s.sd + E;          // h = relu(p1): the first mask
  s.sdh = s.sh + H;         // da W2, before the first mask
  s.sparts = s.sdh + H;     // columns_sum's partial sums
  s.swave = s.sparts + ROWS_THREADS;   // one value per wave, twice: the maximum's and the sum's
  return s;
}

// The forward of one sample by its workgroup, the one body of the training step and of the validation logits: f -> h -> a -> g -> u in LDS
// and z_c = s (u . T_c) to z[0 .. C).  out_h (null: not kept) receives h.  Returns n = |g|, the same bits in every thread, and leaves in `m`
// the maximum over the classes of the thread's own wave; the stores to z are not yet ordered before other waves' loads.
__device__ __forceinline__ float adapter_forward_row(const float* __restrict__ f, const float* __restrict__ text, const float* __restrict__ w1,
                                                     const float* __restrict__ w2, int E, int H, int C, float ratio, float scale, const RowLds& s,
                                                     float* __restrict__ out_h, float* __restrict__ z, float& m) {
#pragma clang fp contract(off)   // z = s * (u . T_c) is rounded before the maximum is subtracted: the largest term is exp(0) exactly
  float *sf = s.sf, *su = s.su, *sa = s.sa, *sh = s.sh;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int e = t; e < E; e += ROWS_THREADS) sf[e] = f[e];
  __syncthreads();
  // h = relu(f W1^T): one wave per hidden unit
  for (int k = wave; k < H; k += ROWS_WAVES) {
    const float p1 = wave_dot(w1 + (int64_t)k * E, sf, E, lane);
    if (lane == 0) {
      sh[k] = fmaxf(p1, 0.f);
      if (out_h) out_h[k] = sh[k];
    }
  }
  __syncthreads();
  // a = relu(h W2^T), g = r a + (1 - r) f: one wave per feature
  for (int e = wave; e < E; e += ROWS_WAVES) {
    const float p2 = wave_dot(w2 + (int64_t)e * H, sh, H, lane);
    if (lane == 0) {
      const float a = fmaxf(p2, 0.f);
      sa[e] = a;
      su[e] = ratio * a + (1.f - ratio) * sf[e];
    }
  }
  __syncthreads();
  // n = |g|: every wave forms the same sum in the same order, so every thread holds the same bits
  float nn = 0.f;
  for (int e = lane; e < E; e += 64) nn += su[e] * su[e];
  const float n = sqrtf(wave_sum(nn));
  __syncthreads();            // every wave has read g
  for (int e = t; e < E; e += ROWS_THREADS) su[e] = su[e] / n;
  __syncthreads();
  // z_c = s (u . T_c): one wave per class; the row maximum on the way
  m = -INFINITY;
  for (int c = wave; c < C; c += ROWS_WAVES) {
    const float zc = scale * wave_dot(text + (int64_t)c * E, su, E, lane);
    if (lane == 0) z[c] = zc;
    m = fmaxf(m, zc);
  }
  return n;
}

__global__ __launch_bounds__(ROWS_THREADS) void adapter_rows_kernel(const float* __restrict__ feats, int64_t ld, const int64_t* __restrict__ labels,
                                                                    const int32_t* __restrict__ order, int first, int rows, int N,
                                                                    const float* __restrict__ text, const float* __restrict__ w1,
                                                                    const float* __restrict__ w2, int E, int H, int C, float ratio, float scale,
                                                                    Workspace ws) {
#pragma clang fp contract(off)
  extern __shared__ float lds[];
  const RowLds s = carve_lds(lds, E, H);
  float *su = s.su, *sa = s.sa, *sd = s.sd, *sh = s.sh, *sdh = s.sdh, *sparts = s.sparts, *swave = s.swave;
  const int t = threadIdx.x, lane = t & 63;
  const int r = blockIdx.x;
  float* out_h = ws.h + (size_t)r * H;
  float* out_da = ws.da + (size_t)r * E;
  float* out_dh = ws.dh + (size_t)r * H;
  float* z = ws.z + (size_t)r * C;
  const int i = order ? order[r] : first + r;
  const int64_t y = i >= 0 && i < N ? labels[i] : -1;
  if (y < 0 || y >= C) {      // the same for every thread of the workgroup: nobody waits at a barrier below
    for (int e = t; e < E; e += ROWS_THREADS) out_da[e] = NAN;
    for (int k = t; k < H; k += ROWS_THREADS) out_h[k] = out_dh[k] = NAN;
    if (t == 0) ws.loss[r] = NAN;
    return;
  }
  float m;
  const float n = adapter_forward_row(feats + (int64_t)i * ld, text, w1, w2, E, H, C, ratio, scale, s, out_h, z, m);
  m = waves_max<ROWS_WAVES>(m, swave);   // its barrier also orders the stores to z before the loads below (workgroup scope)
  // dz_c = (softmax_c - [c == y]) / B, in place of z
  xent_row<ROWS_WAVES>(z, z, C, m, y, 1.f / (float)rows, swave + ROWS_WAVES, ws.loss + r);
  __syncthreads();
  // du = s dz T: the features across the threads, the classes in consecutive parts
  columns_sum(text, E, z, C, E, sparts, sd);
  float dot = 0.f;
  for (int e = lane; e < E; e += 64) {
    const float du = scale * sd[e];
    dot += su[e] * du;
  }
  dot = wave_sum(dot);        // u . du, the same bits in every wave
  __syncthreads();            // every wave has read du
  // dg = (du - u (u . du)) / n;  da = r dg [p2 > 0]
  for (int e = t; e < E; e += ROWS_THREADS) {
    const float du = scale * sd[e];
    const float dg = (du - su[e] * dot) / n;
    const float da = sa[e] > 0.f ? ratio * dg : 0.f;
    sd[e] = out_da[e] = da;
  }
  __syncthreads();
  // dh = (da W2) [p1 > 0]: the hidden units across the threads, the features in consecutive parts
  columns_sum(w2, H, sd, E, H, sparts, sdh);
  for (int k = t; k < H; k += ROWS_THREADS) out_dh[k] = sh[k] > 0.f ? sdh[k] : 0.f;
}

// grid (N_val): the validation logits of row r, the training forward on the weights as they are (DESIGN.md "Fit monitor"): every element
// of out [N_val, C] is written by lane 0 of one wave of one workgroup; a non-finite feature makes g, n and with them the whole row non-finite
__global__ __launch_bounds__(ROWS_THREADS) void adapter_val_logits_kernel(const float* __restrict__ feats, int64_t ld, const float* __restrict__ text,
                                                                          const float* __restrict__ w1, const float* __restrict__ w2, int E, int H,
                                                                          int C, float ratio, float scale, float* __restrict__ out) {
  extern __shared__ float lds[];
  const RowLds s = carve_lds(lds, E, H);
  const int64_t r = blockIdx.x;
  float m;
  adapter_forward_row(feats + r * ld, text, w1, w2, E, H, C, ratio, scale, s, nullptr, out + r * C, m);
}

// Elements [0, E H) are W2 [E, H], elements [E H, 2 E H) are W1 [H, E].  The weights a step's rows kernel read are final before this launch
// starts, and this launch is final before the next step's rows kernel starts: the stream orders them.
__global__ __launch_bounds__(256) void adapter_update_kernel(const float* __restrict__ feats, int64_t ld, const int32_t* __restrict__ order, int first,
                                                             int rows, int N, float* __restrict__ w1, float* __restrict__ w2,
                                                             float* __restrict__ m1, float* __restrict__ m2, int E, int H, Workspace ws,
                                                             const float* __restrict__ lr, SgdArgs a, float* __restrict__ loss_out) {
  const int64_t EH = (int64_t)E * H;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < EH) {                     // dW2[e, k] = sum_b da[b, e] h[b, k]
    const int e = (int)(idx / H), k = (int)(idx % H);
    float g = 0.f;
    for (int b = 0; b < rows; ++b) g += ws.da[(size_t)b * E + e] * ws.h[(size_t)b * H + k];
    sgd_element(w2, m2, idx, g, *lr, a);
  } else if (idx < 2 * EH) {          // dW1[k, e] = sum_b dh[b, k] f[b, e]
    const int64_t j = idx - EH;
    const int k = (int)(j / E), e = (int)(j % E);
    float g = 0.f;
    for (int b = 0; b < rows; ++b) {
      const int i = order ? order[b] : first + b;
      const float fe = i >= 0 && i < N ? feats[(int64_t)i * ld + e] : NAN;
      g += ws.dh[(size_t)b * H + k] * fe;
    }
    sgd_element(w1, m1, j, g, *lr, a);
  }
  if (blockIdx.x != 0 || !loss_out) return;   // the same for every thread of the workgroup
  mean_loss_256(ws.loss, rows, loss_out);
}

struct Problem {
  const float* feats; int64_t ld; const int64_t* labels; const float* text;
  float *w1, *w2, *m1, *m2;
  int n, E, H, C;
  float ratio, scale;
};

bool aligned(const void* p, size_t a) { return (uintptr_t)p % a == 0; }

int check_problem(const char* who, const Problem& p, const float* lr, float momentum, float dampening, float weight_decay, int nesterov) {
  CLIPMI_REQUIRE(p.feats && p.labels && p.text && p.w1 && p.w2 && lr, CLIPMI_ERR_ARG,
                 "%s: null pointer (feats, labels, text, w1, w2 and lr are required)", who);
  if (int rc = check_sgd(who, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE(momentum == 0.f || (p.m1 && p.m2), CLIPMI_ERR_ARG, "%s: null pointer (a momentum needs the buffers m1 and m2)", who);
  CLIPMI_REQUIRE(aligned(p.feats, 4) && aligned(p.text, 4) && aligned(p.w1, 4) && aligned(p.w2, 4) && aligned(p.m1, 4) && aligned(p.m2, 4) &&
                     aligned(lr, 4) && aligned(p.labels, 8),
                 CLIPMI_ERR_ARG, "%s: fp32 arrays must be 4-byte aligned, the labels 8-byte aligned", who);
  CLIPMI_REQUIRE(std::isfinite(p.ratio) && std::isfinite(p.scale), CLIPMI_ERR_ARG, "%s: ratio=%g, scale=%g (both finite)", who, p.ratio, p.scale);
  CLIPMI_REQUIRE(p.n >= 1, CLIPMI_ERR_SHAPE, "%s: n=%d (>= 1)", who, p.n);
  CLIPMI_REQUIRE(p.C >= 2, CLIPMI_ERR_SHAPE, "%s: C=%d (>= 2 classes)", who, p.C);
  CLIPMI_REQUIRE(p.E >= 1 && p.H >= 1, CLIPMI_ERR_SHAPE, "%s: E=%d H=%d (both >= 1)", who, p.E, p.H);
  CLIPMI_REQUIRE(rows_lds_bytes(p.E, p.H) <= ROWS_LDS_MAX, CLIPMI_ERR_SHAPE, "%s: E=%d H=%d need %zu bytes of LDS per sample, %zu at most", who,
                 p.E, p.H, rows_lds_bytes(p.E, p.H), ROWS_LDS_MAX);
  CLIPMI_REQUIRE(p.ld >= p.E, CLIPMI_ERR_SHAPE, "%s: ld=%lld < E=%d", who, (long long)p.ld, p.E);
  return CLIPMI_OK;
}

int check_workspace(const char* who, const void* workspace, size_t bytes, int rows, const Problem& p) {
  CLIPMI_REQUIRE(workspace, CLIPMI_ERR_ARG, "%s: null workspace", who);
  CLIPMI_REQUIRE(aligned(workspace, 8), CLIPMI_ERR_ARG, "%s: the workspace must be 8-byte aligned", who);
  const size_t need = clipmi_adapter_train_workspace_bytes(rows, p.E, p.H, p.C);
  CLIPMI_REQUIRE(bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, bytes, need);
  return CLIPMI_OK;
}

// one step on the samples order[0 .. rows) (or first .. first + rows - 1) of the n cached rows
int launch_step(const Problem& p, const int32_t* order, int first, int rows, const float* lr, const SgdArgs& a, float* loss_out, void* workspace,
                hipStream_t s) {
  const Workspace ws = carve(workspace, rows, p.E, p.H, p.C);
  hipLaunchKernelGGL(adapter_rows_kernel, dim3(rows), dim3(ROWS_THREADS), rows_lds_bytes(p.E, p.H), s, p.feats, p.ld, p.labels, order, first, rows,
                     p.n, p.text, p.w1, p.w2, p.E, p.H, p.C, p.ratio, p.scale, ws);
  if (int rc = check_launch("adapter_rows_kernel")) return rc;
  const int64_t elements = 2 * (int64_t)p.E * p.H;
  hipLaunchKernelGGL(adapter_update_kernel, dim3((unsigned)((elements + 255) / 256)), dim3(256), 0, s, p.feats, p.ld, order, first, rows, p.n, p.w1,
                     p.w2, p.m1, p.m2, p.E, p.H, ws, lr, a, loss_out);
  return check_launch("adapter_update_kernel");
}

// the validation logits: what clipmi_adapter_val_logits refuses, in the vocabulary of check_problem
int check_val(const char* who, const float* feats, int64_t ld, const float* text, const float* w1, const float* w2, int n_val, int E, int H, int C,
              float ratio, float scale, const float* logits) {
  CLIPMI_REQUIRE(feats && text && w1 && w2 && logits, CLIPMI_ERR_ARG, "%s: null pointer (feats, text, w1, w2 and the logits are required)", who);
  CLIPMI_REQUIRE(aligned(feats, 4) && aligned(text, 4) && aligned(w1, 4) && aligned(w2, 4), CLIPMI_ERR_ARG, "%s: fp32 arrays must be 4-byte aligned",
                 who);
  CLIPMI_REQUIRE(aligned(logits, 16), CLIPMI_ERR_ARG, "%s: the logits must be 16-byte aligned (clipmi_val_score reads them)", who);
  CLIPMI_REQUIRE(std::isfinite(ratio) && std::isfinite(scale), CLIPMI_ERR_ARG, "%s: ratio=%g, scale=%g (both finite)", who, ratio, scale);
  CLIPMI_REQUIRE(n_val >= 1, CLIPMI_ERR_SHAPE, "%s: N_val=%d (>= 1)", who, n_val);
  CLIPMI_REQUIRE(C >= 2, CLIPMI_ERR_SHAPE, "%s: C=%d (>= 2 classes)", who, C);
  CLIPMI_REQUIRE(E >= 1 && H >= 1, CLIPMI_ERR_SHAPE, "%s: E=%d H=%d (both >= 1)", who, E, H);
  CLIPMI_REQUIRE(rows_lds_bytes(E, H) <= ROWS_LDS_MAX, CLIPMI_ERR_SHAPE, "%s: E=%d H=%d need %zu bytes of LDS per sample, %zu at most", who, E, H,
                 rows_lds_bytes(E, H), ROWS_LDS_MAX);
  CLIPMI_REQUIRE(ld >= E, CLIPMI_ERR_SHAPE, "%s: ld=%lld < E=%d", who, (long long)ld, E);
  return CLIPMI_OK;
}

int launch_val(const float* feats, int64_t ld, const float* text, const float* w1, const float* w2, int n_val, int E, int H, int C, float ratio,
               float scale, float* logits, hipStream_t s) {
  hipLaunchKernelGGL(adapter_val_logits_kernel, dim3((unsigned)n_val), dim3(ROWS_THREADS), rows_lds_bytes(E, H), s, feats, ld, text, w1, w2, E, H, C,
                     ratio, scale, logits);
  return check_launch("adapter_val_logits_kernel");
}

// The one body of clipmi_adapter_fit and clipmi_adapter_fit_monitored.  Without a monitor the steps are enqueued and nothing else; with one,
// behind the last step of every epoch: the validation logits of the weights as they are, the epoch record and, with a best slot, the selection
// of the block [w1 | w2] -- which is why the monitored run wants w2 == w1 + H E.
int run_fit(const char* who, const Problem& p, const int32_t* order, int batch, int epochs, int drop_last, const float* lr, int first_step,
            float momentum, float dampening, float weight_decay, int nesterov, float* losses, void* workspace, size_t workspace_bytes,
            const FitMonitor* mon, hipStream_t stream) {
  if (int rc = check_problem(who, p, lr, momentum, dampening, weight_decay, nesterov)) return rc;
  CLIPMI_REQUIRE(batch >= 1, CLIPMI_ERR_SHAPE, "%s: batch=%d (>= 1)", who, batch);
  CLIPMI_REQUIRE(epochs >= 0, CLIPMI_ERR_ARG, "%s: epochs=%d (>= 0)", who, epochs);
  const int width = batch < p.n ? batch : p.n;   // the widest batch of the run
  if (int rc = check_workspace(who, workspace, workspace_bytes, width, p)) return rc;
  const int64_t EH = (int64_t)p.E * p.H;
  if (mon) {
    if (int rc = check_fit_monitor(who, *mon, p.E, p.C)) return rc;
    CLIPMI_REQUIRE(!mon->best_block || (p.w2 == p.w1 + EH && aligned(p.w1, 16)), CLIPMI_ERR_ARG,
                   "%s: a best slot needs w1 and w2 as one 16-byte aligned block [w1 | w2] (w2 == w1 + H E)", who);
  }
  const int per_epoch = drop_last ? p.n / batch : (int)(((int64_t)p.n + batch - 1) / batch);
  SgdArgs a = make_sgd_args(momentum, dampening, weight_decay, nesterov, first_step);
  int64_t step = 0;
  for (int e = 0; e < epochs; ++e) {
    const int32_t* epoch_order = order ? order + (int64_t)e * p.n : nullptr;
    for (int k = 0; k < per_epoch; ++k, ++step) {
      const int first = k * batch;   // k < per_epoch <= n: no overflow
      const int rows = p.n - first < batch ? p.n - first : batch;
      if (int rc = launch_step(p, epoch_order ? epoch_order + first : nullptr, first, rows, lr + step, a, losses ? losses + step : nullptr,
                               workspace, stream))
        return rc;
      a.first_step = 0;
    }
    if (!mon) continue;
    if (int rc = launch_val(mon->val_feats, mon->val_ld, p.text, p.w1, p.w2, mon->n_val, p.E, p.H, p.C, p.ratio, p.scale, fit_monitor_logits(*mon),
                            stream))
      return rc;
    if (int rc = fit_monitor_score(*mon, e, p.C, p.w1, 2 * EH, (clipmi_stream_t)stream)) return rc;
  }
  return CLIPMI_OK;
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

size_t clipmi_adapter_train_workspace_bytes(int rows, int E, int H, int C) {
  if (rows < 1 || E < 1 || H < 1 || C < 2) return 0;
  return align256(workspace_floats(rows, E, H, C) * sizeof(float));
}

int clipmi_adapter_train_step(const float* feats, int64_t ld, const int64_t* labels, const float* text, float* w1, float* w2, float* m1, float* m2,
                              int rows, int E, int H, int C, float ratio, float scale, const float* lr, int first_step, float momentum,
                              float dampening, float weight_decay, int nesterov, float* loss, void* workspace, size_t workspace_bytes,
                              clipmi_stream_t stream) {
  const Problem p{feats, ld, labels, text, w1, w2, m1, m2, rows, E, H, C, ratio, scale};
  if (int rc = check_problem("adapter_train_step", p, lr, momentum, dampening, weight_decay, nesterov)) return rc;
  if (int rc = check_workspace("adapter_train_step", workspace, workspace_bytes, rows, p)) return rc;
  const SgdArgs a = make_sgd_args(momentum, dampening, weight_decay, nesterov, first_step);
  return launch_step(p, nullptr, 0, rows, lr, a, loss, workspace, (hipStream_t)stream);
}

int clipmi_adapter_fit(const float* feats, int64_t ld, const int64_t* labels, const int32_t* order, const float* text, float* w1, float* w2,
                       float* m1, float* m2, int n, int E, int H, int C, int batch, int epochs, int drop_last, float ratio, float scale,
                       const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, float* losses,
                       void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  const Problem p{feats, ld, labels, text, w1, w2, m1, m2, n, E, H, C, ratio, scale};
  return run_fit("adapter_fit", p, order, batch, epochs, drop_last, lr, first_step, momentum, dampening, weight_decay, nesterov, losses, workspace,
                 workspace_bytes, nullptr, (hipStream_t)stream);
}

size_t clipmi_adapter_fit_monitored_workspace_bytes(int n_val, int C, int n_bins) { return C >= 2 ? fit_monitor_bytes(n_val, C, n_bins) : 0; }

int clipmi_adapter_fit_monitored(const float* feats, int64_t ld, const int64_t* labels, const int32_t* order, const float* text, float* w1, float* w2,
                                 float* m1, float* m2, int n, int E, int H, int C, int batch, int epochs, int drop_last, float ratio, float scale,
                                 const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, float* losses,
                                 void* workspace, size_t workspace_bytes, const float* val_feats, int64_t val_ld, const int64_t* val_labels,
                                 int n_val, int n_bins, void* records, int criterion, void* best_block, float* best_params,
                                 void* monitor_workspace, size_t monitor_workspace_bytes, clipmi_stream_t stream) {
  const Problem p{feats, ld, labels, text, w1, w2, m1, m2, n, E, H, C, ratio, scale};
  const FitMonitor mon{val_feats, val_ld, val_labels, n_val, n_bins, records, criterion, best_block, best_params, monitor_workspace,
                       monitor_workspace_bytes};
  return run_fit("adapter_fit_monitored", p, order, batch, epochs, drop_last, lr, first_step, momentum, dampening, weight_decay, nesterov, losses,
                 workspace, workspace_bytes, &mon, (hipStream_t)stream);
}

int clipmi_adapter_val_logits(const float* feats, int64_t ld, const float* text, const float* w1, const float* w2, int n_val, int E, int H, int C,
                              float ratio, float scale, float* logits, clipmi_stream_t stream) {
  if (int rc = check_val("adapter_val_logits", feats, ld, text, w1, w2, n_val, E, H, C, ratio, scale, logits)) return rc;
  return launch_val(feats, ld, text, w1, w2, n_val, E, H, C, ratio, scale, logits, (hipStream_t)stream);
}

}  // extern "C"
