// Parameterized temperature scaling (PTS; Tomani, Cremers, Buettner, ECCV 2022): a small MLP on the K largest logits of a row gives that
// row's temperature.  For a row z of C logits:
//   f = the K largest values of z, descending;  h_0 = f;  h_l = relu(W_l h_{l-1} + b_l), l = 1 .. n_layers, each n_nodes wide;
//   t = w_out . h_last + b_out;  T = clamp(|t|, 1e-12, 1e12);  calibrated logits z / T;  p = softmax(z / T);
//   loss = (1 / C) sum_c (p_c - [c == y])^2, the batch mean of it is trained.
// Parameter block, fp32: [W_1 | b_1 | ... | W_n | b_n | w_out | b_out], every W row-major [out, in] (nn.Linear's layout).
//
// Kernels (DESIGN.md "PTS fit"), one wave per row wherever a row is worked on:
//   pts_topk_kernel    K selection rounds over the row: round k takes the largest value behind round k-1's (value, index) in the order
//                      (value descending, index ascending), so equal values are taken one index at a time and nothing is marked.
//   pts_apply_kernel   selection, MLP, T, then out = z / T (IEEE division), lane-strided.
//   pts_rows_kernel    MLP forward from the cached features, T, the softmax sums of z / T, the row loss, d loss / d t, and the MLP's
//                      backward down to every layer's pre-activation gradient: one record of 2 + 2 n_layers n_nodes floats per row,
//                      {loss, dt, delta_1 .. delta_n, h_1 .. h_n}.  A row's record does not depend on its batch.
//   pts_finish_kernel  one workgroup: thread p owns parameter p, adds the rows' products delta x h (exact in float64) in row order in
//                      float64, divides by the rows, rounds once to fp32 and applies torch.optim.SGD's or Adam's rule to its element.
// Two launches per step, ordered by the stream alone; no atomics, no workgroup waits for another: the same inputs give the same bits.
// state, fp32 words: [params P | buffer P | buffer P | steps taken int32 | last batch loss]; SGD's momentum buffer is the first buffer,
// Adam's exp_avg and exp_avg_sq are the two.
#include <climits>
#include <cmath>

#include "common.h"
#include "train_rules.h"

namespace clipmi {
namespace {

struct PtsNet {
  int L, n, K;   // hidden layers, their width, features
};
// offset of hidden layer l's weights in the block, l in [0, L); l == L: w_out
__host__ __device__ inline int pts_off(const PtsNet& g, int l) { return l == 0 ? 0 : g.n * g.K + g.n + (l - 1) * (g.n * g.n + g.n); }
__host__ __device__ inline int pts_last(const PtsNet& g) { return g.L == 0 ? g.K : g.n; }   // width of what w_out multiplies
__host__ __device__ inline int pts_count(const PtsNet& g) { return pts_off(g, g.L) + pts_last(g) + 1; }
__host__ __device__ inline int pts_record(const PtsNet& g) { return 2 + 2 * g.L * g.n; }

struct PtsAdam {
  double beta1, beta2, eps;
};

// The K largest values of row[0 .. C), descending: lane k < K returns the k-th (the other lanes 0).  -inf is an ordinary value.  *has_nan:
// the row holds a NaN (a NaN is never selected: every comparison with it is false).  All 64 lanes call it.
__device__ __forceinline__ float pts_select(const float* row, int C, int K, int lane, bool* has_nan) {
  float mine = 0.f, nan = 0.f;
  float pv = INFINITY;
  int pi = -1;
  for (int k = 0; k < K; ++k) {
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int c = lane; c < C; c += 64) {
      const float v = row[c];
      if (k == 0 && v != v) nan = 1.f;
      const bool behind = v < pv || (v == pv && c > pi);
      if (behind && (v > bv || (v == bv && c < bi))) {
        bv = v;
        bi = c;
      }
    }
    wave_argmax(bv, bi);
    if (lane == k) mine = bv;
    pv = bv;
    pi = bi;
  }
  *has_nan = wave_max(nan) > 0.f;
  return mine;
}

// the sum / maximum over the wave's 64 lanes in float64, the same bits in every lane (a butterfly: both partners add the same two values)
__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// t of one row in every lane: h holds h_0 (lane i < K: f_i, the others 0).  h_rec (or null) receives h_1 .. h_L, L * n floats.  The net is
// tiny, so every dot product is formed in float64 (fp32 products are exact there) and rounded to fp32 once: h_l and t are what a float64
// evaluation of the fp32 inputs rounds to, whatever the order of the sum (up to float64's own rounding next to an fp32 tie).
__device__ __forceinline__ float pts_forward(const float* __restrict__ params, const PtsNet g, float h, int lane, float* __restrict__ h_rec) {
  const float* p = params;
  int n_in = g.K;
  const bool on = lane < g.n;
  for (int l = 0; l < g.L; ++l) {
    double acc = on ? (double)p[g.n * n_in + lane] : 0.0;
    for (int i = 0; i < n_in; ++i) {
      const float hv = __shfl(h, i);
      const float w = on ? p[lane * n_in + i] : 0.f;
      acc += (double)w * (double)hv;
    }
    h = on && !(acc <= 0.0) ? (float)acc : 0.f;   // relu; a NaN stays one
    if (h_rec && on) h_rec[l * g.n + lane] = h;
    p += g.n * n_in + g.n;
    n_in = g.n;
  }
  const float w = lane < n_in ? p[lane] : 0.f;
  return (float)(wave_sum_f64((double)w * (double)h) + (double)p[n_in]);
}

__device__ __forceinline__ float pts_temperature(float t) { return fminf(fmaxf(fabsf(t), 1e-12f), 1e12f); }

__global__ __launch_bounds__(256) void pts_topk_kernel(const float* __restrict__ logits, int64_t ld, int N, int C, int K, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= N) return;
  bool has_nan;
  const float f = pts_select(logits + (int64_t)r * ld, C, K, lane, &has_nan);
  if (lane < K) out[(int64_t)r * K + lane] = has_nan ? NAN : f;
}

// out may be logits itself: a row's reads all precede its writes (T depends on every one of them), and no wave reads another's row
__global__ __launch_bounds__(256) void pts_apply_kernel(const float* logits, int64_t ld, int N, int C, const float* __restrict__ params, PtsNet g,
                                                        float* out, int64_t ld_out, float* __restrict__ temperature) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= N) return;
  const float* row = logits + (int64_t)r * ld;
  bool has_nan;
  float f = pts_select(row, C, g.K, lane, &has_nan);
  if (has_nan) f = NAN;
  const float T = pts_temperature(pts_forward(params, g, lane < g.K ? f : 0.f, lane, nullptr));
  if (temperature && lane == 0) temperature[r] = T;
  float* o = out + (int64_t)r * ld_out;
  for (int c = lane; c < C; c += 64) o[c] = row[c] / T;
}

// rec[r] for batch position r: sample order[r], or first + r without an order.  A sample index outside [0, N) or a label outside [0, C)
// is never used as an address: the whole record is NaN (the host checks both before it launches anything).
__global__ __launch_bounds__(256) void pts_rows_kernel(const float* __restrict__ feat, const float* __restrict__ logits, int64_t ld,
                                                       const int64_t* __restrict__ labels, const int32_t* __restrict__ order, int first, int rows,
                                                       int N, int C, const float* __restrict__ params, PtsNet g, float* __restrict__ rec) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int S = pts_record(g);
  float* out = rec + (int64_t)r * S;
  const int i = order ? order[r] : first + r;
  const bool in = i >= 0 && i < N;
  const int64_t y = in ? labels[i] : -1;
  if (!in || y < 0 || y >= C) {   // the same in every lane of the wave
    for (int q = lane; q < S; q += 64) out[q] = NAN;
    return;
  }
  float* h_rec = out + 2 + g.L * g.n;
  const float t = pts_forward(params, g, lane < g.K ? feat[(int64_t)i * g.K + lane] : 0.f, lane, h_rec);
  const float T = pts_temperature(t);

  // The softmax of z / T and everything behind it in float64, from the fp32 z and T: the loss and d loss / d t are rounded to fp32 once.
  // The label's term is kept apart: 1 - p_y = sum_{c != y} e_c / S has no cancellation.
  const float* __restrict__ row = logits + (int64_t)i * ld;
  const double inv = 1.0 / (double)T;
  double m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmax(m, (double)row[c] * inv);
  m = wave_max_f64(m);
  double So = 0.0, E2 = 0.0, U = 0.0, V = 0.0, ey = 0.0, dy = 0.0;   // over c != y: sum e, e^2, d e, d e^2 with d = z / T - m, e = exp(d)
  for (int c = lane; c < C; c += 64) {
    const double d = (double)row[c] * inv - m;
    const double e = exp(d);
    if (c == y) {
      ey = e;
      dy = d;
    } else {
      So += e;
      E2 += e * e;
      U += d * e;
      V += d * (e * e);
    }
  }
  So = wave_sum_f64(So);
  E2 = wave_sum_f64(E2);
  U = wave_sum_f64(U);
  V = wave_sum_f64(V);
  ey = wave_sum_f64(ey);   // one lane's value and 63 zeros
  dy = wave_sum_f64(dy);
  const double Sm = So + ey;
  const double py = ey / Sm, q = So / Sm;
  const double P2 = E2 / (Sm * Sm);               // sum_{c != y} p_c^2
  const float loss = (float)((P2 + q * q) / (double)C);
  // g_c = d loss / d p_c = (2 / C)(p_c - [c == y]);  G = sum_c p_c g_c;  d loss / d (z_k / T) = p_k (g_k - G), which sums to zero over k, so
  // d loss / d T = -(1 / T) sum_k (z_k / T - m) p_k (g_k - G)
  const double two_c = 2.0 / (double)C;
  const double G = two_c * (P2 - py * q);
  const double X = two_c * (V / (Sm * Sm) - dy * py * q) - G * (U / Sm + dy * py);
  const float a = fabsf(t);
  const double sign = t > 0.f ? 1.0 : (t < 0.f ? -1.0 : 0.0);                        // abs has derivative 0 at 0
  const float dt = a >= 1e-12f && a <= 1e12f ? (float)(sign * (-X * inv)) : 0.f;     // clamp passes the gradient on the closed interval

  // the MLP's backward: delta_l = d loss / d (W_l h_{l-1} + b_l), from the last hidden layer down; every sum in float64, rounded once
  if (g.L > 0) {
    const bool on = lane < g.n;
    float dh = on ? dt * params[pts_off(g, g.L) + lane] : 0.f;
    for (int l = g.L - 1; l >= 0; --l) {
      const float hl = on ? h_rec[l * g.n + lane] : 0.f;   // this lane's own store above
      const float delta = hl > 0.f ? dh : 0.f;
      if (on) out[2 + l * g.n + lane] = delta;
      if (l == 0) break;
      const float* __restrict__ W = params + pts_off(g, l);   // [n, n]: layer l reads layer l-1's n outputs
      double acc = 0.0;
      for (int j = 0; j < g.n; ++j) {
        const float dj = __shfl(delta, j);
        const float w = on ? W[j * g.n + lane] : 0.f;
        acc += (double)w * (double)dj;
      }
      dh = (float)acc;
    }
  }
  if (lane == 0) {
    out[0] = loss;
    out[1] = dt;
  }
}

// lr == nullptr: evaluate only (batch_out receives {mean loss, the mean gradient of the P parameters}).  Otherwise the optimiser's step
// on the state with *lr.
__global__ __launch_bounds__(256) void pts_finish_kernel(const float* __restrict__ rec, const float* __restrict__ feat, const int32_t* __restrict__ order,
                                                         int first, int rows, int N, PtsNet g, float* __restrict__ state, const float* __restrict__ lr,
                                                         int optimizer, SgdArgs sgd, PtsAdam adam, float weight_decay, float* __restrict__ loss_out,
                                                         float* __restrict__ batch_out) {
  __shared__ double sl[1][256];
  const int t = threadIdx.x;
  const int P = pts_count(g), S = pts_record(g);
  const int steps = lr ? reinterpret_cast<const int32_t*>(state)[3 * P] : 0;   // read in front of block_sum_f64's barriers, written behind them
  double ls[1] = {0.0};
  for (int r = t; r < rows; r += 256) ls[0] += (double)rec[(int64_t)r * S];
  block_sum_f64(ls, sl);
  const float loss = (float)(ls[0] / (double)rows);

  const int w_out = pts_off(g, g.L);
  for (int p = t; p < P; p += 256) {
    // parameter p's gradient is sum_r a_r b_r: a at record word ia; b at record word ib, feature ib - S (ib >= S), or 1 (ib < 0)
    int ia, ib;
    if (p >= w_out) {
      ia = 1;
      const int i = p - w_out;
      ib = i == pts_last(g) ? -1 : (g.L == 0 ? S + i : 2 + g.L * g.n + (g.L - 1) * g.n + i);
    } else {
      int l = 0;
      while (l + 1 < g.L && p >= pts_off(g, l + 1)) ++l;
      const int n_in = l == 0 ? g.K : g.n;
      const int q = p - pts_off(g, l);
      if (q >= g.n * n_in) {
        ia = 2 + l * g.n + (q - g.n * n_in);
        ib = -1;
      } else {
        ia = 2 + l * g.n + q / n_in;
        ib = l == 0 ? S + q % n_in : 2 + g.L * g.n + (l - 1) * g.n + q % n_in;
      }
    }
    double acc = 0.0;
    if (ib < 0) {
      for (int r = 0; r < rows; ++r) acc += (double)rec[(int64_t)r * S + ia];
    } else if (ib < S) {
      for (int r = 0; r < rows; ++r) acc += (double)rec[(int64_t)r * S + ia] * (double)rec[(int64_t)r * S + ib];
    } else {
      for (int r = 0; r < rows; ++r) {
        const int i = order ? order[r] : first + r;
        const float f = i >= 0 && i < N ? feat[(int64_t)i * g.K + (ib - S)] : NAN;
        acc += (double)rec[(int64_t)r * S + ia] * (double)f;
      }
    }
    const float grad = (float)(acc / (double)rows);
    if (batch_out) batch_out[1 + p] = grad;
    if (!lr) continue;
    if (optimizer == 0) {
      SgdArgs a = sgd;
      a.first_step = steps == 0;
      sgd_element(state, state + P, p, grad, *lr, a);
    } else {
      const double st = (double)(steps + 1);
      const AdamArgs a{(float)(1.0 - adam.beta1), (float)adam.beta2, (float)(1.0 - adam.beta2), (float)adam.eps, weight_decay,
                       1.0 - pow(adam.beta1, st), sqrt(1.0 - pow(adam.beta2, st))};
      adam_element(state, state + P, state + 2 * P, p, grad, *lr, a);
    }
  }
  if (t != 0) return;
  if (batch_out) batch_out[0] = loss;
  if (loss_out) *loss_out = loss;
  if (lr) {
    reinterpret_cast<int32_t*>(state)[3 * P] = steps + 1;
    state[3 * P + 1] = loss;
  }
}

int check_net(const char* who, int n_layers, int n_nodes, int K, int C) {
  CLIPMI_REQUIRE(n_layers >= 0 && n_layers <= 4, CLIPMI_ERR_SHAPE, "%s: n_layers=%d (0 .. 4)", who, n_layers);
  CLIPMI_REQUIRE(n_nodes >= 1 && n_nodes <= 32, CLIPMI_ERR_SHAPE, "%s: n_nodes=%d (1 .. 32)", who, n_nodes);
  CLIPMI_REQUIRE(K >= 1 && K <= 32, CLIPMI_ERR_SHAPE, "%s: K=%d (1 .. 32)", who, K);
  CLIPMI_REQUIRE(C >= 2, CLIPMI_ERR_SHAPE, "%s: C=%d (>= 2 classes)", who, C);
  CLIPMI_REQUIRE(C >= K, CLIPMI_ERR_SHAPE, "%s: C=%d < K=%d", who, C, K);
  return CLIPMI_OK;
}

int check_rows(const char* who, int N, int64_t ld, int C) {
  CLIPMI_REQUIRE(N >= 0, CLIPMI_ERR_SHAPE, "%s: N=%d (>= 0)", who, N);
  CLIPMI_REQUIRE(ld >= C, CLIPMI_ERR_SHAPE, "%s: ld=%lld < C=%d", who, (long long)ld, C);
  return CLIPMI_OK;
}

int check_workspace(const char* who, const float* workspace, size_t floats, size_t needed) {
  CLIPMI_REQUIRE(workspace, CLIPMI_ERR_ARG, "%s: null workspace", who);
  CLIPMI_REQUIRE((uintptr_t)workspace % 4 == 0, CLIPMI_ERR_ARG, "%s: the workspace must be 4-byte aligned", who);
  CLIPMI_REQUIRE(floats >= needed, CLIPMI_ERR_WORKSPACE, "%s: workspace of %zu floats, %zu needed", who, floats, needed);
  return CLIPMI_OK;
}

int launch_topk(const float* logits, int64_t ld, int N, int C, int K, float* out, hipStream_t s) {
  hipLaunchKernelGGL(pts_topk_kernel, dim3((N + 3) / 4), dim3(256), 0, s, logits, ld, N, C, K, out);
  return check_launch("pts_topk_kernel");
}

int launch_rows(const float* feat, const float* logits, int64_t ld, const int64_t* labels, const int32_t* order, int first, int rows, int N, int C,
                const float* params, const PtsNet& g, float* rec, hipStream_t s) {
  hipLaunchKernelGGL(pts_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, feat, logits, ld, labels, order, first, rows, N, C, params, g, rec);
  return check_launch("pts_rows_kernel");
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

int clipmi_pts_param_count(int n_layers, int n_nodes, int K) {
  if (n_layers < 0 || n_layers > 4 || n_nodes < 1 || n_nodes > 32 || K < 1 || K > 32) return 0;
  return pts_count(PtsNet{n_layers, n_nodes, K});
}

int clipmi_pts_topk(const float* logits, int64_t ld, int N, int C, int K, float* out, clipmi_stream_t stream) {
  if (int rc = check_net("pts_topk", 0, 1, K, C)) return rc;
  if (int rc = check_rows("pts_topk", N, ld, C)) return rc;
  if (N == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(logits && out, CLIPMI_ERR_ARG, "pts_topk: null pointer (logits and out are required)");
  return launch_topk(logits, ld, N, C, K, out, (hipStream_t)stream);
}

int clipmi_pts_apply(const float* logits, int64_t ld, int N, int C, const float* params, int n_layers, int n_nodes, int K, float* out,
                     int64_t ld_out, float* temperature, clipmi_stream_t stream) {
  if (int rc = check_net("pts_apply", n_layers, n_nodes, K, C)) return rc;
  if (int rc = check_rows("pts_apply", N, ld, C)) return rc;
  CLIPMI_REQUIRE(ld_out >= C, CLIPMI_ERR_SHAPE, "pts_apply: ld_out=%lld < C=%d", (long long)ld_out, C);
  if (N == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(logits && params && out, CLIPMI_ERR_ARG, "pts_apply: null pointer (logits, params and out are required)");
  hipLaunchKernelGGL(pts_apply_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, ld, N, C, params,
                     PtsNet{n_layers, n_nodes, K}, out, ld_out, temperature);
  return check_launch("pts_apply_kernel");
}

int clipmi_pts_eval(const float* features, const float* logits, int64_t ld, const int64_t* labels, const int32_t* order, int first, int rows,
                    int N, int C, const float* params, int n_layers, int n_nodes, int K, float* batch_out, float* workspace,
                    size_t workspace_floats, clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_net("pts_eval", n_layers, n_nodes, K, C)) return rc;
  if (int rc = check_rows("pts_eval", N, ld, C)) return rc;
  CLIPMI_REQUIRE(features && logits && labels && params && batch_out, CLIPMI_ERR_ARG,
                 "pts_eval: null pointer (features, logits, labels, params and batch_out are required)");
  CLIPMI_REQUIRE(rows >= 1, CLIPMI_ERR_SHAPE, "pts_eval: rows=%d (>= 1)", rows);
  CLIPMI_REQUIRE(order || (first >= 0 && (int64_t)first + rows <= N), CLIPMI_ERR_SHAPE, "pts_eval: rows %d .. %lld of N=%d without an order", first,
                 (long long)first + rows, N);
  const PtsNet g{n_layers, n_nodes, K};
  if (int rc = check_workspace("pts_eval", workspace, workspace_floats, (size_t)rows * pts_record(g))) return rc;
  if (int rc = launch_rows(features, logits, ld, labels, order, first, rows, N, C, params, g, workspace, s)) return rc;
  hipLaunchKernelGGL(pts_finish_kernel, dim3(1), dim3(256), 0, s, workspace, features, order, first, rows, N, g, nullptr, nullptr, 0, SgdArgs{},
                     PtsAdam{}, 0.f, nullptr, batch_out);
  return check_launch("pts_finish_kernel");
}

int clipmi_pts_fit(const float* logits, int64_t ld, const int64_t* labels, const int32_t* order, int N, int C, int n_layers, int n_nodes, int K,
                   int batch, int epochs, int drop_last, const float* lr, int optimizer, float momentum, float dampening, float weight_decay,
                   int nesterov, double beta1, double beta2, double eps, float* state, float* losses, float* workspace, size_t workspace_floats,
                   clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (int rc = check_net("pts_fit", n_layers, n_nodes, K, C)) return rc;
  if (int rc = check_rows("pts_fit", N, ld, C)) return rc;
  CLIPMI_REQUIRE(N >= 1, CLIPMI_ERR_SHAPE, "pts_fit: N=%d (>= 1)", N);
  CLIPMI_REQUIRE(logits && labels && lr && state, CLIPMI_ERR_ARG, "pts_fit: null pointer (logits, labels, lr and state are required)");
  CLIPMI_REQUIRE((uintptr_t)state % 4 == 0, CLIPMI_ERR_ARG, "pts_fit: the state must be 4-byte aligned");
  CLIPMI_REQUIRE(batch >= 1, CLIPMI_ERR_SHAPE, "pts_fit: batch=%d (>= 1)", batch);
  CLIPMI_REQUIRE(epochs >= 0, CLIPMI_ERR_ARG, "pts_fit: epochs=%d (>= 0)", epochs);
  CLIPMI_REQUIRE(optimizer == 0 || optimizer == 1, CLIPMI_ERR_ARG, "pts_fit: optimizer=%d (0 SGD, 1 Adam)", optimizer);
  if (optimizer == 0) {
    if (int rc = check_sgd("pts_fit", momentum, dampening, weight_decay, nesterov)) return rc;
  } else {
    CLIPMI_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, CLIPMI_ERR_ARG, "pts_fit: betas=(%g, %g) (both in [0, 1))", beta1, beta2);
    CLIPMI_REQUIRE(eps >= 0.0 && std::isfinite(eps), CLIPMI_ERR_ARG, "pts_fit: eps=%g (finite, >= 0)", eps);
    CLIPMI_REQUIRE(weight_decay >= 0.f && std::isfinite(weight_decay), CLIPMI_ERR_ARG, "pts_fit: weight_decay=%g (finite, >= 0)", weight_decay);
  }
  const PtsNet g{n_layers, n_nodes, K};
  const int width = batch < N ? batch : N;   // the widest batch of the run
  const size_t feat_floats = (size_t)N * K;
  if (int rc = check_workspace("pts_fit", workspace, workspace_floats, feat_floats + (size_t)width * pts_record(g))) return rc;
  if (epochs == 0) return CLIPMI_OK;
  float* feat = workspace;
  float* rec = workspace + feat_floats;
  if (int rc = launch_topk(logits, ld, N, C, K, feat, s)) return rc;
  const int per_epoch = drop_last ? N / batch : (int)(((int64_t)N + batch - 1) / batch);
  const SgdArgs sa = optimizer == 0 ? make_sgd_args(momentum, dampening, weight_decay, nesterov, 0) : SgdArgs{};
  const PtsAdam aa{beta1, beta2, eps};
  int64_t step = 0;
  for (int e = 0; e < epochs; ++e) {
    const int32_t* epoch_order = order ? order + (int64_t)e * N : nullptr;
    for (int k = 0; k < per_epoch; ++k, ++step) {
      const int first = k * batch;   // k < per_epoch <= N: no overflow
      const int rows = N - first < batch ? N - first : batch;
      const int32_t* o = epoch_order ? epoch_order + first : nullptr;
      if (int rc = launch_rows(feat, logits, ld, labels, o, first, rows, N, C, state, g, rec, s)) return rc;
      hipLaunchKernelGGL(pts_finish_kernel, dim3(1), dim3(256), 0, s, rec, feat, o, first, rows, N, g, state, lr + step, optimizer, sa, aa, weight_decay,
                         losses ? losses + step : nullptr, nullptr);
      if (int rc = check_launch("pts_finish_kernel")) return rc;
    }
  }
  return CLIPMI_OK;
}

}  // extern "C"
