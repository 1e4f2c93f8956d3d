// ProCal, the proximity-informed density-ratio calibrator (reference trainers/calibration/density_ratio_calibration.py:67-117 on top of
// statsmodels' KDEMultivariate.pdf, nonparametric/_kernel_base.py:456-518 + kernels.py:125).  The reference loops in Python over the test
// samples, one float64 numpy pass over every val sample each; here one launch evaluates
//   c* = T / max(T + ratio * F, 1e-10),   S(c, p) = norm_S * sum_{s in S} exp(-((c - s_c) / h_c)^2 / 2 - ((p - s_p) / h_p)^2 / 2)
// for a block of 64 queries per workgroup (one per lane), the four waves splitting each point set four ways while it streams through
// LDS in tiles of 1024 points (8 B each; every lane of a wave reads the same point: an LDS broadcast).
//
// Pre-scaling.  The host uploads every point as (s_c * k_c, s_p * k_p) in fp64, k = sqrt(log2(e) / 2) / h per set and dimension; the
// query is scaled the same way once per set.  A pair then costs two subtracts, a multiply and an FMA for the exponent
// e = du^2 + dv^2 and one v_exp_f32 for 2^-e = exp(-(d/h)^2 / 2).
//
// Precision.  The exponent is formed in fp64, rounded to fp32 once, the exp is fp32 (v_exp_f32, 1 ulp), and every term is widened to
// fp64 and summed in fp64, in an order fixed by the point counts alone (repeatable, and independent of the batch a row sits in).
// An fp32 exponent is not enough: the terms that carry a sum can have e ~ 40 (the density may fall to 1e-12 before the clamp below
// takes over), and fp32 operands give e a relative error of ~2^-22, i.e. ~1e-5 in e and 7e-6 in the term -- measured, 3.2e-6 on c*
// where both densities sit in their tails.  With the fp64 exponent the one fp32 rounding of e costs e * 2^-24 (< 2.4e-6 in e for
// e < 40), under 2e-6 relative per term.  A term lost to fp32 underflow (2^-e < 1.2e-38, e > 126) cannot matter: the prefactor
// norm_S = 1 / (|S| h_c h_p 2 pi) is at most ~1e8 for any realistic set (|S| >= 2, h >= 1e-4), so such a term moves T or F by less
// than 1e-30, while c* only departs from T / (T + ratio F) where T + ratio F falls below the 1e-10 clamp -- there c* = T / 1e-10 and
// an absolute change of 1e-30 in T is 1e-20 in c*.
//
// The row form (clipmi_procal_rows) first computes, per row and wave, from the logits and the optional DAC factor (the arithmetic of
// row_calibrate_kernel, logits.hip): i1 = argmax, p1 = 1 / sum exp(y - y_i1), the second largest entry y_i2 (lowest index on ties) and
// share = 1 / sum_{j != i1} exp(y_j - y_i2) = p_i2 / S; it keeps them in LDS, runs the KDE on (p1, proximity), and finishes with
// conf' = max(c*, (1 - c*) * share) under numpy's lowest-index tie rule, and optionally the calibrated row
// out[i1] = c*, out[j] = exp(y_j - y_i2) * (1 - c*) * share.
#include <cmath>

#include "common.h"

namespace clipmi {
namespace {

constexpr int QB = 64, NW = 4, TILE = 1024;

struct ProcalArgs {
  const double* pts[2];
  int n[2];
  double scale[2][2];
  double norm[2];
  double ratio;
};

template <bool ROWS>
__global__ __launch_bounds__(256) void procal_kernel(ProcalArgs m, const float* logits, const float* __restrict__ dac,
                                                     const float* __restrict__ conf_in, const float* __restrict__ prox,
                                                     float* probs, float* __restrict__ conf_out, int32_t* __restrict__ pred_out,
                                                     float* __restrict__ cstar_out, int N, int C) {
#pragma clang fp contract(off)   // y = logit * f is rounded once, as the reference's fp32 DAC product; fmaf below stays explicit
  __shared__ double tile[TILE][2];
  __shared__ double part[2][NW][QB];
  __shared__ float s_p1[QB], s_share[QB], s_f[QB], s_v2[QB];
  __shared__ int s_i1[QB], s_i2[QB];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int q0 = blockIdx.x * QB;

  if (ROWS) {   // row statistics: wave w takes rows w, w + 4, ... of the block (a whole wave per row: wave_* need every lane)
    for (int r = w; r < QB; r += NW) {
      const int row = q0 + r;
      if (row >= N) break;
      const float* lr = logits + (int64_t)row * C;
      float f = 1.0f;
      if (dac) {   // distanse_aware_calibration.py:49-58: the factor of the raw argmax
        float b = -INFINITY;
        int bi = 0x7fffffff;
        for (int c = lane; c < C; c += 64)
          if (lr[c] > b) { b = lr[c]; bi = c; }
        wave_argmax(b, bi);
        f = dac[bi == 0x7fffffff ? 0 : bi];
      }
      float mx = -INFINITY;
      int i1 = 0x7fffffff;
      for (int c = lane; c < C; c += 64) {
        const float y = lr[c] * f;
        if (y > mx) { mx = y; i1 = c; }
      }
      wave_argmax(mx, i1);
      if (i1 == 0x7fffffff) i1 = 0;   // no finite maximum
      float se = 0.f, v2 = -INFINITY;
      int i2 = 0x7fffffff;
      for (int c = lane; c < C; c += 64) {
        if (c == i1) continue;
        const float y = lr[c] * f;
        se += __expf(y - mx);
        if (y > v2 || i2 == 0x7fffffff) { v2 = y; i2 = c; }   // ascending c: the first of equal values stays
      }
      wave_argmax(v2, i2);
      se = wave_sum(se);
      float share = 0.f;
      if (i2 != 0x7fffffff && v2 != -INFINITY) {   // else every other probability is exactly zero (C == 1, or all -inf)
        float s2 = 0.f;
        for (int c = lane; c < C; c += 64)
          if (c != i1) s2 += __expf(lr[c] * f - v2);
        share = 1.0f / wave_sum(s2);
      }
      if (lane == 0) {
        s_p1[r] = 1.0f / (1.0f + se);
        s_share[r] = share;
        s_f[r] = f;
        s_v2[r] = v2;
        s_i1[r] = i1;
        s_i2[r] = i2;
      }
    }
    __syncthreads();
  }

  // the two kernel sums: lane = query, wave w takes points w, w + 4, ... of every tile
  const int qi = q0 + lane;
  const bool valid = qi < N;
  const float cq = valid ? (ROWS ? s_p1[lane] : conf_in[qi]) : 0.f;
  const float pq = valid ? prox[qi] : 0.f;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double qc = (double)cq * m.scale[k][0];
    const double qp = (double)pq * m.scale[k][1];
    const double* __restrict__ pts = m.pts[k];
    const int n = m.n[k];
    double acc0 = 0.0, acc1 = 0.0;
    for (int base = 0; base < n; base += TILE) {
      const int cnt = n - base < TILE ? n - base : TILE;
      __syncthreads();
      for (int i = tid; i < cnt; i += 256) {
        const double2 v = *reinterpret_cast<const double2*>(pts + 2 * ((int64_t)base + i));
        tile[i][0] = v.x;
        tile[i][1] = v.y;
      }
      __syncthreads();
      auto term = [&](int j) {
        const double du = qc - tile[j][0], dv = qp - tile[j][1];
        return (double)__builtin_amdgcn_exp2f(-(float)fma(dv, dv, du * du));
      };
      int j = w;
      for (; j + NW < cnt; j += 2 * NW) {
        acc0 += term(j);
        acc1 += term(j + NW);
      }
      if (j < cnt) acc0 += term(j);
    }
    part[k][w][lane] = acc0 + acc1;
  }
  __syncthreads();
  // every wave forms c* of all 64 queries (the same arithmetic in each); wave 0 writes the per-row outputs
  const double T = m.norm[0] * (((part[0][0][lane] + part[0][1][lane]) + part[0][2][lane]) + part[0][3][lane]);
  const double F = m.norm[1] * (((part[1][0][lane] + part[1][1][lane]) + part[1][2][lane]) + part[1][3][lane]);
  const double den = T + F * m.ratio;
  const float cs = (float)(T / (den > 1e-10 ? den : 1e-10));   // density_ratio_calibration.py:103-105
  if (!ROWS) {
    if (w == 0 && valid) cstar_out[qi] = cs;
    return;
  }
  if (w == 0 && valid) {   // the evaluator's argmax of the calibrated row (vl_evaluator.py:68, 83)
    const int i1 = s_i1[lane], i2 = s_i2[lane];
    const float other = (1.0f - cs) * s_share[lane];
    float cf = cs;
    int pd = i1;
    if (other > cs || (other == cs && i2 < i1)) { cf = other; pd = i2; }
    conf_out[qi] = cf;
    pred_out[qi] = pd;
    if (cstar_out) cstar_out[qi] = cs;
  }
  if (!probs) return;
  for (int r = w; r < QB; r += NW) {   // the calibrated rows, a wave per row again
    const int row = q0 + r;
    if (row >= N) break;
    const float* lr = logits + (int64_t)row * C;
    float* pr = probs + (int64_t)row * C;
    const float c = __shfl(cs, r, 64), f = s_f[r], v2 = s_v2[r], share = s_share[r];
    const int i1 = s_i1[r];
    const float a = (1.0f - c) * share;   // the same product as `other` above: conf' == probs[pred']
    for (int j = lane; j < C; j += 64) {
      const float y = lr[j] * f;   // read before the write: probs may alias logits
      pr[j] = j == i1 ? c : (share == 0.f ? 0.f : __expf(y - v2) * a);
    }
  }
}

int check_model(const clipmi_procal_model* m, ProcalArgs& a) {
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "procal: null model");
  CLIPMI_REQUIRE(m->points_true && m->points_false, CLIPMI_ERR_ARG, "procal: null point set");
  CLIPMI_REQUIRE((uintptr_t)m->points_true % 16 == 0 && (uintptr_t)m->points_false % 16 == 0, CLIPMI_ERR_ARG,
                 "procal: point sets must be 16-byte aligned");
  CLIPMI_REQUIRE(m->n_true >= 2 && m->n_false >= 2, CLIPMI_ERR_SHAPE, "procal: n_true=%d n_false=%d (each >= 2)", m->n_true, m->n_false);
  for (int k = 0; k < 2; ++k) {
    for (int d = 0; d < 2; ++d)
      CLIPMI_REQUIRE(std::isfinite(m->scale[k][d]) && m->scale[k][d] > 0.0, CLIPMI_ERR_ARG, "procal: scale[%d][%d]=%g (finite, > 0)", k, d,
                     m->scale[k][d]);
    CLIPMI_REQUIRE(std::isfinite(m->norm[k]) && m->norm[k] > 0.0, CLIPMI_ERR_ARG, "procal: norm[%d]=%g (finite, > 0)", k, m->norm[k]);
  }
  CLIPMI_REQUIRE(std::isfinite(m->ratio) && m->ratio >= 0.0, CLIPMI_ERR_ARG, "procal: ratio=%g (finite, >= 0)", m->ratio);
  a.pts[0] = m->points_true;
  a.pts[1] = m->points_false;
  a.n[0] = m->n_true;
  a.n[1] = m->n_false;
  for (int k = 0; k < 2; ++k) {
    for (int d = 0; d < 2; ++d) a.scale[k][d] = m->scale[k][d];
    a.norm[k] = m->norm[k];
  }
  a.ratio = m->ratio;
  return CLIPMI_OK;
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

int clipmi_procal_kde(const clipmi_procal_model* model, const float* conf, const float* proximity, float* cstar, int n, clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(n > 0, CLIPMI_ERR_SHAPE, "procal_kde: n=%d", n);
  CLIPMI_REQUIRE(conf && proximity && cstar, CLIPMI_ERR_ARG, "procal_kde: null pointer (conf, proximity and cstar are required)");
  ProcalArgs a;
  if (int rc = check_model(model, a)) return rc;
  hipLaunchKernelGGL(procal_kernel<false>, dim3((n + QB - 1) / QB), dim3(256), 0, s, a, (const float*)nullptr, (const float*)nullptr, conf,
                     proximity, (float*)nullptr, (float*)nullptr, (int32_t*)nullptr, cstar, n, 0);
  return check_launch("procal_kernel<kde>");
}

int clipmi_procal_rows(const clipmi_procal_model* model, const float* logits, const float* dac_conf, const float* proximity, float* probs,
                       float* conf, int32_t* pred, float* cstar, int n, int C, clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(n > 0 && C > 0, CLIPMI_ERR_SHAPE, "procal_rows: n=%d C=%d", n, C);
  CLIPMI_REQUIRE(logits && proximity && conf && pred, CLIPMI_ERR_ARG,
                 "procal_rows: null pointer (logits, proximity, conf and pred are required)");
  ProcalArgs a;
  if (int rc = check_model(model, a)) return rc;
  hipLaunchKernelGGL(procal_kernel<true>, dim3((n + QB - 1) / QB), dim3(256), 0, s, a, logits, dac_conf, (const float*)nullptr, proximity,
                     probs, conf, pred, cstar, n, C);
  return check_launch("procal_kernel<rows>");
}

}  // extern "C"
