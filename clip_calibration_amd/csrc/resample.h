// What the two resampling translation units share (preprocess.hip: the test transform; augment.hip: the train transform): Pillow's
// filters, kernel size and tap computation (libImaging/Resample.c), its 8-bit clamp, the tile shape of the resample kernels, their
// 8-wide store, and the host checks of the image descriptors.
#pragma once
#include "common.h"

#pragma clang fp contract(off)   // Pillow's x86 build does not fuse: neither may the tap arithmetic of either unit

namespace clipmi {
namespace {

constexpr int RES_TX = 64;      // output columns per workgroup tile
constexpr int RES_TY = 32;      // output rows per workgroup tile
constexpr int RES_MAXR = 128;   // input rows of the horizontally resampled intermediate held in LDS at a time
constexpr int PRECISION_BITS = 22;
constexpr int MAX_SIDE = 32768;

__host__ __device__ inline double filter_support(int filter) { return filter == CLIPMI_FILTER_BICUBIC ? 2.0 : 1.0; }

__host__ __device__ inline int ksize_of(int in, int out, int filter) {
  double filterscale = (double)(float)in / out;
  if (filterscale < 1.0) filterscale = 1.0;
  return (int)ceil(filter_support(filter) * filterscale) * 2 + 1;
}

__device__ inline double filter_eval(int filter, double x) {
  if (x < 0.0) x = -x;
  if (filter == CLIPMI_FILTER_BICUBIC) {
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
  }
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}

// precompute_coeffs + normalize_coeffs_8bpc (Resample.c), in their own order, for output index xx of an axis resampled from in_size to
// out_size: the fixed-point taps go to k[0 .. count), (xmin, count) to bound[0 .. 1]
__device__ inline void pillow_taps(int in_size, int out_size, int xx, int filter, int kmax, int32_t* __restrict__ k, int32_t* __restrict__ bound) {
  const double scale = (double)(float)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = filter_support(filter) * filterscale;
  const double center = (xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (xmax > kmax) xmax = kmax;   // never, by ksize_of; keeps every write inside the row
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += filter_eval(filter, (x + xmin - center + 0.5) * ss);
  for (int x = 0; x < xmax; ++x) {
    double w = filter_eval(filter, (x + xmin - center + 0.5) * ss);
    if (ww != 0.0) w /= ww;
    k[x] = w < 0 ? (int32_t)(-0.5 + w * (1 << PRECISION_BITS)) : (int32_t)(0.5 + w * (1 << PRECISION_BITS));
  }
  bound[0] = xmin;
  bound[1] = xmax;
}

__device__ inline int clip8(int32_t acc) {
  const int v = acc >> PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

template <typename TO>
__device__ inline void store8(TO* dst, const float (&v)[8], bool vec, int valid) {
  if constexpr (sizeof(TO) == 2) {
    if (vec) {
      *reinterpret_cast<f16x8*>(dst) = f16x8{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3],
                                              (half_t)v[4], (half_t)v[5], (half_t)v[6], (half_t)v[7]};
      return;
    }
    for (int j = 0; j < valid; ++j) dst[j] = (half_t)v[j];
  } else {
    if (vec) {
      *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
      return;
    }
    for (int j = 0; j < valid; ++j) dst[j] = v[j];
  }
}

// B, n_px, the filter and every field of every image descriptor, on the host, before anything reaches a device
inline int check_images(const char* who, const clipmi_image_desc* images, int B, int n_px, int filter, int64_t pixels_bytes, bool check_extent) {
  CLIPMI_REQUIRE(images, CLIPMI_ERR_ARG, "%s: null image descriptors", who);
  CLIPMI_REQUIRE(B >= 1 && B <= 65535, CLIPMI_ERR_SHAPE, "%s: B = %d outside 1 .. 65535", who, B);
  CLIPMI_REQUIRE(n_px >= 1 && n_px <= 4096, CLIPMI_ERR_SHAPE, "%s: n_px = %d outside 1 .. 4096", who, n_px);
  CLIPMI_REQUIRE(filter == CLIPMI_FILTER_BILINEAR || filter == CLIPMI_FILTER_BICUBIC, CLIPMI_ERR_ARG,
                 "%s: unknown filter %d (CLIPMI_FILTER_BILINEAR or CLIPMI_FILTER_BICUBIC)", who, filter);
  for (int b = 0; b < B; ++b) {
    const clipmi_image_desc& d = images[b];
    CLIPMI_REQUIRE(d.height >= 1 && d.width >= 1 && d.height <= MAX_SIDE && d.width <= MAX_SIDE, CLIPMI_ERR_SHAPE,
                   "%s: image %d is %d x %d (each side 1 .. %d)", who, b, d.height, d.width, MAX_SIDE);
    const int64_t lim = (int64_t)1 << 40;
    CLIPMI_REQUIRE(d.offset >= 0 && d.offset < lim && d.stride_y > -lim && d.stride_y < lim && d.stride_x > -lim && d.stride_x < lim &&
                   d.stride_c > -lim && d.stride_c < lim, CLIPMI_ERR_ARG, "%s: image %d: offset or stride out of range", who, b);
    if (check_extent) {
      int64_t lo = d.offset, hi = d.offset;   // lowest and highest byte any (y, x, c) addresses
      const int64_t span[3] = {(int64_t)(d.height - 1) * d.stride_y, (int64_t)(d.width - 1) * d.stride_x, 2 * d.stride_c};
      for (int i = 0; i < 3; ++i) (span[i] < 0 ? lo : hi) += span[i];
      CLIPMI_REQUIRE(lo >= 0 && hi < pixels_bytes, CLIPMI_ERR_ARG,
                     "%s: image %d addresses bytes %lld .. %lld outside the %lld-byte pixel buffer", who, b, (long long)lo, (long long)hi,
                     (long long)pixels_bytes);
    }
  }
  return CLIPMI_OK;
}

}  // namespace
}  // namespace clipmi
