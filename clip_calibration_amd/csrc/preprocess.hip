// Image preprocessing on the device: the reference's test transform (clip/clip.py:74-81, Dassl's test transform) for a ragged batch of
// uint8 RGB images -- torchvision Resize(n_px) on the shorter side with Pillow's 8-bit resampler (libImaging/Resample.c:
// precompute_coeffs, normalize_coeffs_8bpc, ImagingResample{Horizontal,Vertical}_8bpc), CenterCrop(n_px), ToTensor + Normalize
// through a [3][256] lookup table -- written as [B,3,n_px,n_px] fp16 / fp32, the tensor encode_image takes.  Bit-exact by
// construction: the taps are computed in double in Pillow's operation order with FP contraction off, the passes are int32 with
// Pillow's rounding, and the table is built on the host with the reference's own fp32 ops.
//
// Two launches per call:
//   1. taps_kernel: one thread per (image, axis, output index inside the crop) -> (xmin, count) + count fixed-point taps.
//      Only the cropped outputs are computed: each output depends on its own taps only, so this equals resize-then-crop.
//   2. resample_kernel: one workgroup per 64 x 32 output tile (all three channels) of one image.  It runs the horizontal pass for the
//      input rows the tile's output rows read (at most RES_MAXR rows at a time) into an LDS intermediate of uint8 -- Pillow's
//      intermediate is uint8 too --, then the vertical pass of each thread's 3 x 8 outputs from LDS, accumulating int32 sums across row
//      chunks (integer sums: the order does not matter), and stores 8 outputs per channel with one 16-byte (fp16) / two 16-byte (fp32)
//      stores.  No intermediate image goes through HBM.
// Bytes moved per image: the input rows and columns the crop reads (uint8) + 3 n_px^2 * sizeof(out).
#include <algorithm>

#include "resample.h"   // filters, taps, clamp, tile shape, 8-wide store, image checks; turns FP contraction off for the tap arithmetic

namespace clipmi {
namespace {

struct Geometry {
  int new_h, new_w, top, left;
};

// torchvision Resize(int) (shorter side -> n_px, longer side int(n_px * long / short)) and CenterCrop (Python's round: half to even)
__host__ __device__ inline Geometry geometry(int H, int W, int n_px) {
  Geometry g;
  const int s = H < W ? H : W, l = H < W ? W : H;
  const int nl = (int)((double)((int64_t)n_px * l) / (double)s);
  g.new_h = H <= W ? n_px : nl;
  g.new_w = H <= W ? nl : n_px;
  const int dh = g.new_h - n_px, dw = g.new_w - n_px;   // >= 0
  g.top = (dh >> 1) + ((dh & 1) && ((dh >> 1) & 1));     // round(d / 2): k + 0.5 goes to the even one of k, k + 1
  g.left = (dw >> 1) + ((dw & 1) && ((dw >> 1) & 1));
  return g;
}

// bounds[((b * 2 + axis) * n_px + i) * 2 + {0, 1}] = (xmin, count), taps[((b * 2 + axis) * n_px + i) * kmax + t]; axis 0 = x, 1 = y
__global__ __launch_bounds__(256) void taps_kernel(const clipmi_image_desc* __restrict__ desc, int32_t* __restrict__ bounds,
                                                   int32_t* __restrict__ taps, int B, int n_px, int kmax, int filter) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (int64_t)B * 2 * n_px) return;
  const int i = (int)(id % n_px);
  const int axis = (int)((id / n_px) & 1);
  const int b = (int)(id / (2 * (int64_t)n_px));
  const int H = desc[b].height, W = desc[b].width;
  const Geometry g = geometry(H, W, n_px);
  const int in_size = axis == 0 ? W : H;
  const int out_size = axis == 0 ? g.new_w : g.new_h;
  const int xx = i + (axis == 0 ? g.left : g.top);
  pillow_taps(in_size, out_size, xx, filter, kmax, taps + id * kmax, bounds + id * 2);
}

// grid (tiles_x * tiles_y, B), 256 threads; thread t owns output row tile_y0 + (t >> 3), columns tile_x0 + 8 (t & 7) .. + 7, all channels
template <typename TO>
__global__ __launch_bounds__(256) void resample_kernel(const uint8_t* __restrict__ pixels, const clipmi_image_desc* __restrict__ desc,
                                                       const int32_t* __restrict__ bounds, const int32_t* __restrict__ taps,
                                                       const float* __restrict__ table, TO* __restrict__ out, int n_px, int kmax,
                                                       int tiles_x, int vec_ok) {
  __shared__ float lut[3 * 256];
  __shared__ __attribute__((aligned(16))) uint8_t tmp[RES_MAXR * 3 * RES_TX];
  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int x0 = (blockIdx.x % tiles_x) * RES_TX, y0 = (blockIdx.x / tiles_x) * RES_TY;
  for (int e = tid; e < 3 * 256; e += 256) lut[e] = table[e];

  const clipmi_image_desc d = desc[b];
  const uint8_t* img = pixels + d.offset;
  const int32_t* bx = bounds + (int64_t)(b * 2 + 0) * n_px * 2;
  const int32_t* by = bounds + (int64_t)(b * 2 + 1) * n_px * 2;
  const int32_t* kx = taps + (int64_t)(b * 2 + 0) * n_px * kmax;
  const int32_t* ky = taps + (int64_t)(b * 2 + 1) * n_px * kmax;

  const int y_last = min(y0 + RES_TY, n_px) - 1;
  const int ys0 = by[y0 * 2], ye0 = by[y_last * 2] + by[y_last * 2 + 1];
  const int ncols = min(RES_TX, n_px - x0);

  const int xg = tid & 7, r = y0 + (tid >> 3), x = x0 + xg * 8;
  const bool active = r < n_px && x < n_px;
  const int ry = active ? by[r * 2] : 0, rcnt = active ? by[r * 2 + 1] : 0;
  int32_t acc[3][8];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[c][j] = 1 << (PRECISION_BITS - 1);

  for (int ys = ys0; ys < ye0; ys += RES_MAXR) {
    const int nrows = min(RES_MAXR, ye0 - ys);
    // horizontal pass: tmp[row][c][col] for input rows ys .. ys + nrows - 1 and the tile's columns
    for (int e = tid; e < nrows * 3 * RES_TX; e += 256) {
      const int col = e & (RES_TX - 1), c = (e / RES_TX) % 3, row = e / (3 * RES_TX);
      if (col >= ncols) continue;
      const int xo = x0 + col;
      const int xmin = bx[xo * 2], cnt = bx[xo * 2 + 1];
      const int32_t* k = kx + (int64_t)xo * kmax;
      const uint8_t* src = img + (int64_t)(ys + row) * d.stride_y + (int64_t)c * d.stride_c + (int64_t)xmin * d.stride_x;
      int32_t s = 1 << (PRECISION_BITS - 1);
      for (int t = 0; t < cnt; ++t) s += (int32_t)src[(int64_t)t * d.stride_x] * k[t];
      tmp[e] = (uint8_t)clip8(s);
    }
    __syncthreads();
    // vertical pass over the rows of this chunk
    if (active) {
      const int t0 = max(0, ys - ry), t1 = min(rcnt, ys + nrows - ry);
      const int32_t* k = ky + (int64_t)r * kmax;
      for (int t = t0; t < t1; ++t) {
        const int32_t w = k[t];
        const int row = ry + t - ys;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const uint64_t v8 = *reinterpret_cast<const uint64_t*>(&tmp[(row * 3 + c) * RES_TX + xg * 8]);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[c][j] += (int32_t)((v8 >> (8 * j)) & 0xff) * w;
        }
      }
    }
    __syncthreads();
  }
  if (!active) return;
  const int valid = min(8, n_px - x);
  const bool vec = vec_ok && valid == 8;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = lut[c * 256 + clip8(acc[c][j])];
    store8(out + (((int64_t)b * 3 + c) * n_px + r) * n_px + x, v, vec, valid);
  }
}

struct Plan {
  int kmax;
  size_t desc_bytes, bounds_bytes, taps_bytes;
  size_t total() const { return desc_bytes + bounds_bytes + taps_bytes; }
};

// every field of every descriptor, on the host, before anything reaches a device
int plan_preprocess(const clipmi_image_desc* images, int B, int n_px, int filter, int64_t pixels_bytes, bool check_extent, Plan* p) {
  if (const int rc = check_images("preprocess", images, B, n_px, filter, pixels_bytes, check_extent); rc != CLIPMI_OK) return rc;
  int kmax = 1;
  for (int b = 0; b < B; ++b) {
    const clipmi_image_desc& d = images[b];
    const Geometry g = geometry(d.height, d.width, n_px);
    kmax = std::max(kmax, std::max(ksize_of(d.width, g.new_w, filter), ksize_of(d.height, g.new_h, filter)));
  }
  p->kmax = kmax;
  p->desc_bytes = align256(sizeof(clipmi_image_desc) * (size_t)B);
  p->bounds_bytes = align256(sizeof(int32_t) * 2 * 2 * (size_t)B * n_px);
  p->taps_bytes = align256(sizeof(int32_t) * 2 * (size_t)B * n_px * (size_t)kmax);
  return CLIPMI_OK;
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

size_t clipmi_preprocess_workspace_bytes(const clipmi_image_desc* images, int B, int n_px, int filter) {
  Plan p;
  return plan_preprocess(images, B, n_px, filter, 0, false, &p) == CLIPMI_OK ? p.total() : 0;
}

int clipmi_preprocess(const void* pixels, int64_t pixels_bytes, const clipmi_image_desc* images, int B, int n_px, int filter,
                      const float* table, void* out, int out_dtype, void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  CLIPMI_REQUIRE(pixels && table && out && workspace, CLIPMI_ERR_ARG, "preprocess: null pointer");
  CLIPMI_REQUIRE(out_dtype == CLIPMI_F16 || out_dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "preprocess: bad out dtype %d", out_dtype);
  CLIPMI_REQUIRE(pixels_bytes >= 1, CLIPMI_ERR_ARG, "preprocess: empty pixel buffer");
  Plan p;
  if (const int rc = plan_preprocess(images, B, n_px, filter, pixels_bytes, true, &p); rc != CLIPMI_OK) return rc;
  CLIPMI_REQUIRE(workspace_bytes >= p.total(), CLIPMI_ERR_WORKSPACE, "preprocess: workspace %zu < %zu bytes", workspace_bytes, p.total());
  CLIPMI_REQUIRE(((uintptr_t)workspace & 255) == 0, CLIPMI_ERR_ARG, "preprocess: workspace must be 256-byte aligned");

  char* ws = (char*)workspace;
  clipmi_image_desc* d_desc = (clipmi_image_desc*)ws;
  int32_t* d_bounds = (int32_t*)(ws + p.desc_bytes);
  int32_t* d_taps = (int32_t*)(ws + p.desc_bytes + p.bounds_bytes);
  if (hipMemcpyAsync(d_desc, images, sizeof(clipmi_image_desc) * (size_t)B, hipMemcpyHostToDevice, s) != hipSuccess) {
    set_error("preprocess: descriptor upload failed: %s", hipGetErrorString(hipGetLastError()));
    return CLIPMI_ERR_HIP;
  }
  const int64_t n_taps = (int64_t)B * 2 * n_px;
  hipLaunchKernelGGL(taps_kernel, dim3((unsigned)((n_taps + 255) / 256)), dim3(256), 0, s, d_desc, d_bounds, d_taps, B, n_px, p.kmax,
                     filter);
  if (const int rc = check_launch("preprocess taps_kernel"); rc != CLIPMI_OK) return rc;
  const int tiles_x = (n_px + RES_TX - 1) / RES_TX, tiles_y = (n_px + RES_TY - 1) / RES_TY;
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)B);
  const int vec_ok = (n_px % 8 == 0) && (((uintptr_t)out & 15) == 0);
  if (out_dtype == CLIPMI_F16)
    hipLaunchKernelGGL(resample_kernel<half_t>, grid, dim3(256), 0, s, (const uint8_t*)pixels, d_desc, d_bounds, d_taps, table,
                       (half_t*)out, n_px, p.kmax, tiles_x, vec_ok);
  else
    hipLaunchKernelGGL(resample_kernel<float>, grid, dim3(256), 0, s, (const uint8_t*)pixels, d_desc, d_bounds, d_taps, table,
                       (float*)out, n_px, p.kmax, tiles_x, vec_ok);
  return check_launch("preprocess resample_kernel");
}

}  // extern "C"
