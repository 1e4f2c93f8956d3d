// The reference's TRAIN transform on the device (every training config: INPUT.TRANSFORMS ["random_resized_crop", "random_flip",
// "normalize"], SIZE (224, 224), INTERPOLATION "bicubic") for V views of a ragged batch of B uint8 RGB images: torchvision's PIL path
//   img.crop(box).resize((n_px, n_px), filter) [.transpose(FLIP_LEFT_RIGHT)] -> ToTensor -> Normalize
// written as [V, 3, n_px, n_px] fp16 / fp32.  The random draws stay on the host (clip_calibration_amd/augment.py sample_views): a view
// arrives as (image index, box, flip flag).  The geometry is a STRETCH of the box: on each axis Pillow's precompute_coeffs and
// normalize_coeffs_8bpc run with in_size = the box's side and out_size = n_px, so no tap reaches past the box edge and nothing outside
// the box is read -- Pillow crops first.  A pass whose in and out sizes are equal is skipped as Pillow skips it: its outputs get ONE
// tap of weight 1.0 at their own pixel, which returns the byte itself ((2^21 + p 2^22) >> 22 = p).  Bit-exact by construction, as
// preprocess.hip is: taps in double in Pillow's order with FP contraction off, int32 passes with Pillow's rounding, horizontal first
// with a uint8 intermediate, table built on the host.
//
// Two launches per call, the shape of preprocess.hip:
//   1. view_taps_kernel: one thread per (view, axis, output index) -> (xmin, count) + count fixed-point taps, relative to the box.
//   2. view_resample_kernel: one workgroup per 64 x 32 output tile (all three channels) of one view: horizontal pass of the box rows
//      the tile reads into an LDS uint8 intermediate, at most RES_MAXR rows at a time, then the vertical pass of each thread's 3 x 8
//      outputs with int32 sums carried across the row chunks.  The flip is done in the STORE: the 8 outputs of columns x .. x + 7 go,
//      reversed, to columns n_px - 8 - x .. n_px - 1 - x, still one 16-byte (fp16) / two 16-byte (fp32) stores when n_px % 8 == 0.
//      No intermediate image goes through HBM.
#include <algorithm>

#include "resample.h"   // filters, taps, clamp, tile shape, 8-wide store, image checks; turns FP contraction off for the tap arithmetic

namespace clipmi {
namespace {

// bounds[((v * 2 + axis) * n_px + i) * 2 + {0, 1}] = (xmin, count), taps[((v * 2 + axis) * n_px + i) * kmax + t]; axis 0 = x, 1 = y;
// xmin counts from the box's left / top edge
__global__ __launch_bounds__(256) void view_taps_kernel(const clipmi_view_desc* __restrict__ views, int32_t* __restrict__ bounds,
                                                        int32_t* __restrict__ taps, int V, int n_px, int kmax, int filter) {
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (int64_t)V * 2 * n_px) return;
  const int xx = (int)(id % n_px);
  const int axis = (int)((id / n_px) & 1);
  const int v = (int)(id / (2 * (int64_t)n_px));
  const int in_size = axis == 0 ? views[v].width : views[v].height;
  int32_t* k = taps + id * kmax;
  if (in_size == n_px) {   // Pillow skips this pass
    k[0] = 1 << PRECISION_BITS;
    bounds[id * 2] = xx;
    bounds[id * 2 + 1] = 1;
    return;
  }
  pillow_taps(in_size, n_px, xx, filter, kmax, k, bounds + id * 2);
}

// grid (tiles_x * tiles_y, V), 256 threads; thread t owns output row tile_y0 + (t >> 3), unflipped columns tile_x0 + 8 (t & 7) .. + 7, all
// channels.  Every (xmin, count) was computed from a validated box, so xmin + count <= the box's side: no read leaves the box.
template <typename TO>
__global__ __launch_bounds__(256) void view_resample_kernel(const uint8_t* __restrict__ pixels, const clipmi_image_desc* __restrict__ desc,
                                                            const clipmi_view_desc* __restrict__ views, const int32_t* __restrict__ bounds,
                                                            const int32_t* __restrict__ taps, const float* __restrict__ table,
                                                            TO* __restrict__ out, int n_px, int kmax, int tiles_x, int vec_ok) {
  __shared__ float lut[3 * 256];
  __shared__ __attribute__((aligned(16))) uint8_t tmp[RES_MAXR * 3 * RES_TX];
  const int tid = threadIdx.x;
  const int v = blockIdx.y;
  const int x0 = (blockIdx.x % tiles_x) * RES_TX, y0 = (blockIdx.x / tiles_x) * RES_TY;
  for (int e = tid; e < 3 * 256; e += 256) lut[e] = table[e];

  const clipmi_view_desc vw = views[v];
  const clipmi_image_desc d = desc[vw.image];
  const uint8_t* box = pixels + d.offset + (int64_t)vw.top * d.stride_y + (int64_t)vw.left * d.stride_x;
  const int32_t* bx = bounds + (int64_t)(v * 2 + 0) * n_px * 2;
  const int32_t* by = bounds + (int64_t)(v * 2 + 1) * n_px * 2;
  const int32_t* kx = taps + (int64_t)(v * 2 + 0) * n_px * kmax;
  const int32_t* ky = taps + (int64_t)(v * 2 + 1) * n_px * kmax;

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
    // horizontal pass: tmp[row][c][col] for box rows ys .. ys + nrows - 1 and the tile's columns
    for (int e = tid; e < nrows * 3 * RES_TX; e += 256) {
      const int col = e & (RES_TX - 1), c = (e / RES_TX) % 3, row = e / (3 * RES_TX);
      if (col >= ncols) continue;
      const int xo = x0 + col;
      const int xmin = bx[xo * 2], cnt = bx[xo * 2 + 1];
      const int32_t* k = kx + (int64_t)xo * kmax;
      const uint8_t* src = box + (int64_t)(ys + row) * d.stride_y + (int64_t)c * d.stride_c + (int64_t)xmin * d.stride_x;
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
  const bool flip = vw.flip != 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    TO* dst = out + (((int64_t)v * 3 + c) * n_px + r) * n_px;
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = lut[c * 256 + clip8(acc[c][j])];
    if (!flip) {
      store8(dst + x, o, vec, valid);
    } else if (vec) {   // output column n_px - 1 - (x + j) holds o[j]
      const float m[8] = {o[7], o[6], o[5], o[4], o[3], o[2], o[1], o[0]};
      store8(dst + (n_px - 8 - x), m, true, 8);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < valid) dst[n_px - 1 - x - j] = (TO)o[j];
    }
  }
}

struct Plan {
  int kmax;
  size_t desc_bytes, view_bytes, bounds_bytes, taps_bytes;
  size_t total() const { return desc_bytes + view_bytes + bounds_bytes + taps_bytes; }
};

// every field of every image (check_images) and view descriptor, on the host, before anything reaches a device
int plan_augment(const clipmi_image_desc* images, int B, const clipmi_view_desc* views, int V, int n_px, int filter, int64_t pixels_bytes,
                 bool check_extent, Plan* p) {
  if (const int rc = check_images("augment", images, B, n_px, filter, pixels_bytes, check_extent); rc != CLIPMI_OK) return rc;
  CLIPMI_REQUIRE(views, CLIPMI_ERR_ARG, "augment: null view descriptors");
  CLIPMI_REQUIRE(V >= 1 && V <= 65535, CLIPMI_ERR_SHAPE, "augment: V = %d outside 1 .. 65535 (one grid row per view)", V);
  int kmax = 1;
  for (int v = 0; v < V; ++v) {
    const clipmi_view_desc& w = views[v];
    CLIPMI_REQUIRE(w.image >= 0 && w.image < B, CLIPMI_ERR_ARG, "augment: view %d names image %d outside [0, %d)", v, w.image, B);
    const clipmi_image_desc& d = images[w.image];
    CLIPMI_REQUIRE(w.height >= 1 && w.width >= 1, CLIPMI_ERR_SHAPE, "augment: view %d has a %d x %d box (each side >= 1)", v, w.height,
                   w.width);
    // sides are >= 1 and the image's are <= MAX_SIDE: the sums below cannot overflow once top and left are in range
    CLIPMI_REQUIRE(w.top >= 0 && w.left >= 0 && w.top <= d.height - w.height && w.left <= d.width - w.width, CLIPMI_ERR_ARG,
                   "augment: view %d: box (top %d, left %d, %d x %d) outside its %d x %d image %d", v, w.top, w.left, w.height, w.width,
                   d.height, d.width, w.image);
    if (w.width != n_px) kmax = std::max(kmax, ksize_of(w.width, n_px, filter));
    if (w.height != n_px) kmax = std::max(kmax, ksize_of(w.height, n_px, filter));
  }
  p->kmax = kmax;
  p->desc_bytes = align256(sizeof(clipmi_image_desc) * (size_t)B);
  p->view_bytes = align256(sizeof(clipmi_view_desc) * (size_t)V);
  p->bounds_bytes = align256(sizeof(int32_t) * 2 * 2 * (size_t)V * n_px);
  p->taps_bytes = align256(sizeof(int32_t) * 2 * (size_t)V * n_px * (size_t)kmax);
  return CLIPMI_OK;
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

size_t clipmi_augment_workspace_bytes(const clipmi_image_desc* images, int B, const clipmi_view_desc* views, int V, int n_px, int filter) {
  Plan p;
  return plan_augment(images, B, views, V, n_px, filter, 0, false, &p) == CLIPMI_OK ? p.total() : 0;
}

int clipmi_augment(const void* pixels, int64_t pixels_bytes, const clipmi_image_desc* images, int B, const clipmi_view_desc* views, int V,
                   int n_px, int filter, const float* table, void* out, int out_dtype, void* workspace, size_t workspace_bytes,
                   clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  CLIPMI_REQUIRE(pixels && table && out && workspace, CLIPMI_ERR_ARG, "augment: null pointer");
  CLIPMI_REQUIRE(out_dtype == CLIPMI_F16 || out_dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "augment: bad out dtype %d", out_dtype);
  CLIPMI_REQUIRE(pixels_bytes >= 1, CLIPMI_ERR_ARG, "augment: empty pixel buffer");
  Plan p;
  if (const int rc = plan_augment(images, B, views, V, n_px, filter, pixels_bytes, true, &p); rc != CLIPMI_OK) return rc;
  CLIPMI_REQUIRE(workspace_bytes >= p.total(), CLIPMI_ERR_WORKSPACE, "augment: workspace %zu < %zu bytes", workspace_bytes, p.total());
  CLIPMI_REQUIRE(((uintptr_t)workspace & 255) == 0, CLIPMI_ERR_ARG, "augment: workspace must be 256-byte aligned");

  char* ws = (char*)workspace;
  clipmi_image_desc* d_desc = (clipmi_image_desc*)ws;
  clipmi_view_desc* d_views = (clipmi_view_desc*)(ws + p.desc_bytes);
  int32_t* d_bounds = (int32_t*)(ws + p.desc_bytes + p.view_bytes);
  int32_t* d_taps = (int32_t*)(ws + p.desc_bytes + p.view_bytes + p.bounds_bytes);
  if (hipMemcpyAsync(d_desc, images, sizeof(clipmi_image_desc) * (size_t)B, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(d_views, views, sizeof(clipmi_view_desc) * (size_t)V, hipMemcpyHostToDevice, s) != hipSuccess) {
    set_error("augment: descriptor upload failed: %s", hipGetErrorString(hipGetLastError()));
    return CLIPMI_ERR_HIP;
  }
  const int64_t n_taps = (int64_t)V * 2 * n_px;
  hipLaunchKernelGGL(view_taps_kernel, dim3((unsigned)((n_taps + 255) / 256)), dim3(256), 0, s, d_views, d_bounds, d_taps, V, n_px, p.kmax,
                     filter);
  if (const int rc = check_launch("augment view_taps_kernel"); rc != CLIPMI_OK) return rc;
  const int tiles_x = (n_px + RES_TX - 1) / RES_TX, tiles_y = (n_px + RES_TY - 1) / RES_TY;
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)V);
  const int vec_ok = (n_px % 8 == 0) && (((uintptr_t)out & 15) == 0);
  if (out_dtype == CLIPMI_F16)
    hipLaunchKernelGGL(view_resample_kernel<half_t>, grid, dim3(256), 0, s, (const uint8_t*)pixels, d_desc, d_views, d_bounds, d_taps, table,
                       (half_t*)out, n_px, p.kmax, tiles_x, vec_ok);
  else
    hipLaunchKernelGGL(view_resample_kernel<float>, grid, dim3(256), 0, s, (const uint8_t*)pixels, d_desc, d_views, d_bounds, d_taps, table,
                       (float*)out, n_px, p.kmax, tiles_x, vec_ok);
  return check_launch("augment view_resample_kernel");
}

}  // extern "C"
