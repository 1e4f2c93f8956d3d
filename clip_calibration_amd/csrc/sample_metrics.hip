// The evaluator's sample-level metrics on the device (reference evaluators/vl_evaluator.py:77-82 macro-F1, tools/metrics.py:132-178 PIECE,
// :212-236 AdaptiveECE): what is left of them for the host is arithmetic on a few dozen numbers (clip_calibration_amd/metrics.py).
//
//   order_hist_kernel / order_resolve_kernel   exact order statistics by a most-significant-digit radix select.  A float's bits u map to
//       key = u ^ 0x80000000 (u >= 0) or ~u (sign set): unsigned order of the keys = numeric order of the floats, -0.0 right below +0.0;
//       every NaN maps to 0xffffffff and so sorts last, as in numpy.  Pass p (0..3) looks at digit (key >> (24 - 8 p)) & 255 of the
//       elements whose higher bits equal a target's prefix.  The targets' ranks ascend, so their prefixes ascend too and the DISTINCT
//       prefixes ("groups", at most k) are runs: an element finds its group by binary search, and one histogram per group is kept, not one
//       per target.  The histogram launch counts in LDS and adds its non-zero counters to the pass's global histogram with integer
//       atomics; the resolve launch (one workgroup, one wave per target at a time) scans a target's 256 counters for the digit where
//       the running count passes the residual rank, appends it to the prefix, reduces the rank, and regroups.  After pass 3 the prefix
//       IS the key.  Counts are integers: the result does not depend on the order of the atomics.
//   group_gap_kernel     (count, sum conf, sum correct) per (key bin, confidence bin) from edge lists held as float64 -- LDS partials,
//       then float64 global atomics, as ece_accumulate_kernel (logits.hip).
//   class_counts_kernel  true positives / predicted / labelled per class, integer atomics.
#include "common.h"

namespace clipmi {
namespace {

constexpr int MAXK = CLIPMI_ORDER_STATS_MAX_RANKS;
constexpr int MAXG = CLIPMI_GROUP_GAP_MAX_GROUPS;
constexpr int RADIX = 256;
constexpr int HIST_LDS_EXTRA = MAXK * (int)sizeof(uint32_t);   // the group prefixes behind the counters

struct SelectState {
  uint32_t prefix[MAXK];    // per target: the digits fixed so far, as a number of 8 * pass bits
  uint32_t rem[MAXK];       // per target: its rank among the elements that share the prefix
  uint32_t gprefix[MAXK];   // per group: the prefix, ascending
  int32_t group[MAXK];      // per target: its group
  int32_t n_groups;
  int32_t nan;
};
struct Ranks {
  int32_t r[MAXK];
};

__device__ __forceinline__ uint32_t float_key(float v) {
  if (v != v) return 0xffffffffu;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t key) {   // 0xffffffff -> 0x7fffffff, a NaN
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// hist: this pass's uint32 [k][256], zero on entry.  Dynamic LDS: k * 256 counters + MAXK prefixes.
__global__ __launch_bounds__(256) void order_hist_kernel(const float* __restrict__ x, int n, int pass, int k, SelectState* __restrict__ st,
                                                         uint32_t* __restrict__ hist) {
  extern __shared__ uint32_t sh[];
  uint32_t* sprefix = sh + k * RADIX;
  int ng = pass == 0 ? 1 : st->n_groups;
  ng = ng < 1 ? 1 : (ng > k ? k : ng);   // the LDS holds k groups, whatever the state says
  for (int i = threadIdx.x; i < ng * RADIX; i += 256) sh[i] = 0u;
  if ((int)threadIdx.x < ng) sprefix[threadIdx.x] = pass == 0 ? 0u : st->gprefix[threadIdx.x];
  __syncthreads();
  const int shift = 24 - 8 * pass;
  int nans = 0;   // wave-uniform
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    const bool live = i < n;
    const float v = live ? x[i] : 0.f;
    if (pass == 0) nans += __popcll(__ballot(live && v != v));   // every lane of the wave is here: the loop bound is per workgroup
    const uint32_t key = float_key(v);
    int g = live ? 0 : -1;
    if (live && pass > 0) {
      const uint32_t hi = key >> (shift + 8);
      int lo = 0, up = ng;   // first group whose prefix is >= hi
      while (lo < up) {
        const int mid = (lo + up) >> 1;
        if (sprefix[mid] < hi) lo = mid + 1; else up = mid;
      }
      g = (lo < ng && sprefix[lo] == hi) ? lo : -1;
    }
    if (g >= 0) atomicAdd(&sh[g * RADIX + ((key >> shift) & 255u)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ng * RADIX; i += 256)
    if (sh[i]) atomicAdd(&hist[i], sh[i]);
  if (pass == 0 && nans && (threadIdx.x & 63) == 0) atomicAdd(&st->nan, nans);
}

// One workgroup of 16 waves.  Wave w takes targets w, w + 16, ...: lane l holds counters 4 l .. 4 l + 3 of the target's group, a
// wave-wide inclusive scan of the lane sums finds the lane, and that lane the counter, where the running count passes the rank.
__global__ __launch_bounds__(1024) void order_resolve_kernel(int pass, int k, Ranks ranks, SelectState* __restrict__ st,
                                                             const uint32_t* __restrict__ hist, float* __restrict__ out,
                                                             int32_t* __restrict__ nan_count) {
  __shared__ uint32_t sprefix[MAXK], srem[MAXK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < k; j += 16) {
    int g = pass == 0 ? 0 : st->group[j];
    g = g < 0 ? 0 : (g >= k ? k - 1 : g);
    const uint32_t rem = pass == 0 ? (uint32_t)ranks.r[j] : st->rem[j];
    const uint32_t old = pass == 0 ? 0u : st->prefix[j];
    const uint4 c = reinterpret_cast<const uint4*>(hist + (size_t)g * RADIX)[lane];
    const uint32_t own = c.x + c.y + c.z + c.w;
    uint32_t incl = own;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    const uint32_t excl = incl - own;
    const bool hit = excl <= rem && rem < incl;
    if (hit) {
      uint32_t r = rem - excl, digit = 4u * lane;
      if (r >= c.x) { r -= c.x; ++digit;
        if (r >= c.y) { r -= c.y; ++digit;
          if (r >= c.z) { r -= c.z; ++digit; } } }
      sprefix[j] = (old << 8) | digit;
      srem[j] = r;
    }
    if (__ballot(hit) == 0ull && lane == 0) {   // a rank beyond the group's count: the input changed between the passes
      sprefix[j] = (old << 8) | 255u;
      srem[j] = 0u;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < k) {
    const int j = threadIdx.x;
    st->prefix[j] = sprefix[j];
    st->rem[j] = srem[j];
    if (pass == 3) out[j] = key_float(sprefix[j]);
  }
  if (threadIdx.x == 0) {
    int g = 0;
    for (int j = 0; j < k; ++j) {
      if (j > 0 && sprefix[j] != sprefix[j - 1]) ++g;
      st->group[j] = g;
      st->gprefix[g] = sprefix[j];
    }
    st->n_groups = g + 1;
    if (pass == 3) *nan_count = st->nan;
  }
}

// np.searchsorted(edges, v, side="right") for ascending float64 edges in LDS: the number of edges <= v; a NaN sorts behind them all
__device__ __forceinline__ int edges_below(const double* edges, int n, double v) {
  if (v != v) return n;
  int lo = 0, up = n;
  while (lo < up) {
    const int mid = (lo + up) >> 1;
    if (edges[mid] <= v) lo = mid + 1; else up = mid;
  }
  return lo;
}

// Dynamic LDS: 3 * G partial sums, then the nk key edges and the nc confidence edges
__global__ __launch_bounds__(256) void group_gap_kernel(const float* __restrict__ conf, const int32_t* __restrict__ pred,
                                                        const int64_t* __restrict__ labels, const float* __restrict__ key,
                                                        const double* __restrict__ key_edges, int nk, const double* __restrict__ conf_edges,
                                                        int nc, double* __restrict__ groups, int n) {
  extern __shared__ double shd[];
  const int G = (nk + 1) * (nc + 1);
  double* sk = shd + 3 * G;
  double* sc = sk + nk;
  for (int i = threadIdx.x; i < 3 * G; i += 256) shd[i] = 0.0;
  for (int i = threadIdx.x; i < nk; i += 256) sk[i] = key_edges[i];
  for (int i = threadIdx.x; i < nc; i += 256) sc[i] = conf_edges[i];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double c = (double)conf[i];
    const int kb = nk > 0 ? edges_below(sk, nk, (double)key[i]) : 0;
    const int g = kb * (nc + 1) + edges_below(sc, nc, c);
    atomicAdd(&shd[g], 1.0);
    atomicAdd(&shd[G + g], c);
    atomicAdd(&shd[2 * G + g], (labels[i] == (int64_t)pred[i]) ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * G; i += 256)
    if (shd[i] != 0.0) atomicAdd(&groups[i], shd[i]);
}

constexpr int CLASS_LDS_COUNTERS = 8192;   // 32 KB of uint32 partials: 3 C + 1 counters fit up to C = 2730

// LDS: dynamic LDS of 3 C + 1 uint32 partials (a workgroup sees fewer than 2^32 samples), flushed with 64-bit atomics; otherwise
// every sample goes to the global counters directly.
template <bool LDS>
__global__ __launch_bounds__(256) void class_counts_kernel(const int32_t* __restrict__ pred, const int64_t* __restrict__ labels, int n, int C,
                                                           unsigned long long* __restrict__ counts) {
  extern __shared__ uint32_t shc[];
  const int total = 3 * C + 1;
  if (LDS) {
    for (int i = threadIdx.x; i < total; i += 256) shc[i] = 0u;
    __syncthreads();
  }
  int outside = 0;   // wave-uniform
  for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    const bool live = i < n;
    const int64_t p = live ? (int64_t)pred[i] : 0, y = live ? labels[i] : 0;
    const bool ok = p >= 0 && p < C && y >= 0 && y < C;
    outside += __popcll(__ballot(live && !ok));   // every lane of the wave is here: the loop bound is per workgroup
    if (live && ok) {
      if (LDS) {
        atomicAdd(&shc[C + p], 1u);
        atomicAdd(&shc[2 * C + y], 1u);
        if (p == y) atomicAdd(&shc[p], 1u);
      } else {
        atomicAdd(&counts[C + p], 1ull);
        atomicAdd(&counts[2 * C + y], 1ull);
        if (p == y) atomicAdd(&counts[p], 1ull);
      }
    }
  }
  if (outside && (threadIdx.x & 63) == 0) atomicAdd(&counts[3 * (int64_t)C], (unsigned long long)outside);
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < total - 1; i += 256)
      if (shc[i]) atomicAdd(&counts[i], (unsigned long long)shc[i]);
  }
}

int grid_for(int n, int per_thread, int cap) {
  const int64_t blocks = ((int64_t)n + 256 * per_thread - 1) / (256 * per_thread);
  return (int)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

size_t select_state_bytes() { return align256(sizeof(SelectState)); }

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

size_t clipmi_order_stats_workspace_bytes(int n, int k) {
  if (n < 1 || k < 1 || k > MAXK) return 0;
  return select_state_bytes() + align256((size_t)4 * k * RADIX * sizeof(uint32_t));
}

int clipmi_order_stats(const float* x, int n, const int32_t* ranks, int k, float* out, int32_t* nan_count, void* workspace,
                       size_t workspace_bytes, clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  CLIPMI_REQUIRE(n >= 1, CLIPMI_ERR_SHAPE, "order_stats: n=%d (>= 1)", n);
  CLIPMI_REQUIRE(k >= 1 && k <= MAXK, CLIPMI_ERR_SHAPE, "order_stats: k=%d (1 .. %d)", k, MAXK);
  CLIPMI_REQUIRE(x && ranks && out && nan_count, CLIPMI_ERR_ARG, "order_stats: null pointer (x, ranks, out and nan_count are required)");
  Ranks r{};
  for (int j = 0; j < k; ++j) {
    CLIPMI_REQUIRE(ranks[j] >= 0 && ranks[j] < n, CLIPMI_ERR_ARG, "order_stats: ranks[%d]=%d outside [0, %d)", j, ranks[j], n);
    CLIPMI_REQUIRE(j == 0 || ranks[j] >= ranks[j - 1], CLIPMI_ERR_ARG, "order_stats: ranks[%d]=%d below ranks[%d]=%d (ascending)", j,
                   ranks[j], j - 1, ranks[j - 1]);
    r.r[j] = ranks[j];
  }
  CLIPMI_REQUIRE(workspace, CLIPMI_ERR_ARG, "order_stats: null workspace");
  CLIPMI_REQUIRE((uintptr_t)workspace % 16 == 0, CLIPMI_ERR_ARG, "order_stats: the workspace must be 16-byte aligned");
  const size_t need = clipmi_order_stats_workspace_bytes(n, k);
  CLIPMI_REQUIRE(workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "order_stats: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  if (const hipError_t e = hipMemsetAsync(workspace, 0, need, s); e != hipSuccess) {
    (void)hipGetLastError();
    set_error("order_stats: hipMemsetAsync: %s", hipGetErrorString(e));
    return CLIPMI_ERR_HIP;
  }
  SelectState* st = static_cast<SelectState*>(workspace);
  uint32_t* hist = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + select_state_bytes());
  const int lds = k * RADIX * (int)sizeof(uint32_t) + HIST_LDS_EXTRA;
  static DeviceOnce attr_once;
  ensure_dynamic_lds(order_hist_kernel, MAXK * RADIX * (int)sizeof(uint32_t) + HIST_LDS_EXTRA, attr_once);
  const int grid = grid_for(n, 4, 256);
  for (int pass = 0; pass < 4; ++pass) {
    uint32_t* h = hist + (size_t)pass * k * RADIX;
    hipLaunchKernelGGL(order_hist_kernel, dim3(grid), dim3(256), lds, s, x, n, pass, k, st, h);
    if (int rc = check_launch("order_hist_kernel")) return rc;
    hipLaunchKernelGGL(order_resolve_kernel, dim3(1), dim3(1024), 0, s, pass, k, r, st, h, out, nan_count);
    if (int rc = check_launch("order_resolve_kernel")) return rc;
  }
  return CLIPMI_OK;
}

int clipmi_group_gap_accumulate(const float* conf, const int32_t* pred, const int64_t* labels, const float* key, const double* key_edges,
                                int n_key_edges, const double* conf_edges, int n_conf_edges, double* groups, int n, clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  CLIPMI_REQUIRE(n >= 0, CLIPMI_ERR_SHAPE, "group_gap_accumulate: n=%d", n);
  CLIPMI_REQUIRE(n_key_edges >= 0 && n_conf_edges >= 0, CLIPMI_ERR_SHAPE, "group_gap_accumulate: %d key edges, %d confidence edges",
                 n_key_edges, n_conf_edges);
  const int64_t G = ((int64_t)n_key_edges + 1) * ((int64_t)n_conf_edges + 1);
  CLIPMI_REQUIRE(G <= MAXG, CLIPMI_ERR_SHAPE, "group_gap_accumulate: (%d + 1) x (%d + 1) groups (at most %d)", n_key_edges, n_conf_edges, MAXG);
  if (n == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(conf && pred && labels && groups, CLIPMI_ERR_ARG, "group_gap_accumulate: null pointer (conf, pred, labels and groups are required)");
  CLIPMI_REQUIRE(n_key_edges == 0 || (key && key_edges), CLIPMI_ERR_ARG, "group_gap_accumulate: %d key edges need key and key_edges", n_key_edges);
  CLIPMI_REQUIRE(n_conf_edges == 0 || conf_edges, CLIPMI_ERR_ARG, "group_gap_accumulate: %d confidence edges need conf_edges", n_conf_edges);
  const size_t lds = (3 * (size_t)G + n_key_edges + n_conf_edges) * sizeof(double);
  hipLaunchKernelGGL(group_gap_kernel, dim3(grid_for(n, 1, 256)), dim3(256), lds, s, conf, pred, labels, key, key_edges, n_key_edges,
                     conf_edges, n_conf_edges, groups, n);
  return check_launch("group_gap_kernel");
}

int clipmi_class_counts(const int32_t* pred, const int64_t* labels, int n, int C, int64_t* counts, clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  CLIPMI_REQUIRE(n >= 0, CLIPMI_ERR_SHAPE, "class_counts: n=%d", n);
  CLIPMI_REQUIRE(C >= 1 && C <= (0x7fffffff - 1) / 3, CLIPMI_ERR_SHAPE, "class_counts: C=%d", C);
  if (n == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(pred && labels && counts, CLIPMI_ERR_ARG, "class_counts: null pointer");
  CLIPMI_REQUIRE((uintptr_t)counts % 8 == 0, CLIPMI_ERR_ARG, "class_counts: counts must be 8-byte aligned");
  unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
  const int total = 3 * C + 1;
  if (total <= CLASS_LDS_COUNTERS) {
    hipLaunchKernelGGL(class_counts_kernel<true>, dim3(grid_for(n, 4, 64)), dim3(256), total * sizeof(uint32_t), s, pred, labels, n, C, c);
  } else {
    hipLaunchKernelGGL(class_counts_kernel<false>, dim3(grid_for(n, 1, 256)), dim3(256), 0, s, pred, labels, n, C, c);
  }
  return check_launch("class_counts_kernel");
}

}  // extern "C"
