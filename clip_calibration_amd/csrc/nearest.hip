// Nearest reference rows WITH their indices: for every query row the K rows of `refs` at the smallest L2 distance, ascending in the total
// order (distance, index) -- the nearest vocabulary words of a learned context (reference interpret_prompts/interpret_prompt.py:66-76:
// torch.cdist + argsort of the whole [rows, 49408] matrix, generic contexts only).  knn.hip next door returns distances only and gives
// one workgroup the whole reference set; here the grid is (query blocks) x (slices of the reference rows), so 4 context rows against
// 49 408 x 512 embeddings still fill the chip, and a second launch merges the slices' lists.
//
// nearest_partial_kernel: one workgroup = 16 queries (4 per wave) x one slice of 64-row reference tiles.  A tile is staged through LDS in
// 64-column chunks (coalesced 256-B row segments in, rows padded to 68 floats out: conflict-free ds_read_b128), the next chunk's global
// loads are in flight while the current one is consumed.  Lane l owns reference row l of the tile and accumulates sum_e (q_e - r_e)^2 --
// the difference form of knn.hip, no |q|^2 + |r|^2 - 2 q.r cancellation -- for the wave's 4 queries, e ascending, one fmaf per term: the
// sum of a pair is the same instruction sequence whatever the slice count or the query count.  The query values are wave-uniform and are
// read straight from global memory (scalar loads: they are operands of the subtraction, not vector registers).
//
// The K best of a query are NOT per-thread lists (2 x 32 x (distance, index) = 128 registers at K = 32): the wave keeps ONE sorted list
// per query across its lanes -- lane j holds the j-th best pair -- and a running threshold, the K-th best.  After a tile, the lanes whose
// pair beats the threshold are found with one ballot (none, for almost every tile once the list has settled) and inserted one at a time:
// a lane keeps its entry, takes the candidate, or takes its left neighbour's entry.  Two registers per query, no LDS, no spills, and the
// list is exact in the total order (NaN distance = +inf; ties to the lower index; pads are (+inf, INT32_MAX)), so every slice count
// selects the same pairs.  nearest_merge_kernel runs the same list over the `splits` partial lists of a query (one wave per query) and
// takes the square root.  No atomics and no inter-workgroup hand-off: two launches on one stream.
#include "common.h"

#include <limits.h>

namespace clipmi {
namespace {

constexpr int QW = 4, NW = 4, QB = QW * NW;   // queries per wave, waves, queries per workgroup
constexpr int RT = 64, EC = 64, LDR = EC + 4;  // reference rows per tile, columns per chunk, LDS row stride in floats (272 B: 16-B aligned, +1 access width)
constexpr int KMAX = 32;
constexpr int MERGE_WAVES = 4, MERGE_AHEAD = 8;
constexpr int WG_PER_CU = 8;   // resident workgroups per CU (58 VGPRs: 8 waves per SIMD; 17 KiB of LDS each): what hides the scalar-load latency

__device__ __forceinline__ float lane_f(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ bool pair_less(float d, int i, float od, int oi) { return d < od || (d == od && i < oi); }

// The wave's sorted list: lane j holds the j-th smallest (distance, index) pair seen so far.
struct WaveList {
  float d;
  int i;
  float thr_d;   // the K-th best (wave-uniform): what a candidate has to beat
  int thr_i;

  __device__ __forceinline__ void init() {
    d = thr_d = INFINITY;
    i = thr_i = INT_MAX;
  }
  // (cd, ci) wave-uniform
  __device__ __forceinline__ void insert(float cd, int ci, int K) {
    const float pd = __shfl_up(d, 1, 64);
    const int pi = __shfl_up(i, 1, 64);
    const bool first = (threadIdx.x & 63) == 0;
    if (pair_less(cd, ci, d, i)) {            // the candidate goes in front of this lane's entry: take it, or the left neighbour's entry
      const bool shift = !first && pair_less(cd, ci, pd, pi);
      d = shift ? pd : cd;
      i = shift ? pi : ci;
    }
    thr_d = lane_f(d, K - 1);
    thr_i = __builtin_amdgcn_readlane(i, K - 1);
  }
  // one candidate per lane (v == v; lanes without one pass (+inf, INT_MAX), which beats nothing)
  __device__ __forceinline__ void offer(float v, int idx, int K) {
    unsigned long long mask = __ballot(pair_less(v, idx, thr_d, thr_i));
    while (mask) {
      const int src = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const float cd = lane_f(v, src);
      const int ci = __builtin_amdgcn_readlane(idx, src);
      if (pair_less(cd, ci, thr_d, thr_i)) insert(cd, ci, K);   // the threshold may have moved since the ballot
    }
  }
};

__global__ __launch_bounds__(NW * 64) void nearest_partial_kernel(const float* __restrict__ q, const float* __restrict__ refs,
                                                                  float* __restrict__ ws_d, int32_t* __restrict__ ws_i, int Nq, int Nr, int E,
                                                                  int K, int splits, int nqb) {
  __shared__ __attribute__((aligned(16))) float rs[RT * LDR];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qb = blockIdx.x % nqb, s = blockIdx.x / nqb;   // neighbours in the grid share a slice of refs
  const int tiles = (Nr + RT - 1) / RT;
  const int t0 = (int)((int64_t)s * tiles / splits), t1 = (int)((int64_t)(s + 1) * tiles / splits);
  const int ne = E / EC;
  const int64_t chunks = (int64_t)(t1 - t0) * ne;
  const int qw0 = qb * QB + wave * QW;
  const bool live = qw0 < Nq;   // a wave without queries still stages tiles and meets the barriers
  const float* qrow[QW];
#pragma unroll
  for (int a = 0; a < QW; ++a) qrow[a] = q + (int64_t)(qw0 + a < Nq ? qw0 + a : Nq - 1) * E;

  WaveList list[QW];
#pragma unroll
  for (int a = 0; a < QW; ++a) list[a].init();

  // staging: thread t moves the float4 (row t / 16 + 16 k, columns 4 (t % 16) ..) for k < 4
  const int srow = tid >> 4, scol = (tid & 15) * 4;
  f32x4 stage[4];
  auto fetch = [&](int64_t c) {
    const int r0 = (t0 + (int)(c / ne)) * RT, e0 = (int)(c % ne) * EC;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int row = r0 + srow + 16 * k < Nr ? r0 + srow + 16 * k : Nr - 1;
      stage[k] = *reinterpret_cast<const f32x4*>(refs + (int64_t)row * E + e0 + scol);
    }
  };
  if (chunks > 0) fetch(0);
  float d[QW] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t c = 0; c < chunks; ++c) {
    const int ei = (int)(c % ne);
    __syncthreads();   // the previous chunk has been read
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<f32x4*>(&rs[(srow + 16 * k) * LDR + scol]) = stage[k];
    __syncthreads();
    if (c + 1 < chunks) fetch(c + 1);
    if (!live) continue;
    if (ei == 0) {
#pragma unroll
      for (int a = 0; a < QW; ++a) d[a] = 0.f;
    }
    const int e0 = ei * EC;
#pragma unroll 2   // 8 columns = 32 scalar registers of query values in flight; a full unroll spills them
    for (int j = 0; j < EC; j += 4) {
      const f32x4 rv = *reinterpret_cast<const f32x4*>(&rs[lane * LDR + j]);
#pragma unroll
      for (int a = 0; a < QW; ++a) {
        const f32x4 qv = *reinterpret_cast<const f32x4*>(qrow[a] + e0 + j);   // wave-uniform address
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const float t = qv[x] - rv[x];
          d[a] = fmaf(t, t, d[a]);
        }
      }
    }
    if (ei == ne - 1) {
      const int row = (t0 + (int)(c / ne)) * RT + lane;
      const int idx = row < Nr ? row : INT_MAX;
#pragma unroll
      for (int a = 0; a < QW; ++a) {
        const float v = (row < Nr && d[a] == d[a]) ? d[a] : INFINITY;   // NaN counts as +inf
        list[a].offer(v, idx, K);
      }
    }
  }
  if (lane < K) {
#pragma unroll
    for (int a = 0; a < QW; ++a) {
      if (qw0 + a < Nq) {
        const int64_t o = ((int64_t)(qw0 + a) * splits + s) * K + lane;   // [query][slice][K]: a query's lists are contiguous for the merge
        ws_d[o] = list[a].d;
        ws_i[o] = list[a].i;
      }
    }
  }
}

// one wave per query: the K best of the `splits` partial lists (squared distances), then the square root
__global__ __launch_bounds__(MERGE_WAVES * 64) void nearest_merge_kernel(const float* __restrict__ ws_d, const int32_t* __restrict__ ws_i,
                                                                         float* __restrict__ out_d, int32_t* __restrict__ out_i, int Nq, int K,
                                                                         int splits) {
  const int lane = threadIdx.x & 63;
  const int64_t qi = (int64_t)blockIdx.x * MERGE_WAVES + (threadIdx.x >> 6);
  if (qi >= Nq) return;
  WaveList list;
  list.init();
  const int64_t total = (int64_t)splits * K;
  const float* qd = ws_d + qi * total;
  const int32_t* qx = ws_i + qi * total;
  for (int64_t c0 = 0; c0 < total; c0 += 64 * MERGE_AHEAD) {   // MERGE_AHEAD loads in flight, then the offers in order
    float v[MERGE_AHEAD];
    int idx[MERGE_AHEAD];
#pragma unroll
    for (int u = 0; u < MERGE_AHEAD; ++u) {
      const int64_t c = c0 + 64 * u + lane;
      v[u] = c < total ? qd[c] : INFINITY;
      idx[u] = c < total ? qx[c] : INT_MAX;
    }
#pragma unroll
    for (int u = 0; u < MERGE_AHEAD; ++u)
      if (c0 + 64 * u < total) list.offer(v[u], idx[u], K);
  }
  if (lane < K) {
    out_d[qi * K + lane] = sqrtf(list.d);
    out_i[qi * K + lane] = list.i;
  }
}

inline int query_blocks(int Nq) { return (Nq + QB - 1) / QB; }

// splits = 0: as many workgroups as the chip holds at once (WG_PER_CU per CU: the query values arrive by scalar loads whose latency only
// other resident waves hide) where the reference set has the tiles for it, and never more slices than tiles
inline int auto_splits(int Nq, int Nr) {
  const int tiles = (Nr + RT - 1) / RT, nqb = query_blocks(Nq);
  const int want = (WG_PER_CU * device_cus() + nqb - 1) / nqb;
  return want < tiles ? want : tiles;
}

inline bool shape_ok(int Nq, int Nr, int K, int splits) { return Nq >= 0 && Nr >= 1 && K >= 1 && K <= KMAX && K <= Nr && splits >= 0; }

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" {

int clipmi_nearest_rows_splits(int Nq, int Nr) {
  if (Nq < 1 || Nr < 1) return 1;
  return auto_splits(Nq, Nr);
}

size_t clipmi_nearest_rows_workspace(int Nq, int Nr, int K, int splits) {
  if (!shape_ok(Nq, Nr, K, splits)) return 0;
  if (Nq == 0) return 0;
  if (splits == 0) splits = auto_splits(Nq, Nr);
  return (size_t)splits * (size_t)Nq * (size_t)K * (sizeof(float) + sizeof(int32_t));
}

int clipmi_nearest_rows(const float* q, const float* refs, float* out_dist, int32_t* out_idx, int Nq, int Nr, int E, int K, int splits,
                        void* workspace, size_t workspace_bytes, clipmi_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  CLIPMI_REQUIRE(Nq >= 0 && Nr >= 1 && E >= 1 && E % EC == 0, CLIPMI_ERR_SHAPE, "nearest_rows: Nq=%d Nr=%d E=%d (E %% 64 == 0)", Nq, Nr, E);
  CLIPMI_REQUIRE(K >= 1 && K <= KMAX && K <= Nr, CLIPMI_ERR_SHAPE, "nearest_rows: K=%d must be in [1, min(%d, Nr)]", K, KMAX);
  CLIPMI_REQUIRE(splits >= 0, CLIPMI_ERR_SHAPE, "nearest_rows: splits=%d (0 = the library chooses)", splits);
  if (Nq == 0) return CLIPMI_OK;
  if (splits == 0) splits = auto_splits(Nq, Nr);
  const int nqb = query_blocks(Nq);
  CLIPMI_REQUIRE((int64_t)nqb * splits < (1ll << 31), CLIPMI_ERR_SHAPE, "nearest_rows: %d query blocks x %d slices is too many workgroups", nqb, splits);
  CLIPMI_REQUIRE(q && refs && out_dist && out_idx, CLIPMI_ERR_ARG, "nearest_rows: null pointer");
  CLIPMI_REQUIRE((uintptr_t)q % 16 == 0 && (uintptr_t)refs % 16 == 0 && (uintptr_t)out_dist % 16 == 0 && (uintptr_t)out_idx % 16 == 0 &&
                     (uintptr_t)workspace % 16 == 0,
                 CLIPMI_ERR_ARG, "nearest_rows: pointers must be 16-byte aligned");
  const size_t need = clipmi_nearest_rows_workspace(Nq, Nr, K, splits);
  CLIPMI_REQUIRE(workspace && workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "nearest_rows: workspace %zu < %zu bytes", workspace_bytes, need);
  float* ws_d = static_cast<float*>(workspace);
  int32_t* ws_i = reinterpret_cast<int32_t*>(ws_d + (size_t)splits * Nq * K);
  hipLaunchKernelGGL(nearest_partial_kernel, dim3((unsigned)(nqb * splits)), dim3(NW * 64), 0, s, q, refs, ws_d, ws_i, Nq, Nr, E, K, splits, nqb);
  const int rc = check_launch("nearest_partial_kernel");
  if (rc != CLIPMI_OK) return rc;
  hipLaunchKernelGGL(nearest_merge_kernel, dim3((unsigned)((Nq + MERGE_WAVES - 1) / MERGE_WAVES)), dim3(MERGE_WAVES * 64), 0, s, ws_d, ws_i, out_dist,
                     out_idx, Nq, K, splits);
  return check_launch("nearest_merge_kernel");
}

}  // extern "C"
