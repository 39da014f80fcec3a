// The exact k-nearest query of ct_nbr.hip (KDTree.query(X, k), 1 <= k <= 64) and the inverse-distance interpolation over
// its finished table.  Included by ct_nbr.hip only; built with -ffp-contract=off like everything that uses nbr_d2.
//
// One wavefront per query, kKnnWaves queries per workgroup; nothing is shared between waves: no LDS, no atomics, no
// barrier, no waiting of any kind.  The wave walks the shells of cells of nbr_nearest_kernel (the same nbr_cell, the
// same clamping of outside queries into edge cells, the same face-gap bound and eps slack), so that K = 1 gives
// ct_nbr_nearest's bits for every finite query.  What the wave adds is how a cell run is read: an x-row of cells is one
// contiguous run of `sorted`, and the wave takes it 64 records at a time, one coalesced 16-byte load per lane.
//
// The candidate list: lane l holds the l-th smallest key (d2, point id) seen so far, d2 ascending and the lower id first
// among equal d2; empty slots hold (+inf, 0x7fffffff), above every real key (ids are < 2^31 - 1).  All 64 lanes are kept
// sorted whatever K is; the threshold is lane K - 1's key.  A batch is filtered against the threshold with one ballot;
// a survivor is broadcast (readlane), ranked (a ballot of "my key is smaller": the list is sorted, so the set bits are
// a prefix and their count is the rank) and inserted by shifting the tail up one lane; the threshold is re-read and
// the remaining survivors are filtered again, so that most of a batch is dropped without being inserted.
//
// Stop rule, after shell s: the K-th d2 is below (bound - eps)^2 with nearest's bound and eps (an empty slot's +inf never
// is, so this implies K entries), or no unvisited cell remains.  The second condition bounds the walk by the grid's
// dimensions for every input.  A query with a non-finite coordinate keeps no candidate and reads no record: its bound
// is NaN or inf - inf, the first condition never holds, and it ends through the second with -1 / +inf in every slot.
#pragma once
#include "ct_nbr_query.h"

namespace {

constexpr int kKnnKMax = CT_NBR_KNN_K_MAX;     // one list slot per lane
static_assert(kKnnKMax == CT_WAVE, "the candidate list is one slot per lane");
constexpr int kKnnWaves = 4;                   // queries per workgroup
constexpr int kKnnThreads = kKnnWaves * CT_WAVE;
constexpr int kKnnEmpty = 0x7fffffff;

// (ad, ai) < (bd, bi); bitwise on purpose: three compares and two mask operations, no branch
__device__ __forceinline__ bool knn_less(float ad, int ai, float bd, int bi) {
  return (int)(ad < bd) | ((int)(ad == bd) & (int)(ai < bi));
}

// the value of lane - 1 (lane 0 keeps its own): one DPP move, wave_shr:1
__device__ __forceinline__ int knn_from_below(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }

__device__ __forceinline__ float knn_lane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// This wave's list (kd, ki: one sorted slot per lane) and its threshold (td, ti: the key of lane K - 1).
struct KnnList {
  float kd, td;
  int ki, ti;
};

// One record per lane (`live` lanes only): filter against the threshold, insert the survivors.
__device__ __forceinline__ void knn_batch(float4 p, bool live, float qx, float qy, float qz, int K, int lane, KnnList& L) {
  const float d2 = nbr_d2(p, qx, qy, qz);
  const int id = __float_as_int(p.w);
  unsigned long long m = __ballot((int)live & (int)knn_less(d2, id, L.td, L.ti));
  while (m) {
    const int b = __ffsll((long long)m) - 1;
    const float cd = knn_lane_f(d2, b);
    const int ci = __builtin_amdgcn_readlane(id, b);
    const int pos = __popcll(__ballot(knn_less(L.kd, L.ki, cd, ci)));      // <= K - 1: the candidate is below lane K - 1's key
    const float ud = __int_as_float(knn_from_below(__float_as_int(L.kd)));
    const int ui = knn_from_below(L.ki);
    if (lane > pos) L.kd = ud, L.ki = ui;
    if (lane == pos) L.kd = cd, L.ki = ci;
    L.td = knn_lane_f(L.kd, K - 1);
    L.ti = __builtin_amdgcn_readlane(L.ki, K - 1);
    m &= m - 1;
    if (m) m &= __ballot((int)live & (int)knn_less(d2, id, L.td, L.ti));
  }
}

// The records [a0, a1) followed by [b0, b1), 64 at a time.
__device__ __forceinline__ void knn_scan(const float4* __restrict__ sp, int a0, int a1, int b0, int b1, float qx, float qy,
                                         float qz, int K, int lane, KnnList& L) {
  const int na = a1 - a0, n = na + (b1 - b0);
  for (int t0 = 0; t0 < n; t0 += CT_WAVE) {
    const int t = t0 + lane;
    const bool live = t < n;
    const int j = t < na ? a0 + t : b0 + (t - na);
    const float4 p = live ? sp[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    knn_batch(p, live, qx, qy, qz, K, lane, L);
  }
}

// Query blockIdx.x * kKnnWaves + wave: `src` (NbrDirectSource / NbrTableSource) gives its grid and position.
template <class Src>
__global__ void __launch_bounds__(kKnnThreads) nbr_knn_kernel(Src src, long long Q, int K, int64_t* __restrict__ out_idx,
                                                              float* __restrict__ out_d2) {
  const int lane = threadIdx.x & (CT_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / CT_WAVE));
  const long long q = (long long)blockIdx.x * kKnnWaves + wave;
  if (q >= Q) return;
  const NbrQuery qy = src((int)q);
  const float4* __restrict__ sp = qy.sp;
  const int* __restrict__ cs = qy.cs;
  const NbrGrid& g = qy.g;
  const float qx = qy.cx, qy_ = qy.cy, qz = qy.cz;
  const bool finite = __builtin_isfinite(qx) && __builtin_isfinite(qy_) && __builtin_isfinite(qz);
  const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
  const int cx = nbr_cell(qx, g.o[0], g.h, nx), cy = nbr_cell(qy_, g.o[1], g.h, ny), cz = nbr_cell(qz, g.o[2], g.h, nz);
  // nbr_nearest_kernel's slack on the stopping bound
  const float eps = 1e-5f * (fabsf(qx) + fabsf(qy_) + fabsf(qz) + fabsf(g.o[0]) + fabsf(g.o[1]) + fabsf(g.o[2]) +
                             g.h * (float)(nx + ny + nz)) + 1e-3f * g.h;
  KnnList L{__builtin_inff(), __builtin_inff(), kKnnEmpty, kKnnEmpty};
  for (int s = 0;; ++s) {
    const int z0 = max(cz - s, 0), z1 = min(cz + s, nz - 1), y0 = max(cy - s, 0), y1 = min(cy + s, ny - 1);
    const int x0 = max(cx - s, 0), x1 = min(cx + s, nx - 1);
    if (finite) {
      for (int z = z0; z <= z1; ++z) {
        const bool zface = abs(z - cz) == s;
        for (int y = y0; y <= y1; ++y) {
          const int base = (z * ny + y) * nx;
          if (zface || abs(y - cy) == s) {
            knn_scan(sp, cs[base + x0], cs[base + x1 + 1], 0, 0, qx, qy_, qz, K, lane, L);
          } else {
            // an interior row: its two end cells, as one run of candidates
            int a0 = 0, a1 = 0, b0 = 0, b1 = 0;
            if (cx - s >= 0) a0 = cs[base + cx - s], a1 = cs[base + cx - s + 1];
            if (cx + s <= nx - 1) b0 = cs[base + cx + s], b1 = cs[base + cx + s + 1];
            knn_scan(sp, a0, a1, b0, b1, qx, qy_, qz, K, lane, L);
          }
        }
      }
    }
    // every cell not visited yet lies beyond one face of the visited block: its points are at least that face's gap away
    bool more = false;
    float bound = __builtin_inff();
    const float qv[3] = {qx, qy_, qz};
    const int cv[3] = {cx, cy, cz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (cv[a] + s + 1 <= g.n[a] - 1) more = true, bound = fminf(bound, g.o[a] + (float)(cv[a] + s + 1) * g.h - qv[a]);
      if (cv[a] - s - 1 >= 0) more = true, bound = fminf(bound, qv[a] - (g.o[a] + (float)(cv[a] - s) * g.h));
    }
    if (!more) break;
    bound -= eps;
    if (bound > 0.0f && L.td < bound * bound) break;
  }
  if (lane < K) {
    const size_t at = (size_t)q * K + lane;
    out_idx[at] = L.ki == kKnnEmpty ? (int64_t)-1 : (int64_t)L.ki;
    out_d2[at] = L.kd;
  }
}

// ---- inverse-distance interpolation over a finished table: one work-item per (query, 4 columns) ----
//
// w_j = 1.0f / (d2_j + eps) for the slots with idx_j >= 0, s = ((w_0 + w_1) + ...) and
// out[c] = ((w_0 / s) * v[idx_0][c] + (w_1 / s) * v[idx_1][c]) + ..., all in slot order, fp32, true divisions, no
// contraction.  The weights are formed twice (once for s, once for the sum) instead of being kept: K is a run-time
// value, and 64 registers indexed by it would go to scratch.  A row with no slot to use is NaN.
constexpr int kInterpCols = 4;
constexpr int kInterpMaxBlocks = 1 << 20;

__global__ void __launch_bounds__(256) nbr_interp_kernel(const int64_t* __restrict__ idx, const float* __restrict__ d2, long long Q,
                                                         int K, const float* __restrict__ values, int C, float eps,
                                                         float* __restrict__ out) {
  const long long groups = (C + kInterpCols - 1) / kInterpCols;
  const long long total = Q * groups;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const long long q = t / groups;
    const int c0 = (int)(t % groups) * kInterpCols;
    const int64_t* __restrict__ qi = idx + q * K;
    const float* __restrict__ qd = d2 + q * K;
    float s = 0.0f;
    bool any = false;
    for (int j = 0; j < K; ++j) {
      if (qi[j] < 0) continue;
      const float w = 1.0f / (qd[j] + eps);
      s = any ? s + w : w;
      any = true;
    }
    float acc[kInterpCols];
#pragma unroll
    for (int u = 0; u < kInterpCols; ++u) acc[u] = __builtin_nanf("");
    bool first = true;
    for (int j = 0; j < K; ++j) {
      const int64_t i = qi[j];
      if (i < 0) continue;
      const float w = (1.0f / (qd[j] + eps)) / s;
      const float* __restrict__ v = values + (size_t)i * C;
#pragma unroll
      for (int u = 0; u < kInterpCols; ++u) {
        if (c0 + u < C) {
          const float term = w * v[c0 + u];
          acc[u] = first ? term : acc[u] + term;
        }
      }
      first = false;
    }
#pragma unroll
    for (int u = 0; u < kInterpCols; ++u)
      if (c0 + u < C) out[(size_t)q * C + c0 + u] = acc[u];
  }
}

}  // namespace
