// The radius-query workgroup of ct_nbr.hip as a template, shared with ct_kpplan.hip: where the grid comes from (by value
// from the host, or a record of the device-resident index table chosen by a device cloud id) and what happens to each
// kept (d2, index) key besides the write-out (nothing, or the plan's Tukey update) are the two parameters.  Everything here
// has internal linkage; both sources are built with -ffp-contract=off.
#pragma once
#include "ct_common.h"

namespace {

constexpr int kRadThreads = 1024;              // one workgroup per radius query
constexpr int kRadWaves = kRadThreads / CT_WAVE;
constexpr int kKMax = 16384;                   // (d2, index) keys in LDS: 128 KiB
constexpr int kBins = 2048;                    // radix-select digit: up to 11 bits

struct NbrGrid {
  float o[3];
  float h;
  int n[3];
};

// One cloud of the index table (ct_nbr_table_set writes it on the host; private to the library): 64 bytes.
struct NbrRecord {
  const float4* sp;     // `sorted`
  const int* cs;        // `cell_start`
  NbrGrid g;
  int M;
  long long offset;     // the cloud's first point in the concatenated sub-clouds
  long long pad;
};
static_assert(sizeof(NbrRecord) == 64, "ct_nbr_table_bytes");

// What one query workgroup works on.
struct NbrQuery {
  const float4* sp;
  const int* cs;
  NbrGrid g;
  float cx, cy, cz;
  long long offset;
};

// The grid by value, the centre of query q from `centres` (ct_nbr_radius).
struct NbrDirectSource {
  const float4* sp;
  const int* cs;
  NbrGrid g;
  const float* centres;
  __device__ __forceinline__ NbrQuery operator()(int q) const {
    return {sp, cs, g, centres[(size_t)q * 3 + 0], centres[(size_t)q * 3 + 1], centres[(size_t)q * 3 + 2], 0};
  }
};

// The grid from the table record of cloud[q] (clamped into range as a guard), the centre of query q from `centres`.
struct NbrTableSource {
  const NbrRecord* table;
  int n_clouds;
  const int64_t* cloud;
  const float* centres;
  __device__ __forceinline__ NbrQuery operator()(int q) const {
    long long c = cloud[q];
    c = c < 0 ? 0 : (c > n_clouds - 1 ? n_clouds - 1 : c);
    const NbrRecord& rec = table[c];
    return {rec.sp, rec.cs, rec.g, centres[(size_t)q * 3 + 0], centres[(size_t)q * 3 + 1], centres[(size_t)q * 3 + 2],
            rec.offset};
  }
};

// The plain query: its keys go to idx / d2 and nowhere else.
struct NbrNoEpilogue {
  static constexpr bool kStore = true;
  __device__ __forceinline__ void operator()(const NbrQuery&, unsigned long long) const {}
};

__device__ __forceinline__ float nbr_d2(float4 p, float cx, float cy, float cz) {
  const float dx = p.x - cx, dy = p.y - cy, dz = p.z - cz;
  return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// floor((v - o) / h) + delta, clamped to [0, n - 1] in float first (no overflow, NaN -> 0)
__device__ __forceinline__ int nbr_cell(float v, float o, float h, int n, float delta = 0.0f) {
  const float t = floorf((v - o) / h) + delta;
  return (int)fminf(fmaxf(t, 0.0f), (float)(n - 1));
}

// gap between c and the slab of cell row i widened by one cell each side; an edge row reaches to infinity
__device__ __forceinline__ float nbr_slab_gap(float c, float o, float h, int i, int n) {
  const float lo = i == 0 ? -__builtin_inff() : o + (float)(i - 1) * h;
  const float hi = i == n - 1 ? __builtin_inff() : o + (float)(i + 2) * h;
  return fmaxf(0.0f, fmaxf(lo - c, c - hi));
}

__device__ __forceinline__ unsigned wave_incl_scan(unsigned v) {
  const int lane = threadIdx.x & (CT_WAVE - 1);
#pragma unroll
  for (int o = 1; o < CT_WAVE; o <<= 1) {
    const unsigned t = __shfl_up(v, o, CT_WAVE);
    if (lane >= o) v += t;
  }
  return v;
}

// exclusive scan of one value per thread over a 1024-thread workgroup; *total gets the sum.  s16: LDS unsigned[16].
__device__ unsigned block_excl_scan(unsigned v, unsigned* s16, unsigned* total) {
  const int lane = threadIdx.x & (CT_WAVE - 1), wave = threadIdx.x / CT_WAVE;
  const unsigned inc = wave_incl_scan(v);
  if (lane == CT_WAVE - 1) s16[wave] = inc;
  __syncthreads();
  if (wave == 0) {
    const unsigned w = lane < 16 ? s16[lane] : 0u;
    const unsigned wi = wave_incl_scan(w);
    if (lane < 16) s16[lane] = wi - w;
    if (lane == 15) *total = wi;
  }
  __syncthreads();
  const unsigned r = s16[wave] + inc - v;
  __syncthreads();
  return r;
}

// ---- radius query: one 1024-thread workgroup per centre ----

// Calls f(record) for every indexed point of the cells that can meet the ball (c, r): the x-rows of the ball's
// bounding box, each cut to the ball's chord at that row (all with one cell of margin).  Rows are spread over waves,
// the points of a row over lanes.
template <class F>
__device__ __forceinline__ void for_each_candidate(const float4* __restrict__ sp, const int* __restrict__ cs,
                                                   const NbrGrid& g, float cx, float cy, float cz, float r, F&& f) {
  const int lane = threadIdx.x & (CT_WAVE - 1), wave = threadIdx.x / CT_WAVE;
  const int y0 = nbr_cell(cy - r, g.o[1], g.h, g.n[1], -1.0f), y1 = nbr_cell(cy + r, g.o[1], g.h, g.n[1], 1.0f);
  const int z0 = nbr_cell(cz - r, g.o[2], g.h, g.n[2], -1.0f), z1 = nbr_cell(cz + r, g.o[2], g.h, g.n[2], 1.0f);
  const int nyr = y1 - y0 + 1, nrows = nyr * (z1 - z0 + 1);
  const float r2 = r * r;
  for (int row = wave; row < nrows; row += kRadWaves) {
    const int iy = y0 + row % nyr, iz = z0 + row / nyr;
    const float gy = nbr_slab_gap(cy, g.o[1], g.h, iy, g.n[1]), gz = nbr_slab_gap(cz, g.o[2], g.h, iz, g.n[2]);
    const float rem = r2 - gy * gy - gz * gz;
    if (!(rem >= 0.0f)) continue;
    const float hx = sqrtf(rem);
    const int x0 = nbr_cell(cx - hx, g.o[0], g.h, g.n[0], -1.0f), x1 = nbr_cell(cx + hx, g.o[0], g.h, g.n[0], 1.0f);
    const int base = (iz * g.n[1] + iy) * g.n[0];
    const int beg = cs[base + x0], end = cs[base + x1 + 1];
    for (int j = beg + lane; j < end; j += CT_WAVE) f(sp[j]);
  }
}

__device__ __forceinline__ unsigned long long nbr_key(float d2, float4 p) {
  return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(p.w);
}

// Radix select of the K-th smallest key (d2 bits << 32 | index) among the points with d2 <= r2, 11-bit digits from
// the top, each digit one more pass over the candidates with an LDS histogram; it stops at the first digit whose
// bucket is taken whole, usually after the d2 bits.  The keys at or below that bucket (exactly K of them) are
// collected into LDS and bitonic-sorted; fewer than K points in the ball skip the selection.
//
// Query q0 + blockIdx.x: `src` gives its grid and centre.  `epi(query, key)` runs once for each of the min(count, K) kept
// keys, by the work-item that writes it out; with Epi::kStore false nothing is written to out_idx / out_d2 / out_count.
template <class Src, class Epi>
__global__ void __launch_bounds__(kRadThreads) nbr_radius_kernel(Src src, int q0, float r, int K, int64_t* __restrict__ out_idx,
                                                                 float* __restrict__ out_d2, int64_t* __restrict__ out_count,
                                                                 Epi epi) {
  __shared__ unsigned long long s_keys[kKMax];
  __shared__ unsigned s_hist[kBins];
  __shared__ unsigned s16[16], s_tot, s_cnt, s_n, s_bucket, s_k, s_full;
  const int q = q0 + blockIdx.x, tid = threadIdx.x;
  const NbrQuery qy = src(q);
  const float4* __restrict__ sp = qy.sp;
  const int* __restrict__ cs = qy.cs;
  const NbrGrid& g = qy.g;
  const float cx = qy.cx, cy = qy.cy, cz = qy.cz;
  const float r2 = r * r;
  for (int i = tid; i < kBins; i += kRadThreads) s_hist[i] = 0;
  if (tid == 0) s_cnt = 0, s_n = 0;
  __syncthreads();

  // pass 0: the full count and the histogram of the top digit
  unsigned mine = 0;
  for_each_candidate(sp, cs, g, cx, cy, cz, r, [&](float4 p) {
    const float d2 = nbr_d2(p, cx, cy, cz);
    if (d2 <= r2) {
      ++mine;
      atomicAdd(&s_hist[nbr_key(d2, p) >> 53], 1u);
    }
  });
  atomicAdd(&s_cnt, mine);
  __syncthreads();
  const unsigned count = s_cnt;
  const unsigned need = min(count, (unsigned)K);

  bool all = count <= (unsigned)K;
  int sel_shift = 0;
  unsigned long long sel_prefix = 0;
  if (!all) {
    const int shifts[6] = {53, 42, 32, 21, 10, 0};
    unsigned k = (unsigned)K;          // rank of the K-th key among those matching `prefix`
    unsigned long long prefix = 0;     // key >> (shift + width) of the K-th key
    for (int d = 0; d < 6; ++d) {
      const int sh = shifts[d];
      // the bucket of this digit holding rank k
      const unsigned v0 = s_hist[2 * tid], v1 = s_hist[2 * tid + 1];
      const unsigned ex = block_excl_scan(v0 + v1, s16, &s_tot);
      if (ex < k && k <= ex + v0) {
        s_bucket = 2 * tid, s_k = k - ex, s_full = v0 == k - ex;
      } else if (ex + v0 < k && k <= ex + v0 + v1) {
        s_bucket = 2 * tid + 1, s_k = k - ex - v0, s_full = v1 == k - ex - v0;
      }
      __syncthreads();
      const int width = (d == 0 ? 64 : shifts[d - 1]) - sh;
      prefix = (prefix << width) | s_bucket;
      k = s_k;
      if (s_full || d == 5) {          // the last digit's keys are unique: always taken whole
        sel_shift = sh, sel_prefix = prefix;
        break;
      }
      const int nsh = shifts[d + 1];
      const unsigned long long nmask = (1ull << (sh - nsh)) - 1;
      __syncthreads();
      for (int i = tid; i < kBins; i += kRadThreads) s_hist[i] = 0;
      __syncthreads();
      for_each_candidate(sp, cs, g, cx, cy, cz, r, [&](float4 p) {
        const float d2 = nbr_d2(p, cx, cy, cz);
        if (d2 <= r2) {
          const unsigned long long key = nbr_key(d2, p);
          if ((key >> sh) == prefix) atomicAdd(&s_hist[(key >> nsh) & nmask], 1u);
        }
      });
      __syncthreads();
    }
  }

  // collect the `need` selected keys
  for_each_candidate(sp, cs, g, cx, cy, cz, r, [&](float4 p) {
    const float d2 = nbr_d2(p, cx, cy, cz);
    if (d2 <= r2) {
      const unsigned long long key = nbr_key(d2, p);
      if (all || (key >> sel_shift) <= sel_prefix) {
        const unsigned at = atomicAdd(&s_n, 1u);
        if (at < need) s_keys[at] = key;
      }
    }
  });
  __syncthreads();
  int npow = 1;
  while (npow < (int)need) npow <<= 1;
  for (int i = (int)need + tid; i < npow; i += kRadThreads) s_keys[i] = ~0ull;
  __syncthreads();
  for (int kk = 2; kk <= npow; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < npow / 2; i += kRadThreads) {
        const int lo = 2 * i - (i & (j - 1)), hi = lo + j;
        const unsigned long long a = s_keys[lo], b = s_keys[hi];
        if ((a > b) == ((lo & kk) == 0)) s_keys[lo] = b, s_keys[hi] = a;
      }
      __syncthreads();
    }
  }
  const size_t row = (size_t)q * K;
  for (int i = tid; i < K; i += kRadThreads) {
    const bool ok = i < (int)need;
    const unsigned long long key = ok ? s_keys[i] : 0ull;
    if constexpr (Epi::kStore) {
      out_idx[row + i] = ok ? (int64_t)(unsigned)(key & 0xffffffffu) : (int64_t)-1;
      out_d2[row + i] = ok ? __uint_as_float((unsigned)(key >> 32)) : __builtin_inff();
    }
    if (ok) epi(qy, key);
  }
  if constexpr (Epi::kStore) {
    if (tid == 0) out_count[q] = (int64_t)count;
  }
}

}  // namespace
