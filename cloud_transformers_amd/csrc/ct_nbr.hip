// Neighbour search over a uniform grid for gfx950: the index (a counting sort of points by cell), the sorted and
// truncated radius query and the nearest-neighbour query of the S3DIS KPConv protocol (replace the CPU
// sklearn.neighbors.KDTree of datasets/s3dis_closer.py:204,262-265,290,319-322).
//
// Cells are laid out x fastest, cell = (iz * ny + iy) * nx + ix, so one x-row of cells is one contiguous range
// [cell_start[a], cell_start[b + 1]) of the permutation and a query scans whole rows as single ranges.  The index
// also stores the points in cell order as float4 (x, y, z, index bits): a scan reads one 16-byte record per candidate.
//
// Squared distances are ((dx*dx) + (dy*dy)) + (dz*dz) with d = p - c, built with -ffp-contract=off: the same float32
// operations numpy performs, so results are reproducible bit for bit.  Which cells a query visits is decided with a
// margin of one whole cell (and, for the nearest query, an explicit slack on its stopping bound), so the exact
// float32 test decides membership, never the cell geometry.  Points outside the grid box are counted in the nearest
// edge cell; both queries treat the edge cells as reaching to infinity and stay exact for them.
#include "ct_common.h"

namespace {

constexpr int kScanThreads = 1024;
constexpr int kScanChunk = 4 * kScanThreads;   // elements per scan workgroup
constexpr int kRadThreads = 1024;              // one workgroup per radius query
constexpr int kRadWaves = kRadThreads / CT_WAVE;
constexpr int kKMax = 16384;                   // (d2, index) keys in LDS: 128 KiB
constexpr int kBins = 2048;                    // radix-select digit: up to 11 bits
constexpr int kMaxCells = 1 << 26;
constexpr int64_t kNearestMaxQ = 0x7fffffff;   // queries per ct_nbr_nearest call: one launch, < 2^31 work-items

struct NbrGrid {
  float o[3];
  float h;
  int n[3];
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

// ---- index build: count, scan, scatter (the counting sort of ct_plane_sort, over cells instead of plane cells) ----

__global__ void nbr_count_kernel(const float* __restrict__ pts, int M, NbrGrid g, unsigned* counts,
                                 int* __restrict__ cid, int* __restrict__ slot) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const float x = pts[(size_t)i * 3 + 0], y = pts[(size_t)i * 3 + 1], z = pts[(size_t)i * 3 + 2];
  const int c = (nbr_cell(z, g.o[2], g.h, g.n[2]) * g.n[1] + nbr_cell(y, g.o[1], g.h, g.n[1])) * g.n[0] +
                nbr_cell(x, g.o[0], g.h, g.n[0]);
  cid[i] = c;
  slot[i] = (int)atomicAdd(&counts[c], 1u);   // order inside a cell follows the atomics; no query output depends on it
}

// exclusive scan of a[base, base + kScanChunk) ∩ [0, n) in place, offset by `carry`; returns the chunk's sum
__device__ unsigned scan_chunk(unsigned* a, long long base, long long n, unsigned carry, unsigned* s16, unsigned* s_tot) {
  unsigned v[4], sum = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long e = base + 4 * threadIdx.x + u;
    v[u] = e < n ? a[e] : 0u;
    sum += v[u];
  }
  unsigned run = block_excl_scan(sum, s16, s_tot) + carry;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long e = base + 4 * threadIdx.x + u;
    if (e < n) a[e] = run;
    run += v[u];
  }
  const unsigned t = *s_tot;
  __syncthreads();
  return t;
}

__global__ void __launch_bounds__(kScanThreads) nbr_scan_blocks_kernel(unsigned* a, long long n, unsigned* bsum) {
  __shared__ unsigned s16[16], s_tot;
  const unsigned t = scan_chunk(a, (long long)blockIdx.x * kScanChunk, n, 0u, s16, &s_tot);
  if (threadIdx.x == 0) bsum[blockIdx.x] = t;
}

__global__ void __launch_bounds__(kScanThreads) nbr_scan_sums_kernel(unsigned* bsum, int nb) {
  __shared__ unsigned s16[16], s_tot;
  unsigned carry = 0;
  for (long long base = 0; base < nb; base += kScanChunk) carry += scan_chunk(bsum, base, nb, carry, s16, &s_tot);
}

__global__ void nbr_scan_add_kernel(unsigned* a, long long n, const unsigned* __restrict__ bsum) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) a[e] += bsum[e / kScanChunk];
}

__global__ void nbr_scatter_kernel(const float* __restrict__ pts, int M, const int* __restrict__ cid,
                                   const int* __restrict__ slot, const int* __restrict__ cell_start,
                                   int* __restrict__ order, float4* __restrict__ sorted) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const int pos = cell_start[cid[i]] + slot[i];
  order[pos] = i;
  sorted[pos] = make_float4(pts[(size_t)i * 3 + 0], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2], __int_as_float(i));
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
__global__ void __launch_bounds__(kRadThreads) nbr_radius_kernel(const float4* __restrict__ sp, const int* __restrict__ cs,
                                                                 NbrGrid g, const float* __restrict__ centres, float r, int K,
                                                                 int64_t* __restrict__ out_idx, float* __restrict__ out_d2,
                                                                 int64_t* __restrict__ out_count) {
  __shared__ unsigned long long s_keys[kKMax];
  __shared__ unsigned s_hist[kBins];
  __shared__ unsigned s16[16], s_tot, s_cnt, s_n, s_bucket, s_k, s_full;
  const int q = blockIdx.x, tid = threadIdx.x;
  const float cx = centres[(size_t)q * 3 + 0], cy = centres[(size_t)q * 3 + 1], cz = centres[(size_t)q * 3 + 2];
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
    out_idx[row + i] = ok ? (int64_t)(unsigned)(key & 0xffffffffu) : (int64_t)-1;
    out_d2[row + i] = ok ? __uint_as_float((unsigned)(key >> 32)) : __builtin_inff();
  }
  if (tid == 0) out_count[q] = (int64_t)count;
}

// ---- nearest neighbour: one thread per query, shells of cells around the query's (clamped) cell ----

__device__ __forceinline__ void nbr_scan_range(const float4* __restrict__ sp, int beg, int end, float qx, float qy, float qz,
                                               float& best, int& bi) {
  for (int j = beg; j < end; ++j) {
    const float4 p = sp[j];
    const float d2 = nbr_d2(p, qx, qy, qz);
    const int id = __float_as_int(p.w);
    if (d2 < best || (d2 == best && id < bi)) best = d2, bi = id;
  }
}

__global__ void __launch_bounds__(256) nbr_nearest_kernel(const float4* __restrict__ sp, const int* __restrict__ cs, NbrGrid g,
                                                         const float* __restrict__ qs, long long Q, int64_t* __restrict__ out_idx,
                                                         float* __restrict__ out_d2) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Q) return;
  const float qx = qs[i * 3 + 0], qy = qs[i * 3 + 1], qz = qs[i * 3 + 2];
  const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
  const int cx = nbr_cell(qx, g.o[0], g.h, nx), cy = nbr_cell(qy, g.o[1], g.h, ny), cz = nbr_cell(qz, g.o[2], g.h, nz);
  // slack on the stopping bound: float error of cell assignment, face positions and d2, with a wide margin
  const float eps = 1e-5f * (fabsf(qx) + fabsf(qy) + fabsf(qz) + fabsf(g.o[0]) + fabsf(g.o[1]) + fabsf(g.o[2]) +
                             g.h * (float)(nx + ny + nz)) + 1e-3f * g.h;
  float best = __builtin_inff();
  int bi = 0x7fffffff;
  for (int s = 0;; ++s) {
    const int z0 = max(cz - s, 0), z1 = min(cz + s, nz - 1), y0 = max(cy - s, 0), y1 = min(cy + s, ny - 1);
    const int x0 = max(cx - s, 0), x1 = min(cx + s, nx - 1);
    for (int z = z0; z <= z1; ++z) {
      const bool zface = abs(z - cz) == s;
      for (int y = y0; y <= y1; ++y) {
        const int base = (z * ny + y) * nx;
        if (zface || abs(y - cy) == s) {
          nbr_scan_range(sp, cs[base + x0], cs[base + x1 + 1], qx, qy, qz, best, bi);
        } else {
          if (cx - s >= 0) nbr_scan_range(sp, cs[base + cx - s], cs[base + cx - s + 1], qx, qy, qz, best, bi);
          if (cx + s <= nx - 1) nbr_scan_range(sp, cs[base + cx + s], cs[base + cx + s + 1], qx, qy, qz, best, bi);
        }
      }
    }
    // every cell not visited yet lies beyond one face of the visited block: its points are at least that face's gap away
    bool more = false;
    float bound = __builtin_inff();
    const float qv[3] = {qx, qy, qz};
    const int cv[3] = {cx, cy, cz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (cv[a] + s + 1 <= g.n[a] - 1) more = true, bound = fminf(bound, g.o[a] + (float)(cv[a] + s + 1) * g.h - qv[a]);
      if (cv[a] - s - 1 >= 0) more = true, bound = fminf(bound, qv[a] - (g.o[a] + (float)(cv[a] - s) * g.h));
    }
    if (!more) break;
    bound -= eps;
    if (bound > 0.0f && best < bound * bound) break;
  }
  out_idx[i] = bi == 0x7fffffff ? (int64_t)-1 : (int64_t)bi;
  out_d2[i] = best;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// `sorted` is read and written as float4 records
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

bool grid_ok(const float* origin, float h, const int* dims, long long* ncells) {
  if (!origin || !dims || !(h > 0.0f) || !__builtin_isfinite(h)) return false;
  long long n = 1;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1 || dims[a] > kMaxCells || !__builtin_isfinite(origin[a])) return false;
    n *= dims[a];
    if (n > kMaxCells) return false;
  }
  *ncells = n;
  return true;
}

NbrGrid make_grid(const float* origin, float h, const int* dims) {
  NbrGrid g;
  for (int a = 0; a < 3; ++a) g.o[a] = origin[a], g.n[a] = dims[a];
  g.h = h;
  return g;
}

}  // namespace

extern "C" {

size_t ct_nbr_index_workspace_bytes(int64_t M, const int* dims) {
  const float o[3] = {0.0f, 0.0f, 0.0f};
  long long ncells = 0;
  if (M < 1 || M > 0x7fffffffLL || !grid_ok(o, 1.0f, dims, &ncells)) return 0;
  const long long nb = (ncells + 1 + kScanChunk - 1) / kScanChunk;
  return 2 * align256((size_t)M * 4) + align256((size_t)nb * 4);
}

int ct_nbr_index_build(const float* points, int64_t M, const float* origin, float h, const int* dims, int32_t* cell_start,
                       int32_t* order, float* sorted, void* workspace, size_t workspace_bytes, ct_stream_t s) {
  long long ncells = 0;
  if (!points || !cell_start || !order || !sorted || !aligned16(sorted) || M < 1 || M > 0x7fffffffLL ||
      !grid_ok(origin, h, dims, &ncells))
    return CT_EINVAL;
  if (!workspace || workspace_bytes < ct_nbr_index_workspace_bytes(M, dims)) return CT_EWORKSPACE;
  hipStream_t st = (hipStream_t)s;
  const NbrGrid g = make_grid(origin, h, dims);
  const int m = (int)M;
  const long long n = ncells + 1;
  const int nb = (int)((n + kScanChunk - 1) / kScanChunk);
  char* ws = (char*)workspace;
  int* cid = (int*)ws;
  int* slot = (int*)(ws + align256((size_t)M * 4));
  unsigned* bsum = (unsigned*)(ws + 2 * align256((size_t)M * 4));
  unsigned* cnt = (unsigned*)cell_start;
  if (hipMemsetAsync(cell_start, 0, (size_t)n * 4, st) != hipSuccess) return CT_ELAUNCH;
  CT_CLEAR_ERROR();
  hipLaunchKernelGGL(nbr_count_kernel, dim3((m + 255) / 256), dim3(256), 0, st, points, m, g, cnt, cid, slot);
  hipLaunchKernelGGL(nbr_scan_blocks_kernel, dim3(nb), dim3(kScanThreads), 0, st, cnt, n, bsum);
  hipLaunchKernelGGL(nbr_scan_sums_kernel, dim3(1), dim3(kScanThreads), 0, st, bsum, nb);
  hipLaunchKernelGGL(nbr_scan_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cnt, n, (const unsigned*)bsum);
  hipLaunchKernelGGL(nbr_scatter_kernel, dim3((m + 255) / 256), dim3(256), 0, st, points, m, (const int*)cid, (const int*)slot,
                     (const int*)cell_start, order, (float4*)sorted);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

int ct_nbr_radius(const int32_t* cell_start, const float* sorted, const float* origin, float h, const int* dims,
                  const float* centres, int Q, float r, int K, int64_t* idx, float* d2, int64_t* count, ct_stream_t s) {
  long long ncells = 0;
  if (!cell_start || !sorted || !aligned16(sorted) || !centres || !idx || !d2 || !count || Q < 1 || K < 1 || K > kKMax ||
      !(r >= 0.0f) ||
      !grid_ok(origin, h, dims, &ncells))
    return CT_EINVAL;
  hipStream_t st = (hipStream_t)s;
  CT_CLEAR_ERROR();
  hipLaunchKernelGGL(nbr_radius_kernel, dim3(Q), dim3(kRadThreads), 0, st, (const float4*)sorted, cell_start,
                     make_grid(origin, h, dims), centres, r, K, idx, d2, count);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

int ct_nbr_nearest(const int32_t* cell_start, const float* sorted, const float* origin, float h, const int* dims,
                   const float* queries, int64_t Q, int64_t* idx, float* d2, ct_stream_t s) {
  long long ncells = 0;
  if (!cell_start || !sorted || !aligned16(sorted) || !queries || !idx || !d2 || Q < 1 || Q > kNearestMaxQ ||
      !grid_ok(origin, h, dims, &ncells))
    return CT_EINVAL;
  hipStream_t st = (hipStream_t)s;
  CT_CLEAR_ERROR();
  hipLaunchKernelGGL(nbr_nearest_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, st, (const float4*)sorted, cell_start,
                     make_grid(origin, h, dims), queries, (long long)Q, idx, d2);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

}  // extern "C"
