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
#include "ct_nbr_query.h"
#include "ct_nbr_knn.h"

namespace {

constexpr int kScanThreads = 1024;
constexpr int kScanChunk = 4 * kScanThreads;   // elements per scan workgroup
constexpr int kMaxCells = 1 << 26;
constexpr int64_t kNearestMaxQ = 0x7fffffff;   // queries per ct_nbr_nearest call: one launch, < 2^31 work-items

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
  const NbrDirectSource src{(const float4*)sorted, cell_start, make_grid(origin, h, dims), centres};
  hipLaunchKernelGGL((nbr_radius_kernel<NbrDirectSource, NbrNoEpilogue>), dim3(Q), dim3(kRadThreads), 0, st, src, 0, r, K, idx, d2,
                     count, NbrNoEpilogue{});
  CT_CHECK_LAUNCH();
  return CT_OK;
}

size_t ct_nbr_table_bytes(int n_clouds) { return n_clouds < 1 ? 0 : (size_t)n_clouds * sizeof(NbrRecord); }

int ct_nbr_table_set(void* host_table, int n_clouds, int i, const int32_t* cell_start, const float* sorted, const float* origin,
                     float h, const int* dims, int64_t M, int64_t offset) {
  long long ncells = 0;
  if (!host_table || ((uintptr_t)host_table & 7) != 0 || n_clouds < 1 || i < 0 || i >= n_clouds || !cell_start || !sorted ||
      !aligned16(sorted) || M < 1 || M > 0x7fffffffLL || offset < 0 || !grid_ok(origin, h, dims, &ncells))
    return CT_EINVAL;
  NbrRecord rec;
  rec.sp = (const float4*)sorted, rec.cs = cell_start, rec.g = make_grid(origin, h, dims);
  rec.M = (int)M, rec.offset = offset, rec.pad = 0;
  ((NbrRecord*)host_table)[i] = rec;
  return CT_OK;
}

int ct_nbr_radius_multi(const void* table, int n_clouds, const int64_t* cloud, const float* centres, int Q, float r, int K,
                        int64_t* idx, float* d2, int64_t* count, ct_stream_t s) {
  if (!table || ((uintptr_t)table & 7) != 0 || n_clouds < 1 || !cloud || !centres || !idx || !d2 || !count || Q < 1 || K < 1 ||
      K > kKMax || !(r >= 0.0f))
    return CT_EINVAL;
  hipStream_t st = (hipStream_t)s;
  CT_CLEAR_ERROR();
  const NbrTableSource src{(const NbrRecord*)table, n_clouds, cloud, centres};
  hipLaunchKernelGGL((nbr_radius_kernel<NbrTableSource, NbrNoEpilogue>), dim3(Q), dim3(kRadThreads), 0, st, src, 0, r, K, idx, d2,
                     count, NbrNoEpilogue{});
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

int ct_nbr_knn(const int32_t* cell_start, const float* sorted, const float* origin, float h, const int* dims,
               const float* queries, int64_t Q, int K, int64_t* idx, float* d2, ct_stream_t s) {
  long long ncells = 0;
  if (!cell_start || !sorted || !aligned16(sorted) || !queries || !idx || !d2 || Q < 1 || Q > kNearestMaxQ || K < 1 ||
      K > kKnnKMax || !grid_ok(origin, h, dims, &ncells))
    return CT_EINVAL;
  hipStream_t st = (hipStream_t)s;
  CT_CLEAR_ERROR();
  const NbrDirectSource src{(const float4*)sorted, cell_start, make_grid(origin, h, dims), queries};
  hipLaunchKernelGGL(nbr_knn_kernel<NbrDirectSource>, dim3((unsigned)((Q + kKnnWaves - 1) / kKnnWaves)), dim3(kKnnThreads), 0, st,
                     src, (long long)Q, K, idx, d2);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

int ct_nbr_knn_multi(const void* table, int n_clouds, const int64_t* cloud, const float* queries, int64_t Q, int K,
                     int64_t* idx, float* d2, ct_stream_t s) {
  if (!table || ((uintptr_t)table & 7) != 0 || n_clouds < 1 || !cloud || !queries || !idx || !d2 || Q < 1 || Q > kNearestMaxQ ||
      K < 1 || K > kKnnKMax)
    return CT_EINVAL;
  hipStream_t st = (hipStream_t)s;
  CT_CLEAR_ERROR();
  const NbrTableSource src{(const NbrRecord*)table, n_clouds, cloud, queries};
  hipLaunchKernelGGL(nbr_knn_kernel<NbrTableSource>, dim3((unsigned)((Q + kKnnWaves - 1) / kKnnWaves)), dim3(kKnnThreads), 0, st,
                     src, (long long)Q, K, idx, d2);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

int ct_nbr_interp(const int64_t* idx, const float* d2, int64_t Q, int K, const float* values, int64_t M, int C, float eps,
                  float* out, ct_stream_t s) {
  if (!idx || !d2 || !values || !out || Q < 1 || Q > kNearestMaxQ || K < 1 || K > kKnnKMax || M < 1 || C < 1 || !(eps >= 0.0f))
    return CT_EINVAL;
  hipStream_t st = (hipStream_t)s;
  CT_CLEAR_ERROR();
  const long long items = (long long)Q * ((C + kInterpCols - 1) / kInterpCols);
  const long long blocks = (items + 255) / 256;
  hipLaunchKernelGGL(nbr_interp_kernel, dim3((unsigned)(blocks < kInterpMaxBlocks ? blocks : kInterpMaxBlocks)), dim3(256), 0, st,
                     idx, d2, (long long)Q, K, values, C, eps, out);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

}  // extern "C"
