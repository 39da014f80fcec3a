// Barycentre voxel-grid subsampling for gfx950 (KPConv's cpp_wrappers/cpp_subsampling, grid_subsampling.cpp:4-104, behind
// datasets/s3dis_closer.py:13-31): the device twin of csrc/host/grid_subsampling.cpp, held to the same rows in the same
// order with the same bits.
//
//   ct_voxel_bounds  the per-axis minimum and maximum of the points (two launches; a NaN point gives NaN bounds);
//   ct_voxel_keys    every point's cell key, in the host file's fp32 operation sequence (true divisions, no contraction);
//   (caller)         a stable ascending sort of the keys: keys_sorted, order;
//   ct_voxel_reduce  run-head flags -> multi-workgroup scan -> row numbers, run starts, inverse, M; then one wave per run.
//
// The one rule that makes the result equal to the host's and independent of the launch shape: the additions of one
// (voxel, column) happen in input order, from 0.0f.  A wave stages up to kRunPoints rows of its run into LDS with all
// lanes loading (the gathers through `order` are what the kernel waits for; their order is free), then lane k adds
// column k down the tile, one dependent add per point.  Classes are a maximum, so lanes stride the run and the wave
// folds.  A run is never split over waves: its length bounds the kernel's time (DESIGN, KPConv data table).
#include <limits.h>

#include "ct_nbr_query.h"

namespace {

constexpr int kScanThreads = 1024;
constexpr int kScanChunk = 4 * kScanThreads;   // elements per scan workgroup
constexpr int kRunPoints = 128;                // rows of a run staged per step: two gathers per lane in flight
constexpr int kRunCols = 8;                    // float columns (x y z, then features) summed per pass over a run
constexpr int kRunPitch = kRunCols + 1;        // odd pitch: a lane's row and a column's walk are both conflict-free
constexpr int kRunBlocks = 8192;               // 256 CUs x 32 one-wave workgroups, each looping over rows
constexpr unsigned long long kKeyBias = 1ull << 63;
constexpr float kMaxExtent = 4611686018427387904.0f;   // 2^62

struct VoxelGrid {       // the grid record (include/cloudct.h), 40 bytes
  float origin[3];
  int32_t status;
  int64_t n[3];
};
static_assert(sizeof(VoxelGrid) == 40, "ct_voxel_keys: grid record");

constexpr int kBoundsThreads = 256;
constexpr int kBoundsBlocks = 1024;            // partial bounds of the first pass (the workspace holds 6 floats of each)

// folds (lo[3], hi[3], nan) over the workgroup; valid in thread 0.  s: LDS float[7 * kBoundsThreads / CT_WAVE]
__device__ __forceinline__ void bounds_block_fold(float (&lo)[3], float (&hi)[3], int& nan, float* s) {
  const int lane = threadIdx.x & (CT_WAVE - 1), wave = threadIdx.x / CT_WAVE;
#pragma unroll
  for (int o = CT_WAVE / 2; o > 0; o >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, CT_WAVE));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, CT_WAVE));
    }
    nan |= __shfl_xor(nan, o, CT_WAVE);
  }
  if (lane == 0) {
    for (int a = 0; a < 3; ++a) s[7 * wave + a] = lo[a], s[7 * wave + 3 + a] = hi[a];
    s[7 * wave + 6] = nan ? 1.0f : 0.0f;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kBoundsThreads / CT_WAVE; ++w) {
      for (int a = 0; a < 3; ++a) lo[a] = fminf(lo[a], s[7 * w + a]), hi[a] = fmaxf(hi[a], s[7 * w + 3 + a]);
      nan |= s[7 * w + 6] != 0.0f;
    }
}

// fminf / fmaxf drop a NaN, so it is carried beside them and written back at the end: a NaN point gives NaN bounds
__device__ __forceinline__ void bounds_store(float* out, const float (&lo)[3], const float (&hi)[3], int nan) {
  for (int a = 0; a < 3; ++a) out[a] = nan ? NAN : lo[a], out[3 + a] = nan ? NAN : hi[a];
}

// pass 1: rows strided over the grid -> partial[6 * gridDim.x]; pass 2 (one workgroup): partial records -> bounds[6]
__global__ void __launch_bounds__(kBoundsThreads) voxel_bounds_kernel(const float* __restrict__ in, long long rows, float* __restrict__ out) {
  __shared__ float s[7 * kBoundsThreads / CT_WAVE];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int nan = 0;
  for (long long i = (long long)blockIdx.x * kBoundsThreads + threadIdx.x; i < rows; i += (long long)gridDim.x * kBoundsThreads) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = in[3 * i + a];
      lo[a] = fminf(lo[a], v), hi[a] = fmaxf(hi[a], v);
      nan |= v != v;
    }
  }
  bounds_block_fold(lo, hi, nan, s);
  if (threadIdx.x == 0) bounds_store(out + 6 * blockIdx.x, lo, hi, nan);
}

__global__ void __launch_bounds__(kBoundsThreads) voxel_bounds_fold_kernel(const float* __restrict__ partial, int n, float* __restrict__ out) {
  __shared__ float s[7 * kBoundsThreads / CT_WAVE];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int nan = 0;
  for (int i = threadIdx.x; i < n; i += kBoundsThreads) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float l = partial[6 * i + a], h = partial[6 * i + 3 + a];
      lo[a] = fminf(lo[a], l), hi[a] = fmaxf(hi[a], h);
      nan |= l != l;
    }
  }
  bounds_block_fold(lo, hi, nan, s);
  if (threadIdx.x == 0) bounds_store(out, lo, hi, nan);
}

int bounds_blocks(int64_t N) {
  const int64_t nb = (N + kBoundsThreads - 1) / kBoundsThreads;
  return (int)(nb < kBoundsBlocks ? nb : kBoundsBlocks);
}

__global__ void voxel_keys_kernel(const float* __restrict__ pts, long long N, float dl, float inv, const float* __restrict__ bounds,
                                  VoxelGrid* grid, long long* __restrict__ keys) {
  float org[3];
  unsigned long long n[3];
  int status = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = bounds[a], hi = bounds[3 + a];
    if (!(fabsf(lo) < INFINITY) || !(fabsf(hi) < INFINITY)) status = 1;
    org[a] = floorf(lo * inv) * dl;
    const float fl = floorf((hi - org[a]) / dl);
    n[a] = (unsigned long long)fminf(fmaxf(fl, 0.0f), kMaxExtent) + 1;   // fmaxf drops a NaN; the host checks status first
  }
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    for (int a = 0; a < 3; ++a) grid->origin[a] = org[a], grid->n[a] = (int64_t)n[a];
    grid->status = status;
  }
  if (i >= N) return;
  const float x = pts[3 * i + 0], y = pts[3 * i + 1], z = pts[3 * i + 2];
  // (size_t)floor(..) of the host file: a point a rounding below the origin wraps like its two's complement there
  const unsigned long long ix = (unsigned long long)(long long)floorf((x - org[0]) / dl);
  const unsigned long long iy = (unsigned long long)(long long)floorf((y - org[1]) / dl);
  const unsigned long long iz = (unsigned long long)(long long)floorf((z - org[2]) / dl);
  keys[i] = (long long)((ix + n[0] * iy + n[0] * n[1] * iz) ^ kKeyBias);
}

__device__ __forceinline__ unsigned voxel_head(const long long* __restrict__ ks, long long e, long long n) {
  return e < n && (e == 0 || ks[e] != ks[e - 1]) ? 1u : 0u;
}

// row[e] = (run heads in this workgroup's chunk up to and including e) - 1, still without the chunks before it
__global__ void __launch_bounds__(kScanThreads) voxel_scan_blocks_kernel(const long long* __restrict__ ks, long long n,
                                                                         unsigned* __restrict__ row, unsigned* __restrict__ bsum) {
  __shared__ unsigned s16[16], s_tot;
  const long long base = (long long)blockIdx.x * kScanChunk + 4 * threadIdx.x;
  unsigned v[4], sum = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    v[u] = voxel_head(ks, base + u, n);
    sum += v[u];
  }
  unsigned run = block_excl_scan(sum, s16, &s_tot);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    run += v[u];
    if (base + u < n) row[base + u] = run - 1u;
  }
  if (threadIdx.x == 0) bsum[blockIdx.x] = s_tot;
}

// exclusive scan of bsum[0, nb) in place, one workgroup walking it in chunks
__global__ void __launch_bounds__(kScanThreads) voxel_scan_sums_kernel(unsigned* bsum, int nb) {
  __shared__ unsigned s16[16], s_tot;
  unsigned carry = 0;
  for (long long base = 0; base < nb; base += kScanChunk) {
    unsigned v[4], sum = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long e = base + 4 * threadIdx.x + u;
      v[u] = e < nb ? bsum[e] : 0u;
      sum += v[u];
    }
    unsigned run = block_excl_scan(sum, s16, &s_tot) + carry;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long e = base + 4 * threadIdx.x + u;
      if (e < nb) bsum[e] = run;
      run += v[u];
    }
    carry += s_tot;
    __syncthreads();
  }
}

__device__ __forceinline__ long long voxel_point(const long long* __restrict__ order, long long e, long long n) {
  return min(max(order[e], 0LL), n - 1);   // a guard: a permutation never needs it
}

// finishes the row numbers; writes each run's first sorted position, the end sentinel, M and the optional inverse
__global__ void voxel_rows_kernel(const long long* __restrict__ ks, const long long* __restrict__ order, long long n,
                                  unsigned* __restrict__ row, const unsigned* __restrict__ bsum, unsigned* __restrict__ start,
                                  long long* __restrict__ inverse, long long* __restrict__ M) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const unsigned r = row[e] + bsum[e / kScanChunk];
  if (voxel_head(ks, e, n)) start[r] = (unsigned)e;
  if (inverse) inverse[voxel_point(order, e, n)] = r;
  if (e == n - 1) {
    start[r + 1] = (unsigned)n;
    *M = (long long)r + 1;
  }
}

// one wave per run (one-wave workgroups: the barriers below are the wave's own), looping over rows
__global__ void __launch_bounds__(CT_WAVE) voxel_reduce_kernel(const long long* __restrict__ order, const unsigned* __restrict__ start,
                                                               const long long* __restrict__ Mp, const float* __restrict__ points,
                                                               const float* __restrict__ features, const int* __restrict__ classes,
                                                               long long N, int F, int L, float* __restrict__ out_points,
                                                               float* __restrict__ out_features, int* __restrict__ out_classes,
                                                               long long* __restrict__ counts) {
  __shared__ float tile[kRunPoints * kRunPitch];
  const int lane = threadIdx.x;
  const long long M = *Mp;
  const int ncol = 3 + F;
  for (long long row = blockIdx.x; row < M; row += gridDim.x) {
    const long long s = start[row], e = start[row + 1];
    for (int c0 = 0; c0 < ncol; c0 += kRunCols) {
      const int nc = min(kRunCols, ncol - c0);
      float acc = 0.0f;
      for (long long b = s; b < e; b += kRunPoints) {
        const int m = (int)min((long long)kRunPoints, e - b);
#pragma unroll
        for (int u = 0; u < kRunPoints / CT_WAVE; ++u) {
          const int p = lane + CT_WAVE * u;
          if (p < m) {
            const long long i = voxel_point(order, b + p, N);
#pragma unroll
            for (int k = 0; k < kRunCols; ++k) {
              const int c = c0 + k;
              if (k < nc) tile[p * kRunPitch + k] = c < 3 ? points[3 * i + c] : features[i * F + (c - 3)];
            }
          }
        }
        __syncthreads();
        if (lane < nc) {
#pragma unroll 8
          for (int p = 0; p < m; ++p) acc += tile[p * kRunPitch + lane];   // input order: the sort is stable
        }
        __syncthreads();
      }
      if (lane < nc) {
        const int c = c0 + lane;
        if (c < 3)
          out_points[3 * row + c] = acc * (float)(1.0 / (double)(e - s));
        else
          out_features[row * F + (c - 3)] = acc / (float)(e - s);
      }
    }
    for (int l = 0; l < L; ++l) {
      int v = INT_MIN;
      for (long long q = s + lane; q < e; q += CT_WAVE) v = max(v, classes[voxel_point(order, q, N) * L + l]);
#pragma unroll
      for (int o = CT_WAVE / 2; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, CT_WAVE));
      if (lane == 0) out_classes[row * L + l] = v;
    }
    if (lane == 0 && counts) counts[row] = e - s;
  }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
long long scan_blocks(int64_t N) { return (N + kScanChunk - 1) / kScanChunk; }

}  // namespace

extern "C" {

size_t ct_voxel_reduce_workspace_bytes(int64_t N) {
  if (N < 1 || N > 0x7fffffffLL) return 0;
  return align256((size_t)N * 4) + align256(((size_t)N + 1) * 4) + align256((size_t)scan_blocks(N) * 4);
}

size_t ct_voxel_bounds_workspace_bytes(int64_t N) {
  if (N < 1 || N > 0x7fffffffLL) return 0;
  return (size_t)bounds_blocks(N) * 6 * sizeof(float);
}

int ct_voxel_bounds(const float* points, int64_t N, float* bounds, void* workspace, size_t workspace_bytes, ct_stream_t s) {
  if (!points || !bounds || N < 1 || N > 0x7fffffffLL) return CT_EINVAL;
  if (!workspace || ((uintptr_t)workspace & 3) != 0 || workspace_bytes < ct_voxel_bounds_workspace_bytes(N)) return CT_EWORKSPACE;
  hipStream_t st = (hipStream_t)s;
  const int nb = bounds_blocks(N);
  CT_CLEAR_ERROR();
  hipLaunchKernelGGL(voxel_bounds_kernel, dim3(nb), dim3(kBoundsThreads), 0, st, points, (long long)N, (float*)workspace);
  hipLaunchKernelGGL(voxel_bounds_fold_kernel, dim3(1), dim3(kBoundsThreads), 0, st, (const float*)workspace, nb, bounds);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

int ct_voxel_keys(const float* points, int64_t N, float dl, const float* bounds, void* grid, int64_t* keys, ct_stream_t s) {
  if (!points || !bounds || !grid || ((uintptr_t)grid & 7) != 0 || !keys || N < 1 || N > 0x7fffffffLL || !(dl > 0.0f) ||
      !(dl < INFINITY))
    return CT_EINVAL;
  hipStream_t st = (hipStream_t)s;
  const float inv = 1 / dl;
  CT_CLEAR_ERROR();
  hipLaunchKernelGGL(voxel_keys_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, points, (long long)N, dl, inv, bounds,
                     (VoxelGrid*)grid, (long long*)keys);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

int ct_voxel_reduce(const int64_t* keys_sorted, const int64_t* order, const float* points, const float* features,
                    const int32_t* classes, int64_t N, int fdim, int ldim, float* out_points, float* out_features,
                    int32_t* out_classes, int64_t* inverse, int64_t* counts, int64_t* M, void* workspace, size_t workspace_bytes,
                    ct_stream_t s) {
  if (!keys_sorted || !order || !points || !out_points || !M || N < 1 || N > 0x7fffffffLL || fdim < 0 || ldim < 0 ||
      (fdim > 0 && (!features || !out_features)) || (ldim > 0 && (!classes || !out_classes)))
    return CT_EINVAL;
  if (!workspace || workspace_bytes < ct_voxel_reduce_workspace_bytes(N)) return CT_EWORKSPACE;
  hipStream_t st = (hipStream_t)s;
  const long long n = N;
  const int nb = (int)scan_blocks(N);
  char* ws = (char*)workspace;
  unsigned* row = (unsigned*)ws;
  unsigned* start = (unsigned*)(ws + align256((size_t)N * 4));
  unsigned* bsum = (unsigned*)(ws + align256((size_t)N * 4) + align256(((size_t)N + 1) * 4));
  CT_CLEAR_ERROR();
  hipLaunchKernelGGL(voxel_scan_blocks_kernel, dim3(nb), dim3(kScanThreads), 0, st, (const long long*)keys_sorted, n, row, bsum);
  hipLaunchKernelGGL(voxel_scan_sums_kernel, dim3(1), dim3(kScanThreads), 0, st, bsum, nb);
  hipLaunchKernelGGL(voxel_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const long long*)keys_sorted,
                     (const long long*)order, n, row, (const unsigned*)bsum, start, (long long*)inverse, (long long*)M);
  hipLaunchKernelGGL(voxel_reduce_kernel, dim3((unsigned)(n < kRunBlocks ? n : kRunBlocks)), dim3(CT_WAVE), 0, st,
                     (const long long*)order, (const unsigned*)start, (const long long*)M, points, features, classes, n, fdim, ldim,
                     out_points, out_features, out_classes, (long long*)counts);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

}  // extern "C"
