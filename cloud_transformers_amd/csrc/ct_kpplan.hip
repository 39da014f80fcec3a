// The epoch plan of the S3DIS KPConv sampler for gfx950 (datasets/s3dis_closer.py:247-276, the potential-field picking of
// S3DISSeg) as a device procedure: n picks enqueued by one call, no value read back by the host in between.
//
// begin:  every cloud's (min, lowest argmin) of its potentials, recomputed from the buffers as they are, and pick 0.
// pick i: query — the table-driven radius workgroup of ct_nbr_query.h at picks[i] in cloud[i]; the work-item that holds a kept
//                 (d2, index) key adds its Tukey weight to that point's potential (the indices of one ball are distinct and
//                 one query runs at a time: a plain read-modify-write);
//         step  — the (min, lowest argmin) of cloud[i]'s potentials over several workgroups; the workgroup that arrives
//                 last folds the partials, writes min_potentials[cloud[i]], chooses the next cloud from the minima and that
//                 cloud's cached argmin (a cloud's potentials change only when it is picked), and writes pick i + 1.
// Kernel boundaries order the picks; no workgroup waits for another.  Every float expression is the one the torch sequence
// it replaces evaluates, built with -ffp-contract=off: results are equal bit for bit.
#include "ct_nbr_query.h"

namespace {

constexpr int kStepThreads = 256;
constexpr int kStepWaves = kStepThreads / CT_WAVE;
constexpr int kStepBlocksMax = 256;   // the last workgroup folds one partial per work-item
constexpr int kStepSpan = 4096;       // points per workgroup the grid is sized for
constexpr int kCloudsMax = 65535;     // begin: one grid row per cloud

// torch: pot.index_add_(0, idx, square(1 - d2 / (r * r))), the division by a Python number being a multiplication by
// its fp32 reciprocal
struct KpTukey {
  static constexpr bool kStore = false;
  float* pot;
  float inv;
  __device__ __forceinline__ void operator()(const NbrQuery& qy, unsigned long long key) const {
    const float d2 = __uint_as_float((unsigned)(key >> 32));
    const float t = 1.0f - d2 * inv;
    float* p = pot + qy.offset + (long long)(unsigned)(key & 0xffffffffu);
    *p = *p + t * t;
  }
};

// (value, index) ascending: the minimum with the lowest index; a NaN never wins
__device__ __forceinline__ bool kp_before(float v, int i, float bv, int bi) { return v < bv || (v == bv && i < bi); }

__device__ __forceinline__ unsigned long long kp_pack(float v, int i) {
  return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)i;
}

// the workgroup's best (value, index), valid in work-item 0
__device__ __forceinline__ void kp_block_min(float& bv, int& bi, float* s_v, int* s_i) {
#pragma unroll
  for (int off = CT_WAVE / 2; off > 0; off >>= 1) {
    const float ov = __shfl_down(bv, off, CT_WAVE);
    const int oi = __shfl_down(bi, off, CT_WAVE);
    if (kp_before(ov, oi, bv, bi)) bv = ov, bi = oi;
  }
  if ((threadIdx.x & (CT_WAVE - 1)) == 0) s_v[threadIdx.x / CT_WAVE] = bv, s_i[threadIdx.x / CT_WAVE] = bi;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kStepWaves; ++w)
      if (kp_before(s_v[w], s_i[w], bv, bi)) bv = s_v[w], bi = s_i[w];
  }
  __syncthreads();
}

// i < 0: begin, grid (blocks, n_clouds), row y reduces cloud y.  i >= 0: the step after pick i, grid (blocks, 1), reduces
// cloud[i].  Partials and ticket follow the arrival pattern of occupancy_ratio_kernel (ct_raster.hip): agent-scope stores,
// drained before the ticket is taken; the last arriver hands the ticket back as zero and acquires before it reads them.
__global__ void __launch_bounds__(kStepThreads)
kp_plan_step_kernel(const NbrRecord* __restrict__ table, int n_clouds, const float* __restrict__ points,
                    const float* __restrict__ pot, float* __restrict__ min_pot, const float* __restrict__ noise, int i, int n,
                    int64_t* __restrict__ cloud, int64_t* __restrict__ point, float* __restrict__ picks, unsigned* ticket,
                    long long* __restrict__ arg, unsigned long long* partial) {
  __shared__ float s_v[kStepWaves];
  __shared__ int s_i[kStepWaves];
  __shared__ unsigned s_last;
  const bool begin = i < 0;
  const int tid = threadIdx.x;
  int c = blockIdx.y;
  if (!begin) {
    const long long ci = cloud[i];
    c = (int)(ci < 0 ? 0 : (ci > n_clouds - 1 ? n_clouds - 1 : ci));
  }
  const int M = table[c].M;
  const float* __restrict__ base = pot + table[c].offset;
  float bv = __builtin_inff();
  int bi = 0x7fffffff;
  const long long stride = (long long)gridDim.x * kStepThreads;
  for (long long j = (long long)blockIdx.x * kStepThreads + tid; j < M; j += stride) {
    const float v = base[j];
    if (kp_before(v, (int)j, bv, bi)) bv = v, bi = (int)j;
  }
  kp_block_min(bv, bi, s_v, s_i);
  if (tid == 0) {
    __hip_atomic_store(partial + (size_t)blockIdx.y * gridDim.x + blockIdx.x, kp_pack(bv, bi), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the partial has left before the ticket is taken
    const unsigned total = gridDim.x * gridDim.y;
    const unsigned old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = old == total - 1u;
    if (old == total - 1u) {
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!s_last) return;      // block-uniform: only the workgroup that arrived last goes on

  for (int y = 0; y < (int)gridDim.y; ++y) {
    float fv = __builtin_inff();
    int fi = 0x7fffffff;
    if (tid < (int)gridDim.x) {
      const unsigned long long k =
          __hip_atomic_load(partial + (size_t)y * gridDim.x + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      fv = __uint_as_float((unsigned)(k >> 32)), fi = (int)(unsigned)(k & 0xffffffffu);
    }
    kp_block_min(fv, fi, s_v, s_i);
    if (tid == 0) {
      const int cy = begin ? y : c;
      min_pot[cy] = fv;
      arg[cy] = fi;
    }
  }
  const int next = i + 1;
  if (tid != 0 || next >= n) return;
  int cn = 0;
  float mv = min_pot[0];
  for (int k = 1; k < n_clouds; ++k) {
    const float v = min_pot[k];
    if (v < mv) mv = v, cn = k;
  }
  long long pn = arg[cn];
  const long long Mn = table[cn].M;
  pn = pn < 0 ? 0 : (pn > Mn - 1 ? Mn - 1 : pn);      // a guard: an argmin is always in range
  const long long g = table[cn].offset + pn;
  cloud[next] = cn;
  point[next] = pn;
#pragma unroll
  for (int a = 0; a < 3; ++a) picks[3 * (size_t)next + a] = points[3 * g + a] + noise[3 * (size_t)next + a];
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int step_blocks(int64_t max_points) {
  const int64_t b = (max_points + kStepSpan - 1) / kStepSpan;
  return (int)(b < 1 ? 1 : (b > kStepBlocksMax ? kStepBlocksMax : b));
}

}  // namespace

extern "C" {

size_t ct_kp_plan_workspace_bytes(int n_clouds, int64_t max_points) {
  if (n_clouds < 1 || n_clouds > kCloudsMax || max_points < 1 || max_points > 0x7fffffffLL) return 0;
  return 256 + align256((size_t)n_clouds * 8) + align256((size_t)n_clouds * step_blocks(max_points) * 8);
}

int ct_kp_plan(const void* table, int n_clouds, int64_t max_points, const float* points, float* potentials,
               float* min_potentials, const float* noise, double r, int K, int n, int64_t* cloud, int64_t* point, float* picks,
               void* workspace, size_t workspace_bytes, ct_stream_t s) {
  if (!table || ((uintptr_t)table & 7) != 0 || !points || !potentials || !min_potentials || !noise || !cloud || !point ||
      !picks || n_clouds < 1 || n_clouds > kCloudsMax || max_points < 1 || max_points > 0x7fffffffLL || n < 1 || K < 1 ||
      K > kKMax || !(r >= 0.0) || !__builtin_isfinite(r))
    return CT_EINVAL;
  if (!workspace || ((uintptr_t)workspace & 7) != 0 || workspace_bytes < ct_kp_plan_workspace_bytes(n_clouds, max_points))
    return CT_EWORKSPACE;
  hipStream_t st = (hipStream_t)s;
  const int nblk = step_blocks(max_points);
  char* ws = (char*)workspace;
  unsigned* ticket = (unsigned*)ws;
  long long* arg = (long long*)(ws + 256);
  unsigned long long* partial = (unsigned long long*)(ws + 256 + align256((size_t)n_clouds * 8));
  const NbrRecord* tab = (const NbrRecord*)table;
  const float rf = (float)r;                    // the radius the query is given
  const float inv = 1.0f / (float)(r * r);      // torch: d2 / (r * r) with r a Python number
  if (hipMemsetAsync(ticket, 0, 4, st) != hipSuccess) return CT_ELAUNCH;
  CT_CLEAR_ERROR();
  hipLaunchKernelGGL(kp_plan_step_kernel, dim3(nblk, n_clouds), dim3(kStepThreads), 0, st, tab, n_clouds, points,
                     (const float*)potentials, min_potentials, noise, -1, n, cloud, point, picks, ticket, arg, partial);
  const NbrTableSource src{tab, n_clouds, cloud, picks};
  const KpTukey tukey{potentials, inv};
  for (int i = 0; i < n; ++i) {
    hipLaunchKernelGGL((nbr_radius_kernel<NbrTableSource, KpTukey>), dim3(1), dim3(kRadThreads), 0, st, src, i, rf, K,
                       (int64_t*)nullptr, (float*)nullptr, (int64_t*)nullptr, tukey);
    hipLaunchKernelGGL(kp_plan_step_kernel, dim3(nblk, 1), dim3(kStepThreads), 0, st, tab, n_clouds, points,
                       (const float*)potentials, min_potentials, noise, i, n, cloud, point, picks, ticket, arg, partial);
  }
  CT_CHECK_LAUNCH();
  return CT_OK;
}

}  // extern "C"
