// Batch assembly of the ShapeNet completion items for gfx950 (utils/pcd_utils.py:24-51, `partial_postproces`, with the
// `2 *` of train_inpainter.py:180 folded in as `scale`) in one launch.
//
// A cloud's work is two exclusive scans of validity flags (one in row order, one in `perm` order) and a gather.  The
// scans are tiny (<= 16384 flags, 256 ballot words) and the outputs are not (noise is 4 * gt floats per cloud), so a
// cloud is given to G workgroups and EVERY one of them recomputes the flags and both scans from L2 into its own LDS;
// they then split the cloud's output: workgroup g writes the g-th slice of noise's columns and handles the g-th slice
// of `perm` positions / duplicate rows of part.  Nothing is published between workgroups, so there is no second launch,
// no flag to spin on and no ordering between them; the price is n_in * 20 bytes of L2 reads per workgroup.
//
//   flags     one ballot per 64 rows -> vmask[w]; pmask[w] = the same flags looked up through perm
//   scans     256 popcounts, one per thread: a wave scan by __shfl_up and four wave totals through LDS
//   rank      pre[w] + popc(mask[w] & lanes below)
//   select    cidx[k] = the k-th valid row (u16, LDS), written by every valid row at its rank
//
// The only arithmetic is `scale * x` (one fp32 multiply; the library is built with -ffp-contract=off), so with a power
// of two the result is a bit-exact rearrangement of the input.  Plain vector loads and stores only.
#include "ct_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / CT_WAVE;
constexpr int kNMax = 16384;                  // rows of one partial cloud: cidx is u16, the masks are 256 words
constexpr int kWords = kNMax / CT_WAVE;       // == kThreads: the scans take one word per thread
constexpr int kColsPerGroup = 1024;           // a workgroup gets at least this many columns of noise
constexpr int kGroupsTarget = 512;            // workgroups in flight the launch aims at (2 per CU)
static_assert(kWords == kThreads, "one ballot word per thread in the scans");

__device__ __forceinline__ int rank_below(unsigned long long m, int bit) { return __popcll(m & ((1ull << bit) - 1ull)); }

template <int VEC>
__global__ void __launch_bounds__(kThreads)
completion_items_kernel(const float* __restrict__ partial, const int64_t* __restrict__ perm, const float* __restrict__ u_dup,
                        const float* __restrict__ sphere, float scale, int n_in, int gt, int G, float* __restrict__ part,
                        float* __restrict__ noise, int32_t* __restrict__ count) {
  __shared__ unsigned long long vmask[kWords], pmask[kWords];
  __shared__ int vpre[kWords], ppre[kWords];
  __shared__ int wtot[2][kWaves];
  __shared__ unsigned short cidx[kNMax];
  const int b = blockIdx.y, g = blockIdx.x, t = threadIdx.x;
  const int lane = t & (CT_WAVE - 1), wave = t / CT_WAVE;
  const int NW = (n_in + CT_WAVE - 1) / CT_WAVE;
  const float* P = partial + (size_t)b * n_in * 3;
  const int64_t* PM = perm + (size_t)b * n_in;

  // validity of row i: ~(q == 0).all() of q = scale * partial[b, i] (IEEE ==: -0 is zero, NaN is not)
  for (int w = wave; w < NW; w += kWaves) {
    const int i = w * CT_WAVE + lane;
    bool ok = false;
    if (i < n_in) {
      const float x = scale * P[3 * i + 0], y = scale * P[3 * i + 1], z = scale * P[3 * i + 2];
      ok = !(x == 0.0f && y == 0.0f && z == 0.0f);
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) vmask[w] = m;
  }
  __syncthreads();
  // the same flags in perm order
  for (int w = wave; w < NW; w += kWaves) {
    const int j = w * CT_WAVE + lane;
    bool ok = false;
    if (j < n_in) {
      long long s = PM[j];
      s = s < 0 ? 0 : (s > n_in - 1 ? n_in - 1 : s);                  // a guard: an argsort's values are always in range
      ok = (vmask[s >> 6] >> (s & 63)) & 1ull;
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) pmask[w] = m;
  }
  __syncthreads();
  // exclusive scans of the words' popcounts, one word per thread
  const int cv = t < NW ? __popcll(vmask[t]) : 0, cp = t < NW ? __popcll(pmask[t]) : 0;
  int sv = cv, sp = cp;
  for (int d = 1; d < CT_WAVE; d <<= 1) {
    const int a = __shfl_up(sv, d), c = __shfl_up(sp, d);
    if (lane >= d) sv += a, sp += c;
  }
  if (lane == CT_WAVE - 1) wtot[0][wave] = sv, wtot[1][wave] = sp;
  __syncthreads();
  int ov = 0, op = 0, v = 0;
  for (int k = 0; k < kWaves; ++k) {
    if (k < wave) ov += wtot[0][k], op += wtot[1][k];
    v += wtot[0][k];
  }
  vpre[t] = ov + sv - cv;
  ppre[t] = op + sp - cp;
  __syncthreads();
  // select: the k-th valid row
  for (int w = wave; w < NW; w += kWaves) {
    const unsigned long long m = vmask[w];
    if ((m >> lane) & 1ull) cidx[vpre[w] + rank_below(m, lane)] = (unsigned short)(w * CT_WAVE + lane);
  }
  __syncthreads();
  if (g == 0 && t == 0) count[b] = v;

  // part: this workgroup's slice of perm positions (rows below v) and of duplicate rows (v and above)
  {
    const int chunk = (n_in + G - 1) / G;
    const int j0 = g * chunk, j1 = min(n_in, j0 + chunk);
    float* O = part + (size_t)b * n_in * 3;
    const float* U = u_dup + (size_t)b * n_in;
    for (int j = j0 + t; j < j1; j += kThreads) {
      const int w = j >> 6, bit = j & 63;
      const unsigned long long m = pmask[w];
      if ((m >> bit) & 1ull) {
        const int r = ppre[w] + rank_below(m, bit);
        if (r < v) {                                                  // (always, when perm is a permutation)
          long long s = PM[j];
          s = s < 0 ? 0 : (s > n_in - 1 ? n_in - 1 : s);
          O[3 * r + 0] = scale * P[3 * s + 0], O[3 * r + 1] = scale * P[3 * s + 1], O[3 * r + 2] = scale * P[3 * s + 2];
        }
      }
      if (j >= v) {
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (v > 0) {
          // k = clamp((int)floorf(u * (float)v), 0, v - 1); a NaN draw gives 0
          const float f = floorf(U[j] * (float)v);
          const int k = f >= (float)(v - 1) ? v - 1 : (f > 0.0f ? (int)f : 0);
          const int s = cidx[k];
          x = scale * P[3 * s + 0], y = scale * P[3 * s + 1], z = scale * P[3 * s + 2];
        }
        O[3 * j + 0] = x, O[3 * j + 1] = y, O[3 * j + 2] = z;
      }
    }
  }

  // noise: this workgroup's slice of columns, VEC at a time; sphere columns first, then the valid rows in row order
  {
    const int units = gt / VEC;                                       // (VEC == 4 only when gt % 4 == 0)
    const int chunk = (units + G - 1) / G;
    const int u0 = g * chunk, u1 = min(units, u0 + chunk);
    const int nz = gt - v;
    const float* S = sphere + (size_t)b * 3 * gt;
    float* N = noise + (size_t)b * 4 * gt;
    for (int u = u0 + t; u < u1; u += kThreads) {
      const int m0 = u * VEC;
      float val[4][VEC];
      if (m0 < nz) {
        for (int c = 0; c < 3; ++c) {
          if constexpr (VEC == 4) {
            const float4 q = *(const float4*)(S + (size_t)c * gt + m0);
            val[c][0] = q.x, val[c][1] = q.y, val[c][2] = q.z, val[c][3] = q.w;
          } else {
            val[c][0] = S[(size_t)c * gt + m0];
          }
        }
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const int m = m0 + e;
        val[3][e] = 0.0f;
        if (m >= nz) {
          const int s = cidx[m - nz];
          val[0][e] = scale * P[3 * s + 0], val[1][e] = scale * P[3 * s + 1], val[2][e] = scale * P[3 * s + 2];
          val[3][e] = 1.0f;
        }
      }
      for (int c = 0; c < 4; ++c) {
        if constexpr (VEC == 4) {
          *(float4*)(N + (size_t)c * gt + m0) = make_float4(val[c][0], val[c][1], val[c][2], val[c][3]);
        } else {
          N[(size_t)c * gt + m0] = val[c][0];
        }
      }
    }
  }
}

}  // namespace

extern "C" {

int ct_completion_items(const float* partial, const int64_t* perm, const float* u_dup, const float* sphere, float scale, int B,
                        int n_in, int64_t gt, float* part, float* noise, int32_t* count, ct_stream_t st) {
  if (!partial || !perm || !u_dup || !sphere || !part || !noise || !count) return CT_EINVAL;
  if (B < 1 || B > 65535 || n_in < 1 || n_in > kNMax || gt < (int64_t)n_in || gt > ((int64_t)1 << 24)) return CT_EINVAL;
  if (!(scale == scale) || scale == 0.0f || scale - scale != 0.0f) return CT_EINVAL;      // NaN, zero, +-inf
  const int gti = (int)gt;
  int G = (kGroupsTarget + B - 1) / B;
  const int most = (gti + kColsPerGroup - 1) / kColsPerGroup;
  G = G > most ? most : G;
  G = G < 1 ? 1 : G;
  // four columns per work-item when every row of sphere and noise starts on 16 bytes
  const bool vec = gti % 4 == 0 && ((uintptr_t)sphere % 16) == 0 && ((uintptr_t)noise % 16) == 0;
  CT_CLEAR_ERROR();
  if (vec)
    hipLaunchKernelGGL(completion_items_kernel<4>, dim3(G, B), dim3(kThreads), 0, (hipStream_t)st, partial, perm, u_dup, sphere,
                       scale, n_in, gti, G, part, noise, count);
  else
    hipLaunchKernelGGL(completion_items_kernel<1>, dim3(G, B), dim3(kThreads), 0, (hipStream_t)st, partial, perm, u_dup, sphere,
                       scale, n_in, gti, G, part, noise, count);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

}  // extern "C"
