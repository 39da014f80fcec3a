// Batch assembly of the ShapeNet completion items for gfx950 (utils/pcd_utils.py:24-51, `partial_postproces`, with the
// `2 *` of train_inpainter.py:180 folded in as `scale`) in one launch: ct_completion_items.  Further down, the items
// themselves gathered from a split that stays on the device: ct_completion_gather.
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

// ---------------------------------------------------------------------------------------------------------------------
// The items themselves, gathered from the split that stays on the device (datasets/grnet_completion.py: Dataset.__getitem__,
// the Compose chain of RandomSamplePoints and RandomMirrorPoints, collate_fn) in one launch: ct_completion_gather.
//
// The grid is (partial groups + gt groups, B).  blockIdx.x below the partial side's G works on out_partial[b], the rest on
// out_gt[b]; both sides run the same code on their own cloud, permutation, cap and slot count.  Every workgroup of a side
// recomputes the row's flags `perm[b, j] < length` (one ballot per 64 entries, <= 1024 words) up to the end of its slice of the
// positions j and their exclusive scan in its own LDS, then handles that slice: a flagged position of rank r < min(n, length)
// writes slot r.  The slots
// past the cloud's length are zero rows; they, and the whole row when there is no permutation (an in-order copy), are written
// as a flat range of floats, 16 bytes per work-item where the output row starts on 16 bytes.  Nothing is published between
// workgroups.  The arithmetic is a sign flip and, on the gt side, one multiply.
constexpr int kGatherCapMax = 1 << 16;                // entries of one permutation: 1024 ballot words
constexpr int kGatherWords = kGatherCapMax / CT_WAVE;
constexpr int kGatherWordsPerThread = kGatherWords / kThreads;
constexpr int kGatherInMax = 16384;                   // slots of out_partial (ct_completion_items' n_in)
constexpr int kGatherOutMax = 1 << 16;                // slots of out_gt
constexpr int kGatherSlotsPerGroup = 1024;            // a workgroup gets at least this many positions or slots
constexpr int kGatherGroupsMax = 32;                  // workgroups of one side of one row
constexpr int kGatherFlagWords = 4;                   // ballot words a wave takes per step of the flag pass
static_assert(kGatherWords % kThreads == 0, "the scan takes a whole number of words per thread");

struct GatherSide {
  const float* points;        // all clouds concatenated, f32[., 3]
  const int64_t* offsets;     // cloud c is points[offsets[c] .. offsets[c + 1])
  const int64_t* perm;        // i64[B, cap], or null: copy in order
  float* out;                 // f32[B, n, 3]
  float scale;
  int scaled;                 // multiply by scale (the gt side)
  int cap, n, G;
  int vec;                    // every output row starts on 16 bytes
};

__device__ __forceinline__ float gather_value(float v, int c, bool nx, bool nz, bool scaled, float scale) {
  if ((c == 0 && nx) || (c == 2 && nz)) v = -v;
  return scaled ? scale * v : v;
}

__global__ void __launch_bounds__(kThreads)
completion_gather_kernel(GatherSide pa, GatherSide gs, long long M, int R, const int64_t* __restrict__ item,
                         const int64_t* __restrict__ rendering, const float* __restrict__ u_mirror) {
  __shared__ unsigned long long pmask[kGatherWords];
  __shared__ int ppre[kGatherWords];
  __shared__ int wtot[kWaves];
  const int b = blockIdx.y, t = threadIdx.x;
  const int lane = t & (CT_WAVE - 1), wave = t / CT_WAVE;
  const bool is_gt = (int)blockIdx.x >= pa.G;
  const int grp = is_gt ? (int)blockIdx.x - pa.G : (int)blockIdx.x;
  const float* points = is_gt ? gs.points : pa.points;
  const int64_t* offsets = is_gt ? gs.offsets : pa.offsets;
  const int64_t* perm = is_gt ? gs.perm : pa.perm;
  float* out = is_gt ? gs.out : pa.out;
  const float scale = is_gt ? gs.scale : pa.scale;
  const bool scaled = (is_gt ? gs.scaled : pa.scaled) != 0;
  const int cap = is_gt ? gs.cap : pa.cap, n = is_gt ? gs.n : pa.n, G = is_gt ? gs.G : pa.G;
  const bool vec = (is_gt ? gs.vec : pa.vec) != 0;

  // the row's clouds; the clamps are guards, the sampler's indices are in range
  long long m = item[b];
  m = m < 0 ? 0 : (m > M - 1 ? M - 1 : m);
  long long r = rendering[b];
  r = r < 0 ? 0 : (r > R - 1 ? R - 1 : r);
  const long long c = is_gt ? m : m * R + r;
  const long long off = offsets[c];
  const long long len = offsets[c + 1] - off;
  const int L = (int)(len < 0 ? 0 : (len > cap ? cap : len));
  const int mm = min(n, L);
  const float* S = points + (size_t)off * 3;
  float* O = out + (size_t)b * 3 * n;
  bool nx = false, nz = false;
  if (u_mirror) {
    const float u = u_mirror[b];
    nx = u <= 0.5f;
    nz = u <= 0.25f || (0.5f < u && u <= 0.75f);
  }

  int lo = 0, copy_end = 3 * mm;                      // without a permutation: the whole row as a flat range
  if (perm) {
    // this group's slice of the perm positions; it needs the flags of its own positions and the count of those before them,
    // so it reads the row up to the end of its slice only (the first group 1 / G of it, the last all of it)
    const int chunk = (cap + G - 1) / G;
    const int j0 = min(cap, grp * chunk), j1 = min(cap, j0 + chunk);
    const int NW = j0 < j1 ? (j1 + CT_WAVE - 1) / CT_WAVE : 0;
    const int64_t* PM = perm + (size_t)b * cap;
    // flags in perm order: the entry names a point of this cloud
    // (kGatherFlagWords words per wave and step, their loads issued together)
    for (int w0 = wave * kGatherFlagWords; w0 < NW; w0 += kWaves * kGatherFlagWords) {
      long long s[kGatherFlagWords];
#pragma unroll
      for (int e = 0; e < kGatherFlagWords; ++e) {
        const int j = (w0 + e) * CT_WAVE + lane;
        s[e] = j < j1 ? PM[j] : -1;
      }
#pragma unroll
      for (int e = 0; e < kGatherFlagWords; ++e) {
        const unsigned long long mk = __ballot(s[e] >= 0 && s[e] < L);
        if (lane == 0 && w0 + e < NW) pmask[w0 + e] = mk;
      }
    }
    __syncthreads();
    // exclusive scan of the words' popcounts, kGatherWordsPerThread consecutive words per thread
    int cnt[kGatherWordsPerThread], tot = 0;
#pragma unroll
    for (int e = 0; e < kGatherWordsPerThread; ++e) {
      const int w = t * kGatherWordsPerThread + e;
      cnt[e] = w < NW ? __popcll(pmask[w]) : 0;
      tot += cnt[e];
    }
    int sc = tot;
    for (int d = 1; d < CT_WAVE; d <<= 1) {
      const int up = __shfl_up(sc, d);
      if (lane >= d) sc += up;
    }
    if (lane == CT_WAVE - 1) wtot[wave] = sc;
    __syncthreads();
    int before = sc - tot;
    for (int k = 0; k < wave; ++k) before += wtot[k];
#pragma unroll
    for (int e = 0; e < kGatherWordsPerThread; ++e) {
      const int w = t * kGatherWordsPerThread + e;
      if (w < NW) ppre[w] = before;
      before += cnt[e];
    }
    __syncthreads();
    // a flagged position of rank r < mm fills slot r
    for (int j = j0 + t; j < j1; j += kThreads) {
      const int w = j >> 6, bit = j & 63;
      const unsigned long long mk = pmask[w];
      if ((mk >> bit) & 1ull) {
        const int rk = ppre[w] + rank_below(mk, bit);
        if (rk < mm) {
          const long long s = PM[j];                  // (flagged: 0 <= s < L)
          O[3 * rk + 0] = gather_value(S[3 * s + 0], 0, nx, nz, scaled, scale);
          O[3 * rk + 1] = gather_value(S[3 * s + 1], 1, nx, nz, scaled, scale);
          O[3 * rk + 2] = gather_value(S[3 * s + 2], 2, nx, nz, scaled, scale);
        }
      }
    }
    lo = 3 * mm, copy_end = 0;                        // what is left: the zero rows
  }

  // the flat range [lo, 3 n) of the row: floats below copy_end come from the cloud in order, the rest are zeros
  {
    const int hi = 3 * n;
    const int V = vec ? 4 : 1;
    const int u_lo = lo / V, u_hi = (hi + V - 1) / V;
    const int chunk = (u_hi - u_lo + G - 1) / G;
    const int u0 = u_lo + grp * chunk, u1 = min(u_hi, u0 + chunk);
    for (int u = u0 + t; u < u1; u += kThreads) {
      const int i0 = u * V;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = i0 + e;
        v[e] = (e < V && i < copy_end) ? gather_value(S[i], i % 3, nx, nz, scaled, scale) : 0.0f;
      }
      if (V == 4 && i0 >= lo && i0 + 4 <= hi) {
        *(float4*)(O + i0) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < V && i0 + e >= lo && i0 + e < hi) O[i0 + e] = v[e];
      }
    }
  }
}

inline int gather_groups(int cap, int n) {
  const int most = cap > n ? cap : n;
  const int G = (most + kGatherSlotsPerGroup - 1) / kGatherSlotsPerGroup;
  return G > kGatherGroupsMax ? kGatherGroupsMax : (G < 1 ? 1 : G);
}

}  // namespace

extern "C" {

int ct_completion_gather(const float* partial_points, const int64_t* partial_offsets, const float* gt_points,
                         const int64_t* gt_offsets, int64_t M, int R, int p_cap, int g_cap, const int64_t* item,
                         const int64_t* rendering, const int64_t* perm_in, const int64_t* perm_gt, const float* u_mirror,
                         float gt_scale, int B, int n_in, int n_out, float* out_partial, float* out_gt, ct_stream_t st) {
  if (!partial_points || !partial_offsets || !gt_points || !gt_offsets || !item || !rendering || !perm_in || !out_partial || !out_gt)
    return CT_EINVAL;
  if (B < 1 || B > 65535 || R < 1 || M < 1 || M > INT64_MAX / R) return CT_EINVAL;
  if (n_in < 1 || n_in > kGatherInMax || n_out < 1 || n_out > kGatherOutMax) return CT_EINVAL;
  if (p_cap < 1 || p_cap > kGatherCapMax || g_cap < 1 || g_cap > kGatherCapMax) return CT_EINVAL;
  if (!(gt_scale == gt_scale) || gt_scale == 0.0f || gt_scale - gt_scale != 0.0f) return CT_EINVAL;      // NaN, zero, +-inf
  GatherSide pa, gs;
  pa.points = partial_points, pa.offsets = partial_offsets, pa.perm = perm_in, pa.out = out_partial;
  pa.scale = 1.0f, pa.scaled = 0, pa.cap = p_cap, pa.n = n_in, pa.G = gather_groups(p_cap, n_in);
  pa.vec = n_in % 4 == 0 && ((uintptr_t)out_partial % 16) == 0;
  gs.points = gt_points, gs.offsets = gt_offsets, gs.perm = perm_gt, gs.out = out_gt;
  gs.scale = gt_scale, gs.scaled = 1, gs.cap = g_cap, gs.n = n_out, gs.G = gather_groups(g_cap, n_out);
  gs.vec = n_out % 4 == 0 && ((uintptr_t)out_gt % 16) == 0;
  CT_CLEAR_ERROR();
  hipLaunchKernelGGL(completion_gather_kernel, dim3(pa.G + gs.G, B), dim3(kThreads), 0, (hipStream_t)st, pa, gs, (long long)M, R,
                     item, rendering, u_mirror);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

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
