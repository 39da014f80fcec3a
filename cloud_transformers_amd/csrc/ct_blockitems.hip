// The S3DIS 1x1 m block protocol on gfx950 (datasets/s3dis_v2.py:537-560 with the collate and the `permute` of
// train_segmentation.py:180 folded in; train_segmentation.py:198-205 for the confusion matrix).
//
// ct_block_items   one batch in one launch: a gather of B blocks' first N points out of the resident split, the shuffle, the
//                  eight transforms of the loader on explicit draws, written channels first.  The only stage that is not per
//                  point is the auto-contrast's per-channel min / max over the block's N pool points: every workgroup of a
//                  block whose draw takes the stage (one in five) recomputes them itself from L2 (N <= 16384 rows of 24
//                  bytes), as ct_completion_items recomputes its scans — no second launch, no workspace, no float atomics.
//                  The reduction runs on order-preserving integer keys of the floats, so it is exact and does not depend on
//                  the order of the lanes (-0 sorts below +0).
//                  VEC 4: a work-item takes four consecutive slots: one 16-byte store per channel row, two for the labels,
//                  the two jitters as three 16-byte loads each, the source rows as three 8-byte loads.  Needs N % 4 == 0 and
//                  16-byte addressable outputs and jitters.  VEC 1: everything else, scalar accesses.
// ct_seg_confusion one pass over pred[B,C,N]: a work-item per point walks the C rows (coalesced along N), the counts go to
//                  per-workgroup LDS bins and from there with one 64-bit integer atomic per non-empty bin into conf.
//
// Arithmetic (-ffp-contract=off): every operation below is one fp32 rounding, in the order include/cloudct.h states.
#include "ct_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / CT_WAVE;
constexpr int kPMax = 16384;
constexpr int kCMax = 64;

// float <-> unsigned key with the floats' order (-0 < +0; NaNs at the two ends)
__device__ __forceinline__ uint32_t order_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// np.remainder(x, 1) in fp32: x - trunc(x) is fmod(x, 1), exactly; a negative remainder takes + 1 (one rounding)
__device__ __forceinline__ float rem1(float x) {
  float m = x - truncf(x);
  if (m != 0.0f) {
    if (m < 0.0f) m += 1.0f;
  } else {
    m = 0.0f;
  }
  return m;
}

__device__ __forceinline__ float level(float v) { return (float)(int)fminf(fmaxf(v, 0.0f), 255.0f) / 255.0f; }

// the eight transforms on one row v = (x, y, z, r, g, b); A: the block's 16 draws, j / cj: the slot's two jitters
__device__ __forceinline__ void augment(float (&v)[6], const float* __restrict__ A, const float (&j)[3], const float (&cj)[3],
                                        bool contrast, const float (&lo)[3], const float (&hi)[3], float sigma, float clip,
                                        float cstd) {
  const float c = A[0], s = A[1];
  const float x = (v[0] * c) - (v[1] * s), y = (v[0] * s) + (v[1] * c);
  v[0] = x, v[1] = y;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    v[i] = v[i] * A[2 + i];
    v[i] = v[i] + fminf(fmaxf(sigma * j[i], -clip), clip);
  }
  if (contrast) {
    const float w = A[5], u = 1.0f - w;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (hi[i] != lo[i]) {
        const float st = (v[3 + i] - lo[i]) * (1.0f / (hi[i] - lo[i]));
        v[3 + i] = (u * v[3 + i]) + (w * st);
      }
    }
  }
  if (A[9] != 0.0f) {
#pragma unroll
    for (int i = 0; i < 3; ++i) v[3 + i] = clip01(A[6 + i] + v[3 + i]);
  }
  if (A[10] != 0.0f) {
#pragma unroll
    for (int i = 0; i < 3; ++i) v[3 + i] = clip01((cj[i] * cstd) + v[3 + i]);
  }
  // hue / saturation through HSV on the 0..255 scale (data.datasets.HueSaturationTranslation)
  const float r = v[3] * 255.0f, g = v[4] * 255.0f, b = v[5] * 255.0f;
  const float mx = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b);
  const float span = mx - mn;
  const bool grey = span == 0.0f;
  float h = 0.0f, sat = 0.0f;
  if (!grey) {
    const float rc = (mx - r) / span, gc = (mx - g) / span, bc = (mx - b) / span;
    h = r == mx ? bc - gc : (g == mx ? (2.0f + rc) - bc : (4.0f + gc) - rc);
    sat = span / (mx == 0.0f ? 1.0f : mx);
  }
  h = rem1(h / 6.0f);
  h = rem1((A[11] + h) + 1.0f);
  sat = clip01(A[12] * sat);
  const float h6 = h * 6.0f;
  int sector = (int)h6;
  const float f = h6 - (float)sector;
  const float p = mx * (1.0f - sat), q = mx * (1.0f - (sat * f)), t = mx * (1.0f - (sat * (1.0f - f)));
  sector %= 6;
  float R = mx, G = t, Bl = p;                                            // sector 0
  if (sat == 0.0f) {
    R = mx, G = mx, Bl = mx;
  } else if (sector == 1) {
    R = q, G = mx, Bl = p;
  } else if (sector == 2) {
    R = p, G = mx, Bl = t;
  } else if (sector == 3) {
    R = p, G = q, Bl = mx;
  } else if (sector == 4) {
    R = t, G = p, Bl = mx;
  } else if (sector == 5) {
    R = mx, G = p, Bl = q;
  }
  v[3] = level(R), v[4] = level(G), v[5] = level(Bl);
}

template <int VEC>
__global__ void __launch_bounds__(kThreads)
block_items_kernel(const float* __restrict__ data, const uint8_t* __restrict__ label, int64_t M, int P,
                   const int64_t* __restrict__ item, const int64_t* __restrict__ perm, const float* __restrict__ aug,
                   const float* __restrict__ jit, const float* __restrict__ cjit, float sigma, float clip, float cstd, int N,
                   float* __restrict__ out, int64_t* __restrict__ out_label) {
  static_assert(VEC == 1 || VEC == 4, "one slot or four");
  __shared__ uint32_t red[6][kWaves];
  const int b = blockIdx.y;
  long long g = item[b];
  g = g < 0 ? 0 : (g > M - 1 ? M - 1 : g);                              // a guard: the sampler's indices are in range
  const float* D = data + (size_t)g * P * 6;
  const uint8_t* L = label + (size_t)g * P;
  const float* A = aug ? aug + (size_t)b * 16 : nullptr;

  // the auto-contrast's bounds: uniform over the workgroup (they hang on b alone), so the barrier is reached by all or none
  float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
  const bool contrast = A != nullptr && A[5] >= 0.0f;
  if (contrast) {
    uint32_t klo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, khi[3] = {0u, 0u, 0u};
    for (int n = threadIdx.x; n < N; n += kThreads) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const uint32_t k = order_key(D[(size_t)n * 6 + 3 + i]);
        klo[i] = min(klo[i], k), khi[i] = max(khi[i], k);
      }
    }
#pragma unroll
    for (int off = CT_WAVE / 2; off > 0; off >>= 1) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        klo[i] = min(klo[i], (uint32_t)__shfl_xor((unsigned int)klo[i], off, CT_WAVE));
        khi[i] = max(khi[i], (uint32_t)__shfl_xor((unsigned int)khi[i], off, CT_WAVE));
      }
    }
    if ((threadIdx.x & (CT_WAVE - 1)) == 0) {
#pragma unroll
      for (int i = 0; i < 3; ++i) red[i][threadIdx.x / CT_WAVE] = klo[i], red[3 + i][threadIdx.x / CT_WAVE] = khi[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      uint32_t a = red[i][0], c = red[3 + i][0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) a = min(a, red[i][w]), c = max(c, red[3 + i][w]);
      lo[i] = order_unkey(a), hi[i] = order_unkey(c);
    }
  }

  const int n0 = (blockIdx.x * kThreads + threadIdx.x) * VEC;
  if (n0 >= N) return;                                                  // (VEC 4: N % 4 == 0, so n0 + 3 < N)

  float v[VEC][6];
  long long lab[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    int src = n0 + k;
    if (perm) {
      const long long s = perm[(size_t)b * N + n0 + k];
      src = (int)(s < 0 ? 0 : (s > N - 1 ? N - 1 : s));                 // a guard: a permutation's values are in range
    }
    const float* R = D + (size_t)src * 6;
    if constexpr (VEC == 4) {                                           // (rows are 24 bytes: 8-byte addressable with data)
      const float2 a = *(const float2*)R, c = *(const float2*)(R + 2), e = *(const float2*)(R + 4);
      v[k][0] = a.x, v[k][1] = a.y, v[k][2] = c.x, v[k][3] = c.y, v[k][4] = e.x, v[k][5] = e.y;
    } else {
#pragma unroll
      for (int i = 0; i < 6; ++i) v[k][i] = R[i];
    }
    lab[k] = (long long)L[src];
  }

  if (A) {                                                              // (jit and cjit are given with it: the entry point checks)
    const float* J = jit + ((size_t)b * N + n0) * 3;
    const float* CJ = cjit + ((size_t)b * N + n0) * 3;
    float j[VEC][3], cj[VEC][3];
    if constexpr (VEC == 4) {
      float4 a = *(const float4*)J, c = *(const float4*)(J + 4), e = *(const float4*)(J + 8);
      j[0][0] = a.x, j[0][1] = a.y, j[0][2] = a.z, j[1][0] = a.w, j[1][1] = c.x, j[1][2] = c.y;
      j[2][0] = c.z, j[2][1] = c.w, j[2][2] = e.x, j[3][0] = e.y, j[3][1] = e.z, j[3][2] = e.w;
      a = *(const float4*)CJ, c = *(const float4*)(CJ + 4), e = *(const float4*)(CJ + 8);
      cj[0][0] = a.x, cj[0][1] = a.y, cj[0][2] = a.z, cj[1][0] = a.w, cj[1][1] = c.x, cj[1][2] = c.y;
      cj[2][0] = c.z, cj[2][1] = c.w, cj[2][2] = e.x, cj[3][0] = e.y, cj[3][1] = e.z, cj[3][2] = e.w;
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) j[0][i] = J[i], cj[0][i] = CJ[i];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) augment(v[k], A, j[k], cj[k], contrast, lo, hi, sigma, clip, cstd);
  }

  float* O = out + (size_t)b * 6 * N + n0;
  long long* Q = (long long*)out_label + (size_t)b * N + n0;
  if constexpr (VEC == 4) {
#pragma unroll
    for (int ch = 0; ch < 6; ++ch) *(float4*)(O + (size_t)ch * N) = make_float4(v[0][ch], v[1][ch], v[2][ch], v[3][ch]);
    *(longlong2*)Q = make_longlong2(lab[0], lab[1]);
    *(longlong2*)(Q + 2) = make_longlong2(lab[2], lab[3]);
  } else {
#pragma unroll
    for (int ch = 0; ch < 6; ++ch) O[(size_t)ch * N] = v[0][ch];
    Q[0] = lab[0];
  }
}

__global__ void __launch_bounds__(kThreads)
seg_confusion_kernel(const float* __restrict__ pred, const int64_t* __restrict__ labels, int C, int N, long long total,
                     unsigned long long* __restrict__ conf) {
  __shared__ unsigned int bins[kCMax * kCMax];
  const int cells = C * C;
  for (int k = threadIdx.x; k < cells; k += kThreads) bins[k] = 0u;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const long long b = i / N;
    const int n = (int)(i - b * N);
    const float* X = pred + ((size_t)b * C) * N + n;
    // np.argmax: the first index of the maximum, a NaN counting as the maximum (the first NaN wins)
    float best = X[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
      const float x = X[(size_t)c * N];
      if (best == best && (x > best || x != x)) best = x, arg = c;
    }
    const long long t = labels[i];
    if (t >= 0 && t < C) atomicAdd(&bins[(int)t * C + arg], 1u);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < cells; k += kThreads) {
    const unsigned int c = bins[k];
    if (c != 0u) atomicAdd(&conf[k], (unsigned long long)c);
  }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }
inline bool finite(float v) { return v - v == 0.0f; }

}  // namespace

extern "C" {

int ct_block_items(const float* data, const uint8_t* label, int64_t M, int P, const int64_t* item, const int64_t* perm,
                   const float* aug, const float* jit, const float* cjit, float sigma, float clip, float cstd, int B, int N,
                   float* out, int64_t* out_label, ct_stream_t st) {
  if (!data || !label || !item || !out || !out_label) return CT_EINVAL;
  if ((aug == nullptr) != (jit == nullptr) || (aug == nullptr) != (cjit == nullptr)) return CT_EINVAL;
  if (B < 1 || B > 65535 || N < 1 || P < N || P > kPMax || M < 1) return CT_EINVAL;
  if (!(clip > 0.0f) || !finite(sigma) || !finite(cstd)) return CT_EINVAL;      // clip <= 0 or NaN; sigma, cstd NaN or +-inf
  // four slots per work-item when every output row and jitter row starts on 16 bytes (and the 24-byte source rows on 8)
  const bool vec = N % 4 == 0 && aligned(out, 16) && aligned(out_label, 16) && aligned(data, 8) &&
                   (!aug || (aligned(jit, 16) && aligned(cjit, 16)));
  const int units = vec ? N / 4 : N;
  const dim3 grid((units + kThreads - 1) / kThreads, B), block(kThreads);
  CT_CLEAR_ERROR();
  if (vec)
    hipLaunchKernelGGL((block_items_kernel<4>), grid, block, 0, (hipStream_t)st, data, label, M, P, item, perm, aug, jit, cjit,
                       sigma, clip, cstd, N, out, out_label);
  else
    hipLaunchKernelGGL((block_items_kernel<1>), grid, block, 0, (hipStream_t)st, data, label, M, P, item, perm, aug, jit, cjit,
                       sigma, clip, cstd, N, out, out_label);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

int ct_seg_confusion(const float* pred, const int64_t* labels, int B, int C, int N, int64_t* conf, ct_stream_t st) {
  if (!pred || !labels || !conf) return CT_EINVAL;
  if (B < 1 || N < 1 || C < 1 || C > kCMax) return CT_EINVAL;
  const long long total = (long long)B * N;
  if (total > 0x7fffffffLL) return CT_EINVAL;                           // (a workgroup's 32-bit LDS bins cannot overflow)
  // enough workgroups to fill the device, few enough that the flushes (<= C * C atomics each) stay a small part
  const long long want = (total + kThreads - 1) / kThreads;
  const dim3 grid((unsigned)(want < 1024 ? want : 1024)), block(kThreads);
  CT_CLEAR_ERROR();
  hipLaunchKernelGGL(seg_confusion_kernel, grid, block, 0, (hipStream_t)st, pred, labels, C, N, total,
                     (unsigned long long*)conf);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

}  // extern "C"
