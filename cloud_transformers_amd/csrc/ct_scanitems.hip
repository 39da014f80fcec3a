// Batch assembly of the ScanObjectNN classification items for gfx950 (datasets/scanobjectnn.py:102-122 with the collate and
// the `permute` of train_classification.py:195 folded in) in one launch: a gather of B clouds out of the resident split,
// the optional subsample, jitter and rotation about y, written channels first.
//
// A gather with a transposing write and nothing else: no LDS, no atomics, no barrier, so a workgroup is one wave and the
// launch is a flat grid of them (blockIdx.y = the batch row).  At the protocol's B 8 / N 2048 it is launch-bound; the
// narrow groups spread its 64 waves over as many CUs instead of stacking them on 16.
//
//   VEC 4   a work-item takes four consecutive slots of one cloud: one 16-byte store per channel row and one for the
//           mask (64 lanes x 16 B = 1 KiB per store instruction, contiguous), the jitter as three 16-byte loads.
//           Needs N % 4 == 0 and 16-byte addressable output and jitter rows.
//   WIDE    (VEC 4, no perm) the four source rows are 48 contiguous bytes: three 16-byte loads, and the four mask
//           bytes one 4-byte load.  Needs P % 4 == 0 as well, so that every cloud's rows start on 16 bytes.
//   VEC 1   everything else, one slot per work-item, scalar accesses.
//
// Arithmetic (-ffp-contract=off, each operation one fp32 rounding): d = min(max(sigma * j, -clip), clip); q = p + d;
// x' = (q.x * c) - (q.z * s); y' = q.y; z' = (q.x * s) + (q.z * c).
#include "ct_common.h"

namespace {

constexpr int kThreads = CT_WAVE;
constexpr int kPMax = 16384;

__device__ __forceinline__ float jitter(float p, float j, float sigma, float clip) {
  return p + fminf(fmaxf(sigma * j, -clip), clip);
}

template <int VEC, bool WIDE>
__global__ void __launch_bounds__(kThreads)
scan_items_kernel(const float* __restrict__ data, const uint8_t* __restrict__ mask, const int64_t* __restrict__ label, int64_t M,
                  int P, const int64_t* __restrict__ item, const int64_t* __restrict__ perm, const float* __restrict__ rot,
                  const float* __restrict__ jit, float sigma, float clip, int N, float* __restrict__ out_points,
                  float* __restrict__ out_mask, int64_t* __restrict__ out_label) {
  static_assert(VEC == 1 || VEC == 4, "one slot or four");
  static_assert(!WIDE || VEC == 4, "the wide read belongs to the vector path");
  const int b = blockIdx.y;
  const int u = blockIdx.x * kThreads + threadIdx.x;
  long long g = item[b];
  g = g < 0 ? 0 : (g > M - 1 ? M - 1 : g);                              // a guard: the sampler's indices are in range
  if (u == 0) out_label[b] = label[g];
  const int n0 = u * VEC;
  if (n0 >= N) return;                                                  // (VEC 4: N % 4 == 0, so n0 + 3 < N)
  const float* D = data + (size_t)g * P * 3;
  const uint8_t* K = mask + (size_t)g * P;

  float p[VEC][3], m[VEC];
  if constexpr (WIDE) {
    const float4 a = *(const float4*)(D + (size_t)n0 * 3), c = *(const float4*)(D + (size_t)n0 * 3 + 4),
                 e = *(const float4*)(D + (size_t)n0 * 3 + 8);
    p[0][0] = a.x, p[0][1] = a.y, p[0][2] = a.z, p[1][0] = a.w, p[1][1] = c.x, p[1][2] = c.y;
    p[2][0] = c.z, p[2][1] = c.w, p[2][2] = e.x, p[3][0] = e.y, p[3][1] = e.z, p[3][2] = e.w;
    const uint32_t w = *(const uint32_t*)(K + n0);
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = (float)((w >> (8 * k)) & 0xffu);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      int src = n0 + k;
      if (perm) {
        long long s = perm[(size_t)b * P + n0 + k];
        src = (int)(s < 0 ? 0 : (s > P - 1 ? P - 1 : s));               // a guard: an argsort's values are in range
      }
      p[k][0] = D[(size_t)src * 3 + 0], p[k][1] = D[(size_t)src * 3 + 1], p[k][2] = D[(size_t)src * 3 + 2];
      m[k] = (float)K[src];
    }
  }

  if (jit) {                                                            // (rot is given with it: checked by the entry point)
    const float* J = jit + ((size_t)b * N + n0) * 3;
    float j[VEC][3];
    if constexpr (VEC == 4) {
      const float4 a = *(const float4*)J, c = *(const float4*)(J + 4), e = *(const float4*)(J + 8);
      j[0][0] = a.x, j[0][1] = a.y, j[0][2] = a.z, j[1][0] = a.w, j[1][1] = c.x, j[1][2] = c.y;
      j[2][0] = c.z, j[2][1] = c.w, j[2][2] = e.x, j[3][0] = e.y, j[3][1] = e.z, j[3][2] = e.w;
    } else {
      j[0][0] = J[0], j[0][1] = J[1], j[0][2] = J[2];
    }
    const float c = rot[2 * b + 0], s = rot[2 * b + 1];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float qx = jitter(p[k][0], j[k][0], sigma, clip), qy = jitter(p[k][1], j[k][1], sigma, clip),
                  qz = jitter(p[k][2], j[k][2], sigma, clip);
      p[k][0] = (qx * c) - (qz * s);
      p[k][1] = qy;
      p[k][2] = (qx * s) + (qz * c);
    }
  }

  float* O = out_points + (size_t)b * 3 * N + n0;
  float* Q = out_mask + (size_t)b * N + n0;
  if constexpr (VEC == 4) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) *(float4*)(O + (size_t)ch * N) = make_float4(p[0][ch], p[1][ch], p[2][ch], p[3][ch]);
    *(float4*)Q = make_float4(m[0], m[1], m[2], m[3]);
  } else {
    O[0] = p[0][0], O[(size_t)N] = p[0][1], O[(size_t)2 * N] = p[0][2];
    Q[0] = m[0];
  }
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p % a) == 0; }

}  // namespace

extern "C" {

int ct_scan_items(const float* data, const uint8_t* mask, const int64_t* label, int64_t M, int P, const int64_t* item,
                  const int64_t* perm, const float* rot, const float* jit, float sigma, float clip, int B, int N, float* out_points,
                  float* out_mask, int64_t* out_label, ct_stream_t st) {
  if (!data || !mask || !label || !item || !out_points || !out_mask || !out_label) return CT_EINVAL;
  if ((rot == nullptr) != (jit == nullptr)) return CT_EINVAL;
  if (B < 1 || B > 65535 || N < 1 || P < N || P > kPMax || M < 1) return CT_EINVAL;
  if (!(clip > 0.0f) || !(sigma - sigma == 0.0f)) return CT_EINVAL;     // clip <= 0 or NaN; sigma NaN or +-inf
  // four slots per work-item when every output row (and jitter row) starts on 16 bytes
  const bool vec = N % 4 == 0 && aligned(out_points, 16) && aligned(out_mask, 16) && (!jit || aligned(jit, 16));
  // ... and the source rows as 16-byte loads when they are contiguous (no perm) and every cloud starts on 16 bytes
  const bool wide = vec && !perm && P % 4 == 0 && aligned(data, 16) && aligned(mask, 4);
  const int units = vec ? N / 4 : N;
  const dim3 grid((units + kThreads - 1) / kThreads, B), block(kThreads);
  CT_CLEAR_ERROR();
#define CT_SCAN_LAUNCH(VEC, WIDE)                                                                                              \
  hipLaunchKernelGGL((scan_items_kernel<VEC, WIDE>), grid, block, 0, (hipStream_t)st, data, mask, label, M, P, item, perm, rot, \
                     jit, sigma, clip, N, out_points, out_mask, out_label)
  if (wide)
    CT_SCAN_LAUNCH(4, true);
  else if (vec)
    CT_SCAN_LAUNCH(4, false);
  else
    CT_SCAN_LAUNCH(1, false);
#undef CT_SCAN_LAUNCH
  CT_CHECK_LAUNCH();
  return CT_OK;
}

}  // extern "C"
