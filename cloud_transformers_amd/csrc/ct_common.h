// Shared device helpers for libcloudct (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/cloudct.h"

#define CT_WAVE 64

// float32(-1 + 1e-7) and float32(1 - 1e-7): the bounds torch uses when the
// reference clamps an fp32 tensor with python doubles
// (layers/cloud_transform.py:59,91).
#define CT_KEY_LO (-0.99999988f)
#define CT_KEY_HI (0.99999988f)

template <int DIM>
struct GridW {
  int W[DIM];      // extents, axis 0 slowest
  float hw[DIM];   // (W-1)*0.5f
  int G;           // cells
};

// A square grid whose extent is a template constant (WT > 0: the headline's 32 x 32, the zoo's 64 x 64 and 16 x 16): extents,
// half-widths and cell count as immediates (see grid3_of in ct_raster_hot3d.h); WT = 0: the caller's grid.
template <int WT>
__device__ __forceinline__ GridW<2> grid2_of(const GridW<2>& g) {
  if constexpr (WT == 0) {
    return g;
  } else {
    GridW<2> c;
    c.W[0] = c.W[1] = WT;
    c.hw[0] = c.hw[1] = (float)(WT - 1) * 0.5f;
    c.G = WT * WT;
    return c;
  }
}

// The zoo's 3D grids are cubes of 8 and 16 cells (model_zoo: 8^3 C32, 16^3 C16): with the extent a template constant the cell count,
// the corner offsets and the half-widths are immediates instead of registers in kernels that have none to spare (W3 = 0: any grid).
template <int W3>
__device__ __forceinline__ GridW<3> grid3_of(const GridW<3>& g) {
  if constexpr (W3 == 0) {
    return g;
  } else {
    GridW<3> c;
    c.W[0] = c.W[1] = c.W[2] = W3;
    c.hw[0] = c.hw[1] = c.hw[2] = (float)(W3 - 1) * 0.5f;
    c.G = W3 * W3 * W3;
    return c;
  }
}

// Per-axis terms of one key (layers/cloud_transform.py:91-94,
// layers/utils.py:122,168): clamp, (k+1)*((W-1)/2) in that rounding order,
// floor, low/high weights.
__device__ __forceinline__ void ct_axis(float key, float hw, int Wj, float& w0, float& w1, int& f) {
  float k = fminf(fmaxf(key, CT_KEY_LO), CT_KEY_HI);
  float s = (k + 1.0f) * hw;
  float fl = floorf(s);
  w0 = (fl + 1.0f) - s;
  w1 = s - fl;
  f = min((int)fl, Wj - 2);   // memory safety only: f <= W-2 already holds for W < 2^22
}

// clamp passes the gradient only inside [lo, hi] (torch.clamp backward)
__device__ __forceinline__ float ct_key_mask(float key) {
  return (key >= CT_KEY_LO && key <= CT_KEY_HI) ? 1.0f : 0.0f;
}

template <int DIM>
struct Corners {
  static constexpr int V = 1 << DIM;
  int cell[V];
  float w[V];
};

// corner v = dx + 2dy (+ 4dz); weight (wx*wy)*wz; cell = x*W1(*W2) + y(*W2) + z
template <int DIM>
__device__ __forceinline__ void ct_corners(const float (&w0)[DIM], const float (&w1)[DIM],
                                           const int (&f)[DIM], const GridW<DIM>& g, Corners<DIM>& c) {
  if constexpr (DIM == 2) {
    int base = f[0] * g.W[1] + f[1];
    c.cell[0] = base;
    c.cell[1] = base + g.W[1];
    c.cell[2] = base + 1;
    c.cell[3] = base + g.W[1] + 1;
    c.w[0] = w0[0] * w0[1];
    c.w[1] = w1[0] * w0[1];
    c.w[2] = w0[0] * w1[1];
    c.w[3] = w1[0] * w1[1];
  } else {
    int sx = g.W[1] * g.W[2], sy = g.W[2];
    int base = f[0] * sx + f[1] * sy + f[2];
    float xy00 = w0[0] * w0[1], xy10 = w1[0] * w0[1], xy01 = w0[0] * w1[1], xy11 = w1[0] * w1[1];
    c.cell[0] = base;
    c.cell[1] = base + sx;
    c.cell[2] = base + sy;
    c.cell[3] = base + sx + sy;
    c.cell[4] = base + 1;
    c.cell[5] = base + sx + 1;
    c.cell[6] = base + sy + 1;
    c.cell[7] = base + sx + sy + 1;
    c.w[0] = xy00 * w0[2];
    c.w[1] = xy10 * w0[2];
    c.w[2] = xy01 * w0[2];
    c.w[3] = xy11 * w0[2];
    c.w[4] = xy00 * w1[2];
    c.w[5] = xy10 * w1[2];
    c.w[6] = xy01 * w1[2];
    c.w[7] = xy11 * w1[2];
  }
}

// d(weights)/d(s_j) contracted with the corner cotangents gw[v]:
//   gs_j = sum_v gw[v] * sign_j(v) * prod_{i != j} w_i(d_i(v))
template <int DIM>
__device__ __forceinline__ void ct_corner_grad(const float (&w0)[DIM], const float (&w1)[DIM],
                                               const float (&gw)[1 << DIM], float (&gs)[DIM]) {
  if constexpr (DIM == 2) {
    gs[0] = (gw[1] - gw[0]) * w0[1] + (gw[3] - gw[2]) * w1[1];
    gs[1] = (gw[2] - gw[0]) * w0[0] + (gw[3] - gw[1]) * w1[0];
  } else {
    float yz00 = w0[1] * w0[2], yz10 = w1[1] * w0[2], yz01 = w0[1] * w1[2], yz11 = w1[1] * w1[2];
    float xz00 = w0[0] * w0[2], xz10 = w1[0] * w0[2], xz01 = w0[0] * w1[2], xz11 = w1[0] * w1[2];
    float xy00 = w0[0] * w0[1], xy10 = w1[0] * w0[1], xy01 = w0[0] * w1[1], xy11 = w1[0] * w1[1];
    gs[0] = (gw[1] - gw[0]) * yz00 + (gw[3] - gw[2]) * yz10 + (gw[5] - gw[4]) * yz01 + (gw[7] - gw[6]) * yz11;
    gs[1] = (gw[2] - gw[0]) * xz00 + (gw[3] - gw[1]) * xz10 + (gw[6] - gw[4]) * xz01 + (gw[7] - gw[5]) * xz11;
    gs[2] = (gw[4] - gw[0]) * xy00 + (gw[5] - gw[1]) * xy10 + (gw[6] - gw[2]) * xy01 + (gw[7] - gw[3]) * xy11;
  }
}

__device__ __forceinline__ float ct_load_pad(const void* pad, int pad_dtype, size_t i) {
  if (pad_dtype == CT_PAD_F32) return ((const float*)pad)[i];
  if (pad_dtype == CT_PAD_I32) return (float)((const int*)pad)[i];
  return 1.0f;
}

typedef float ct_f4 __attribute__((ext_vector_type(4)));

// Streaming (read-once / write-once) global accesses carry the non-temporal hint, so that what IS re-read inside a
// kernel — keys, and the second quad's g_out rows of the fused Slice backward — stays in the XCD's 4 MiB L2 instead
// of being pushed out by the streams (the re-reads then never reach the memory-side counters, nor HBM).
__device__ __forceinline__ float4 ld_stream4(const float* p) {
  const ct_f4 v = __builtin_nontemporal_load((const ct_f4*)p);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_stream4(float* p, float4 v) {
  const ct_f4 t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, (ct_f4*)p);
}
__device__ __forceinline__ float ld_stream(const float* p) { return __builtin_nontemporal_load(p); }

// ---- the NORM epilogue of the Slice write-outs (ct_slice_fwd_norm: ct_raster.hip; ct_mhct_core_fwd_norm: ct_mhct.hip) ----
// Eval-mode BatchNorm (+ ReLU) on the value a gather would have stored.  A workgroup leaves one record per channel of its
// chunk in LDS — (mean, 1 / sqrt(var + eps), weight, bias), computed once — and applies bn_eval_one's operation sequence
// (ct_bnorm.hip; contraction is off for the whole library, and the mean is subtracted first: no folded scale / shift) at its
// stores: the bits of the plain gather followed by ct_bn_eval_group_fwd.
__device__ __forceinline__ float4 ct_norm_record(float mean, float var, float eps, float weight, float bias) {
  return make_float4(mean, 1.0f / sqrtf(var + eps), weight, bias);
}
// A record read back from LDS: the channel is the same for every lane of the wave, so the four values move to scalar registers —
// the epilogue then costs the gather kernels no vector registers beside their own (held in vector registers the records of a
// four-channel group pushed gather_ci_kernel past its 128: 20-36 bytes of scratch).
__device__ __forceinline__ float ct_uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
__device__ __forceinline__ float4 ct_norm_uniform(const float4 r) {
  return make_float4(ct_uniform(r.x), ct_uniform(r.y), ct_uniform(r.z), ct_uniform(r.w));
}
__device__ __forceinline__ float ct_norm_one(float v, const float4 r, int relu) {
  const float o = ((v - r.x) * r.y) * r.z + r.w;
  return relu ? fmaxf(o, 0.0f) : o;
}
// four values of one channel (r: its record, through ct_norm_uniform); am = max(am, |stored values|)
__device__ __forceinline__ float4 ct_norm_four(float4 v, const float4 r, int relu, float& am) {
  float4 o;
  o.x = ct_norm_one(v.x, r, relu); o.y = ct_norm_one(v.y, r, relu); o.z = ct_norm_one(v.z, r, relu); o.w = ct_norm_one(v.w, r, relu);
  am = fmaxf(fmaxf(am, fmaxf(fabsf(o.x), fabsf(o.y))), fmaxf(fabsf(o.z), fabsf(o.w)));
  return o;
}
// max of `am` over the workgroup -> *slot, the workgroup's own partial maximum (a plain store: no atomics, nothing to zero; a
// workgroup without points stores 0).  `red`: 16 floats of LDS nobody reads any more once every thread has arrived here.
// Called by all threads of the workgroup; slot is block-uniform (null: no maxima asked for).
__device__ __forceinline__ void ct_norm_fold_amax(float am, float* red, float* slot) {
  if (slot == nullptr) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) am = fmaxf(am, __shfl_xor(am, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = am;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = (int)(blockDim.x + 63) >> 6;
    for (int i = 1; i < nw; ++i) am = fmaxf(am, red[i]);
    *slot = am;
  }
}

// Launch tags (test hooks, host state): every entry point that picks among kernel families calls note_reset() on entry and
// note("family") for each kernel it launches; ct_debug_last_launch() returns the tags joined with '+'.  Defined once, in
// ct_raster.hip (the library is linked from one object per source); internal to the library.
namespace ct_tags {
__attribute__((visibility("hidden"))) void note_reset();
__attribute__((visibility("hidden"))) void note(const char* tag);
}  // namespace ct_tags

// hipGetLastError() is sticky across unrelated runtime calls of the host
// framework (e.g. a hipEventQuery that returned hipErrorNotReady), so every
// entry point clears it first (CT_CLEAR_ERROR) and checks after its launches.
#define CT_CLEAR_ERROR() ((void)hipGetLastError())
#define CT_CHECK_LAUNCH()                         \
  do {                                            \
    hipError_t e__ = hipGetLastError();           \
    if (e__ != hipSuccess) return CT_ELAUNCH;     \
  } while (0)
