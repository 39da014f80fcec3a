// Splat(max0) backward in deterministic mode (ct_set_deterministic, include/cloudct.h): the kernel, its plan and its launch.
// Included by ct_raster.hip inside its anonymous namespace, after the generic kernels' helpers (load_point, store_gpos,
// stage_tile), the planner (make_plan, splat_bwd_ncg), launch_sum_parts and CT_LAUNCH, ahead of run_splat_max_bwd, which
// routes every call here while the mode is on.  The launch tags of this file (splat_max_bwd_det, _det_groups, _det_global)
// cannot be reached by the rows of tests/raster_families.py, which have no mode column: tests/test_deterministic_gpu.py pins them.
#pragma once

// ---------------------------------------------------------------------------
// K5d: Splat(max0) backward under the deterministic rule (ct_set_deterministic): the winner of a (cell, channel) is the
//   LOWEST POINT INDEX among the contributions whose product is positive and bit-equal to z — and the lowest corner of that
//   point, should two of its corners name the same cell.  Two phases per channel chunk instead of K5's compare-and-swap,
//   whose winner is whichever wave arrives first:
//     claim : every matching contribution does atomicMin(claim[c, cell], n)  (claim tile preset to all ones)
//     award : after a barrier, the contribution whose n equals the claim word receives g_z
//   The whole N range of a plane stays in one workgroup per chunk (no point segments), so the barrier covers every claimant.
//   MODE 3: z tile, claim tile and g_z tile of the chunk in LDS; 2: z and claim tiles (g_z read from memory, winners only);
//   1: the claim tile alone (a grid whose two tiles of ONE channel exceed a CU: z is read from memory, it is never written);
//   0: nothing fits — the claim words live in the workspace (a.claim, preset by the host), read back past the L1 after the barrier.
//   g_keys: a thread owns its points and adds chunk after chunk in its own store; chunk GROUPS write partials
//   (a.gpos_stride) that sum_parts_kernel adds in group order — never a.atomic_gpos.
//   grid = (ncg, H, B).
// ---------------------------------------------------------------------------
template <int DIM, bool FROM_KEYS, int MODE>
__global__ void __launch_bounds__(1024, DIM == 2 ? 8 : 4) splat_max_bwd_det_kernel(RasterArgs a, GridW<DIM> g) {
  constexpr int V = 1 << DIM;
  constexpr bool K_LDS = MODE >= 1, Z_LDS = MODE >= 2, GZ_LDS = MODE == 3;
  extern __shared__ __align__(16) float lds[];
  const BlockXHB blk = block_xhb();
  const int cg = blk.x;
  const int h = blk.h, b = blk.b;
  const size_t bh = (size_t)b * a.H + h;
  const bool has_pad = a.pad_dtype != CT_PAD_NONE;
  bool first = true;
  for (int chunk = cg; chunk < a.nchunks; chunk += a.ncg) {
    const int c0 = chunk * a.CC;
    const int cc = min(a.CC, a.C - c0);
    const size_t toff = (bh * a.C + c0) * (size_t)g.G;
    const unsigned* Z = Z_LDS ? (const unsigned*)lds : (const unsigned*)(a.tile_in + toff);
    unsigned* K = K_LDS ? (unsigned*)lds + (Z_LDS ? (size_t)a.CC * g.G : 0) : (a.claim + toff);
    const float* gz = GZ_LDS ? (lds + (size_t)2 * a.CC * g.G) : (a.tile_in2 + toff);
    if (K_LDS) {
      __syncthreads();
      if (Z_LDS) stage_tile(lds, a.tile_in + toff, cc * g.G);
      if (GZ_LDS) {
        // (the LDS-DMA of stage_tile writes 16-byte pieces: a g_z tile that starts off that grid is copied element-wise)
        float* gl = lds + (size_t)2 * a.CC * g.G;
        if ((((size_t)2 * a.CC * g.G) & 3) == 0) stage_tile(gl, a.tile_in2 + toff, cc * g.G);
        else for (int i = threadIdx.x; i < cc * g.G; i += blockDim.x) gl[i] = a.tile_in2[toff + i];
      }
      for (int i = threadIdx.x; i < cc * g.G; i += blockDim.x) K[i] = 0xFFFFFFFFu;
      __syncthreads();
    }
    const float* src = a.src + (bh * a.C + c0) * (size_t)a.N;
    float* dst = a.dst + (bh * a.C + c0) * (size_t)a.N;
    // claim
    for (int n = threadIdx.x; n < a.N; n += blockDim.x) {
      Corners<DIM> c;
      PointPos<DIM, FROM_KEYS> pp;
      load_point<DIM, FROM_KEYS>(a.pos, g, bh, a.N, n, c, pp);
      const float p = ct_load_pad(a.pad, a.pad_dtype, (size_t)b * a.N + n);
      for (int ch = 0; ch < cc; ++ch) {
        float f = src[(size_t)ch * a.N + n];
        if (has_pad) f = f * p;
        const unsigned* Zc = Z + (size_t)ch * g.G;
        unsigned* Kc = K + (size_t)ch * g.G;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const unsigned zb = Zc[c.cell[v]], bits = __float_as_uint(f * c.w[v]);
          if ((zb == bits) & (zb != 0u)) atomicMin(&Kc[c.cell[v]], (unsigned)n);
        }
      }
    }
    if (!K_LDS) __threadfence();
    __syncthreads();
    // award
    for (int n = threadIdx.x; n < a.N; n += blockDim.x) {
      Corners<DIM> c;
      PointPos<DIM, FROM_KEYS> pp;
      load_point<DIM, FROM_KEYS>(a.pos, g, bh, a.N, n, c, pp);
      const float p = ct_load_pad(a.pad, a.pad_dtype, (size_t)b * a.N + n);
      float gw[V];
#pragma unroll
      for (int v = 0; v < V; ++v) gw[v] = 0.0f;
      for (int ch = 0; ch < cc; ++ch) {
        float f = src[(size_t)ch * a.N + n];
        if (has_pad) f = f * p;
        const unsigned* Zc = Z + (size_t)ch * g.G;
        unsigned* Kc = K + (size_t)ch * g.G;
        const float* Gc = gz + (size_t)ch * g.G;
        bool m[V];
        bool any = false;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const unsigned zb = Zc[c.cell[v]], bits = __float_as_uint(f * c.w[v]);
          m[v] = (zb == bits) & (zb != 0u);
          any = any | m[v];
        }
        float gf = 0.0f;
        if (any) {
#pragma unroll
          for (int v = 0; v < V; ++v) {
            bool win = false;
            if (m[v]) {
              const unsigned owner = K_LDS ? Kc[c.cell[v]]
                                              : __hip_atomic_load(&Kc[c.cell[v]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              win = owner == (unsigned)n;
#pragma unroll
              for (int u = 0; u < v; ++u) win = win & !(m[u] & (c.cell[u] == c.cell[v]));   // the point's lowest matching corner of a cell
            }
            const float gzw = win ? Gc[c.cell[v]] : 0.0f;
            gf += gzw * c.w[v];
            gw[v] += gzw * f;
          }
        }
        if (has_pad) gf = gf * p;
        dst[(size_t)ch * a.N + n] = gf;
      }
      store_gpos<DIM, FROM_KEYS>(a.g_pos + (size_t)cg * a.gpos_stride, bh, a.N, n, pp, gw, first && !a.accumulate, false);
    }
    first = false;
  }
}

// Deterministic mode (splat_max_bwd_det_kernel): the plan shared by the workspace query and the launch.  LDS holds the z tile and
// the claim tile of a channel chunk, and the g_z tile too where three single-channel tiles fit the 64 KiB budget; the chunk
// shrinks (make_plan) rather than spill.  A grid whose two tiles of ONE channel exceed a CU keeps the claim tile alone in LDS
// (32^3: 128 KiB); one whose single tile does not fit either keeps its claim words in the workspace (256^2).  Chunk groups (few planes) write partial g_keys to the workspace, added in group order.
struct DetPlan {
  Plan p;
  int mode;      // the kernel's MODE: tiles of a channel in LDS (3: z, claim, g_z; 2: z, claim; 1: claim; 0: none)
  int ncg;
  size_t claim_bytes, parts_bytes;
  size_t workspace() const { return std::max(claim_bytes, parts_bytes); }
};
DetPlan splat_bwd_det_plan(int B, int H, int C, int N, int dim, int G) {
  DetPlan d;
  d.mode = (size_t)G * 12 <= (size_t)kMaxLdsBytes ? 3 : (size_t)G * 8 <= (size_t)kBigLdsBytes ? 2 : 1;
  d.p = make_plan(B, H, C, N, G, d.mode);
  if (!d.p.lds_tile) d.mode = 0;
  d.ncg = d.p.lds_tile ? splat_bwd_ncg(B, H, d.p.nchunks) : 1;
  d.claim_bytes = d.p.lds_tile ? 0 : (size_t)B * H * C * G * 4;
  d.parts_bytes = d.ncg > 1 ? (size_t)d.ncg * B * H * ((size_t)1 << dim) * N * 4 : 0;
  return d;
}

template <int DIM, bool FROM_KEYS>
int run_splat_max_bwd_det(RasterArgs a, const GridW<DIM>& g, void* ws, size_t ws_bytes, hipStream_t st) {
  if (a.gpos_add != nullptr && a.gpos_add != a.g_pos) return CT_EINVAL;     // the caller computes the plain cotangent and adds
  const DetPlan d = splat_bwd_det_plan(a.B, a.H, a.C, a.N, DIM, g.G);
  a.CC = d.p.CC; a.nchunks = d.p.nchunks; a.nsplit = 1; a.atomic_gpos = 0; a.tickets = nullptr;
  float* const g_pos_out = a.g_pos;
  const int accumulate = a.accumulate;
  const size_t gpos_n = gpos_bytes<DIM, FROM_KEYS>(a) / 4;
  // without the partials' scratch one workgroup walks all chunks of its plane: slower, the same bits from run to run
  const bool parts = d.ncg > 1 && ws && ws_bytes >= (size_t)d.ncg * gpos_n * 4 && ((uintptr_t)ws & 3) == 0;
  a.ncg = parts ? d.ncg : 1;
  if (parts) { a.g_pos = (float*)ws; a.gpos_stride = gpos_n; a.accumulate = 0; }
  dim3 grid(a.ncg, a.H, a.B);
  if (!d.p.lds_tile) {
    if (!ws || ws_bytes < d.claim_bytes || ((uintptr_t)ws & 3) != 0) return CT_EWORKSPACE;
    if (hipMemsetAsync(ws, 0xFF, d.claim_bytes, st) != hipSuccess) return CT_ELAUNCH;
    a.claim = (unsigned*)ws;
    CT_LAUNCH((splat_max_bwd_det_kernel<DIM, FROM_KEYS, 0>), grid, d.p.threads, 0, st, a, g);
    note("splat_max_bwd_det_global");
    return CT_OK;
  }
  if (d.mode == 3) CT_LAUNCH((splat_max_bwd_det_kernel<DIM, FROM_KEYS, 3>), grid, d.p.threads, d.p.lds_bytes, st, a, g);
  else if (d.mode == 2) CT_LAUNCH((splat_max_bwd_det_kernel<DIM, FROM_KEYS, 2>), grid, d.p.threads, d.p.lds_bytes, st, a, g);
  else CT_LAUNCH((splat_max_bwd_det_kernel<DIM, FROM_KEYS, 1>), grid, d.p.threads, d.p.lds_bytes, st, a, g);
  note(parts ? "splat_max_bwd_det_groups" : "splat_max_bwd_det");
  if (parts) return launch_sum_parts((const float*)ws, g_pos_out, gpos_n, gpos_n, a.ncg, accumulate ? g_pos_out : nullptr, st);
  return CT_OK;
}
