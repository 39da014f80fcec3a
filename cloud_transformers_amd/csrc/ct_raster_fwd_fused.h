// Splat(max) forward and Slice forward of a (b, h) plane in ONE kernel.  Included by ct_raster.hip inside its anonymous namespace,
// behind ct_raster_hot.h (uses RasterArgs, GridW, block_xhb, pt2_from_keys, st_stream4 ... from there).
//
// The two forward ops of a step that chains them directly run on the same keys: the gather re-reads from memory the tile the
// scatter held in LDS a moment earlier, re-reads the keys and recomputes every point's base cell and corner weights.  Here a
// workgroup keeps its points' cells and weights in registers and the tile in LDS across both: `z` is written once (a side output,
// the backward passes read it) and never read back, the keys are read once per channel chunk, and one launch replaces two.
//
// It serves callers that chain ct_splat_fwd and ct_slice_fwd on one key tensor with nothing in between (SplatSliceStep.run()).  The
// zoo's blocks have a grouped convolution between the two ops and run ct_mhct_core_fwd where their grids fit: not served here.
#pragma once

constexpr int kFusedFwdThreads = 1024;

// ---------------------------------------------------------------------------
// KZ: z = Splat(max0)(keys, feat), out = Slice(keys, z).  One workgroup per (b, h, chunk of CC channels), thread = one quad of 4
//   consecutive points (N <= 4 * blockDim), corners from keys, N % 4 == 0, CC % 4 == 0, G % 4 == 0, 16-byte aligned rows.
//   LDS: integer tile [CC][G] (the scatter's form, as scatter_quad_kernel) | channel-interleaved tile [CC/4][G] x float4 (the
//        gather's form, as gather_ci_kernel)
//   phases: zero the tile (keys in flight) | scatter-max: a four-channel group's feat rows requested, then its 64 atomics per thread
//           | barrier | one pass over the tile: z rows -> memory as float4, the same words -> the interleaved tile (the 4 x 4
//           transpose in registers, as stage_tile_ci) | barrier | gather_ci_kernel's inner loop over the thread's own quad.
//   The weights of both halves come from pt2_from_keys — the same products as ct_corners<2> (w0x*w0y, w1x*w0y, w0x*w1y, w1x*w1y;
//   the library is built without contraction) — so z carries ct_splat_fwd's bits and out carries ct_slice_fwd's.
//   Workgroups are independent: nothing but the kernel's own barriers to wait on.
//   MINW: waves per SIMD the launch bound asks for — 4 (128 registers): one workgroup per CU, whatever its LDS (a whole plane's 16
//         channels at 32 x 32: 128 KiB); 8 (64 registers): two co-resident workgroups of eight channels (64 KiB each at 32 x 32), on
//         one XCD through block_xhb.  Only the 32 x 32 instance fits 64 registers without scratch (its corner offsets are
//         immediates): the general-grid and the padded forms are built at 128 whatever the chunking.
//   grid = (nchunks, H, B)
// ---------------------------------------------------------------------------
template <bool HAS_PAD, int WT, int MINW>
__global__ void __launch_bounds__(kFusedFwdThreads, MINW) splat_slice_fwd_kernel(RasterArgs a, GridW<2> g_arg) {
  const GridW<2> g = grid2_of<WT>(g_arg);
  extern __shared__ __align__(16) float lds[];
  const int G = WT ? WT * WT : g.G, W1 = WT ? WT : g.W[1], N = a.N;
  unsigned* acc = (unsigned*)lds;
  float4* T4 = (float4*)(lds + (size_t)a.CC * G);
  const BlockXHB blk = block_xhb();
  const int chunk = blk.x, h = blk.h, b = blk.b;
  const size_t bh = (size_t)b * a.H + h;
  const int c0 = chunk * a.CC;
  const int cc = min(a.CC, a.C - c0);            // multiple of 4
  const int tid = threadIdx.x, nq = N >> 2;
  const bool mine = tid < nq;                    // (a thread without a quad reads the plane's last one and neither scatters nor stores)
  const int n0 = min(tid, nq - 1) << 2;
  const int off[4] = {0, W1, 1, W1 + 1};

  // the quad's keys are requested in front of the tile's zeroes
  const float4 tx = *(const float4*)(a.pos.keys + (bh * 2 + 0) * N + n0);
  const float4 ty = *(const float4*)(a.pos.keys + (bh * 2 + 1) * N + n0);
  for (int i = tid; i < (cc * G) >> 2; i += blockDim.x) ((int4*)acc)[i] = make_int4(0, 0, 0, 0);
  // HOLD: the cells and weights stay in registers for both halves; at 64 registers (MINW = 8) the gather computes them again from
  // the keys it kept, by the same routine (20 registers less across the kernel; the same bits)
  constexpr bool HOLD = MINW <= 4;
  const float kx[4] = {tx.x, tx.y, tx.z, tx.w}, ky[4] = {ty.x, ty.y, ty.z, ty.w};
  float cw[4][4], pv[4];
  int base[4];
  {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      Pt2 p;
      pt2_from_keys(kx[i], ky[i], g, W1, p);
      base[i] = p.base;
#pragma unroll
      for (int v = 0; v < 4; ++v) cw[i][v] = p.cw[v];
      pv[i] = HAS_PAD ? ct_load_pad(a.pad, a.pad_dtype, (size_t)b * N + n0 + i) : 1.0f;
    }
  }
  __syncthreads();

  // ---- scatter-max, as scatter_quad_kernel<2, false>: positive products only, atomic max on the bit pattern ----
  if (mine) {
    const float* src = a.src + (bh * a.C + c0) * (size_t)N + n0;
    for (int cg0 = 0; cg0 < cc; cg0 += 4) {
      float fv[4][4];
#pragma unroll
      for (int cj = 0; cj < 4; ++cj) {
        const float4 t = *(const float4*)(src + (size_t)(cg0 + cj) * N);
        fv[cj][0] = t.x; fv[cj][1] = t.y; fv[cj][2] = t.z; fv[cj][3] = t.w;
      }
#pragma unroll
      for (int cj = 0; cj < 4; ++cj) {
        unsigned* Tc = acc + (size_t)(cg0 + cj) * G;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float f = HAS_PAD ? fv[cj][i] * pv[i] : fv[cj][i];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const float prod = f * cw[i][v];
            // zero floor: only positive products can win, and positive IEEE-754 floats order like their bit patterns
            if (prod > 0.0f) atomicMax(Tc + base[i] + off[v], __float_as_uint(prod));
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- the tile, once: z rows to memory, the same words channel-interleaved for the gather ----
  {
    const int G4 = G >> 2, n = (cc >> 2) * G4;
    float* zout = a.tile_out + (bh * a.C + c0) * (size_t)G;
    for (int j = tid; j < n; j += blockDim.x) {
      const int q = j / G4, cell = (j - q * G4) << 2;
      const size_t row = (size_t)(q * 4) * G + cell;
      float4 r[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = *(const float4*)(lds + row + (size_t)k * G);
#pragma unroll
      for (int k = 0; k < 4; ++k) *(float4*)(zout + row + (size_t)k * G) = r[k];
      float4* d = T4 + ((size_t)j << 2);       // q * G + cell
      d[0] = make_float4(r[0].x, r[1].x, r[2].x, r[3].x);
      d[1] = make_float4(r[0].y, r[1].y, r[2].y, r[3].y);
      d[2] = make_float4(r[0].z, r[1].z, r[2].z, r[3].z);
      d[3] = make_float4(r[0].w, r[1].w, r[2].w, r[3].w);
    }
  }
  __syncthreads();

  // ---- gather, as gather_ci_kernel: one ds_read_b128 per (point, corner, four channels) ----
  if (mine) {
    float* drow = a.dst + (bh * a.C + c0) * (size_t)N + n0;      // one running row pointer (sixteen of them, hoisted, are 32 registers)
    const float4* Tq = T4;
    for (int cq = 0; cq < (cc >> 2); ++cq, Tq += G) {
      float o[4][4];       // [channel][point]
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float w[4];
        int bi;
        if constexpr (HOLD) {
          bi = base[i];
#pragma unroll
          for (int v = 0; v < 4; ++v) w[v] = cw[i][v];
        } else {
          // (the keys made opaque: the compiler would otherwise keep the first computation's 20 values alive instead; and one
          //  point's reads at a time, or all sixteen are hoisted in front of the sums as in gather_ci_kernel — 110 registers)
          float kxi = kx[i], kyi = ky[i];
          asm volatile("" : "+v"(kxi), "+v"(kyi));
          __builtin_amdgcn_sched_barrier(0);
          Pt2 p;
          pt2_from_keys(kxi, kyi, g, W1, p);
          bi = p.base;
#pragma unroll
          for (int v = 0; v < 4; ++v) w[v] = p.cw[v];
        }
        float4 cv[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) cv[v] = Tq[bi + off[v]];
        // same order as the reference's sum over corners: ((v0 + v1) + v2) + v3
        float s0 = cv[0].x * w[0], s1 = cv[0].y * w[0], s2 = cv[0].z * w[0], s3 = cv[0].w * w[0];
#pragma unroll
        for (int v = 1; v < 4; ++v) {
          s0 += cv[v].x * w[v];
          s1 += cv[v].y * w[v];
          s2 += cv[v].z * w[v];
          s3 += cv[v].w * w[v];
        }
        o[0][i] = HAS_PAD ? s0 * pv[i] : s0;
        o[1][i] = HAS_PAD ? s1 * pv[i] : s1;
        o[2][i] = HAS_PAD ? s2 * pv[i] : s2;
        o[3][i] = HAS_PAD ? s3 * pv[i] : s3;
        if constexpr (!HOLD) {
          asm volatile("" : "+v"(o[0][i]), "+v"(o[1][i]), "+v"(o[2][i]), "+v"(o[3][i]));
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int cj = 0; cj < 4; ++cj, drow += N) st_stream4(drow, make_float4(o[cj][0], o[cj][1], o[cj][2], o[cj][3]));
    }
  }
}
