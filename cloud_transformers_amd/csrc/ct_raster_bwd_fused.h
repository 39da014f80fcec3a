// Slice backward and Splat(max) backward of a (b, h) plane in ONE kernel.  Included by ct_raster.hip inside its anonymous namespace,
// behind ct_raster_sorted.h (uses sort_plane, SortLds, SortedPlane and the item body's helpers from there, splat_bwd_quad,
// stage_tile_pairs and kNoMatch from ct_raster_hot.h).
//
// The two backward ops of a step that chains Splat and Slice directly hand each other four tensors through memory: g_z (written
// by Slice backward, read back by Splat backward), z (read by both), the keys (read by both) and Slice's key cotangent (written
// by one, added by the other).  Here the sorted Slice backward's workgroup keeps going: when a four-channel group's g_z tile is
// complete in LDS it is stored (g_z stays an output) AND turned, in place, into the {z, z, g_z, g_z} pair tile the Splat backward
// reads; the workgroup's threads then run the optimistic Splat(max) backward pass over their own quad of points for these four
// channels.  Both key cotangents meet in registers behind the last group: one g_keys store per point.
//
// It serves callers that run ct_slice_bwd_tk and ct_splat_bwd_tk(add = Slice's key cotangent) on one key tensor with nothing in
// between (SplatSliceStep.run()).  The arithmetic of either half is the stand-alone kernel's, in its order: the bits of
// slice_bwd_sorted_kernel and splat_max_bwd_hot_kernel with one workgroup per plane (tests/test_slice_splat_bwd_fused_gpu.py).
// What the group loop does NOT do (profiles/fused_bwd_loop_ab.txt): recompute a point's corner set-up from the keys — the base
// cells are parked behind the sort (16 bits each, over the dead first-item marks), (w1x, w1y) are the entry's weights in LDS,
// w0 = 1 - w1, the clamp mask of the g_keys store is the rank's flags: the keys are read once per plane (the rare tied-group
// redo reads them again); touch scratch or wait for vector memory on its behalf — the five streams (g_out, feat, z cells in,
// g_z, g_feat out) go through wave-uniform buffer descriptors with a scalar row offset and one shared 32-bit lane offset, so the
// only vmcnt waits in the loop are the staging of g_out / z cells and the first use of feat in the Splat body (the headline
// instance: no scratch at all).  Measured and not kept: matches and non-zero cells counted per wave by ballot and popcount
// instead of per lane — fewer vector instructions, a slower step.
// Measured on the headline step (profiles/fused_bwd_ab.txt, fused_bwd_loop_ab.txt).  Not served: padding masks
// (that instance is not built), the deterministic mode, a plane-sort record as input, N > 4096, grids of more than 1024 cells,
// 3D, reduce=sum.
// Ties: per four-channel group, non-zero cells against matches; a tied group is redone behind the loop with single-winner claims
// (first come between threads, the lower index inside a thread's quad: as the stand-alone kernel's group redo).  The stand-alone
// kernel's repair of a single tie by value (lowest point index) is not built in: a chance tie costs one group's redo here.
#pragma once

// ---------------------------------------------------------------------------
// KB: g_z, (g_keys_slice) = Slice backward(keys, z, g_out);  g_feat, g_keys = Splat(max) backward(keys, feat, z, g_z) + g_keys_slice.
//   One kSortThreads workgroup per (b, h) plane, the carve-up of slice_bwd_sorted_kernel (SortLds), G <= kSortThreads cells (a
//   thread converts one cell), C <= 256 (a 64-bit mask of tied groups).
//   a.src = g_out, a.tile_in = z, a.tile_in2 = FEAT (point-sized here), a.tile_out = g_z, a.dst = g_feat, a.g_pos = g_keys,
//   a.fold_gpos = Slice's key cotangent alone (or null).
//   Per four-channel group:
//     stage (g_out in sorted order, the z cells)  | barrier | items (slice_bwd_sorted_kernel's; the first item carries the requests
//     of the group's FEAT rows, one channel per entry) | barrier | thread = cell: its four accumulator words and its z word,
//     the g_z elements stored, its accumulator words cleared, the non-zero cells counted, its two words of the pair tile
//     {z(2p), z(2p+1), g(2p), g(2p+1)} written over the dead STAGE area (empty cells: kNoMatch; a thread touches its own words
//     only: no barrier in between) | barrier | splat_bwd_quad's optimistic body on the thread's quad (one point carries one channel
//     of the NEXT group's g_out requests), g_feat rows stored, matches counted | barrier | the group's tie test (non-zero cells
//     against matches).  Four barriers per group; the next staging restores the stage area's zero entry.
//   Behind the loop: a tied group is redone as splat_max_bwd_hot_kernel redoes it (pairs staged again from z and the g_z this
//   workgroup stored, over the tile and accumulator areas, splat_bwd_quad<.., CLAIMS, DELTA>); then the key cotangents.
//   Vector instructions the loop does without (profiles/fused_bwd_valu_ab.txt): the cross-row steps, readlane and lane election of
//   its six reductions (row_max_u32 / row_sum_i32 below), the convert phase's second fx_quantum (q from iq's bits on the scalar
//   unit), the register copies of the Splat body's loaded pairs.
//   grid = (1, H, B)
// ---------------------------------------------------------------------------
// A stream of the plane behind a buffer descriptor: raw buffer, 32-bit byte offsets (a scalar row + the lane's), range-checked
// against the plane's bytes.  Built from wave-uniform values only.
typedef unsigned ct_u4 __attribute__((ext_vector_type(4)));
struct StreamBuf {
  __amdgpu_buffer_rsrc_t r;
};
constexpr int kBufNt = 2;      // the non-temporal bit of a buffer access (the `nt` of ld_stream4 / st_stream4)
__device__ __forceinline__ StreamBuf stream_buf(const float* base, unsigned bytes) {
  StreamBuf b;
  b.r = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, 0x00020000);
  return b;
}
__device__ __forceinline__ float4 buf_ld_stream4(const StreamBuf& b, unsigned voff, unsigned soff) {
  const ct_u4 v = __builtin_amdgcn_raw_buffer_load_b128(b.r, (int)voff, (int)soff, kBufNt);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ float buf_ld_stream(const StreamBuf& b, unsigned voff, unsigned soff) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(b.r, (int)voff, (int)soff, kBufNt));
}
__device__ __forceinline__ void buf_st_stream4(const StreamBuf& b, unsigned voff, unsigned soff, float4 v) {
  const ct_u4 t = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
  __builtin_amdgcn_raw_buffer_store_b128(t, b.r, (int)voff, (int)soff, kBufNt);
}
__device__ __forceinline__ void buf_st_stream(const StreamBuf& b, unsigned voff, unsigned soff, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), b.r, (int)voff, (int)soff, kBufNt);
}

// The group loop's own reductions: the four row steps of wave_max_u32 / wave_sum_i32 (lanes without a source read 0, the identity
// of both) and no more — lane 15 of each 16-lane row holds its row's result and hands it to the LDS atomic itself: four lanes a
// wave instead of one, and neither the two cross-row steps nor the readlane.  Integer max and add: exact in any order.
__device__ __forceinline__ unsigned row_max_u32(unsigned v) {
#define CT_UMAX(a, b) max((a), (b))
  CT_DPP_STEP(v, CT_UMAX, 0x111, 0xf);
  CT_DPP_STEP(v, CT_UMAX, 0x112, 0xf);
  CT_DPP_STEP(v, CT_UMAX, 0x114, 0xf);
  CT_DPP_STEP(v, CT_UMAX, 0x118, 0xf);
#undef CT_UMAX
  asm volatile("" : "+v"(v));      // (the last step stays here, folded like the others, and does not sink to the user's branch)
  return v;
}
__device__ __forceinline__ int row_sum_i32(int v) {
#define CT_IADD(a, b) ((a) + (b))
  CT_DPP_STEP(v, CT_IADD, 0x111, 0xf);
  CT_DPP_STEP(v, CT_IADD, 0x112, 0xf);
  CT_DPP_STEP(v, CT_IADD, 0x114, 0xf);
  CT_DPP_STEP(v, CT_IADD, 0x118, 0xf);
#undef CT_IADD
  asm volatile("" : "+v"(v));
  return v;
}

template <bool HAS_PAD, int WT, int NT = 0, int CT = 0>
__global__ void __launch_bounds__(kSortThreads) slice_splat_bwd_kernel(RasterArgs a_arg, GridW<2> g_arg) {
  const GridW<2> g = grid2_of<WT>(g_arg);
  RasterArgs a = a_arg;
  if constexpr (NT > 0) a.N = NT;
  if constexpr (CT > 0) a.C = CT;
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const int G = WT ? WT * WT : g.G, W1 = WT ? WT : g.W[1], N = a.N, C = a.C;
  const SortLds L = sort_lds(G, N, C);
  float4* T4 = (float4*)(lds_raw + L.tile);
  int* acc = (int*)(lds_raw + L.acc);
  float4* ZG = (float4*)(lds_raw + L.tile);          // the tied-group redo's pair tile: the tile and accumulator areas together
  float4* Sg = (float4*)(lds_raw + L.stage);
  const float2* AB = (const float2*)(lds_raw + L.ab);
  unsigned* s_max = (unsigned*)(lds_raw + L.misc);
  unsigned* s_k = s_max + C;
  int* s_tie = (int*)(s_k + 1);                       // the sort's scan scratch, dead behind it: [parity][non-zero cells, matches]
  float4* PZ = (float4*)(lds_raw + L.stage);          // the group loop's pair tile: over the stage area (2 x 16 G bytes of its >= 64 G)
  const bool row_last = (threadIdx.x & 15) == 15;
  const int b = blockIdx.z;
  const size_t bh = (size_t)b * a.H + blockIdx.y;
  const int tid = threadIdx.x;
  const int off[4] = {0, W1, 1, W1 + 1};
  const bool has = (tid << 2) < N;
  const int n0 = has ? (tid << 2) : 0;
  const int ngroups = C >> 2;
  const float* const feat = a.tile_in2;

  float gq[4][4];           // [channel][point] of the thread's quad: g_out of the group being staged
  float fq[4][4];           // the same of feat: requested during the group's items, consumed (and overwritten by g_feat) behind them
  float cvq[4];
  // The plane's five streams go through buffer descriptors built from kernel arguments and block indices alone (wave-uniform:
  // scalar registers), a channel row is the scalar offset, and the lanes share ONE 32-bit offset: the byte offset of the thread's
  // quad in a point row (a quarter of it: of its cell in a grid row).  No per-lane 64-bit address is left for the compiler to keep
  // across the group loop.  The accesses keep the non-temporal hint of ld_stream4 / st_stream4.
  const unsigned ln0 = (unsigned)n0;
  const unsigned pt_row = (unsigned)N * 4u, cell_row = (unsigned)G * 4u;      // bytes
  const StreamBuf b_src = stream_buf(a.src + bh * C * (size_t)N, (unsigned)C * pt_row);
  const StreamBuf b_fea = stream_buf(feat + bh * C * (size_t)N, (unsigned)C * pt_row);
  const StreamBuf b_dst = stream_buf(a.dst + bh * C * (size_t)N, (unsigned)C * pt_row);
  const StreamBuf b_cnv = stream_buf(a.tile_in + bh * C * (size_t)G, (unsigned)C * cell_row);
  const StreamBuf b_gz = stream_buf(a.tile_out + bh * C * (size_t)G, (unsigned)C * cell_row);
  const unsigned vo_pt = ln0 * 4u, vo_cell = tid < G ? (unsigned)tid * 4u : 0u;
  auto request1 = [&](int grp, int cj) {
    const float4 t = buf_ld_stream4(b_src, vo_pt, (unsigned)(grp * 4 + cj) * pt_row);
    gq[cj][0] = t.x; gq[cj][1] = t.y; gq[cj][2] = t.z; gq[cj][3] = t.w;
    cvq[cj] = buf_ld_stream(b_cnv, vo_cell, (unsigned)(grp * 4 + cj) * cell_row);
  };
  auto request_feat1 = [&](int grp, int cj) {
    const float4 t = buf_ld_stream4(b_fea, vo_pt, (unsigned)(grp * 4 + cj) * pt_row);
    fq[cj][0] = t.x; fq[cj][1] = t.y; fq[cj][2] = t.z; fq[cj][3] = t.w;
  };
  PlaneKeys PK;
  load_plane_keys(a, g, W1, bh, PK);
  SortedPlane S;
  float pv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) pv[i] = (HAS_PAD && has) ? ct_load_pad(a.pad, a.pad_dtype, (size_t)b * N + n0 + i) : 1.0f;

  sort_plane(a, PK, G, W1, sort_ptrs(lds_raw, L, C), C, S, nullptr, [&]() {
#pragma unroll
    for (int cj = 0; cj < 4; ++cj) request1(0, cj);
  });
  // (sort_plane's last barrier is behind its last use of the scan scratch; the first group's barriers order these stores)
  // The quad's base cells, 16 bits each (G <= 1024), parked in point order over the first-item marks: their last readers are in
  // front of sort_plane's last barrier, and a thread reads back only the word it wrote.
  uint2* const s_cell = (uint2*)(lds_raw + L.mark);
  s_cell[tid] = make_uint2((unsigned)PK.base[0] | (unsigned)PK.base[1] << 16, (unsigned)PK.base[2] | (unsigned)PK.base[3] << 16);
  for (int i = tid; i < G; i += kSortThreads) ((int4*)acc)[i] = make_int4(0, 0, 0, 0);
  if (tid < 4) s_tie[tid] = 0;
  const float Kf = (float)(*s_k);

  float gsx[2][kItemLen], gsy[2][kItemLen];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int j = 0; j < kItemLen; ++j) gsx[u][j] = gsy[u][j] = 0.0f;
  float gs[4][2];           // Splat's key cotangent of the quad's points
#pragma unroll
  for (int i = 0; i < 4; ++i) gs[i][0] = gs[i][1] = 0.0f;
  // the two items' cells in one register (G <= 1024; -1: no item), unpacked per group
  unsigned cell01 = ((unsigned)S.cell[0] & 0xffffu) | (unsigned)S.cell[1] << 16;
  unsigned long long tied = 0ull;      // block-uniform: bit i — group i has more matches than non-zero cells

  auto group = [&](const int grp, auto more) {
    const int ch0 = grp * 4;
    // (opaque per group, as the items' offsets below: the unpacked positions would otherwise be kept across the loop, in scratch)
    asm volatile("" : "+v"(S.rk01), "+v"(S.rk23), "+v"(cell01));
    const int cell[2] = {(int)(short)(cell01 & 0xffffu), (int)cell01 >> 16};
    unsigned rowmax[4];
    // (a lane offset the compiler cannot see through: with a wave-uniform address its atomic optimizer folds the rows' atomics into
    // one lane's, through a scalar loop over the active lanes.  To recheck with another toolchain, read the headline instance's ISA:
    // the staging phase holds four ds_max_u32 under one exec mask and no s_cbranch loop with v_readlane in front of them, the
    // convert phase and the end of the Splat body one ds_add_u32 each.  Bits are the same either way; the loop is slower.)
    unsigned lane0;
    asm volatile("v_mov_b32 %0, 0" : "=v"(lane0));
    unsigned* const s_max_lane = s_max + lane0;
    int* const s_tie_lane = s_tie + lane0;
#pragma unroll
    for (int cj = 0; cj < 4; ++cj) {
      float m = 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float x = HAS_PAD ? gq[cj][i] * pv[i] : gq[cj][i];
        x = has ? x : 0.0f;
        gq[cj][i] = x;
        x = fabsf(x);
        m = fmaxf(m, (x < __builtin_inff()) ? x : __builtin_inff());     // inf / NaN -> inf
      }
      rowmax[cj] = row_max_u32(__float_as_uint(m));
    }
    if (row_last) {
#pragma unroll
      for (int cj = 0; cj < 4; ++cj) atomicMax(s_max_lane + ch0 + cj, rowmax[cj]);
    }
    // The stage area's zero entry, which padded item slots read: written here for every group, the first included (nowhere else) —
    // the previous group's pair tile lay over the stage area, over this entry too where N < 2 G.
    if (tid == 0) Sg[N] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (has) {
      const unsigned rk[4] = {S.rk01 & kRankMask, (S.rk01 >> 16) & kRankMask, S.rk23 & kRankMask, (S.rk23 >> 16) & kRankMask};
#pragma unroll
      for (int i = 0; i < 4; ++i) Sg[rk[i]] = make_float4(gq[0][i], gq[1][i], gq[2][i], gq[3][i]);
    }
    if (tid < G) T4[tid] = make_float4(cvq[0], cvq[1], cvq[2], cvq[3]);
    __syncthreads();

    float iq[4], qs[4];
    bool any_float = false;
#pragma unroll
    for (int cj = 0; cj < 4; ++cj) {
      float q;
      bool fixed;
      fx_quantum(__uint_as_float(s_max[ch0 + cj]) * Kf, q, iq[cj], fixed);
      if (!fixed) {
        iq[cj] = 0.0f;
        any_float = true;
      }
      iq[cj] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(iq[cj])));
      // The quantum the convert phase multiplies by, kept from here: q = 2^(ex - 30) and iq = 2^(30 - ex) are both normal (-90 <= ex
      // <= 123), so q's bits are 0x7f000000 - iq's, a scalar subtraction on the wave-uniform iq (iq == 0: the float path).
      qs[cj] = __uint_as_float(0x7f000000u - __float_as_uint(iq[cj]));
    }
    // the item body of slice_bwd_sorted_kernel; the first item carries the requests of this group's feat rows
    auto item = [&](auto U) {
      constexpr int u = decltype(U)::value;
      int Y = cell[u] < 0 ? 0 : cell[u];
      // (opaque per group, the cell too: its accumulator byte offset was otherwise kept beside its tile offset, in scratch)
      asm volatile("" : "+v"(S.ent8[u][0]), "+v"(S.ent8[u][1]), "+v"(Y));
      float4 cv[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) cv[v] = T4[Y + off[v]];
      float4 xn = *(const float4*)((const unsigned char*)Sg + 2u * CT_E8(S, u, 0));
      float2 wn = *(const float2*)((const unsigned char*)AB + CT_E8(S, u, 0));
      ct_f2 s01[4], s23[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) s01[v] = s23[v] = ct_f2{0.0f, 0.0f};
#pragma unroll
      for (int j = 0; j < kItemLen; ++j) {
        if constexpr (u == 0) request_feat1(grp, j);
        const float4 x = xn;
        const float2 wf = wn;
        if (j + 1 < kItemLen) {
          xn = *(const float4*)((const unsigned char*)Sg + 2u * CT_E8(S, u, j + 1));
          wn = *(const float2*)((const unsigned char*)AB + CT_E8(S, u, j + 1));
        }
        const ct_f2 x01 = {x.x, x.y}, x23 = {x.z, x.w};
        const float w1x = wf.x, w1y = wf.y, w0x = 1.0f - w1x, w0y = 1.0f - w1y;
        const float cw[4] = {w0x * w0y, w1x * w0y, w0x * w1y, w1x * w1y};
        float gw[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const ct_f2 cwv = {cw[v], cw[v]};
          s01[v] = __builtin_elementwise_fma(x01, cwv, s01[v]);
          s23[v] = __builtin_elementwise_fma(x23, cwv, s23[v]);
          const ct_f2 c01 = {cv[v].x, cv[v].y}, c23 = {cv[v].z, cv[v].w};
          const ct_f2 pr = __builtin_elementwise_fma(c23, x23, c01 * x01);
          gw[v] = pr.x + pr.y;
        }
        gsx[u][j] = __builtin_fmaf(gw[3] - gw[2], w1y, __builtin_fmaf(gw[1] - gw[0], w0y, gsx[u][j]));
        gsy[u][j] = __builtin_fmaf(gw[3] - gw[1], w1x, __builtin_fmaf(gw[2] - gw[0], w0x, gsy[u][j]));
        asm volatile("" : "+v"(gsx[u][j]), "+v"(gsy[u][j]));
        CT_SB;
      }
      if (cell[u] >= 0) {
        const ct_f2 iq01 = {iq[0], iq[1]}, iq23 = {iq[2], iq[3]};
        int* Tc = acc + Y;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const ct_f2 a01 = s01[v] * iq01, a23 = s23[v] * iq23;
          atomicAdd(Tc + off[v], cvt_rpi(a01.x));
          atomicAdd(Tc + G + off[v], cvt_rpi(a01.y));
          atomicAdd(Tc + 2 * G + off[v], cvt_rpi(a23.x));
          atomicAdd(Tc + 3 * G + off[v], cvt_rpi(a23.y));
        }
      }
      CT_SB;
    };
    item(std::integral_constant<int, 0>{});
    if (cell[1] >= 0) item(std::integral_constant<int, 1>{});
    if (any_float) {
#pragma unroll 1
      for (int cj = 0; cj < 4; ++cj)
        if (iq[cj] == 0.0f) scatter_float_channel<HAS_PAD>(a, g, bh, b, ch0 + cj, (float*)(acc + cj * G), 1, 0);
    }
    __syncthreads();

    // ---- convert: thread = cell.  Its four accumulator words -> g_z (slice_bwd_sorted_kernel's arithmetic per word), its z word, the
    // group's non-zero cells.  (A thread per 16-byte accumulator word — four cells of one channel, one 16-byte g_z store — reads and
    // writes the interleaved words at a stride of 16 dwords: a 16-way bank conflict on each of twelve LDS operations, +18 us on
    // the headline step.  Here every LDS operation has its lanes on consecutive words; g_z leaves as four 256-byte rows per wave.)
    float4 zc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float gv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (tid < G) {
      zc = T4[tid];
#pragma unroll
      for (int cj = 0; cj < 4; ++cj) {
        const int r = acc[cj * G + tid];
        gv[cj] = iq[cj] != 0.0f ? (float)r * qs[cj] : __int_as_float(r);
        buf_st_stream(b_gz, vo_cell, (unsigned)(ch0 + cj) * cell_row, gv[cj]);
        acc[cj * G + tid] = 0;      // the thread's own words, cleared for the next group's items
      }
    }
    const unsigned zw[4] = {__float_as_uint(zc.x), __float_as_uint(zc.y), __float_as_uint(zc.z), __float_as_uint(zc.w)};
    // The pair tile goes over the stage area: read by the items only, dead since the barrier above until the next group's staging
    // behind this group's last barrier, and never smaller than 64 G bytes (the sort's histograms).  A thread has touched its own
    // words only: no barrier between the accumulators' last readers and the pair words' writers.
    if (tid < G) {
      PZ[tid] = make_float4(__uint_as_float(zw[0] ? zw[0] : kNoMatch), __uint_as_float(zw[1] ? zw[1] : kNoMatch), gv[0], gv[1]);
      PZ[G + tid] = make_float4(__uint_as_float(zw[2] ? zw[2] : kNoMatch), __uint_as_float(zw[3] ? zw[3] : kNoMatch), gv[2], gv[3]);
    }
    {
      int nzt = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) nzt += (zw[k] != 0u);
      nzt = row_sum_i32(nzt);
      if (row_last && nzt) atomicAdd(s_tie_lane + (grp & 1) * 2, nzt);
    }
    __syncthreads();

    // ---- Splat(max) backward, the optimistic pass of splat_bwd_quad<HAS_PAD, false, WT> on the thread's quad and these channels ----
    int nm = 0;
    if (has) {
      // The points' set-up is the sort's, not recomputed from the keys: the base cells parked behind the sort, (w1x, w1y) from the
      // entry's weights, w0 = 1 - w1 (bit for bit, as the items), the corner products in pt2_from_keys' order.
      const uint2 bc = s_cell[tid];
      const unsigned rk[4] = {S.rk01 & kRankMask, (S.rk01 >> 16) & kRankMask, S.rk23 & kRankMask, (S.rk23 >> 16) & kRankMask};
      const int pbase[4] = {(int)(bc.x & 0xffffu), (int)(bc.x >> 16), (int)(bc.y & 0xffffu), (int)(bc.y >> 16)};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if constexpr (decltype(more)::value) request1(grp + 1, i);      // one channel of the next group's g_out per point
        const float2 w1 = AB[rk[i]];
        Pt2 p;
        p.w1x = w1.x; p.w1y = w1.y; p.w0x = 1.0f - w1.x; p.w0y = 1.0f - w1.y;
        p.base = pbase[i];
        p.cw[0] = p.w0x * p.w0y; p.cw[1] = p.w1x * p.w0y; p.cw[2] = p.w0x * p.w1y; p.cw[3] = p.w1x * p.w1y;
        float gw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
          const float4* Zp = PZ + (size_t)pr * G + p.base;
          const float xa = HAS_PAD ? fq[2 * pr][i] * pv[i] : fq[2 * pr][i];
          const float xb = HAS_PAD ? fq[2 * pr + 1][i] * pv[i] : fq[2 * pr + 1][i];
          ct_f4 zg[4];
#pragma unroll
          for (int v = 0; v < 4; ++v) zg[v] = *(const ct_f4*)(Zp + off[v]);
          // (the general-grid instance alone keeps its loaded pairs pinned: without the pin two scratch reloads land in its group
          // loop; with it the tiled instances copy them around — 94 v_mov per group in the headline instance)
          if constexpr (WT == 0) {
#pragma unroll
            for (int v = 0; v < 4; ++v) asm volatile("" : "+v"(zg[v].x), "+v"(zg[v].y), "+v"(zg[v].z), "+v"(zg[v].w));
          }
          float gfa = 0.0f, gfb = 0.0f;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            // the products as the forward formed them (one rounding); empty cells are kNoMatch: bit equality is the winner test
            const unsigned ba = __float_as_uint(xa * p.cw[v]), bb = __float_as_uint(xb * p.cw[v]);
            const bool ma = ba == __float_as_uint(zg[v].x), mb = bb == __float_as_uint(zg[v].y);
            nm += (int)ma;
            nm += (int)mb;
            asm volatile("" : "+v"(nm));
            const float ga = ma ? zg[v].z : 0.0f, gb = mb ? zg[v].w : 0.0f;
            gfa = __builtin_fmaf(ga, p.cw[v], gfa);
            gfb = __builtin_fmaf(gb, p.cw[v], gfb);
            gw[v] = __builtin_fmaf(gb, xb, __builtin_fmaf(ga, xa, gw[v]));
          }
          fq[2 * pr][i] = HAS_PAD ? gfa * pv[i] : gfa;
          fq[2 * pr + 1][i] = HAS_PAD ? gfb * pv[i] : gfb;
        }
        gs[i][0] = __builtin_fmaf(gw[3] - gw[2], p.w1y, __builtin_fmaf(gw[1] - gw[0], p.w0y, gs[i][0]));
        gs[i][1] = __builtin_fmaf(gw[3] - gw[1], p.w1x, __builtin_fmaf(gw[2] - gw[0], p.w0x, gs[i][1]));
        asm volatile("" : "+v"(gs[i][0]), "+v"(gs[i][1]), "+v"(fq[0][i]), "+v"(fq[1][i]), "+v"(fq[2][i]), "+v"(fq[3][i]));
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int cj = 0; cj < 4; ++cj)
        buf_st_stream4(b_dst, vo_pt, (unsigned)(ch0 + cj) * pt_row, make_float4(fq[cj][0], fq[cj][1], fq[cj][2], fq[cj][3]));
    } else if constexpr (decltype(more)::value) {
#pragma unroll
      for (int cj = 0; cj < 4; ++cj) request1(grp + 1, cj);      // (a thread without a quad still stages its conv cell)
    }
    nm = row_sum_i32(nm);
    if (row_last && nm) atomicAdd(s_tie_lane + (grp & 1) * 2 + 1, nm);
    __syncthreads();
    // the group's tie test (block-uniform); the other parity's words — read behind the previous group's barrier here, added to
    // behind the next group's later barriers — are cleared for the next group
    const int* tw = s_tie + (grp & 1) * 2;
    if (tw[0] != tw[1]) tied |= 1ull << grp;
    if (tid < 2) s_tie[((grp & 1) ^ 1) * 2 + tid] = 0;
  };
  int grp = 0;
  for (; grp + 1 < ngroups; ++grp) group(grp, std::true_type{});
  group(grp, std::false_type{});

  // ---- tied groups, as splat_max_bwd_hot_kernel redoes them: the pairs staged again from z and g_z, single-winner claims, the
  // key cotangent corrected by the difference ----
  if (tied != 0ull) {           // block-uniform, rare
    // The g_z rows re-read here were stored above by other waves of THIS workgroup and by no one else in this launch; nobody
    // read them before.  Every wave waits for its own stores to be acknowledged (the release fence and the explicit wait), all
    // waves meet at the barrier, and the acquire fence keeps the loads behind it: a load issued after the barrier reaches the
    // vector cache — shared by all waves of a workgroup, write-through, holding no line of g_z from before the stores since the
    // kernel started with it invalidated and this workgroup alone touches the plane — or L2, where the stores have arrived.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    RasterArgs a2 = a;
    a2.src = feat;            // splat_bwd_quad reads the features at src
    PtRows R;
    R.Nr = N; R.so = 0; R.wt = false;
    for (int gi = 0; gi < ngroups; ++gi) {
      if (!((tied >> gi) & 1ull)) continue;
      const int cabs = gi << 2;
      const float* zin = a.tile_in + (bh * C + cabs) * (size_t)G;
      const float* gin = a.tile_out + (bh * C + cabs) * (size_t)G;
      __syncthreads();
      {
        int nz_unused = 0;
        unsigned long long nzp_unused = 0ull;
        unsigned xzp_unused = 0u;
        stage_tile_pairs<false>(ZG, zin, gin, 2, G, nz_unused, nzp_unused, xzp_unused);
      }
      __syncthreads();
      if (has) {
        const float* const key0 = a.pos.keys + bh * 2 * (size_t)N;
        const float4 tx = *(const float4*)(key0 + ln0), ty = *(const float4*)(key0 + N + ln0);
        const float kx[4] = {tx.x, tx.y, tx.z, tx.w}, ky[4] = {ty.x, ty.y, ty.z, ty.w};
        int nm_unused = 0;
        unsigned u0 = 0u, u1 = 0u;
        splat_bwd_quad<HAS_PAD, true, WT, true>(a2, g, ZG, bh, b, cabs, 4, n0, R, kx, ky, gs, nm_unused, u0, u1, false);
      }
    }
    __syncthreads();          // the stage area below is not the pair tile, but the claims' readers are done with LDS here
  }

  // ---- key cotangents: Slice's from the item owners to the point owners through LDS, Splat's from the registers ----
  float2* Gs = (float2*)Sg;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int j = 0; j < kItemLen; ++j)
      *(float2*)((unsigned char*)Gs + CT_E8(S, u, j)) = make_float2(gsx[u][j], gsy[u][j]);
  __syncthreads();
  if (has) {
    const unsigned rw[4] = {S.rk01 & 0xffffu, S.rk01 >> 16, S.rk23 & 0xffffu, S.rk23 >> 16};
    float2 gk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gk[i] = Gs[rw[i] & kRankMask];
      gk[i].x *= (rw[i] & kInsideX) ? 1.0f : 0.0f;
      gk[i].y *= (rw[i] & kInsideY) ? 1.0f : 0.0f;
    }
    if (a.fold_gpos != nullptr) {
      st_stream4(a.fold_gpos + (bh * 2 + 0) * N + n0, make_float4(gk[0].x, gk[1].x, gk[2].x, gk[3].x));
      st_stream4(a.fold_gpos + (bh * 2 + 1) * N + n0, make_float4(gk[0].y, gk[1].y, gk[2].y, gk[3].y));
    }
    // gs * mask + add: the order of splat_max_bwd_hot_kernel's store with an incoming cotangent; the mask is the rank's clamp flag
    // (ct_key_mask's {0, 1}, taken by the sort)
    float mx[4], my[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      mx[i] = (rw[i] & kInsideX) ? 1.0f : 0.0f;
      my[i] = (rw[i] & kInsideY) ? 1.0f : 0.0f;
    }
    float4 ox = make_float4(gs[0][0] * mx[0], gs[1][0] * mx[1], gs[2][0] * mx[2], gs[3][0] * mx[3]);
    float4 oy = make_float4(gs[0][1] * my[0], gs[1][1] * my[1], gs[2][1] * my[2], gs[3][1] * my[3]);
    ox.x += gk[0].x; ox.y += gk[1].x; ox.z += gk[2].x; ox.w += gk[3].x;
    oy.x += gk[0].y; oy.y += gk[1].y; oy.z += gk[2].y; oy.w += gk[3].y;
    *(float4*)(a.g_pos + (bh * 2 + 0) * N + n0) = ox;
    *(float4*)(a.g_pos + (bh * 2 + 1) * N + n0) = oy;
  }
}
