// Chamfer distance for gfx950: brute-force bidirectional nearest neighbour and
// its gradient (replaces chamfer_extension/chamfer.cu:12-195 of the reference).
//
// Forward is O(n*m) fp32 VALU work.  One 1024-thread workgroup owns 64*Q query
// points (Q per lane, in registers); each of its 16 waves scans one sixteenth
// of the target cloud.  Target coordinates are wave-uniform, so they are fetched
// with scalar loads (s_load_dwordx*) straight into SGPRs — no LDS staging and
// no barriers in the scan loop.  The 16 partial (min, argmin) pairs are
// merged through LDS in ascending target order, which preserves the
// reference's tie rule (strict '<' while scanning ascending: lowest index
// wins, chamfer.cu:36,46,126).
//
// The *_counts entry points take clouds of different lengths in one batch (a template flag on the same kernels); further
// down, the row filter ct_rows_compact and the per-cloud metric table ct_chamfer_metrics of the batched evaluation.
#include "ct_common.h"

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int kUnroll = 8;     // targets per scalar-load batch
constexpr int kWaves = 16;     // waves per workgroup = target slices (B*n/256 query groups alone would
                               // leave most of the 256 CUs idle: 16 slices give ~2k waves at n = 16k)

// kQ = queries per lane (4, or 2 when 256-query workgroups would leave CUs without one).
// kCounts (ct_chamfer_fwd_counts): cloud b has cnt_q[b] query rows and cnt_t[b] target rows of the n_pad and m_pad the
// arrays are strided by (a null pointer: all of them); from there on n and m are the cloud's own.  Both are wave-uniform and
// read once; the rows at or beyond a count are never loaded, as queries or as targets, and the target slices `per`, `j_beg`,
// `j_end` are cut from the cloud's own m, so rows below the count get the bits the dense kernel gives that pair alone (the
// minimum is exact, and the lowest index wins a tie however the targets are dealt to waves).  Rows from n on, and every row
// when m == 0, get dist 0 / idx -1.  A workgroup whose first query is past n writes those and leaves before any barrier.  The dense instantiations
// (kCounts = false) never touch the two pointers and compile to the instructions they had before the flag.
template <int kQ, bool kCounts>
__global__ void __launch_bounds__(64 * kWaves)
nn_kernel(const float* __restrict__ q, const float* __restrict__ t, float* __restrict__ dist,
          int* __restrict__ idx, int n, int m, const int* __restrict__ cnt_q, const int* __restrict__ cnt_t) {
  __shared__ float s_best[kWaves][64 * kQ];
  __shared__ int s_idx[kWaves][64 * kQ];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q0 = blockIdx.x * (64 * kQ);
  const int n_pad = n, m_pad = m;            // the strides of the arrays
  if constexpr (kCounts) {
    if (cnt_q) n = min(max(cnt_q[b], 0), n_pad);      // (the clamps are guards: a count is within its array)
    if (cnt_t) m = min(max(cnt_t[b], 0), m_pad);
    if (q0 >= n || m == 0) {                  // wave-uniform: nothing to search for this workgroup's rows
      const int i = q0 + threadIdx.x;
      if (threadIdx.x < 64 * kQ && i < n_pad) {
        dist[(size_t)b * n_pad + i] = 0.0f;
        idx[(size_t)b * n_pad + i] = -1;
      }
      return;
    }
  }
  q += (size_t)b * n_pad * 3;
  t += (size_t)b * m_pad * 3;

  // Queries sit in registers as float pairs so the distance arithmetic runs on the packed fp32 pipe
  // (v_pk_add/mul/fma_f32: two queries per issue slot).  The scan only tracks, per query, the running minimum and
  // the 8-target block it came from (one compare per block instead of one per target); the index inside the block
  // is recovered afterwards by recomputing those 8 distances with the same expression.
  f2 qx[kQ / 2], qy[kQ / 2], qz[kQ / 2];
  float best[kQ];
  int blk[kQ];
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    int i = min(q0 + k * 64 + lane, n - 1);
    qx[k >> 1][k & 1] = q[i * 3 + 0];
    qy[k >> 1][k & 1] = q[i * 3 + 1];
    qz[k >> 1][k & 1] = q[i * 3 + 2];
    best[k] = __builtin_inff();
    blk[k] = 0;
  }
  const int per = (m + kWaves - 1) / kWaves;
  const int j_beg = min(wave * per, m);
  const int j_end = min(m, j_beg + per);
  auto dist2 = [&](int p, float tx, float ty, float tz) -> f2 {
    const f2 dx = f2{tx, tx} - qx[p], dy = f2{ty, ty} - qy[p], dz = f2{tz, tz} - qz[p];
    return __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
  };
  auto scan_block = [&](int j, const float* buf) {
#pragma unroll
    for (int p = 0; p < kQ / 2; ++p) {
      f2 mn = dist2(p, buf[0], buf[1], buf[2]);
#pragma unroll
      for (int u = 1; u < kUnroll; ++u) {
        const f2 d = dist2(p, buf[3 * u], buf[3 * u + 1], buf[3 * u + 2]);
        mn.x = fminf(mn.x, d.x), mn.y = fminf(mn.y, d.y);
      }
      if (mn.x < best[2 * p]) best[2 * p] = mn.x, blk[2 * p] = j;          // strict: the earlier block keeps a tie
      if (mn.y < best[2 * p + 1]) best[2 * p + 1] = mn.y, blk[2 * p + 1] = j;
    }
  };
  int j = j_beg;
  const float* tp = t + (size_t)j_beg * 3;   // wave-uniform address -> scalar loads
  for (; j + kUnroll <= j_end; j += kUnroll, tp += 3 * kUnroll) {
    float buf[3 * kUnroll];
#pragma unroll
    for (int u = 0; u < 3 * kUnroll; ++u) buf[u] = tp[u];
    scan_block(j, buf);
  }
  if (j < j_end) {                           // ragged last block: repeat the slice's last target
    float buf[3 * kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int o = 3 * (min(j + u, j_end - 1) - j);
      buf[3 * u] = tp[o], buf[3 * u + 1] = tp[o + 1], buf[3 * u + 2] = tp[o + 2];
    }
    scan_block(j, buf);
  }
  int bi[kQ];
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    bi[k] = 0;
    if (j_beg < j_end) {
#pragma unroll
      for (int u = kUnroll - 1; u >= 0; --u) {   // descending, so the lowest index among equal distances wins
        const int jj = min(blk[k] + u, j_end - 1);
        const float dx = t[jj * 3 + 0] - qx[k >> 1][k & 1], dy = t[jj * 3 + 1] - qy[k >> 1][k & 1],
                    dz = t[jj * 3 + 2] - qz[k >> 1][k & 1];
        if (fmaf(dz, dz, fmaf(dy, dy, dx * dx)) == best[k]) bi[k] = jj;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    s_best[wave][k * 64 + lane] = best[k];
    s_idx[wave][k * 64 + lane] = bi[k];
  }
  __syncthreads();
  if (threadIdx.x < 64 * kQ) {
    float bb = s_best[0][threadIdx.x];
    int ii = s_idx[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      float o = s_best[w][threadIdx.x];
      if (o < bb) {   // strict: the earlier (lower-index) range wins ties
        bb = o;
        ii = s_idx[w][threadIdx.x];
      }
    }
    int i = q0 + threadIdx.x;
    if (i < n) {
      dist[(size_t)b * n_pad + i] = bb;
      idx[(size_t)b * n_pad + i] = ii;
    } else if (kCounts && i < n_pad) {
      dist[(size_t)b * n_pad + i] = 0.0f;
      idx[(size_t)b * n_pad + i] = -1;
    }
  }
}

// chamfer.cu:155-174: g = 2*grad_dist[i]; grad_a[i] += g (a_i - b_idx);  grad_b[idx] -= g (a_i - b_idx)
// kCounts (ct_chamfer_bwd_counts): only the rows below cnt_a[b] contribute; a cloud whose target cloud is empty (idx -1)
// contributes nothing.  The rows at or beyond a count keep the +0.0 of the memset.
template <bool kCounts>
__global__ void nn_grad_kernel(const float* __restrict__ a, const float* __restrict__ bpts,
                               const float* __restrict__ g_dist, const int* __restrict__ idx,
                               float* g_a, float* g_b, int n, int m, const int* __restrict__ cnt_a,
                               const int* __restrict__ cnt_b) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if constexpr (kCounts) {
    if (cnt_a && i >= cnt_a[b]) return;
    if (cnt_b && cnt_b[b] <= 0) return;
  }
  const size_t ia = ((size_t)b * n + i) * 3;
  const int j = idx[(size_t)b * n + i];
  if constexpr (kCounts) {
    if (j < 0 || j >= m) return;             // a guard: the forward's indices of rows below the count are in range
  }
  const size_t ib = ((size_t)b * m + j) * 3;
  const float g = g_dist[(size_t)b * n + i] * 2.0f;
  const float dx = g * (a[ia + 0] - bpts[ib + 0]);
  const float dy = g * (a[ia + 1] - bpts[ib + 1]);
  const float dz = g * (a[ia + 2] - bpts[ib + 2]);
  atomicAdd(&g_a[ia + 0], dx);
  atomicAdd(&g_a[ia + 1], dy);
  atomicAdd(&g_a[ia + 2], dz);
  atomicAdd(&g_b[ib + 0], -dx);
  atomicAdd(&g_b[ib + 1], -dy);
  atomicAdd(&g_b[ib + 2], -dz);
}

// Deterministic form (ct_set_deterministic): every destination row of cloud `a` is written once, by the lane that owns it.
//   g_a[i] = 2 g_dist_a[i] (a_i - b_idx_a[i])                                  its own term first,
//          + sum over j with idx_b[j] == i, ascending j, of -(2 g_dist_b[j] (b_j - a_i))   then its sources in index order
// — the very terms nn_grad_kernel adds with atomics in arrival order.  A wave owns kDetDst consecutive destinations (lane d
// keeps the sum of i0 + d) and scans idx_b 64 entries at a time: O(n m / (64 kDetDst)) coalesced integer loads per cloud, no
// sort.  The matches of a block are added lane by lane, lowest j first, each by the lane of its destination.
// kDetDst = 8 where that still leaves a few waves per CU (B2 n = m = 16384: 350 -> 112 us against one destination per wave),
// 1 for a small destination cloud, whose few rows take many sources each and would otherwise queue up in one wave.
constexpr int kDetWaves = 4;
// kCounts (ct_chamfer_bwd_counts): the cloud's own na = cnt_a[b] and mb = cnt_b[b] bound the rows that have a term of their
// own and the sources that are scanned; the order of a row's terms is the dense kernel's on that pair alone, so the bits
// are too.  Rows from na on are written +0.0 (nothing is cleared beforehand in this form), without a scan when the wave's
// first row is past na.
template <int kDetDst, bool kCounts>
__global__ void __launch_bounds__(64 * kDetWaves)
nn_grad_det_kernel(const float* __restrict__ a, const float* __restrict__ bpts, const float* __restrict__ g_dist_a,
                   const float* __restrict__ g_dist_b, const int* __restrict__ idx_a, const int* __restrict__ idx_b,
                   float* __restrict__ g_a, int n, int m, const int* __restrict__ cnt_a, const int* __restrict__ cnt_b) {
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int i0 = (blockIdx.x * kDetWaves + (threadIdx.x >> 6)) * kDetDst;      // wave-uniform
  if (i0 >= n) return;
  const int n_pad = n, m_pad = m;            // the strides of the arrays
  if constexpr (kCounts) {
    if (cnt_a) n = min(max(cnt_a[b], 0), n_pad);
    if (cnt_b) m = min(max(cnt_b[b], 0), m_pad);
    if (i0 >= n) {                            // wave-uniform: padding rows only
      const int i = i0 + lane;
      if (lane < kDetDst && i < n_pad) {
        const size_t ia = ((size_t)b * n_pad + i) * 3;
        g_a[ia + 0] = 0.0f, g_a[ia + 1] = 0.0f, g_a[ia + 2] = 0.0f;
      }
      return;
    }
  }
  const float* ap = a + (size_t)b * n_pad * 3;
  const float* bp = bpts + (size_t)b * m_pad * 3;
  const int* ib = idx_b + (size_t)b * m_pad;
  const float* gb = g_dist_b + (size_t)b * m_pad;
  const int i = i0 + lane;
  const bool pad = kCounts && lane < kDetDst && i >= n && i < n_pad;      // a padding row in a wave that has real ones
  const bool own = lane < kDetDst && i < n;
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  if (own && (!kCounts || m > 0)) {          // (an empty target cloud: idx_a is -1, no term)
    const int j = kCounts ? min(max(idx_a[(size_t)b * n_pad + i], 0), m - 1) : idx_a[(size_t)b * n_pad + i];
    const float g = g_dist_a[(size_t)b * n_pad + i] * 2.0f;
    sx = g * (ap[(size_t)i * 3 + 0] - bp[(size_t)j * 3 + 0]);
    sy = g * (ap[(size_t)i * 3 + 1] - bp[(size_t)j * 3 + 1]);
    sz = g * (ap[(size_t)i * 3 + 2] - bp[(size_t)j * 3 + 2]);
  }
  for (int j0 = 0; j0 < m; j0 += 64) {
    const int j = j0 + lane;
    const int d = (j < m ? ib[j] : -1) - i0;          // which of the wave's destinations this source feeds, if any
    const bool hit = j < m && d >= 0 && d < kDetDst && (!kCounts || i0 + d < n);  // (idx_b < n: i0 + d is a row of the cloud)
    unsigned long long mask = __ballot(hit);
    if (mask == 0ull) continue;
    float tx = 0.0f, ty = 0.0f, tz = 0.0f;
    if (hit) {
      const float g = gb[j] * 2.0f;
      const size_t ia = (size_t)(i0 + d) * 3;
      tx = -(g * (bp[(size_t)j * 3 + 0] - ap[ia + 0]));
      ty = -(g * (bp[(size_t)j * 3 + 1] - ap[ia + 1]));
      tz = -(g * (bp[(size_t)j * 3 + 2] - ap[ia + 2]));
    }
    while (mask) {
      const int l = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int dd = __shfl(d, l);
      const float vx = __shfl(tx, l), vy = __shfl(ty, l), vz = __shfl(tz, l);
      if (lane == dd) {
        sx += vx;
        sy += vy;
        sz += vz;
      }
    }
  }
  if (own || pad) {                          // (a padding lane never matched: its sums are still +0.0)
    const size_t ia = ((size_t)b * n_pad + i) * 3;
    g_a[ia + 0] = sx;
    g_a[ia + 1] = sy;
    g_a[ia + 2] = sz;
  }
}

// Both directions of the search; kCounts picks the instantiation, the kQ rule is the dense one on the arrays' n and m.
template <bool kCounts>
void launch_nn_pair(const float* xyz1, const float* xyz2, const int32_t* cnt1, const int32_t* cnt2, float* dist1, float* dist2,
                    int32_t* idx1, int32_t* idx2, int B, int n, int m, hipStream_t st) {
  auto launch = [&](const float* q, const float* t, float* d, int32_t* i, int nq, int nt, const int32_t* cq, const int32_t* ct) {
    if ((size_t)B * ((nq + 255) / 256) >= 256 /* CUs on MI355X */)
      hipLaunchKernelGGL((nn_kernel<4, kCounts>), dim3((nq + 255) / 256, B), dim3(64 * kWaves), 0, st, q, t, d, i, nq, nt, cq, ct);
    else
      hipLaunchKernelGGL((nn_kernel<2, kCounts>), dim3((nq + 127) / 128, B), dim3(64 * kWaves), 0, st, q, t, d, i, nq, nt, cq, ct);
  };
  launch(xyz1, xyz2, dist1, idx1, n, m, cnt1, cnt2);
  launch(xyz2, xyz1, dist2, idx2, m, n, cnt2, cnt1);
}

template <bool kCounts>
int launch_nn_grad_pair(const float* xyz1, const float* xyz2, const int32_t* cnt1, const int32_t* cnt2, const float* g_dist1,
                        const float* g_dist2, const int32_t* idx1, const int32_t* idx2, float* g_xyz1, float* g_xyz2, int B, int n,
                        int m, hipStream_t st) {
  if (ct_get_deterministic()) {      // ordered form: every row written once by the lane that owns it, nothing to clear
    CT_CLEAR_ERROR();
    auto launch = [&](const float* a, const float* b, const float* ga, const float* gb, const int32_t* ia, const int32_t* ib,
                      float* out, int na, int nb, const int32_t* ca, const int32_t* cb) {
      if ((long long)B * na >= 8 * 1024) {        // >= 1024 waves of eight rows
        constexpr int per = kDetWaves * 8;        // destination rows per workgroup
        hipLaunchKernelGGL((nn_grad_det_kernel<8, kCounts>), dim3((na + per - 1) / per, B), dim3(64 * kDetWaves), 0, st, a, b, ga, gb, ia,
                           ib, out, na, nb, ca, cb);
      } else {
        hipLaunchKernelGGL((nn_grad_det_kernel<1, kCounts>), dim3((na + kDetWaves - 1) / kDetWaves, B), dim3(64 * kDetWaves), 0, st, a, b,
                           ga, gb, ia, ib, out, na, nb, ca, cb);
      }
    };
    launch(xyz1, xyz2, g_dist1, g_dist2, idx1, idx2, g_xyz1, n, m, cnt1, cnt2);
    launch(xyz2, xyz1, g_dist2, g_dist1, idx2, idx1, g_xyz2, m, n, cnt2, cnt1);
    CT_CHECK_LAUNCH();
    return CT_OK;
  }
  if (hipMemsetAsync(g_xyz1, 0, (size_t)B * n * 3 * 4, st) != hipSuccess) return CT_ELAUNCH;
  if (hipMemsetAsync(g_xyz2, 0, (size_t)B * m * 3 * 4, st) != hipSuccess) return CT_ELAUNCH;
  CT_CLEAR_ERROR();
  hipLaunchKernelGGL(nn_grad_kernel<kCounts>, dim3((n + 255) / 256, B), dim3(256), 0, st, xyz1, xyz2, g_dist1, idx1, g_xyz1, g_xyz2, n, m,
                     cnt1, cnt2);
  hipLaunchKernelGGL(nn_grad_kernel<kCounts>, dim3((m + 255) / 256, B), dim3(256), 0, st, xyz2, xyz1, g_dist2, idx2, g_xyz2, g_xyz1, m, n,
                     cnt2, cnt1);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// ct_rows_compact: per cloud, the rows with (x + y) + z != 0 in their input order, then zero rows, and the number kept
// (utils/grdnet_utils.py:19-21, the boolean index of `ignore_zeros`, for a whole batch).  One workgroup per cloud walks it
// kCompactThreads rows at a time: a ballot per wave, the waves' popcounts through LDS (two alternating sets, so one barrier
// per step), rank = rows kept so far + waves before + lanes below.  No atomics: the order is the input order on every run.
constexpr int kCompactThreads = 1024;
constexpr int kCompactWaves = kCompactThreads / CT_WAVE;

__global__ void __launch_bounds__(kCompactThreads)
rows_compact_kernel(const float* __restrict__ x, float* __restrict__ y, int32_t* __restrict__ count, int n) {
  __shared__ int wcnt[2][kCompactWaves];
  const int b = blockIdx.x, t = threadIdx.x;
  const int lane = t & (CT_WAVE - 1), wave = t / CT_WAVE;
  const float* X = x + (size_t)b * n * 3;
  float* Y = y + (size_t)b * n * 3;
  int base = 0;                                                       // rows kept so far (the same in every thread)
  for (int c0 = 0, par = 0; c0 < n; c0 += kCompactThreads, par ^= 1) {
    const int i = c0 + t;
    float vx = 0.0f, vy = 0.0f, vz = 0.0f;
    if (i < n) vx = X[3 * (size_t)i + 0], vy = X[3 * (size_t)i + 1], vz = X[3 * (size_t)i + 2];
    const bool keep = i < n && (vx + vy) + vz != 0.0f;                // torch.sum(xyz, dim=2).ne(0): NaN is kept
    const unsigned long long mk = __ballot(keep);
    if (lane == 0) wcnt[par][wave] = __popcll(mk);
    __syncthreads();
    int before = 0, total = 0;
    for (int k = 0; k < kCompactWaves; ++k) {
      const int c = wcnt[par][k];
      if (k < wave) before += c;
      total += c;
    }
    if (keep) {
      const size_t r = (size_t)(base + before + __popcll(mk & ((1ull << lane) - 1ull)));       // r <= i
      Y[3 * r + 0] = vx, Y[3 * r + 1] = vy, Y[3 * r + 2] = vz;
    }
    base += total;
  }
  for (int i = base + t; i < n; i += kCompactThreads) Y[3 * (size_t)i + 0] = 0.0f, Y[3 * (size_t)i + 1] = 0.0f, Y[3 * (size_t)i + 2] = 0.0f;
  if (t == 0) count[b] = base;
}

// ---------------------------------------------------------------------------------------------------------------------
// ct_chamfer_metrics: one workgroup per cloud, each direction in turn.  A thread takes the rows t, t + 256, ... of
// [0, cnt) in order; its three partials meet the other lanes' in a fixed xor tree and the four waves' in wave order, so the
// sums are the same bits on every run.  hits counts sqrtf(d) < th in float32; both sums are float64.
constexpr int kMetricThreads = 256;
constexpr int kMetricWaves = kMetricThreads / CT_WAVE;

__device__ __forceinline__ void metric_direction(const float* __restrict__ d, int cnt, float th, int t, double (*sh)[3], double out[3]) {
  const int lane = t & (CT_WAVE - 1), wave = t / CT_WAVE;
  double hits = 0.0, sd = 0.0, ss = 0.0;                              // (hits: an exact integer below 2^53)
  for (int i = t; i < cnt; i += kMetricThreads) {
    const float v = d[i];
    const float r = sqrtf(v);
    hits += r < th ? 1.0 : 0.0;
    sd += (double)v;
    ss += (double)r;
  }
  for (int o = CT_WAVE / 2; o > 0; o >>= 1) {
    hits += __shfl_xor(hits, o);
    sd += __shfl_xor(sd, o);
    ss += __shfl_xor(ss, o);
  }
  __syncthreads();                                                    // (sh is free again: the previous direction was read)
  if (lane == 0) sh[wave][0] = hits, sh[wave][1] = sd, sh[wave][2] = ss;
  __syncthreads();
  out[0] = out[1] = out[2] = 0.0;
  for (int w = 0; w < kMetricWaves; ++w) out[0] += sh[w][0], out[1] += sh[w][1], out[2] += sh[w][2];
}

__global__ void __launch_bounds__(kMetricThreads)
chamfer_metrics_kernel(const float* __restrict__ dist1, const float* __restrict__ dist2, const int32_t* __restrict__ cnt1,
                       const int32_t* __restrict__ cnt2, float th, double* __restrict__ stats, float* __restrict__ table, int n,
                       int m) {
  __shared__ double sh[kMetricWaves][3];
  const int b = blockIdx.x, t = threadIdx.x;
  const int c1 = cnt1 ? min(max(cnt1[b], 0), n) : n, c2 = cnt2 ? min(max(cnt2[b], 0), m) : m;
  double s1[3], s2[3];
  metric_direction(dist1 + (size_t)b * n, c1, th, t, sh, s1);
  metric_direction(dist2 + (size_t)b * m, c2, th, t, sh, s2);
  if (t != 0) return;
  if (stats) {
    double* S = stats + (size_t)b * 6;
    S[0] = s1[0], S[1] = s1[1], S[2] = s1[2], S[3] = s2[0], S[4] = s2[1], S[5] = s2[2];
  }
  float f = 0.0f, p = 0.0f, r = 0.0f, c = __builtin_nanf("");
  if (c1 > 0 && c2 > 0) {
    p = (float)s1[0] * (1.0f / (float)c1);              // torch's mean: the sum times the float32 reciprocal of the length
    r = (float)s2[0] * (1.0f / (float)c2);
    const float s = r + p;
    f = s > 0.0f ? 2.0f * r * p / s : 0.0f;
    c = (float)(s1[1] / (double)c1 + s2[1] / (double)c2);
  }
  float* T = table + (size_t)b * 4;
  T[0] = f, T[1] = p, T[2] = r, T[3] = c;
}

}  // namespace

extern "C" {

int ct_chamfer_fwd(const float* xyz1, const float* xyz2, float* dist1, float* dist2, int32_t* idx1, int32_t* idx2,
                   int B, int n, int m, ct_stream_t s) {
  if (!xyz1 || !xyz2 || !dist1 || !dist2 || !idx1 || !idx2 || B <= 0 || n <= 0 || m <= 0 || B > 65535) return CT_EINVAL;
  CT_CLEAR_ERROR();
  launch_nn_pair<false>(xyz1, xyz2, nullptr, nullptr, dist1, dist2, idx1, idx2, B, n, m, (hipStream_t)s);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

int ct_chamfer_fwd_counts(const float* xyz1, const float* xyz2, const int32_t* cnt1, const int32_t* cnt2, float* dist1, float* dist2,
                          int32_t* idx1, int32_t* idx2, int B, int n, int m, ct_stream_t s) {
  if (!xyz1 || !xyz2 || !dist1 || !dist2 || !idx1 || !idx2 || B <= 0 || n <= 0 || m <= 0 || B > 65535) return CT_EINVAL;
  CT_CLEAR_ERROR();
  launch_nn_pair<true>(xyz1, xyz2, cnt1, cnt2, dist1, dist2, idx1, idx2, B, n, m, (hipStream_t)s);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

int ct_chamfer_bwd(const float* xyz1, const float* xyz2, const float* g_dist1, const float* g_dist2,
                   const int32_t* idx1, const int32_t* idx2, float* g_xyz1, float* g_xyz2,
                   int B, int n, int m, ct_stream_t s) {
  if (!xyz1 || !xyz2 || !g_dist1 || !g_dist2 || !idx1 || !idx2 || !g_xyz1 || !g_xyz2 || B <= 0 || n <= 0 || m <= 0 || B > 65535)
    return CT_EINVAL;
  return launch_nn_grad_pair<false>(xyz1, xyz2, nullptr, nullptr, g_dist1, g_dist2, idx1, idx2, g_xyz1, g_xyz2, B, n, m, (hipStream_t)s);
}

int ct_chamfer_bwd_counts(const float* xyz1, const float* xyz2, const int32_t* cnt1, const int32_t* cnt2, const float* g_dist1,
                          const float* g_dist2, const int32_t* idx1, const int32_t* idx2, float* g_xyz1, float* g_xyz2,
                          int B, int n, int m, ct_stream_t s) {
  if (!xyz1 || !xyz2 || !g_dist1 || !g_dist2 || !idx1 || !idx2 || !g_xyz1 || !g_xyz2 || B <= 0 || n <= 0 || m <= 0 || B > 65535)
    return CT_EINVAL;
  return launch_nn_grad_pair<true>(xyz1, xyz2, cnt1, cnt2, g_dist1, g_dist2, idx1, idx2, g_xyz1, g_xyz2, B, n, m, (hipStream_t)s);
}

int ct_rows_compact(const float* x, float* y, int32_t* count, int B, int n, ct_stream_t s) {
  if (!x || !y || !count || x == y || B <= 0 || n <= 0 || B > 65535) return CT_EINVAL;
  CT_CLEAR_ERROR();
  hipLaunchKernelGGL(rows_compact_kernel, dim3(B), dim3(kCompactThreads), 0, (hipStream_t)s, x, y, count, n);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

int ct_chamfer_metrics(const float* dist1, const float* dist2, const int32_t* cnt1, const int32_t* cnt2, float th, double* stats,
                       float* table, int B, int n, int m, ct_stream_t s) {
  if (!dist1 || !dist2 || !table || B <= 0 || n <= 0 || m <= 0 || B > 65535) return CT_EINVAL;
  CT_CLEAR_ERROR();
  hipLaunchKernelGGL(chamfer_metrics_kernel, dim3(B), dim3(kMetricThreads), 0, (hipStream_t)s, dist1, dist2, cnt1, cnt2, th, stats,
                     table, n, m);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

}  // extern "C"
