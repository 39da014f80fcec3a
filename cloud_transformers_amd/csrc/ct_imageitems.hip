// Batch assembly of the What3D single-view reconstruction items for gfx950 (datasets/image_point.py:128-150 with the collate
// folded in) in one launch: per batch row the stored RGB image resized the way Pillow's 8-bit BILINEAR resample does it, then
// ToTensor and Normalize, written planar; and `resample_pcd` of the row's cloud, written channels first.
//
// The grid is (image bands + point groups, B).  blockIdx.x below `bands` is an image workgroup, the rest are point workgroups.
//
// Image workgroup (b, band of R output rows).  Pillow resamples in two integer passes, horizontal first, with 8-bit
// intermediates; the band's vertical taps reach source rows r0 .. r0 + rows - 1 (from the `by` table), so:
//   1. four source rows at a time, one per wave: the row's interleaved RGB bytes come in as coalesced dword loads (the row
//      start rounded down to 4 bytes; the dword that would reach past the end of the stored set is read byte by byte) into the
//      wave's row buffer in LDS; then lane xx runs output column xx's taps on the three channels out of that buffer and writes
//      the three bytes into the staged plane [row][channel][OW].
//   2. the vertical pass runs on the staged bytes: work-items walk (y, channel, xx) with xx fastest, so a wave reads 64
//      consecutive bytes of one staged row per tap (16 banks, four lanes per dword: no conflict) and stores 64 consecutive
//      floats.  The float stage is v = ((float)byte / 255.0f - mean) / std, each operation one fp32 rounding.
// R is sized by the host so that the staged rows fit kStageBytes, and no smaller than needed to keep every CU busy; source rows
// shared by neighbouring bands are resampled by both.
//
// Point workgroup (b, group g of G): every group recomputes the row's flags `perm[b, j] < P` and their exclusive scan in its
// own LDS (<= 1024 ballot words), then handles its slice of the positions j: a flagged position of rank r < min(n, P) writes
// slot r; and its slice of the top-up slots P .. n-1.  Nothing is published between workgroups (ct_completion.hip's scheme).
//
// Integer arithmetic and plain vector loads and stores only.
#include "ct_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / CT_WAVE;
constexpr int kTapsMax = 64;                          // taps of one output pixel per axis
constexpr int kWMax = 2048;                           // source width: a row of 3 * W bytes (+ 3 of alignment) per wave in LDS
constexpr int kRowDwords = (3 * kWMax + 3 + 3) / 4 + 1;
constexpr int kStageBytes = 36 * 1024;                // the band's horizontally resampled rows
constexpr int kSizeMax = 4096;                        // H, OH, OW
constexpr int kBandMin = 2;                           // output rows of a band at least (a band's time is its rounds of four source rows)
constexpr int kGroupsTarget = 256;                    // image workgroups the launch aims at (one per CU)
constexpr int kPMax = 1 << 16;                        // points of one stored cloud: 1024 ballot words
constexpr int kWords = kPMax / CT_WAVE;
constexpr int kWordsPerThread = kWords / kThreads;
constexpr int kNMax = 1 << 20;                        // slots of one output cloud
constexpr int kPointGroupsMax = 16;
constexpr int kSlotsPerGroup = 2048;
constexpr int kFlagWords = 4;                         // ballot words a wave takes per step of the flag pass
constexpr int kPrecisionBits = 32 - 8 - 2;            // Pillow's PRECISION_BITS
static_assert(kWords % kThreads == 0, "the scan takes a whole number of words per thread");
static_assert(kWaves * kRowDwords * 4 + kStageBytes <= 64 * 1024, "static LDS of the image workgroup");

struct ImageArgs {
  const uint8_t* images;
  long long M, total_bytes;
  int H, W, OH, OW, ksx, ksy, R, rows_cap, bands;
  const int32_t *kx, *bx, *ky, *by;
  float mean[3], stdv[3];
  float* out_img;
};

struct PointArgs {
  const float* points;
  const int64_t* offsets;
  const int64_t* perm;
  const float* u_dup;
  int p_cap, n, G;
  float* out_pcd;
};

__device__ __forceinline__ int clamp_i(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int rank_below(unsigned long long m, int bit) { return __popcll(m & ((1ull << bit) - 1ull)); }
__device__ __forceinline__ int clip8(int acc) { return clamp_i(acc >> kPrecisionBits, 0, 255); }

__device__ void image_group(const ImageArgs& a, long long g, int b, int band, uint32_t (*rowbuf)[kRowDwords], uint8_t* stage) {
  const int t = threadIdx.x, lane = t & (CT_WAVE - 1), wave = t / CT_WAVE;
  const int H = a.H, W = a.W, OH = a.OH, OW = a.OW;
  const int y0 = band * a.R, y1 = min(OH, y0 + a.R);
  // the source rows the band's taps reach; the clamps are guards, the tables of a valid caller never need them
  const int r0 = clamp_i(a.by[2 * y0], 0, H - 1);
  const int r_end = a.by[2 * (y1 - 1)] + a.by[2 * (y1 - 1) + 1];
  const int rows = clamp_i(r_end - r0, 1, min(a.rows_cap, H - r0));
  const long long row_bytes = 3ll * W;
  const long long base = g * H * row_bytes;

  // 1. horizontal pass, one source row per wave
  for (int rb = 0; rb < rows; rb += kWaves) {
    const int r = rb + wave;
    int shift = 0;
    if (r < rows) {
      const long long first = base + (r0 + r) * row_bytes;             // byte offset of the row in the stored set
      const long long d0 = first >> 2;
      shift = (int)(first & 3);
      const int nd = (int)(((first + row_bytes + 3) >> 2) - d0);          // dwords that cover the row
      const uint32_t* src = (const uint32_t*)a.images;                  // (4-byte aligned: checked by the entry point)
      for (int d = lane; d < nd; d += CT_WAVE) {
        const long long at = (d0 + d) * 4;
        uint32_t v;
        if (at + 4 <= a.total_bytes) {
          v = src[d0 + d];
        } else {                                                         // the last dword of the set, cut short
          v = 0;
          for (int e = 0; e < 4; ++e)
            if (at + e < a.total_bytes) v |= (uint32_t)a.images[at + e] << (8 * e);
        }
        rowbuf[wave][d] = v;
      }
    }
    __syncthreads();
    if (r < rows) {
      const uint8_t* px = (const uint8_t*)rowbuf[wave] + shift;
      uint8_t* dst = stage + (size_t)r * 3 * OW;
      for (int xx = lane; xx < OW; xx += CT_WAVE) {
        const int taps = clamp_i(a.bx[2 * xx + 1], 0, min(a.ksx, W));
        const int xmin = clamp_i(a.bx[2 * xx], 0, W - taps);
        const int32_t* k = a.kx + (size_t)xx * a.ksx;
        int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
        for (int x = 0; x < taps; ++x) {
          const int w = k[x];
          const uint8_t* p = px + 3 * (xmin + x);
          s0 += (int)p[0] * w, s1 += (int)p[1] * w, s2 += (int)p[2] * w;
        }
        dst[xx] = (uint8_t)clip8(s0), dst[OW + xx] = (uint8_t)clip8(s1), dst[2 * OW + xx] = (uint8_t)clip8(s2);
      }
    }
    __syncthreads();
  }

  // 2. vertical pass on the staged bytes, the float stage, planar stores
  const int per_row = 3 * OW, work = (y1 - y0) * per_row;
  for (int i = t; i < work; i += kThreads) {
    const int y = y0 + i / per_row, rem = i % per_row;
    const int c = rem / OW, xx = rem % OW;
    const int taps = clamp_i(a.by[2 * y + 1], 0, a.ksy);
    const int top = clamp_i(a.by[2 * y] - r0, 0, rows - min(taps, rows));
    const int n_taps = min(taps, rows);
    const int32_t* k = a.ky + (size_t)y * a.ksy;
    const uint8_t* col = stage + ((size_t)top * 3 + c) * OW + xx;
    int s = 1 << (kPrecisionBits - 1);
    for (int x = 0; x < n_taps; ++x) s += (int)col[(size_t)x * per_row] * k[x];
    const float v = ((float)clip8(s) / 255.0f - a.mean[c]) / a.stdv[c];
    a.out_img[(((size_t)b * 3 + c) * OH + y) * OW + xx] = v;
  }
}

__device__ void point_group(const PointArgs& a, long long g, int b, int grp, unsigned long long* pmask, int* ppre, int* wtot) {
  const int t = threadIdx.x, lane = t & (CT_WAVE - 1), wave = t / CT_WAVE;
  const int p_cap = a.p_cap, n = a.n;
  const long long off = a.offsets[g];
  long long len = a.offsets[g + 1] - off;
  const int P = (int)(len < 0 ? 0 : (len > p_cap ? p_cap : len));       // a guard: a stored cloud has 1 .. p_cap points
  const int m = min(n, P);
  const int NW = (p_cap + CT_WAVE - 1) / CT_WAVE;
  const int64_t* PM = a.perm + (size_t)b * p_cap;
  const float* S = a.points + (size_t)off * 3;
  float* O = a.out_pcd + (size_t)b * 3 * n;

  // flags in perm order: the entry names a point of this cloud
  // (kFlagWords words per wave and step, their loads issued together)
  for (int w0 = wave * kFlagWords; w0 < NW; w0 += kWaves * kFlagWords) {
    long long s[kFlagWords];
#pragma unroll
    for (int e = 0; e < kFlagWords; ++e) {
      const int j = (w0 + e) * CT_WAVE + lane;
      s[e] = j < p_cap ? PM[j] : -1;
    }
#pragma unroll
    for (int e = 0; e < kFlagWords; ++e) {
      const unsigned long long mk = __ballot(s[e] >= 0 && s[e] < P);
      if (lane == 0 && w0 + e < NW) pmask[w0 + e] = mk;
    }
  }
  __syncthreads();
  // exclusive scan of the words' popcounts, kWordsPerThread consecutive words per thread
  int cnt[kWordsPerThread], c = 0;
#pragma unroll
  for (int e = 0; e < kWordsPerThread; ++e) {
    const int w = t * kWordsPerThread + e;
    cnt[e] = w < NW ? __popcll(pmask[w]) : 0;
    c += cnt[e];
  }
  int sc = c;
  for (int d = 1; d < CT_WAVE; d <<= 1) {
    const int up = __shfl_up(sc, d);
    if (lane >= d) sc += up;
  }
  if (lane == CT_WAVE - 1) wtot[wave] = sc;
  __syncthreads();
  int before = sc - c;
  for (int k = 0; k < wave; ++k) before += wtot[k];
#pragma unroll
  for (int e = 0; e < kWordsPerThread; ++e) {
    const int w = t * kWordsPerThread + e;
    if (w < NW) ppre[w] = before;
    before += cnt[e];
  }
  __syncthreads();

  // this group's slice of the perm positions: a flagged position of rank r < m fills slot r
  {
    const int chunk = (p_cap + a.G - 1) / a.G;
    const int j0 = grp * chunk, j1 = min(p_cap, j0 + chunk);
    for (int j = j0 + t; j < j1; j += kThreads) {
      const int w = j >> 6, bit = j & 63;
      const unsigned long long mk = pmask[w];
      if ((mk >> bit) & 1ull) {
        const int r = ppre[w] + rank_below(mk, bit);
        if (r < m) {
          const long long s = PM[j];
          O[r] = S[3 * s + 0], O[(size_t)n + r] = S[3 * s + 1], O[(size_t)2 * n + r] = S[3 * s + 2];
        }
      }
    }
  }
  // ... and of the top-up slots P .. n - 1: min((int)(u * P), P - 1), a NaN draw gives 0
  if (n > P) {
    const int extra = n - P;
    const int chunk = (extra + a.G - 1) / a.G;
    const int j0 = P + grp * chunk, j1 = min(n, j0 + chunk);
    const float* U = a.u_dup + (size_t)b * n;
    for (int j = j0 + t; j < j1; j += kThreads) {
      float x = 0.0f, y = 0.0f, z = 0.0f;
      if (P > 0) {
        const float f = U[j] * (float)P;
        const int k = f >= (float)(P - 1) ? P - 1 : (f > 0.0f ? (int)f : 0);
        x = S[3 * k + 0], y = S[3 * k + 1], z = S[3 * k + 2];
      }
      O[j] = x, O[(size_t)n + j] = y, O[(size_t)2 * n + j] = z;
    }
  }
}

__global__ void __launch_bounds__(kThreads)
image_items_kernel(ImageArgs ia, PointArgs pa, const int64_t* __restrict__ class_id, const int64_t* __restrict__ item,
                   int64_t* __restrict__ out_class) {
  // one block of LDS, laid out per role: the image workgroup's row buffers and staged plane; the point workgroup's scan
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWaves * kRowDwords * 4 + kStageBytes];
  static_assert(kWords * (8 + 4) + kWaves * 4 <= kWaves * kRowDwords * 4 + kStageBytes, "the scan fits the same block");
  const int b = blockIdx.y;
  long long g = item[b];
  g = g < 0 ? 0 : (g > ia.M - 1 ? ia.M - 1 : g);                        // a guard: the sampler's indices are in range
  if ((int)blockIdx.x < ia.bands) {
    if (blockIdx.x == 0 && threadIdx.x == 0) out_class[b] = class_id[g];
    image_group(ia, g, b, blockIdx.x, (uint32_t(*)[kRowDwords])lds, lds + kWaves * kRowDwords * 4);
  } else {
    unsigned long long* pmask = (unsigned long long*)lds;
    int* ppre = (int*)(lds + kWords * 8);
    point_group(pa, g, b, blockIdx.x - ia.bands, pmask, ppre, ppre + kWords);
  }
}

// The source rows a band of R output rows can reach: with s = in / out the first row is int((y0 + 0.5) s - support + 0.5) and
// the end int((y0 + R - 0.5) s + support + 0.5), so the span is below (R - 1) s + 2 support + 1 <= (R - 1) s + ksy.
inline int rows_cap(int R, int H, int OH, int ksy) {
  const double span = (double)(R - 1) * ((double)H / (double)OH);
  const long long cap = (long long)span + ksy;
  return cap > H ? H : (int)cap;
}

}  // namespace

extern "C" {

int ct_image_items(const uint8_t* images, int64_t M, int H, int W, int OH, int OW, const int32_t* kx, const int32_t* bx, int ksx,
                   const int32_t* ky, const int32_t* by, int ksy, const float* mean, const float* stdv, const float* points,
                   const int64_t* offsets, const int64_t* class_id, int p_cap, const int64_t* item, const int64_t* perm,
                   const float* u_dup, int B, int n, float* out_img, float* out_pcd, int64_t* out_class, ct_stream_t st) {
  if (!images || !kx || !bx || !ky || !by || !mean || !stdv || !points || !offsets || !class_id || !item || !perm || !u_dup ||
      !out_img || !out_pcd || !out_class)
    return CT_EINVAL;
  if (((uintptr_t)images % 4) != 0) return CT_EINVAL;
  if (B < 1 || B > 65535 || M < 1) return CT_EINVAL;
  if (H < 1 || H > kSizeMax || W < 1 || W > kWMax || OH < 1 || OH > kSizeMax || OW < 1 || OW > kSizeMax) return CT_EINVAL;
  if (ksx < 1 || ksx > kTapsMax || ksy < 1 || ksy > kTapsMax) return CT_EINVAL;
  if (p_cap < 1 || p_cap > kPMax || n < 1 || n > kNMax) return CT_EINVAL;
  for (int c = 0; c < 3; ++c)
    if (!(mean[c] - mean[c] == 0.0f) || !(stdv[c] - stdv[c] == 0.0f) || stdv[c] == 0.0f) return CT_EINVAL;   // NaN, +-inf, zero
  // the band: as many output rows as the staged plane holds, no more than keeps kGroupsTarget workgroups busy, kBandMin at least
  const long long stage_row = 3ll * OW;
  if (rows_cap(1, H, OH, ksy) * stage_row > kStageBytes) return CT_EINVAL;      // not even one output row fits
  const int per_image = (kGroupsTarget + B - 1) / B;
  int R = (OH + per_image - 1) / per_image;
  R = R < kBandMin ? kBandMin : R;
  R = R > OH ? OH : R;
  while (R > 1 && rows_cap(R, H, OH, ksy) * stage_row > kStageBytes) --R;

  ImageArgs ia;
  ia.images = images, ia.M = M, ia.total_bytes = (long long)M * H * W * 3;
  ia.H = H, ia.W = W, ia.OH = OH, ia.OW = OW, ia.ksx = ksx, ia.ksy = ksy, ia.R = R, ia.rows_cap = rows_cap(R, H, OH, ksy);
  ia.bands = (OH + R - 1) / R;
  ia.kx = kx, ia.bx = bx, ia.ky = ky, ia.by = by, ia.out_img = out_img;
  for (int c = 0; c < 3; ++c) ia.mean[c] = mean[c], ia.stdv[c] = stdv[c];
  PointArgs pa;
  pa.points = points, pa.offsets = offsets, pa.perm = perm, pa.u_dup = u_dup, pa.p_cap = p_cap, pa.n = n, pa.out_pcd = out_pcd;
  const int most = p_cap > n ? p_cap : n;
  int G = (most + kSlotsPerGroup - 1) / kSlotsPerGroup;
  pa.G = G > kPointGroupsMax ? kPointGroupsMax : G;

  CT_CLEAR_ERROR();
  hipLaunchKernelGGL(image_items_kernel, dim3(ia.bands + pa.G, B), dim3(kThreads), 0, (hipStream_t)st, ia, pa, class_id, item,
                     out_class);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

}  // extern "C"
