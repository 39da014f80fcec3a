// Batch assembly of the S3DIS KPConv items for gfx950 (datasets/s3dis_closer.py:319-361, the item layout of S3DISSeg, and
// datasets/s3dis_closer_utils.py:38-93, the rotation and the scale / jitter of its training transforms) in one launch.
//
// One work-item per slot (b, n).  It picks the slot's source (a permuted valid slot, or for padding a valid slot drawn
// with replacement), gathers the point, its colour and label from the concatenated sub-clouds, centres it on the pick
// point, applies the optional augmentation, and writes the item's five outputs.  Feature rows are written along n, so the
// writes of a wave are contiguous.  Every float expression is the one the torch sequence it replaces evaluates, in the
// same order and built with -ffp-contract=off: results are equal bit for bit.
#include "ct_common.h"

namespace {

constexpr int kItemThreads = 256;
constexpr int kKMax = 16384;   // ct_nbr_radius's K bound: one item's slots

struct KpColour {
  float mean[3];
  float std[3];
};

__global__ void __launch_bounds__(kItemThreads)
kp_items_kernel(const int64_t* __restrict__ qidx, const int64_t* __restrict__ count, const int64_t* __restrict__ perm,
                const float* __restrict__ u_pad, const int64_t* __restrict__ offset, const float* __restrict__ pick,
                const float* __restrict__ drop, const float* __restrict__ P, const float* __restrict__ C,
                const int64_t* __restrict__ L, long long M, KpColour col, const float* __restrict__ R,
                const float* __restrict__ s, const float* __restrict__ j, int N, int F, float* __restrict__ out_points,
                int32_t* __restrict__ mask, float* __restrict__ features, int64_t* __restrict__ labels,
                int64_t* __restrict__ input_inds) {
  const int n = blockIdx.x * kItemThreads + threadIdx.x;
  const int b = blockIdx.y;
  if (n >= N) return;
  const size_t row = (size_t)b * N;
  const long long cnt = count[b];
  const long long nvalid = cnt < (long long)N ? cnt : (long long)N;
  const bool live = (long long)n < nvalid;
  // pad = floor(u * float(nvalid)).long().clamp(0, N - 1); src = live ? perm[n] : perm[pad]
  long long pad = (long long)floorf(u_pad[row + n] * (float)nvalid);
  pad = pad < 0 ? 0 : (pad > N - 1 ? N - 1 : pad);
  long long src = perm[row + (live ? n : (int)pad)];
  src = src < 0 ? 0 : (src > N - 1 ? N - 1 : src);               // a guard: an argsort's values are always in range
  long long ind = qidx[row + src];
  ind = ind < 0 ? 0 : ind;                                          // -1 (past the ball) -> 0, as clamp_(min=0)
  long long g = ind + offset[b];
  g = g < 0 ? 0 : (g > M - 1 ? M - 1 : g);                          // a guard: valid ball indices stay inside their cloud
  const float ox = P[3 * g + 0], oy = P[3 * g + 1], oz = P[3 * g + 2];
  float px = ox - pick[3 * b + 0], py = oy - pick[3 * b + 1], pz = oz - pick[3 * b + 2];
  if (R) {
    const float* r = R + 9 * (size_t)b;
    const float qx = (r[0] * px + r[1] * py) + r[2] * pz;
    const float qy = (r[3] * px + r[4] * py) + r[5] * pz;
    const float qz = (r[6] * px + r[7] * py) + r[8] * pz;
    const float* jj = j + 3 * (row + n);
    px = qx * s[3 * b + 0] + jj[0];
    py = qy * s[3 * b + 1] + jj[1];
    pz = qz * s[3 * b + 2] + jj[2];
  }
  const float d = drop[b];
  const float cr = ((C[3 * g + 0] - col.mean[0]) / col.std[0]) * d;
  const float cg = ((C[3 * g + 1] - col.mean[1]) / col.std[1]) * d;
  const float cb = ((C[3 * g + 2] - col.mean[2]) / col.std[2]) * d;

  float* op = out_points + 3 * (row + n);
  op[0] = px, op[1] = py, op[2] = pz;
  mask[row + n] = live ? 1 : 0;
  labels[row + n] = L[g];
  input_inds[row + n] = ind;
  // scene_seg_features: [B, F, N], feature f of slot n at f * N + n
  float* fb = features + (size_t)b * F * N + n;
  const size_t sN = (size_t)N;
  switch (F) {
    case 1: fb[0] = oz; break;
    case 3: fb[0] = cr, fb[sN] = cg, fb[2 * sN] = cb; break;
    case 4: fb[0] = cr, fb[sN] = cg, fb[2 * sN] = cb, fb[3 * sN] = oz; break;
    case 5: fb[0] = 1.0f, fb[sN] = cr, fb[2 * sN] = cg, fb[3 * sN] = cb, fb[4 * sN] = oz; break;
    case 6: fb[0] = cr, fb[sN] = cg, fb[2 * sN] = cb, fb[3 * sN] = px, fb[4 * sN] = py, fb[5 * sN] = pz; break;
    default:
      fb[0] = cr, fb[sN] = cg, fb[2 * sN] = cb, fb[3 * sN] = oz, fb[4 * sN] = px, fb[5 * sN] = py, fb[6 * sN] = pz;
      break;
  }
}

}  // namespace

extern "C" {

int ct_kp_items(const int64_t* qidx, const int64_t* count, const int64_t* perm, const float* u_pad, const int64_t* offset,
                const float* pick, const float* drop, const float* points, const float* colors, const int64_t* labels,
                int64_t M, const float* color_mean, const float* color_std, const float* R, const float* s, const float* j,
                int B, int N, int F, float* out_points, int32_t* mask, float* features, int64_t* out_labels,
                int64_t* input_inds, ct_stream_t st) {
  if (!qidx || !count || !perm || !u_pad || !offset || !pick || !drop || !points || !colors || !labels || !color_mean ||
      !color_std || !out_points || !mask || !features || !out_labels || !input_inds)
    return CT_EINVAL;
  if (B < 1 || B > 65535 || N < 1 || N > kKMax || M < 1) return CT_EINVAL;
  if (!(F == 1 || F == 3 || F == 4 || F == 5 || F == 6 || F == 7)) return CT_EINVAL;
  const int aug = (R != nullptr) + (s != nullptr) + (j != nullptr);
  if (aug != 0 && aug != 3) return CT_EINVAL;                       // the augmentation: all three or none
  KpColour col;
  for (int a = 0; a < 3; ++a) col.mean[a] = color_mean[a], col.std[a] = color_std[a];
  CT_CLEAR_ERROR();
  hipLaunchKernelGGL(kp_items_kernel, dim3((N + kItemThreads - 1) / kItemThreads, B), dim3(kItemThreads), 0, (hipStream_t)st,
                     qidx, count, perm, u_pad, offset, pick, drop, points, colors, labels, (long long)M, col, R, s, j, N, F,
                     out_points, mask, features, out_labels, input_inds);
  CT_CHECK_LAUNCH();
  return CT_OK;
}

}  // extern "C"
