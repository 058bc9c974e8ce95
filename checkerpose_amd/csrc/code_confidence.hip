// Per-keypoint, per-axis pixel variance of the decoded code, from the code logits' confidences.  The post-forward
// path keeps only the logits' signs (cp_code_decode / cp_correspondences); this step keeps how sure each bit was, as the variance that
// cp_pnp_refine_wlm (csrc/pnp_refine_w.hip) whitens its residuals with.  The reference has no such step: opt-in, the rule is this
// project's own (tests/wlm_stages.py restates it in numpy).
//
// THE RULE.  bits (B, rows, N) fp32: row 0 the RoI bit, rows 1..r the x bits MSB first, rows 1+r..2r the y bits (1 <= r <= 30,
// rows >= 1 + 2r: the layout cp_code_decode reads); bbox (B, 4) int32 = the crops' final boxes (x, y, w, h), as cp_correspondences_bbox
// reads them; the code grid is (Hc, Wc); floor > 0, finite, in cells^2.  Everything in fp64, no contraction.
//   bit j (j = 0 the MSB) with logit z:  e = exp(-|z|), q_j = e / ((1 + e) (1 + e))      = p (1 - p) with p = sigmoid(z), in a form
//                                        that cannot overflow: z = +-inf gives 0, NaN stays NaN
//   per axis                             v = sum_j 4^(r-1-j) q_j, summed for j ascending from 0: the variance, in cells^2, of the
//                                        decoded integer under independent Bernoulli bits
//   sigma2[b,n,0] = (w / Wc)^2 (floor + v_x),  sigma2[b,n,1] = (h / Hc)^2 (floor + v_y)
//                                        (w / Wc) = (double)w / (double)Wc, the quotient correspondences_kernel forms; the square is
//                                        s * s, then one product with (floor + v).  An empty box (w = 0 or h = 0) gives 0 on its
//                                        axis (NaN where a logit of that axis is NaN).
// floor = 1 / 12 (the Python default) is the variance of a uniform quantisation to one cell: derived, not tuned.
// UNPINNED: whether a trained network's logits are calibrated enough for v to be a variance in fact -- no trained weights exist here;
// the rule is the textbook one for the inputs it is given.  The RoI bit's confidence plays no part.
//
// One lane per (crop, keypoint); no atomics, no LDS; 2r coalesced fp32 loads and 16 bytes stored per lane.
#include "pnp_core.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ double code_axis_variance(const float* __restrict__ z, int r, size_t N) {
  double v = 0.0;
  for (int j = 0; j < r; ++j) {
    const double e = exp(-fabs((double)z[(size_t)j * N]));
    const double q = e / ((1.0 + e) * (1.0 + e));
    v = v + (double)(1LL << (2 * (r - 1 - j))) * q;
  }
  return v;
}

__global__ __launch_bounds__(256) void code_confidence_kernel(const float* __restrict__ bits, int rows, int r, const int32_t* __restrict__ bbox,
                                                              int N, int Hc, int Wc, double floor_, double* __restrict__ sigma2, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // over B*N
  if (i >= total) return;
  const size_t b = i / (size_t)N;
  const size_t n = i - b * (size_t)N;
  const float* z = bits + b * (size_t)rows * (size_t)N + n;
  const double vx = code_axis_variance(z + (size_t)N, r, (size_t)N);
  const double vy = code_axis_variance(z + (size_t)(1 + r) * (size_t)N, r, (size_t)N);
  const int32_t* bb = bbox + 4 * b;
  const double sx = (double)bb[2] / (double)Wc, sy = (double)bb[3] / (double)Hc;
  sigma2[2 * i + 0] = sx * sx * (floor_ + vx);
  sigma2[2 * i + 1] = sy * sy * (floor_ + vy);
}

}  // namespace

extern "C" int cp_code_confidence(cp_stream_t stream, const float* bits, int rows, int r, const int32_t* final_bbox, int B, int N, int Hc,
                                  int Wc, double floor_cells2, double* sigma2) {
  if (!bits || !final_bbox || !sigma2) return CP_ERR_INVALID;
  if (B < 0 || N <= 0 || r < 1 || r > 30 || rows < 1 + 2 * r || Hc <= 0 || Wc <= 0 || !cp_finite_positive(floor_cells2)) return CP_ERR_INVALID;
  if (cp_misaligned(bits, 3) || cp_misaligned(final_bbox, 3) || cp_misaligned(sigma2, 7)) return CP_ERR_ALIGN;
  if (B == 0) return CP_OK;
  const size_t total = (size_t)B * (size_t)N;
  if ((total + 255) / 256 > 0x7FFFFFFFull) return CP_ERR_RANGE;
  CP_LAUNCH(code_confidence_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bits, rows, r, final_bbox, N, Hc,
            Wc, floor_cells2, sigma2, total);
  return cp_check_launch();
}
