// Ground-truth side on the device: the labels the reference's data loader makes one sample at a time on the host
// (bop_dataset_pytorch.py:293,356-380; lm_dataset_pytorch.py:393,438-462) and the code / mask figures its test loop prints beside ADD
// (test.py:432-457).
//
// cp_encode_targets.  One lane per (crop, keypoint), the keypoint index fastest: every output row is a coalesced store.  Arithmetic is
// the reference's, in fp64 and in its order -- P = K [R|t], P [p;1], the division by the third row, (u - bx) / (bw / S), truncation
// toward zero, out of the RoI = u < bx or v < by or id >= S, then the clip to [0, S-1].  This whole file is compiled with
// `#pragma clang fp contract(off)`: no product is fused into a following sum, so the bits do not depend on what the optimiser
// pairs up (hipcc's default is -ffp-contract=fast).  The float -> int conversion SATURATES: the quotient is clamped to the int32 range
// before the cast (numpy's astype(int) is undefined for such values); a NaN quotient (depth 0 with a zero numerator, non-finite pose)
// is out of the RoI with id 0.  A box with w <= 0 or h <= 0 is the loader's "no detection" dummy (:328-338): all-zero labels, nothing
// is divided by its size (the entry point lets only flagged boxes through in that state).
//
// cp_code_report.  One workgroup per crop; every figure of test.py:432-457 is a quotient of INTEGER counts, so the counts are what is
// reduced: per-lane int32 partial sums, a wave-64 butterfly (__shfl_xor), then one LDS row per wave summed by the first lanes.  No
// atomics and no floating-point sums: bit-identical between calls and independent of B.  Decisions are logit > 0 (sigmoid(z) > 0.5 <=>
// z > 0 in fp32, tests/golden/sigmoid_threshold.npz).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TG_THREADS = 256;
constexpr int TG_MAX_BITS = 8;                       // S <= 256
constexpr int TG_COUNTS_FIXED = 10;                  // counts row: 10 + 2 nb entries (include/checkerpose_hip.h)
constexpr int TG_MAX_COUNTS = TG_COUNTS_FIXED + 2 * TG_MAX_BITS;

struct EncParams {
  const double* p3d;          // (N,3) | (B,N,3) | (n_obj,N,3)
  long long p3d_bstride;      // elements between crops (0: shared); ignored with obj_ids
  const int32_t* obj_ids;     // 1-based, or nullptr
  const double* K;
  long long K_bstride;
  const double* R;
  const double* t;
  const int32_t* boxes;
  float* roi;
  float* xcode;
  float* ycode;
  int32_t* xid;
  int32_t* yid;
  double* proj;
  double* depth;
  int n_obj, B, N, S, bits;
};

// trunc toward zero with saturation; `nan` reports a NaN operand (the id is 0 then)
__device__ inline int sat_trunc(double q, bool& nan) {
  nan = q != q;
  if (nan) return 0;
  q = fmin(fmax(q, -2147483648.0), 2147483647.0);
  return (int)q;
}

__global__ __launch_bounds__(TG_THREADS) void encode_targets_kernel(EncParams p) {
  const int n = blockIdx.x * TG_THREADS + threadIdx.x, b = blockIdx.y;
  if (n >= p.N) return;
  const int S = p.S, bits = p.bits, N = p.N;
  const int32_t* bx = p.boxes + 4 * (size_t)b;
  const int x0 = bx[0], y0 = bx[1], bw = bx[2], bh = bx[3];
  const double* pts = p.p3d;
  bool ok = bw > 0 && bh > 0;
  if (p.obj_ids) {
    const int o = p.obj_ids[b];
    if (o < 1 || o > p.n_obj) ok = false;             // (the host wrapper refuses such ids; never read outside the table)
    else pts += (size_t)(o - 1) * N * 3;
  } else {
    pts += (size_t)b * p.p3d_bstride;
  }
  int xi = 0, yi = 0;
  float in_roi = 0.f;
  double u = 0.0, v = 0.0, z = 0.0;
  if (ok) {
    const double* K = p.K + (size_t)b * p.K_bstride;
    const double* R = p.R + 9 * (size_t)b;
    const double* t = p.t + 3 * (size_t)b;
    const double px = pts[3 * (size_t)n], py = pts[3 * (size_t)n + 1], pz = pts[3 * (size_t)n + 2];
    double h[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double k0 = K[3 * i], k1 = K[3 * i + 1], k2 = K[3 * i + 2];
      // row i of P = K [R|t], each entry summed over k = 0, 1, 2; then P [p;1] summed over the four columns
      const double P0 = k0 * R[0] + k1 * R[3] + k2 * R[6];
      const double P1 = k0 * R[1] + k1 * R[4] + k2 * R[7];
      const double P2 = k0 * R[2] + k1 * R[5] + k2 * R[8];
      const double P3 = k0 * t[0] + k1 * t[1] + k2 * t[2];
      h[i] = P0 * px + P1 * py + P2 * pz + P3;
    }
    z = h[2];
    u = h[0] / z;
    v = h[1] / z;
    const double sx = (double)bw / (double)S, sy = (double)bh / (double)S;      // exact: S is a power of two
    bool nx, ny;
    const int qx = sat_trunc((u - (double)x0) / sx, nx);
    const int qy = sat_trunc((v - (double)y0) / sy, ny);
    const bool out = nx || ny || u < (double)x0 || v < (double)y0 || qx >= S || qy >= S;
    in_roi = out ? 0.f : 1.f;
    xi = min(max(qx, 0), S - 1);
    yi = min(max(qy, 0), S - 1);
  }
  p.roi[(size_t)b * N + n] = in_roi;
  p.xid[(size_t)b * N + n] = xi;
  p.yid[(size_t)b * N + n] = yi;
  for (int i = 0; i < bits; ++i) {                     // MSB first
    const int sh = bits - 1 - i;
    p.xcode[((size_t)b * bits + i) * N + n] = (float)((xi >> sh) & 1);
    p.ycode[((size_t)b * bits + i) * N + n] = (float)((yi >> sh) & 1);
  }
  if (p.proj) {
    p.proj[2 * ((size_t)b * N + n)] = u;
    p.proj[2 * ((size_t)b * N + n) + 1] = v;
  }
  if (p.depth) p.depth[(size_t)b * N + n] = z;
}

struct RepParams {
  const float* pred_roi;      // (B,1,N)
  const float* pred_x;        // (B,nb,N) rows N apart
  const float* pred_y;
  long long roi_bstride, x_bstride, y_bstride;
  const float* seg;           // (B,2,H,W)
  const float* gt_roi;        // (B,1,N)
  const float* gt_x;          // (B,bits,N): the first nb rows are read
  const float* gt_y;
  const void* m_vis;          // (B,S,S) uint8 (non-zero = set) or f32 (> 0.5 = set)
  const void* m_full;
  int32_t* counts;            // (B, 10 + 2 nb)
  double* figures;            // (B, 8 + 2 nb)
  int B, N, nb, bits, H, W, S, mask_f32;
};

__device__ inline int wave_sum(int v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ inline bool mask_on(const void* m, size_t i, int f32) { return f32 ? ((const float*)m)[i] > 0.5f : ((const uint8_t*)m)[i] != 0; }

__global__ __launch_bounds__(TG_THREADS) void code_report_kernel(RepParams p) {
  __shared__ int s_part[TG_THREADS / 64][TG_MAX_COUNTS];
  __shared__ int s_tot[TG_MAX_COUNTS];
  const int tid = threadIdx.x, b = blockIdx.x, N = p.N, nb = p.nb;
  int c[TG_MAX_COUNTS];
#pragma unroll
  for (int k = 0; k < TG_MAX_COUNTS; ++k) c[k] = 0;
  const float* pr = p.pred_roi + (size_t)b * p.roi_bstride;
  const float* px = p.pred_x + (size_t)b * p.x_bstride;
  const float* py = p.pred_y + (size_t)b * p.y_bstride;
  const float* gr = p.gt_roi + (size_t)b * N;
  const float* gx = p.gt_x + (size_t)b * p.bits * N;
  const float* gy = p.gt_y + (size_t)b * p.bits * N;
  for (int n = tid; n < N; n += TG_THREADS) {
    const int g = gr[n] > 0.5f, q = pr[n] > 0.f;
    c[0] += g;
    c[1] += g != q;
    int dx = 0, dy = 0;
#pragma unroll
    for (int i = 0; i < TG_MAX_BITS; ++i) {
      if (i < nb) {
        const int ex = (int)(gx[(size_t)i * N + n] > 0.5f) - (int)(px[(size_t)i * N + n] > 0.f);
        const int ey = (int)(gy[(size_t)i * N + n] > 0.5f) - (int)(py[(size_t)i * N + n] > 0.f);
        dx = 2 * dx + ex;                               // = sum_i e_i 2^(nb-1-i): the signed id difference over the nb leading bits
        dy = 2 * dy + ey;
        c[TG_COUNTS_FIXED + i] += g & (ex != 0);
        c[TG_COUNTS_FIXED + TG_MAX_BITS + i] += g & (ey != 0);
      }
    }
    c[2] += g ? abs(dx) : 0;
    c[3] += g ? abs(dy) : 0;
  }
  // GT masks at F.interpolate(mode="nearest") positions for the seg size: src = min(floor(dst * (float)S / dst_size), S - 1)
  const int HW = p.H * p.W, S = p.S;
  const float sy = (float)S / (float)p.H, sx = (float)S / (float)p.W;
  const float* sv = p.seg + (size_t)b * 2 * HW;
  const float* sf = sv + HW;
  for (int i = tid; i < HW; i += TG_THREADS) {
    const int y = i / p.W, x = i - y * p.W;
    const int my = min((int)floorf((float)y * sy), S - 1), mx = min((int)floorf((float)x * sx), S - 1);
    const size_t mi = ((size_t)b * S + my) * S + mx;
    const int gv = mask_on(p.m_vis, mi, p.mask_f32), gf = mask_on(p.m_full, mi, p.mask_f32);
    const int qv = sv[i] > 0.f, qf = sf[i] > 0.f;
    c[4] += gv != qv; c[5] += gv & qv; c[6] += gv | qv;
    c[7] += gf != qf; c[8] += gf & qf; c[9] += gf | qf;
  }
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int k = 0; k < TG_MAX_COUNTS; ++k) {
    const int s = wave_sum(c[k]);
    if (lane == 0) s_part[wave][k] = s;
  }
  __syncthreads();
  if (tid < TG_MAX_COUNTS) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < TG_THREADS / 64; ++w) s += s_part[w][tid];
    s_tot[tid] = s;
  }
  __syncthreads();
  const int ncnt = TG_COUNTS_FIXED + 2 * nb;
  int32_t* co = p.counts + (size_t)b * ncnt;
  if (tid < TG_COUNTS_FIXED) co[tid] = s_tot[tid];
  else if (tid < TG_COUNTS_FIXED + nb) co[tid] = s_tot[tid];
  else if (tid < ncnt) co[tid] = s_tot[TG_COUNTS_FIXED + TG_MAX_BITS + (tid - TG_COUNTS_FIXED - nb)];
  // the figures as test.py:433-457 forms them, in fp64 from the counts
  double* f = p.figures + (size_t)b * (8 + 2 * nb);
  const double npoint = (double)max(s_tot[0], 1), full = (double)(1 << nb);
  if (tid == 0) {
    const double err_roi = (double)s_tot[1] / (double)N;
    f[0] = 1.0 - err_roi;
    f[1] = 1.0 - ((double)s_tot[2] / npoint) / full;
    f[2] = 1.0 - ((double)s_tot[3] / npoint) / full;
    f[3] = 1.0 - (double)s_tot[4] / (double)HW;
    f[4] = s_tot[6] < 1 ? 1.0 : (double)s_tot[5] / (double)s_tot[6];
    f[5] = 1.0 - (double)s_tot[7] / (double)HW;
    f[6] = s_tot[9] < 1 ? 1.0 : (double)s_tot[8] / (double)s_tot[9];
    f[7] = err_roi;
  }
  if (tid >= 1 && tid <= nb) f[7 + tid] = (double)s_tot[TG_COUNTS_FIXED + tid - 1] / npoint;
  else if (tid > nb && tid <= 2 * nb) f[7 + tid] = (double)s_tot[TG_COUNTS_FIXED + TG_MAX_BITS + tid - nb - 1] / npoint;
}

bool pow2_in(int S, int lo, int hi, int& bits) {
  if (S < lo || S > hi || (S & (S - 1))) return false;
  bits = 0;
  while ((1 << bits) < S) ++bits;
  return true;
}

}  // namespace

extern "C" int cp_encode_targets(cp_stream_t stream, const double* p3d, long long p3d_bstride, const int32_t* obj_ids, int n_obj,
                                 const double* cam_K, long long K_bstride, const double* R, const double* t, const int32_t* boxes,
                                 const int32_t* boxes_host, const uint8_t* no_detection_host, int B, int N, int S, float* roi_mask_bit,
                                 float* pixel_x_code, float* pixel_y_code, int32_t* x_id, int32_t* y_id, double* proj_xy, double* depth) {
  if (!p3d || !cam_K || !R || !t || !boxes || !boxes_host) return CP_ERR_INVALID;
  if (!roi_mask_bit || !pixel_x_code || !pixel_y_code || !x_id || !y_id) return CP_ERR_INVALID;
  int bits = 0;
  if (B <= 0 || N <= 0 || !pow2_in(S, 8, 256, bits)) return CP_ERR_INVALID;
  if (obj_ids ? n_obj <= 0 : (p3d_bstride != 0 && p3d_bstride != 3LL * N)) return CP_ERR_INVALID;
  if (K_bstride != 0 && K_bstride != 9) return CP_ERR_INVALID;
  for (int b = 0; b < B; ++b) {                                   // a flagged box is the dummy (0, 0, 0, 0); any other box has an area
    const int32_t* bx = boxes_host + 4 * (size_t)b;
    const bool flagged = no_detection_host && no_detection_host[b];
    if (flagged ? (bx[2] != 0 || bx[3] != 0) : (bx[2] <= 0 || bx[3] <= 0)) return CP_ERR_INVALID;
  }
  if (((uintptr_t)p3d & 7) || ((uintptr_t)cam_K & 7) || ((uintptr_t)R & 7) || ((uintptr_t)t & 7) || ((uintptr_t)proj_xy & 7) ||
      ((uintptr_t)depth & 7) || ((uintptr_t)boxes & 3) || ((uintptr_t)obj_ids & 3) || ((uintptr_t)roi_mask_bit & 3) ||
      ((uintptr_t)pixel_x_code & 3) || ((uintptr_t)pixel_y_code & 3) || ((uintptr_t)x_id & 3) || ((uintptr_t)y_id & 3))
    return CP_ERR_ALIGN;
  if (B > 65535 || (long long)B * N * bits >= (1LL << 31)) return CP_ERR_RANGE;
  EncParams p;
  p.p3d = p3d; p.p3d_bstride = p3d_bstride; p.obj_ids = obj_ids; p.K = cam_K; p.K_bstride = K_bstride; p.R = R; p.t = t; p.boxes = boxes;
  p.roi = roi_mask_bit; p.xcode = pixel_x_code; p.ycode = pixel_y_code; p.xid = x_id; p.yid = y_id; p.proj = proj_xy; p.depth = depth;
  p.n_obj = n_obj; p.B = B; p.N = N; p.S = S; p.bits = bits;
  CP_LAUNCH(encode_targets_kernel, dim3((unsigned)((N + TG_THREADS - 1) / TG_THREADS), (unsigned)B), dim3(TG_THREADS), 0,
            (hipStream_t)stream, p);
  return cp_check_launch();
}

extern "C" int cp_code_report(cp_stream_t stream, const float* pred_roi, long long roi_bstride, const float* pred_x, long long x_bstride,
                              const float* pred_y, long long y_bstride, int nb, const float* seg, int H, int W, const float* gt_roi,
                              const float* gt_x, const float* gt_y, int bits, const void* mask_visib, const void* mask_full, int mask_f32,
                              int S, int B, int N, int32_t* counts, double* figures) {
  if (!pred_roi || !pred_x || !pred_y || !seg || !gt_roi || !gt_x || !gt_y || !mask_visib || !mask_full || !counts || !figures)
    return CP_ERR_INVALID;
  int sbits = 0;
  if (B <= 0 || N <= 0 || H <= 0 || W <= 0 || !pow2_in(S, 8, 256, sbits)) return CP_ERR_INVALID;
  if (bits < 1 || bits > TG_MAX_BITS || nb < 1 || nb > bits) return CP_ERR_INVALID;
  if (roi_bstride < N || x_bstride < (long long)nb * N || y_bstride < (long long)nb * N) return CP_ERR_INVALID;
  if (mask_f32 != 0 && mask_f32 != 1) return CP_ERR_INVALID;
  if (((uintptr_t)pred_roi & 3) || ((uintptr_t)pred_x & 3) || ((uintptr_t)pred_y & 3) || ((uintptr_t)seg & 3) || ((uintptr_t)gt_roi & 3) ||
      ((uintptr_t)gt_x & 3) || ((uintptr_t)gt_y & 3) || ((uintptr_t)counts & 3) || ((uintptr_t)figures & 7) ||
      (mask_f32 && (((uintptr_t)mask_visib & 3) || ((uintptr_t)mask_full & 3))))
    return CP_ERR_ALIGN;
  // int32 sums: the largest is sum |id difference| < N * 2^nb; pixel counts <= H * W
  if ((long long)N << nb >= (1LL << 31) || (long long)H * W >= (1LL << 31)) return CP_ERR_RANGE;
  RepParams p;
  p.pred_roi = pred_roi; p.pred_x = pred_x; p.pred_y = pred_y; p.roi_bstride = roi_bstride; p.x_bstride = x_bstride; p.y_bstride = y_bstride;
  p.seg = seg; p.gt_roi = gt_roi; p.gt_x = gt_x; p.gt_y = gt_y; p.m_vis = mask_visib; p.m_full = mask_full; p.counts = counts;
  p.figures = figures; p.B = B; p.N = N; p.nb = nb; p.bits = bits; p.H = H; p.W = W; p.S = S; p.mask_f32 = mask_f32;
  CP_LAUNCH(code_report_kernel, dim3((unsigned)B), dim3(TG_THREADS), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}
