// cp_coco_* (SURVEY.md 8f row N15): the BOP'22 COCO detection / segmentation task of bop_toolkit -- scripts/calc_gt_coco.py,
// scripts/eval_bop22_coco.py, bop_toolkit_lib/pycoco_utils.py, and pycocotools' COCOeval.evaluate / accumulate as the script drives
// them -- for masks and boxes resident on the device.  Five stages, each an entry point of its own:
//
//   cp_coco_pack        a workgroup per mask: uint8 (N,H,W), nonzero = set -> bit rows of WW = ceil(W / 32) 32-bit words (bit x & 31 of
//                       word x >> 5; a wave ballot over 64 pixels of a row yields two words; bits past W are zero), the pixel count and
//                       [xmin ymin xmax ymax] (-1s for an empty mask).  The ballot is wave-uniform: no shuffle is needed within a
//                       wave, the waves meet in LDS.
//   cp_coco_unpack      the inverse for callers who want a picture: bit rows -> uint8 0 / 1 (N,H,W), a thread per pixel (row N27).
//   cp_coco_rle_count / cp_coco_rle_write
//                       pycoco_utils.binary_mask_to_rle: run lengths of the mask ravelled column-major (i = x H + y; runs go on across
//                       the column boundary; a leading 0 when pixel 0 is set).  A workgroup per mask; every thread owns a contiguous
//                       stretch of i, counts the run STARTS in it (i == 0, or a value unlike its predecessor's) and remembers the last
//                       one; a block scan (sum of the counts, max of the last starts) gives each thread the index of its first run and
//                       the start before its stretch, so that it writes length = start - previous start for every start it meets.  The
//                       count launch gives runs per mask; the caller makes the offsets (a cumulative sum) and the write launch fills
//                       the concatenated int32 counts.  A mask whose offsets do not fit the buffer is not written.
//   cp_coco_mask_iou    a one-wave workgroup per listed (detection, ground truth) pair: popcount of a & b over the word window where the
//                       two boxes overlap (no read when they miss), union from the packed areas; 0.0 when the intersection is empty,
//                       else ONE float64 quotient of two integers.
//   cp_coco_box_iou     a thread per pair: maskApi's bbIou on x y w h in float64, contraction off.
//   cp_coco_match       COCOeval.evaluateImg: a wave per (image, category) group, a lane per (area range, threshold) = 40 lanes.  The
//                       reference's stable "unignored first" reorder of the ground truth is two passes over the input order (the
//                       unignored ones, then -- only while nothing is matched, which is its `break` -- the ignored ones); `iou < best`
//                       skips, so an equal IoU moves the match to the LATER ground truth.  One scratch byte per (ground truth, lane):
//                       bit 0 taken, bit 1 ignored; the kernel initialises it.
//   cp_coco_accumulate  COCOeval.accumulate: a workgroup per (category, area range, maxDet), the ten thresholds one after the other.  It
//                       walks the category's detections in the caller's globally sorted order (stable, descending score) in chunks of
//                       256 with a block scan of (tp, fp) packed in one 64-bit integer.  A detection past maxDet in its image is
//                       treated as an ignored one: it adds nothing to either sum, so it repeats its predecessor's (recall, precision)
//                       and can never be the first element that reaches a recall threshold with a larger precision -- the tables are
//                       those of the shortened list.  precision[r] = max of tp / (fp + tp + 2^-52) over the elements whose recall
//                       tp / npig is >= recThrs[r] (the reference's running maximum from the right read at searchsorted(rc, thr,
//                       'left')): each element finds j = #{r: recThrs[r] <= rc} and raises bucket j with an INTEGER atomic maximum on the
//                       float64's bit pattern (non-negative doubles order as their bits), then precision[r] = max of buckets j > r.
//
// No floating-point atomics; every output is a function of integer counts and IEEE float64 quotients: bit-identical from call to
// call, for an item alone or in its batch.
#include <limits.h>

#include "common.h"

namespace {

constexpr int CE_T = CP_COCO_THRS, CE_R = CP_COCO_RECS, CE_A = CP_COCO_AREAS, CE_M = CP_COCO_MAXDETS, CE_LANES = CE_A * CE_T;
constexpr int CE_PACK_THREADS = 512, CE_RLE_THREADS = 512, CE_ACC_THREADS = 256, CE_THREADS = 256;

// ---- pack
__global__ __launch_bounds__(CE_PACK_THREADS) void coco_pack_kernel(const uint8_t* __restrict__ masks, uint32_t* __restrict__ bits,
                                                                    int32_t* __restrict__ area, int32_t* __restrict__ box, int H, int W,
                                                                    int WW) {
  __shared__ int s_red[CE_PACK_THREADS / 64][5];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.x;
  const uint8_t* __restrict__ m = masks + (size_t)n * H * W;
  uint32_t* __restrict__ b = bits + (size_t)n * H * WW;
  const int chunks = (W + 63) >> 6;
  int cnt = 0, x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
  for (int it = wave; it < H * chunks; it += CE_PACK_THREADS / 64) {      // (uniform per wave)
    const int y = it / chunks, c = it - y * chunks, x = c * 64 + lane;
    const bool set = x < W && m[(size_t)y * W + x] != 0;
    const unsigned long long bal = __ballot(set);
    if (lane == 0) {
      b[(size_t)y * WW + 2 * c] = (uint32_t)bal;
      if (2 * c + 1 < WW) b[(size_t)y * WW + 2 * c + 1] = (uint32_t)(bal >> 32);
    }
    if (bal) {
      cnt += __popcll(bal);
      x0 = min(x0, c * 64 + __ffsll((long long)bal) - 1);
      x1 = max(x1, c * 64 + 63 - __clzll((long long)bal));
      y0 = min(y0, y);
      y1 = max(y1, y);
    }
  }
  if (lane == 0) { s_red[wave][0] = cnt; s_red[wave][1] = x0; s_red[wave][2] = y0; s_red[wave][3] = x1; s_red[wave][4] = y1; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < CE_PACK_THREADS / 64; ++w) {
      cnt += s_red[w][0]; x0 = min(x0, s_red[w][1]); y0 = min(y0, s_red[w][2]); x1 = max(x1, s_red[w][3]); y1 = max(y1, s_red[w][4]);
    }
    area[n] = cnt;
    box[4 * n] = cnt ? x0 : -1; box[4 * n + 1] = cnt ? y0 : -1; box[4 * n + 2] = cnt ? x1 : -1; box[4 * n + 3] = cnt ? y1 : -1;
  }
}

// ---- unpack: cp_coco_pack's inverse for the bits, a thread per pixel
__global__ __launch_bounds__(CE_THREADS) void coco_unpack_kernel(const uint32_t* __restrict__ bits, uint8_t* __restrict__ masks, int H, int W,
                                                                 int WW, size_t total) {
  const size_t i = (size_t)blockIdx.x * CE_THREADS + threadIdx.x;     // over N * H * W
  if (i >= total) return;
  const size_t row = i / W;                                          // n * H + y
  const int x = (int)(i - row * W);
  masks[i] = (uint8_t)((bits[row * WW + (x >> 5)] >> (x & 31)) & 1u);
}

// ---- rle
template <bool WRITE>
__global__ __launch_bounds__(CE_RLE_THREADS) void coco_rle_kernel(const uint32_t* __restrict__ bits, int H, int W, int WW,
                                                                  const int64_t* __restrict__ off, int32_t* __restrict__ n_runs,
                                                                  int32_t* __restrict__ counts, long long total) {
  __shared__ int s_scan[CE_RLE_THREADS / 64][2];
  const int tid = threadIdx.x, mi = blockIdx.x;
  const uint32_t* __restrict__ b = bits + (size_t)mi * H * WW;
  const int n = H * W;                                               // (< 2^31 - 512: checked by the caller)
  const int L = (n + CE_RLE_THREADS - 1) / CE_RLE_THREADS;
  const int i0 = (int)min((long long)tid * L, (long long)n), i1 = min(i0 + L, n);
  auto bit = [&](int x, int y) -> int { return (int)((b[(size_t)y * WW + (x >> 5)] >> (x & 31)) & 1u); };
  int before = -1;                                                   // pixel i0 - 1; -1 makes pixel 0 a start
  if (i0 > 0 && i0 < n) { const int x = (i0 - 1) / H; before = bit(x, (i0 - 1) - x * H); }
  int cnt = 0, last = -1;
  {
    int x = i0 / H, y = i0 - x * H, prev = before;
    for (int i = i0; i < i1; ++i) {
      const int v = bit(x, y);
      if (v != prev) { ++cnt; last = i; }
      prev = v;
      if (++y == H) { y = 0; ++x; }
    }
  }
  int ec, el;
  cp_scan_sum_max(cnt, last, ec, el, s_scan);                                // cnt / last are inclusive now
  const int lead = bit(0, 0);
  if (!WRITE) {
    if (tid == CE_RLE_THREADS - 1) n_runs[mi] = cnt + lead;
    return;
  }
  const long long base = off[mi], cap = off[mi + 1] - base;
  if (base < 0 || cap < 0 || base + cap > total) return;             // (uniform) offsets that do not fit the buffer: nothing written
  int32_t* __restrict__ out = counts + base;
  {
    int x = i0 / H, y = i0 - x * H, prev = before, k = ec, prv = el;
    for (int i = i0; i < i1; ++i) {
      const int v = bit(x, y);
      if (v != prev) {
        if (i == 0) {
          if (lead && cap > 0) out[0] = 0;
        } else {
          const int at = k - 1 + lead;                               // the run that ends here
          if (at < cap) out[at] = i - prv;
        }
        prv = i;
        ++k;
      }
      prev = v;
      if (++y == H) { y = 0; ++x; }
    }
  }
  if (tid == CE_RLE_THREADS - 1) {
    const int at = cnt - 1 + lead;
    if (at < cap) out[at] = n - last;
  }
}

// ---- iou
struct IouParams {
  const uint32_t* dbits; const int32_t* darea; const int32_t* dbox; int ND;
  const uint32_t* gbits; const int32_t* garea; const int32_t* gbox; int NG;
  int H, W, WW;
  const int32_t* pairs; int P;
  double* out;
};

__global__ __launch_bounds__(64) void coco_mask_iou_kernel(IouParams p) {
  const int lane = threadIdx.x, pr = blockIdx.x;
  const int d = p.pairs[2 * (size_t)pr], g = p.pairs[2 * (size_t)pr + 1];
  if (d < 0 || d >= p.ND || g < 0 || g >= p.NG) {                    // (uniform)
    if (lane == 0) p.out[pr] = __builtin_nan("");
    return;
  }
  const int da = p.darea[d], ga = p.garea[g];
  int inter = 0;
  if (da > 0 && ga > 0) {
    const int32_t* __restrict__ db = p.dbox + 4 * (size_t)d;
    const int32_t* __restrict__ gb = p.gbox + 4 * (size_t)g;
    const int x0 = max(max(db[0], gb[0]), 0), y0 = max(max(db[1], gb[1]), 0);
    const int x1 = min(min(db[2], gb[2]), p.W - 1), y1 = min(min(db[3], gb[3]), p.H - 1);
    if (x0 <= x1 && y0 <= y1) {
      const uint32_t* __restrict__ a = p.dbits + (size_t)d * p.H * p.WW;
      const uint32_t* __restrict__ b = p.gbits + (size_t)g * p.H * p.WW;
      const int w0 = x0 >> 5, nw = (x1 >> 5) - w0 + 1, rows = y1 - y0 + 1;
      for (int it = lane; it < nw * rows; it += 64) {
        const int r = it / nw, w = it - r * nw;
        const size_t at = (size_t)(y0 + r) * p.WW + w0 + w;
        inter += __popc(a[at] & b[at]);
      }
    }
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) inter += __shfl_xor(inter, w, 64);
  if (lane == 0) p.out[pr] = inter == 0 ? 0.0 : (double)inter / (double)((long long)da + ga - inter);
}

__global__ __launch_bounds__(CE_THREADS) void coco_box_iou_kernel(const double* __restrict__ dbox, int ND, const double* __restrict__ gbox,
                                                                  int NG, const int32_t* __restrict__ pairs, int P,
                                                                  double* __restrict__ out) {
#pragma clang fp contract(off)
  const int pr = blockIdx.x * CE_THREADS + threadIdx.x;
  if (pr >= P) return;
  const int d = pairs[2 * (size_t)pr], g = pairs[2 * (size_t)pr + 1];
  if (d < 0 || d >= ND || g < 0 || g >= NG) { out[pr] = __builtin_nan(""); return; }
  const double* __restrict__ T = dbox + 4 * (size_t)d;
  const double* __restrict__ G = gbox + 4 * (size_t)g;
  const double da = T[2] * T[3], ga = G[2] * G[3];
  double w = fmin(T[2] + T[0], G[2] + G[0]) - fmax(T[0], G[0]);
  if (w <= 0) w = 0;
  double h = fmin(T[3] + T[1], G[3] + G[1]) - fmax(T[1], G[1]);
  if (h <= 0) h = 0;
  const double i = w * h;
  const double u = da + ga - i;
  out[pr] = i / u;
}

// ---- match
struct MatchParams {
  const double* iou;          // per group (D, G) row-major at iou_off
  const int32_t* offs;        // device: det_off, gt_off, iou_off, n_groups + 1 each
  int n_groups, ND, NGT, P;
  const double* det_area;
  const double* gt_area;
  const uint8_t* gt_ignore;
  const double* iou_thrs;     // (10)
  const double* area_rng;     // (4, 2)
  int32_t* dt_match;          // (ND, 4, 10): index of the matched ground truth in its group + 1, 0 = none
  uint8_t* dt_ignore;         // (ND, 4, 10)
  uint8_t* gt_ignore_out;     // (NGT, 4)
  uint8_t* scratch;           // (NGT, 40)
};

__global__ __launch_bounds__(64) void coco_match_kernel(MatchParams p) {
  const int lane = threadIdx.x, grp = blockIdx.x;
  const int32_t* __restrict__ doff = p.offs;
  const int32_t* __restrict__ goff = p.offs + (p.n_groups + 1);
  const int32_t* __restrict__ ioff = p.offs + 2 * (size_t)(p.n_groups + 1);
  const int d0 = doff[grp], D = doff[grp + 1] - d0, g0 = goff[grp], G = goff[grp + 1] - g0, i0 = ioff[grp];
  // the device copy of the offsets is checked like the host copy was: a group that does not fit is left alone
  if (d0 < 0 || D < 0 || D > CP_COCO_KEEP || (long long)d0 + D > p.ND || g0 < 0 || G < 0 || (long long)g0 + G > p.NGT || i0 < 0 ||
      (long long)i0 + (long long)D * G > p.P)
    return;
  if (lane >= CE_LANES) return;                                      // (no barrier or shuffle below)
  const int a = lane / CE_T, t = lane - a * CE_T;
  const double lo = p.area_rng[2 * a], hi = p.area_rng[2 * a + 1], thr = p.iou_thrs[t];
  uint8_t* __restrict__ flag = p.scratch + (size_t)g0 * CE_LANES + lane;          // this lane's byte of ground truth g: flag[g * 40]
  for (int g = 0; g < G; ++g) {
    const double ar = p.gt_area[g0 + g];
    const int ig = (p.gt_ignore[g0 + g] != 0 || ar < lo || ar > hi) ? 1 : 0;
    flag[(size_t)g * CE_LANES] = (uint8_t)(ig << 1);
    if (t == 0) p.gt_ignore_out[(size_t)(g0 + g) * CE_A + a] = (uint8_t)ig;
  }
  const double cap = 1.0 - 1e-10;
  for (int d = 0; d < D; ++d) {
    const double* __restrict__ row = p.iou + (size_t)i0 + (size_t)d * G;
    double best = thr < cap ? thr : cap;
    int m = -1;
    for (int g = 0; g < G; ++g) {                                    // the unignored ones, in input order
      if (flag[(size_t)g * CE_LANES] != 0) continue;
      const double v = row[g];
      if (v < best) continue;
      best = v; m = g;
    }
    if (m < 0)
      for (int g = 0; g < G; ++g) {                                  // then the ignored ones that are not taken
        if (flag[(size_t)g * CE_LANES] != 2) continue;
        const double v = row[g];
        if (v < best) continue;
        best = v; m = g;
      }
    int ig;
    if (m >= 0) {
      const uint8_t f = flag[(size_t)m * CE_LANES];
      ig = f >> 1;
      flag[(size_t)m * CE_LANES] = f | 1;
    } else {
      const double ar = p.det_area[d0 + d];
      ig = (ar < lo || ar > hi) ? 1 : 0;
    }
    p.dt_match[(size_t)(d0 + d) * CE_LANES + lane] = m + 1;
    p.dt_ignore[(size_t)(d0 + d) * CE_LANES + lane] = (uint8_t)ig;
  }
}

// ---- accumulate
struct AccParams {
  const int32_t* dt_match; const uint8_t* dt_ignore; const uint8_t* gt_ignore;   // cp_coco_match's tables
  const int32_t* det_rank;    // (ND) position of the detection in its image's score order
  const int32_t* order;       // (ND) detection indices, each category's stretch in stable descending score order
  const int32_t* offs;        // device: cat_det_off, cat_gt_off, K + 1 each
  int K, ND, NGT;
  int max_dets[CE_M];
  const double* rec_thrs;     // (101)
  double* precision;          // (10, 101, K, 4, 3)
  double* recall;             // (10, K, 4, 3)
};

__global__ __launch_bounds__(CE_ACC_THREADS) void coco_accumulate_kernel(AccParams p) {
  __shared__ unsigned long long s_bucket[CE_R + 1];
  __shared__ double s_thr[CE_R];
  __shared__ unsigned long long s_wave[CE_ACC_THREADS / 64];
  __shared__ unsigned long long s_carry;
  __shared__ int s_n[CE_ACC_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = blockIdx.x % CE_M, a = (blockIdx.x / CE_M) % CE_A, k = blockIdx.x / (CE_M * CE_A);
  const int c0 = p.offs[k], c1 = p.offs[k + 1], q0 = p.offs[p.K + 1 + k], q1 = p.offs[p.K + 1 + k + 1];
  if (c0 < 0 || c1 < c0 || c1 > p.ND || q0 < 0 || q1 < q0 || q1 > p.NGT) return;      // (uniform)
  const int maxdet = p.max_dets[m];
  int cnt = 0;
  for (int g = q0 + tid; g < q1; g += CE_ACC_THREADS) cnt += p.gt_ignore[(size_t)g * CE_A + a] ? 0 : 1;
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) cnt += __shfl_xor(cnt, w, 64);
  if (lane == 0) s_n[wave] = cnt;
  for (int r = tid; r < CE_R; r += CE_ACC_THREADS) s_thr[r] = p.rec_thrs[r];
  __syncthreads();
  int npig = 0;
  for (int w = 0; w < CE_ACC_THREADS / 64; ++w) npig += s_n[w];
  auto pat = [&](int t, int r) -> size_t { return ((((size_t)t * CE_R + r) * p.K + k) * CE_A + a) * CE_M + m; };
  auto rat = [&](int t) -> size_t { return (((size_t)t * p.K + k) * CE_A + a) * CE_M + m; };
  if (npig == 0) {                                                   // (uniform) the reference leaves its -1 here
    for (int i = tid; i < CE_T * CE_R; i += CE_ACC_THREADS) p.precision[pat(i / CE_R, i % CE_R)] = -1.0;
    if (tid < CE_T) p.recall[rat(tid)] = -1.0;
    return;
  }
  const double dn = (double)npig;
  for (int t = 0; t < CE_T; ++t) {
    for (int j = tid; j <= CE_R; j += CE_ACC_THREADS) s_bucket[j] = 0ull;
    if (tid == 0) s_carry = 0ull;
    __syncthreads();
    const int col = a * CE_T + t;
    for (int base = c0; base < c1; base += CE_ACC_THREADS) {         // (uniform)
      const int i = base + tid;
      unsigned long long inc = 0ull;                                 // tp in the low word, fp in the high one
      if (i < c1) {
        const int di = p.order[i];
        if (di >= c0 && di < c1 && p.det_rank[di] < maxdet && !p.dt_ignore[(size_t)di * CE_LANES + col])
          inc = p.dt_match[(size_t)di * CE_LANES + col] ? 1ull : (1ull << 32);
      }
      unsigned long long v = inc;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
      }
      if (lane == 63) s_wave[wave] = v;
      __syncthreads();
      v += s_carry;
      for (int w = 0; w < wave; ++w) v += s_wave[w];
      const unsigned long long tp = v & 0xffffffffull, fp = v >> 32;
      if (inc == 1ull) {                                             // precision can rise only where tp does
        const double rc = (double)tp / dn;
        const double pr = (double)tp / ((double)(fp + tp) + 2.220446049250313e-16);      // np.spacing(1)
        int lo = 0, hi = CE_R;                                       // j = #{r: recThrs[r] <= rc}
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (s_thr[mid] <= rc) lo = mid + 1; else hi = mid;
        }
        if (lo > 0) atomicMax(&s_bucket[lo], (unsigned long long)__double_as_longlong(pr));
      }
      __syncthreads();
      if (tid == CE_ACC_THREADS - 1) s_carry = v;
    }
    __syncthreads();
    for (int r = tid; r < CE_R; r += CE_ACC_THREADS) {
      unsigned long long best = 0ull;
      for (int j = r + 1; j <= CE_R; ++j) best = max(best, s_bucket[j]);
      p.precision[pat(t, r)] = __longlong_as_double((long long)best);
    }
    if (tid == 0) p.recall[rat(t)] = (double)(s_carry & 0xffffffffull) / dn;
    __syncthreads();
  }
}

// offsets (n + 1 values) start at 0, ascend and end at `end`
bool ce_ascending(const int32_t* off, int n, long long end) {
  if (off[0] != 0 || off[n] != end) return false;
  for (int i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return false;
  return true;
}

}  // namespace

extern "C" int cp_coco_pack(cp_stream_t stream, const uint8_t* masks, int N, int H, int W, uint32_t* bits, int32_t* area, int32_t* box) {
  if (!masks || !bits || !area || !box) return CP_ERR_INVALID;
  if (N < 1 || H < 1 || W < 1) return CP_ERR_INVALID;
  if (cp_misaligned(bits, 3) || cp_misaligned(area, 3) || cp_misaligned(box, 3)) return CP_ERR_ALIGN;
  if ((long long)H * W >= (1LL << 31) - 4096 || N >= (1 << 24)) return CP_ERR_RANGE;
  CP_LAUNCH(coco_pack_kernel, dim3((unsigned)N), dim3(CE_PACK_THREADS), 0, (hipStream_t)stream, masks, bits, area, box, H, W, (W + 31) / 32);
  return cp_check_launch();
}

extern "C" int cp_coco_unpack(cp_stream_t stream, const uint32_t* bits, int N, int H, int W, uint8_t* masks) {
  if (!bits || !masks) return CP_ERR_INVALID;
  if (N < 1 || H < 1 || W < 1) return CP_ERR_INVALID;
  if (cp_misaligned(bits, 3)) return CP_ERR_ALIGN;
  if ((long long)H * W >= (1LL << 31) - 4096 || N >= (1 << 24)) return CP_ERR_RANGE;
  const size_t total = (size_t)N * H * W, blocks = (total + CE_THREADS - 1) / CE_THREADS;
  if (blocks >= ((size_t)1 << 31)) return CP_ERR_RANGE;
  CP_LAUNCH(coco_unpack_kernel, dim3((unsigned)blocks), dim3(CE_THREADS), 0, (hipStream_t)stream, bits, masks, H, W, (W + 31) / 32, total);
  return cp_check_launch();
}

extern "C" int cp_coco_rle_count(cp_stream_t stream, const uint32_t* bits, int N, int H, int W, int32_t* n_runs) {
  if (!bits || !n_runs) return CP_ERR_INVALID;
  if (N < 1 || H < 1 || W < 1) return CP_ERR_INVALID;
  if (cp_misaligned(bits, 3) || cp_misaligned(n_runs, 3)) return CP_ERR_ALIGN;
  if ((long long)H * W >= (1LL << 31) - 4096 || N >= (1 << 24)) return CP_ERR_RANGE;
  CP_LAUNCH(coco_rle_kernel<false>, dim3((unsigned)N), dim3(CE_RLE_THREADS), 0, (hipStream_t)stream, bits, H, W, (W + 31) / 32,
            (const int64_t*)nullptr, n_runs, (int32_t*)nullptr, 0LL);
  return cp_check_launch();
}

extern "C" int cp_coco_rle_write(cp_stream_t stream, const uint32_t* bits, int N, int H, int W, const int64_t* offsets, int32_t* counts,
                                 long long total) {
  if (!bits || !offsets || !counts) return CP_ERR_INVALID;
  if (N < 1 || H < 1 || W < 1 || total < 1) return CP_ERR_INVALID;
  if (cp_misaligned(bits, 3) || cp_misaligned(offsets, 7) || cp_misaligned(counts, 3)) return CP_ERR_ALIGN;
  if ((long long)H * W >= (1LL << 31) - 4096 || N >= (1 << 24)) return CP_ERR_RANGE;
  CP_LAUNCH(coco_rle_kernel<true>, dim3((unsigned)N), dim3(CE_RLE_THREADS), 0, (hipStream_t)stream, bits, H, W, (W + 31) / 32, offsets,
            (int32_t*)nullptr, counts, total);
  return cp_check_launch();
}

extern "C" int cp_coco_mask_iou(cp_stream_t stream, const uint32_t* det_bits, const int32_t* det_area, const int32_t* det_box, int ND,
                                const uint32_t* gt_bits, const int32_t* gt_area, const int32_t* gt_box, int NG, int H, int W,
                                const int32_t* pairs, int P, double* out) {
  if (!det_bits || !det_area || !det_box || !gt_bits || !gt_area || !gt_box || !pairs || !out) return CP_ERR_INVALID;
  if (ND < 1 || NG < 1 || H < 1 || W < 1 || P < 1) return CP_ERR_INVALID;
  if (cp_misaligned(det_bits, 3) || cp_misaligned(det_area, 3) || cp_misaligned(det_box, 3) || cp_misaligned(gt_bits, 3) ||
      cp_misaligned(gt_area, 3) || cp_misaligned(gt_box, 3) || cp_misaligned(pairs, 3) || cp_misaligned(out, 7))
    return CP_ERR_ALIGN;
  if ((long long)H * W >= (1LL << 31) - 4096) return CP_ERR_RANGE;
  IouParams p = {};
  p.dbits = det_bits; p.darea = det_area; p.dbox = det_box; p.ND = ND; p.gbits = gt_bits; p.garea = gt_area; p.gbox = gt_box; p.NG = NG;
  p.H = H; p.W = W; p.WW = (W + 31) / 32; p.pairs = pairs; p.P = P; p.out = out;
  CP_LAUNCH(coco_mask_iou_kernel, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}

extern "C" int cp_coco_box_iou(cp_stream_t stream, const double* det_box, int ND, const double* gt_box, int NG, const int32_t* pairs,
                               int P, double* out) {
  if (!det_box || !gt_box || !pairs || !out) return CP_ERR_INVALID;
  if (ND < 1 || NG < 1 || P < 1) return CP_ERR_INVALID;
  if (cp_misaligned(det_box, 7) || cp_misaligned(gt_box, 7) || cp_misaligned(pairs, 3) || cp_misaligned(out, 7)) return CP_ERR_ALIGN;
  CP_LAUNCH(coco_box_iou_kernel, dim3((unsigned)((P + CE_THREADS - 1) / CE_THREADS)), dim3(CE_THREADS), 0, (hipStream_t)stream, det_box, ND,
            gt_box, NG, pairs, P, out);
  return cp_check_launch();
}

extern "C" size_t cp_coco_match_scratch_bytes(int NGT) { return NGT > 0 ? (size_t)NGT * CE_LANES : 0; }

extern "C" int cp_coco_match(cp_stream_t stream, const double* iou, const int32_t* offsets_host, const int32_t* offsets_dev, int n_groups,
                             int ND, int NGT, int P, const double* det_area, const double* gt_area, const uint8_t* gt_ignore,
                             const double* iou_thrs, const double* area_rng, int32_t* dt_match, uint8_t* dt_ignore,
                             uint8_t* gt_ignore_out, void* scratch) {
  if (!offsets_host || !offsets_dev || !iou_thrs || !area_rng) return CP_ERR_INVALID;
  if (n_groups < 1 || ND < 0 || NGT < 0 || P < 0) return CP_ERR_INVALID;
  if ((ND > 0 && (!det_area || !dt_match || !dt_ignore)) || (NGT > 0 && (!gt_area || !gt_ignore || !gt_ignore_out || !scratch)) ||
      (P > 0 && !iou))
    return CP_ERR_INVALID;
  const int32_t* doff = offsets_host;
  const int32_t* goff = offsets_host + (n_groups + 1);
  const int32_t* ioff = offsets_host + 2 * (size_t)(n_groups + 1);
  if (!ce_ascending(doff, n_groups, ND) || !ce_ascending(goff, n_groups, NGT) || !ce_ascending(ioff, n_groups, P)) return CP_ERR_INVALID;
  for (int g = 0; g < n_groups; ++g) {
    const long long D = (long long)doff[g + 1] - doff[g], G = (long long)goff[g + 1] - goff[g];
    if (D > CP_COCO_KEEP || (long long)ioff[g + 1] - ioff[g] != D * G) return CP_ERR_INVALID;
  }
  if (cp_misaligned(iou, 7) || cp_misaligned(offsets_dev, 3) || cp_misaligned(det_area, 7) || cp_misaligned(gt_area, 7) ||
      cp_misaligned(iou_thrs, 7) || cp_misaligned(area_rng, 7) || cp_misaligned(dt_match, 3))
    return CP_ERR_ALIGN;
  MatchParams p = {};
  p.iou = iou; p.offs = offsets_dev; p.n_groups = n_groups; p.ND = ND; p.NGT = NGT; p.P = P; p.det_area = det_area; p.gt_area = gt_area;
  p.gt_ignore = gt_ignore; p.iou_thrs = iou_thrs; p.area_rng = area_rng; p.dt_match = dt_match; p.dt_ignore = dt_ignore;
  p.gt_ignore_out = gt_ignore_out; p.scratch = (uint8_t*)scratch;
  CP_LAUNCH(coco_match_kernel, dim3((unsigned)n_groups), dim3(64), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}

extern "C" int cp_coco_accumulate(cp_stream_t stream, const int32_t* dt_match, const uint8_t* dt_ignore, const uint8_t* gt_ignore,
                                  const int32_t* det_rank, const int32_t* order, const int32_t* offsets_host, const int32_t* offsets_dev,
                                  int K, int ND, int NGT, const int32_t* max_dets, const double* rec_thrs, double* precision,
                                  double* recall) {
  if (!offsets_host || !offsets_dev || !max_dets || !rec_thrs || !precision || !recall) return CP_ERR_INVALID;
  if (K < 1 || ND < 0 || NGT < 0 || K >= (1 << 20)) return CP_ERR_INVALID;
  if ((ND > 0 && (!dt_match || !dt_ignore || !det_rank || !order)) || (NGT > 0 && !gt_ignore)) return CP_ERR_INVALID;
  if (!ce_ascending(offsets_host, K, ND) || !ce_ascending(offsets_host + (K + 1), K, NGT)) return CP_ERR_INVALID;
  for (int m = 0; m < CE_M; ++m)
    if (max_dets[m] < 1 || max_dets[m] > CP_COCO_KEEP) return CP_ERR_INVALID;
  if (cp_misaligned(dt_match, 3) || cp_misaligned(det_rank, 3) || cp_misaligned(order, 3) || cp_misaligned(offsets_dev, 3) ||
      cp_misaligned(rec_thrs, 7) || cp_misaligned(precision, 7) || cp_misaligned(recall, 7))
    return CP_ERR_ALIGN;
  AccParams p = {};
  p.dt_match = dt_match; p.dt_ignore = dt_ignore; p.gt_ignore = gt_ignore; p.det_rank = det_rank; p.order = order; p.offs = offsets_dev;
  p.K = K; p.ND = ND; p.NGT = NGT; p.rec_thrs = rec_thrs; p.precision = precision; p.recall = recall;
  for (int m = 0; m < CE_M; ++m) p.max_dets[m] = max_dets[m];
  CP_LAUNCH(coco_accumulate_kernel, dim3((unsigned)(K * CE_A * CE_M)), dim3(CE_ACC_THREADS), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}
