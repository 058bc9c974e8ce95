// cp_coco_rle_unpack: pycoco_utils.rle_to_binary_mask on the device -- the column-major run lists that
// cp_coco_rle_write / cp_paste_rle_write make (and that COCO annotation / result files carry) -> PackedMasks bit rows, area and box in
// cp_coco_pack's layout, with no dense mask on either side.
//
// THE RULE.  Mask n has m = offsets[n + 1] - offsets[n] run lengths c_0 .. c_{m-1} at counts[offsets[n] : offsets[n + 1]] (int32 counts,
// int64 offsets).  E_j = c_0 + ... + c_j are the inclusive ends, summed in 64 bits.  Pixel i = x H + y (column-major) has
// k(i) = #{ j : E_j <= i }; it is SET iff k < m and k is odd.  That is rle_to_binary_mask including its corners: zero-length runs
// anywhere, a list whose sum is below H W (the rest is background), m = 0 and m = 1 (an empty mask).
//   bits    bit x & 31 of word x >> 5, WW = ceil(W / 32) words per row, bits past W zero (cp_coco_pack's)
//   area    the sum of the odd-indexed counts
//   box     from the runs, not from the bits: an odd run with c_k > 0 covers [s, e) = [E_k - c_k, E_k); xa = s / H, xb = (e - 1) / H;
//           xmin = min xa, xmax = max xb; if xa == xb the run adds the rows s - xa H .. e - 1 - xb H, otherwise rows 0 and H - 1 (it
//           crosses a column boundary: it touches the bottom of one column and the top of the next).  xmin ymin xmax ymax, -1s for an
//           empty mask: cp_coco_pack's box of the dense mask.
//   status  0 ok; 3 the offsets do not fit (off[n] < 0, off[n + 1] < off[n] or off[n + 1] > total; no count is read); otherwise 1 a
//           negative count; otherwise 2 E_{m-1} > H W.  A mask with a nonzero status gets all-zero bits, area 0 and a box of -1s
//           (the reference clips an over-long list silently; this project's rle_decode raises, and that stays the rule).
// The numpy restatement is tests/rle_stages.py.
//
// TWO LAUNCHES.
//   rle_scan_kernel   a workgroup per mask walks the counts in passes of RU_SCAN_THREADS: a block scan of 64-bit sums (a wave scan by
//                     shuffles, the waves meet in LDS), the running sum, the area and the box carried across the passes in registers.
//                     It writes the inclusive ends, clamped to H W, into the int32 scratch (ends[offsets[n] + j]; an end above H W
//                     compares like H W against every pixel index, and such a mask has status 2 anyway), then reduces status, area
//                     and box and writes them.  [2^31 - 1, 2^31 - 1] ends as status 2: at most 2^31 counts below 2^31 sum below 2^62.
//   rle_bits_kernel   a wave per (64-column strip, 64-row band) of a mask, RU_BITS_WAVES waves per workgroup, the workgroups of all
//                     masks in one flat grid.  A lane owns column x: it finds k(x H + y0) by a binary search over the mask's ends (at
//                     most 32 steps) and walks down its column with a monotone cursor (while k < m and ends[k] <= i: ++k; bounded by
//                     m).  Per row __ballot(set) is the strip's two words; lane r KEEPS the ballot of the band's row r, and after the
//                     band every lane stores its own row's two words -- one store instruction per wave and band instead of one per
//                     row.  Every lane reaches every ballot: a lane with x >= W votes 0 and does not return, the cursor loop ends
//                     before the ballot.  A mask with a nonzero status has m = 0 here: zeros.
// Every bit word of every mask is written exactly once, the zero words included.  No floating point, no atomics, every loop has an
// explicit bound; the same bits for a mask alone or in a batch.  The stretches [offsets[n], offsets[n + 1]) of two masks must not
// overlap (they share the scratch); every access stays inside [0, total) whatever the offsets hold.
#include <limits.h>

#include "common.h"

namespace {

constexpr int RU_SCAN_THREADS = 512, RU_SCAN_WAVES = RU_SCAN_THREADS / 64;
constexpr int RU_BAND = 64, RU_BITS_WAVES = 4;

__global__ __launch_bounds__(RU_SCAN_THREADS) void rle_scan_kernel(const int32_t* __restrict__ counts, const int64_t* __restrict__ off,
                                                                    int H, int W, long long total, int32_t* __restrict__ ends,
                                                                    int32_t* __restrict__ area, int32_t* __restrict__ box,
                                                                    int32_t* __restrict__ status) {
  __shared__ long long s_tot[RU_SCAN_WAVES];
  __shared__ long long s_area[RU_SCAN_WAVES];
  __shared__ int s_red[RU_SCAN_WAVES][5];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.x;
  const long long base = off[n], m = off[n + 1] - base, HW = (long long)H * W;      // (HW < 2^31 - 4096: checked by the caller)
  if (base < 0 || m < 0 || base + m > total) {                       // (uniform) no count is read
    if (tid == 0) { status[n] = 3; area[n] = 0; box[4 * n] = -1; box[4 * n + 1] = -1; box[4 * n + 2] = -1; box[4 * n + 3] = -1; }
    return;
  }
  const int32_t* __restrict__ c = counts + base;
  int32_t* __restrict__ e = ends + base;
  long long carry = 0, my_area = 0;                                  // carry: E of the last count of the passes before (uniform)
  int neg = 0, x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
  for (long long j0 = 0; j0 < m; j0 += RU_SCAN_THREADS) {            // ceil(m / RU_SCAN_THREADS) passes, m < 2^31
    const long long j = j0 + tid;
    int cj = 0;
    if (j < m) {
      cj = c[j];
      if (cj < 0) { neg = 1; cj = 0; }
    }
    long long v = cj;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long o = __shfl_up(v, d, 64);
      if (lane >= d) v += o;
    }
    if (lane == 63) s_tot[wave] = v;
    __syncthreads();
    long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < RU_SCAN_WAVES; ++w) {
      const long long t = s_tot[w];
      if (w < wave) before += t;
      all += t;
    }
    __syncthreads();                                                 // s_tot is rewritten by the next pass
    const long long E = carry + before + v;                          // the inclusive end of count j
    if (j < m) {
      e[j] = (int32_t)min(E, HW);
      if ((j & 1) && cj > 0 && E <= HW) {                            // an odd run that lies in the frame: area and box
        my_area += cj;
        const int s = (int)(E - cj), l = (int)(E - 1);
        const int xa = s / H, xb = l / H;
        x0 = min(x0, xa);
        x1 = max(x1, xb);
        if (xa == xb) {
          y0 = min(y0, s - xa * H);
          y1 = max(y1, l - xb * H);
        } else {
          y0 = 0;
          y1 = H - 1;
        }
      }
    }
    carry += all;
  }
  // ---- status, area and box of the mask
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    my_area += __shfl_xor(my_area, d, 64);
    neg |= __shfl_xor(neg, d, 64);
    x0 = min(x0, __shfl_xor(x0, d, 64));
    y0 = min(y0, __shfl_xor(y0, d, 64));
    x1 = max(x1, __shfl_xor(x1, d, 64));
    y1 = max(y1, __shfl_xor(y1, d, 64));
  }
  if (lane == 0) { s_area[wave] = my_area; s_red[wave][0] = neg; s_red[wave][1] = x0; s_red[wave][2] = y0; s_red[wave][3] = x1; s_red[wave][4] = y1; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < RU_SCAN_WAVES; ++w) {
      my_area += s_area[w]; neg |= s_red[w][0];
      x0 = min(x0, s_red[w][1]); y0 = min(y0, s_red[w][2]); x1 = max(x1, s_red[w][3]); y1 = max(y1, s_red[w][4]);
    }
    const int st = neg ? 1 : (carry > HW ? 2 : 0);
    const bool some = st == 0 && my_area > 0;
    status[n] = st;
    area[n] = st == 0 ? (int32_t)my_area : 0;
    box[4 * n] = some ? x0 : -1; box[4 * n + 1] = some ? y0 : -1; box[4 * n + 2] = some ? x1 : -1; box[4 * n + 3] = some ? y1 : -1;
  }
}

__global__ __launch_bounds__(RU_BITS_WAVES * 64) void rle_bits_kernel(const int32_t* __restrict__ ends, const int64_t* __restrict__ off,
                                                                       const int32_t* __restrict__ status, int H, int W, int WW,
                                                                       int strips, int items, unsigned blocks_per_mask,
                                                                       uint32_t* __restrict__ bits) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned n = blockIdx.x / blocks_per_mask;
  const int item = (int)(blockIdx.x - n * blocks_per_mask) * RU_BITS_WAVES + wave;      // (strip, band) of this wave
  if (item >= items) return;                                         // (uniform per wave; the kernel has no barrier)
  const int band = item / strips, strip = item - band * strips;
  const int ya = band * RU_BAND, yb = min(ya + RU_BAND, H), x = strip * 64 + lane;
  int m = 0;
  const int32_t* __restrict__ e = ends;
  if (status[n] == 0) {                                              // (uniform) offsets that fit, checked by the scan launch
    const long long base = off[n];
    m = (int)(off[n + 1] - base);                                    // (<= total < 2^31)
    e = ends + base;
  }
  const bool live = x < W;
  int i = live ? x * H + ya : 0, k = 0;                              // (x H + y < H W < 2^31)
  if (live) {                                                        // k = #{ j : e[j] <= i }: the ends ascend
    int lo = 0, hi = m;
    for (int step = 0; step < 32 && lo < hi; ++step) {
      const int mid = lo + ((hi - lo) >> 1);
      if (e[mid] <= i) lo = mid + 1; else hi = mid;
    }
    k = lo;
  }
  int nxt = (live && k < m) ? e[k] : INT_MAX;                        // the end of run k; INT_MAX: past the list
  unsigned long long mine = 0;
  for (int y = ya; y < yb; ++y, ++i) {                               // (uniform) at most RU_BAND rows
    while (k < m && nxt <= i) {                                      // the monotone cursor: at most m steps over the whole band
      ++k;
      nxt = k < m ? e[k] : INT_MAX;
    }
    const bool set = live && k < m && (k & 1);
    const unsigned long long bal = __ballot(set);                    // reached by every lane of the wave
    if (lane == y - ya) mine = bal;
  }
  if (ya + lane < yb) {
    uint32_t* __restrict__ row = bits + ((size_t)n * H + ya + lane) * WW + 2 * strip;
    row[0] = (uint32_t)mine;
    if (2 * strip + 1 < WW) row[1] = (uint32_t)(mine >> 32);
  }
}

}  // namespace

extern "C" size_t cp_coco_rle_unpack_scratch_bytes(long long total) { return total > 0 ? (size_t)total * sizeof(int32_t) : 0; }

extern "C" int cp_coco_rle_unpack(cp_stream_t stream, const int32_t* counts, const int64_t* offsets, int N, int H, int W, long long total,
                                  int32_t* ends_scratch, uint32_t* bits, int32_t* area, int32_t* box, int32_t* status) {
  if (!offsets || !area || !box || !status) return CP_ERR_INVALID;
  if (N < 1 || H < 1 || W < 1 || total < 0) return CP_ERR_INVALID;
  if (total > 0 && (!counts || !ends_scratch)) return CP_ERR_INVALID;
  if (cp_misaligned(counts, 3) || cp_misaligned(offsets, 7) || cp_misaligned(ends_scratch, 3) || cp_misaligned(bits, 3) ||
      cp_misaligned(area, 3) || cp_misaligned(box, 3) || cp_misaligned(status, 3))
    return CP_ERR_ALIGN;
  if ((long long)H * W >= (1LL << 31) - 4096 || N >= (1 << 24) || total >= (1LL << 31)) return CP_ERR_RANGE;
  const int strips = (W + 63) / 64, bands = (H + RU_BAND - 1) / RU_BAND;
  const long long items = (long long)strips * bands, blocks_per_mask = (items + RU_BITS_WAVES - 1) / RU_BITS_WAVES;
  if (bits && blocks_per_mask * N >= (1LL << 31)) return CP_ERR_RANGE;
  CP_LAUNCH(rle_scan_kernel, dim3((unsigned)N), dim3(RU_SCAN_THREADS), 0, (hipStream_t)stream, counts, offsets, H, W, total, ends_scratch,
            area, box, status);
  if (bits)
    CP_LAUNCH(rle_bits_kernel, dim3((unsigned)(blocks_per_mask * N)), dim3(RU_BITS_WAVES * 64), 0, (hipStream_t)stream,
              (const int32_t*)ends_scratch, offsets, (const int32_t*)status, H, W, (W + 31) / 32, strips, (int)items,
              (unsigned)blocks_per_mask, bits);
  return cp_check_launch();
}
