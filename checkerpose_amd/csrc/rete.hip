// Rotation / translation errors on the device, symmetry-aware: bop_toolkit_lib.pose_error.re / .te for a batch
// of pose pairs, the rotation error optionally against the closest symmetric copy of the second pose, and the integer pass counts
// the reference's LM report is made of.
//
// THE RULE of cp_pose_rete.  It restates checkerpose/test_lm.py:33-55 (get_closest_rot) over bop_toolkit_lib/pose_error.py:187-214
// (re, te); tests/rete_stages.py restates it in numpy.  Per pair: A = [R_A | t_A], B = [R_B | t_B] (fp64), the symmetry set of the
// pair's mesh S_0 .. S_{S-1} (rows of the SymmetrySet table; only the ROTATION part of a row is read, as get_closest_rot reads only
// sym["R"]; the identity is not assumed to be a member).  Everything in fp64, no contraction.
//   candidates  in order: index -1 is R_B itself, then R_B . S_k for k = 0 .. S-1 (test_lm.py:50: rot_gt.dot(sym_info[i])), each entry
//               b_i0 s_0j + b_i1 s_1j + b_i2 s_2j summed left to right
//   cos_k       = 1 + 0.5 * (sum((R_A - R_cand) o cof(R_cand)) / det(R_cand)), the sum taken row by row: (trace(R_A . inv(R_cand)) - 1) / 2
//               of pose_error.py:196-199 with the inverse formed from the cofactors, so that equal matrices give cos = 1 exactly
//   re_k        = acos(min(1, max(-1, cos_k))) * (180 / pi); NaN where cos_k is not finite
//   winner      the FIRST candidate with the smallest re_k: candidate k replaces the best so far iff re_k < best (test_lm.py:52, strict;
//               the comparison is on re_k, after the clamp and acos).  NaN never replaces; a NaN plain candidate stays: NaN, index -1
//               (UNPINNED: the reference's min / max turn a NaN cosine into 180 degrees and np.linalg.inv raises on a singular matrix)
//   te          = sqrt(sum((t_B - t_A)^2)), independent of the symmetry (pose_error.py:202-214); a symmetry's translation is not used
//   outputs     re (degrees), te, cos (the winner's cos_k BEFORE the clamp), index (the winner's k, -1 for R_B itself)
// Every candidate goes through ONE device function (rete_cos, then rete_deg) on IEEE operations that the compiler may neither fuse
// nor reorder, so bitwise-equal candidate matrices give bitwise-equal re: R_B and R_B . I tie exactly and the earlier one is kept.
// A mesh id outside [0, M) or offsets that leave the table give NaN / NaN / index -1 for that pair (te is still computed).
//
// ONE launch, one wave per pair, four pairs per 256-thread workgroup.  Lane l evaluates the members s = l, l + 64, ... in ascending
// order and keeps its first minimum, starting from the plain candidate (every lane evaluates it: the same bits in all 64 lanes).  The
// wave joins by a lexicographic (re, index) minimum through __shfl_xor: the smaller index wins an equal re, NaN loses to a number.
// A fixed order, no atomics, no LDS.  A set is at most 1256 x 96 bytes: after the first wave it is read from L2.  Without a table
// S = 0 and the kernel is the plain re / te.
//
// cp_rete_pass_counts: the nine pass flags of test_lm.py:319-327 and the sample count, summed per object slot.  NaN counts as 10000
// first (test_lm.py:306-317), every `<` is strict.  Each workgroup sums into (n_obj, 10) int32 words in LDS, then adds its non-zero
// words to the result with integer vector atomics: integers, so the result does not depend on the order.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int RETE_THREADS = 256, RETE_WAVES = RETE_THREADS / 64, RETE_COLS = 10, RETE_MAX_OBJ = 256;

struct ReteParams {
  const double* A; const double* B; const double* syms; const int32_t* s_off; const int32_t* mesh_id;
  double* re; double* te; double* cs; int32_t* index;
  int P, M, sumS;
};

// (trace(Ra . inv(C)) - 1) / 2 with the inverse from the cofactors: rows of cof = r1 x r2, r2 x r0, r0 x r1 (the columns of adj C)
__device__ __forceinline__ double rete_cos(const double* Ra, const double* C) {
  const double c0 = C[4] * C[8] - C[5] * C[7], c1 = C[5] * C[6] - C[3] * C[8], c2 = C[3] * C[7] - C[4] * C[6];
  const double c3 = C[7] * C[2] - C[8] * C[1], c4 = C[8] * C[0] - C[6] * C[2], c5 = C[6] * C[1] - C[7] * C[0];
  const double c6 = C[1] * C[5] - C[2] * C[4], c7 = C[2] * C[3] - C[0] * C[5], c8 = C[0] * C[4] - C[1] * C[3];
  const double det = C[0] * c0 + C[1] * c1 + C[2] * c2;
  double s = (Ra[0] - C[0]) * c0;
  s += (Ra[1] - C[1]) * c1; s += (Ra[2] - C[2]) * c2;
  s += (Ra[3] - C[3]) * c3; s += (Ra[4] - C[4]) * c4; s += (Ra[5] - C[5]) * c5;
  s += (Ra[6] - C[6]) * c6; s += (Ra[7] - C[7]) * c7; s += (Ra[8] - C[8]) * c8;
  return 1.0 + 0.5 * (s / det);
}

__device__ __forceinline__ double rete_deg(double c) {
  if (!isfinite(c)) return NAN;
  return acos(fmin(1.0, fmax(-1.0, c))) * (180.0 / 3.14159265358979323846);
}

// (re_o, cos_o, idx_o) replaces (re, cos, idx) in the wave's join: smaller re, or equal re and smaller index; NaN loses to a number
__device__ __forceinline__ bool rete_better(double re_o, int idx_o, double re, int idx) {
  return re_o < re || (re_o == re && idx_o < idx) || (re != re && re_o == re_o);
}

__global__ __launch_bounds__(RETE_THREADS) void pose_rete_kernel(const ReteParams p) {
  const int lane = threadIdx.x & 63;
  const long long pair = (long long)blockIdx.x * RETE_WAVES + (threadIdx.x >> 6);
  if (pair >= p.P) return;                                                     // whole waves leave: no barrier follows
  const double* a = p.A + (size_t)pair * 12;
  const double* b = p.B + (size_t)pair * 12;
  double Ra[9], Rb[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) { Ra[i] = a[i]; Rb[i] = b[i]; }
  int s0 = 0, s1 = 0;
  bool bad = false;
  if (p.syms) {
    const int m = p.mesh_id ? p.mesh_id[pair] : 0;
    if (m < 0 || m >= p.M) {
      bad = true;
    } else {
      s0 = p.s_off[m]; s1 = p.s_off[m + 1];
      if (s0 < 0 || s1 < s0 || s1 > p.sumS) { bad = true; s0 = s1 = 0; }
    }
  }
  double best_cos = rete_cos(Ra, Rb);
  double best_re = rete_deg(best_cos);
  int best_idx = -1;
  if (bad) { best_cos = NAN; best_re = NAN; }
  for (int k = lane; k < s1 - s0; k += 64) {
    const double* S = p.syms + (size_t)(s0 + k) * 12;
    double Sm[9], C[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Sm[i] = S[i];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) C[3 * i + j] = Rb[3 * i] * Sm[j] + Rb[3 * i + 1] * Sm[3 + j] + Rb[3 * i + 2] * Sm[6 + j];
    const double c = rete_cos(Ra, C);
    const double r = rete_deg(c);
    if (r < best_re) { best_re = r; best_cos = c; best_idx = k; }               // strict: the earlier candidate keeps an equal re
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double re_o = __shfl_xor(best_re, d, 64), cos_o = __shfl_xor(best_cos, d, 64);
    const int idx_o = __shfl_xor(best_idx, d, 64);
    if (rete_better(re_o, idx_o, best_re, best_idx)) { best_re = re_o; best_cos = cos_o; best_idx = idx_o; }
  }
  if (lane != 0) return;
  const double d0 = b[9] - a[9], d1 = b[10] - a[10], d2 = b[11] - a[11];
  p.re[pair] = best_re;
  p.te[pair] = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  if (p.cs) p.cs[pair] = best_cos;
  if (p.index) p.index[pair] = best_idx;
}

__global__ __launch_bounds__(RETE_THREADS) void rete_pass_counts_kernel(const double* __restrict__ re, const double* __restrict__ te,
                                                                        const double* __restrict__ adx, const double* __restrict__ diam,
                                                                        const int32_t* __restrict__ slot, int P, int n_obj,
                                                                        int32_t* __restrict__ counts) {
  __shared__ int32_t part[RETE_MAX_OBJ * RETE_COLS];
  const int n = n_obj * RETE_COLS;
  for (int i = threadIdx.x; i < n; i += RETE_THREADS) part[i] = 0;
  __syncthreads();
  const long long i = (long long)blockIdx.x * RETE_THREADS + threadIdx.x;
  if (i < P) {
    const int s = slot[i];
    if (s >= 0 && s < n_obj) {
      double e = adx[i], r = re[i], t = te[i];
      const double d = diam[i];
      if (e != e) e = 10000.0;
      if (r != r) r = 10000.0;
      if (t != t) t = 10000.0;
      const bool f[RETE_COLS] = {true, e < d * 0.02, e < d * 0.05, e < d * 0.1, r < 2.0 && t < 20.0, r < 5.0 && t < 50.0,
                                 r < 2.0, r < 5.0, t < 20.0, t < 50.0};
#pragma unroll
      for (int c = 0; c < RETE_COLS; ++c)
        if (f[c]) atomicAdd(&part[s * RETE_COLS + c], 1);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < n; k += RETE_THREADS)
    if (part[k]) atomicAdd(&counts[k], part[k]);
}

}  // namespace

extern "C" int cp_rete_pass_columns(void) { return RETE_COLS; }

extern "C" int cp_pose_rete(cp_stream_t stream, const double* pose_a, const double* pose_b, int P, const double* syms,
                            const int32_t* s_offsets, const int32_t* s_offsets_host, int M, const int32_t* mesh_ids,
                            const int32_t* mesh_ids_host, double* re, double* te, double* cos_out, int32_t* index) {
  if (!pose_a || !pose_b || !re || !te) return CP_ERR_INVALID;
  if (P < 0) return CP_ERR_INVALID;
  int sumS = 0;
  if (syms) {
    if (!s_offsets || !s_offsets_host || M < 1) return CP_ERR_INVALID;
    if (!mesh_ids && M != 1) return CP_ERR_INVALID;
    if (s_offsets_host[0] != 0) return CP_ERR_INVALID;
    for (int m = 0; m < M; ++m)
      if (s_offsets_host[m + 1] < s_offsets_host[m]) return CP_ERR_INVALID;   // the offsets must ascend (an empty set is S = 0)
    sumS = s_offsets_host[M];
    if (mesh_ids && mesh_ids_host)
      for (int i = 0; i < P; ++i)
        if (mesh_ids_host[i] < 0 || mesh_ids_host[i] >= M) return CP_ERR_INVALID;
  } else if (s_offsets || s_offsets_host || mesh_ids || mesh_ids_host) {
    return CP_ERR_INVALID;                                                    // the table's companions without the table
  }
  if (((uintptr_t)pose_a & 7) || ((uintptr_t)pose_b & 7) || ((uintptr_t)syms & 7) || ((uintptr_t)re & 7) || ((uintptr_t)te & 7) ||
      ((uintptr_t)cos_out & 7) || ((uintptr_t)s_offsets & 3) || ((uintptr_t)mesh_ids & 3) || ((uintptr_t)index & 3))
    return CP_ERR_ALIGN;
  if (P == 0) return CP_OK;
  ReteParams p;
  p.A = pose_a; p.B = pose_b; p.syms = syms; p.s_off = s_offsets; p.mesh_id = mesh_ids;
  p.re = re; p.te = te; p.cs = cos_out; p.index = index; p.P = P; p.M = M; p.sumS = sumS;
  const unsigned blocks = (unsigned)(((long long)P + RETE_WAVES - 1) / RETE_WAVES);
  CP_LAUNCH(pose_rete_kernel, dim3(blocks), dim3(RETE_THREADS), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}

extern "C" int cp_rete_pass_counts(cp_stream_t stream, const double* re, const double* te, const double* adx, const double* diam,
                                   const int32_t* slot, const int32_t* slot_host, int P, int n_obj, int32_t* counts) {
  if (!re || !te || !adx || !diam || !slot || !counts) return CP_ERR_INVALID;
  if (P < 0 || n_obj < 1 || n_obj > RETE_MAX_OBJ) return CP_ERR_INVALID;
  if (slot_host)
    for (int i = 0; i < P; ++i)
      if (slot_host[i] < 0 || slot_host[i] >= n_obj) return CP_ERR_INVALID;
  if (((uintptr_t)re & 7) || ((uintptr_t)te & 7) || ((uintptr_t)adx & 7) || ((uintptr_t)diam & 7) || ((uintptr_t)slot & 3) ||
      ((uintptr_t)counts & 3))
    return CP_ERR_ALIGN;
  if (hipMemsetAsync(counts, 0, (size_t)n_obj * RETE_COLS * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return CP_ERR_HIP;
  if (P == 0) return CP_OK;
  const unsigned blocks = (unsigned)(((long long)P + RETE_THREADS - 1) / RETE_THREADS);
  CP_LAUNCH(rete_pass_counts_kernel, dim3(blocks), dim3(RETE_THREADS), 0, (hipStream_t)stream, re, te, adx, diam, slot, P, n_obj, counts);
  return cp_check_launch();
}
