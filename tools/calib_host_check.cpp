// The host halves of csrc/calibrate.hip -- the argument checks of cp_code_reliability, cp_fit_code_scale and cp_sigma2_consistency, the
// edge-table checks, the size queries and the B = 0 paths -- exercised by a stand-alone program, so that they can be built under
// AddressSanitizer + UndefinedBehaviorSanitizer (`make -C checkerpose_amd/csrc calib_host_check`, then run
// checkerpose_amd/csrc/calib_host_check).  Every call below returns before any launch: no device is needed, nothing is loaded into
// Python.  The host tables (scales, edges, groups) are sized EXACTLY: a read past their end is the sanitizer's to report.  Exit status
// 0 = every refusal as expected.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../include/checkerpose_hip.h"

static int failures = 0, refusals = 0;
#define EXPECT(what, want)                                                                          \
  do {                                                                                              \
    const long long got_ = (long long)(what);                                                       \
    if (got_ != (long long)(want)) { printf("FAIL %s: %lld, expected %lld\n", #what, got_, (long long)(want)); ++failures; } \
    else if ((long long)(want) < 0) ++refusals;                                                     \
  } while (0)

int main() {
  alignas(16) static unsigned char buf[4096];
  float* f = (float*)buf;
  int32_t* i32 = (int32_t*)buf;
  double* d = (double*)buf;
  long long* i64 = (long long*)buf;
  uint8_t* u8 = buf;
  const int N = 64, r = 6, K = 13, M = 15;
  std::vector<double> scale(K, 1.0), edges(M - 1);
  for (int k = 1; k < M; ++k) edges[k - 1] = log((double)k / (double)(M - k));
  std::vector<int32_t> group(K);
  for (int k = 0; k < K; ++k) group[k] = k;

  // cp_code_reliability
  struct R {
    const float* bits; long long bs; int rows, r; const float* roi; const float* gx; const float* gy; int gb; const double* scale;
    const double* edges; int M, B, N; long long* ints; double* sums; void* scratch;
  };
  const R rok = {f, 13LL * N, 13, r, f, f, f, 6, scale.data(), edges.data(), M, 2, N, i64, d, buf};
  auto rel = [](const R& a) {
    return cp_code_reliability(nullptr, a.bits, a.bs, a.rows, a.r, a.roi, a.gx, a.gy, a.gb, a.scale, a.edges, a.M, a.B, a.N, a.ints, a.sums, a.scratch);
  };
  R a;
  a = rok; a.bits = nullptr; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.roi = nullptr; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.gx = nullptr; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.gy = nullptr; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.scale = nullptr; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.edges = nullptr; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.ints = nullptr; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.sums = nullptr; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.scratch = nullptr; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.B = 0; a.sums = nullptr; EXPECT(rel(a), CP_ERR_INVALID);          // also with nothing to do
  a = rok; a.B = -1; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.N = 0; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.N = -4; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.r = 0; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.r = 31; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.rows = 12; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.gb = 5; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.bs = 13LL * N - 1; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.bs = -13LL * N; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.M = 0; EXPECT(rel(a), CP_ERR_INVALID);
  a = rok; a.M = 65; EXPECT(rel(a), CP_ERR_INVALID);
  // the scales: each finite and > 0
  const double bad_scale[] = {0.0, -1.0, NAN, INFINITY, -INFINITY};
  for (double v : bad_scale) {
    std::vector<double> s2 = scale;
    s2[K - 1] = v;
    a = rok; a.scale = s2.data(); EXPECT(rel(a), CP_ERR_INVALID);
    s2 = scale; s2[0] = v;
    a = rok; a.scale = s2.data(); EXPECT(rel(a), CP_ERR_INVALID);
  }
  // the edge table: no NaN, strictly ascending
  { std::vector<double> e = edges; e[3] = NAN; a = rok; a.edges = e.data(); EXPECT(rel(a), CP_ERR_INVALID); }
  { std::vector<double> e = edges; e[0] = NAN; a = rok; a.edges = e.data(); EXPECT(rel(a), CP_ERR_INVALID); }
  { std::vector<double> e = edges; e[M - 2] = NAN; a = rok; a.edges = e.data(); EXPECT(rel(a), CP_ERR_INVALID); }
  { std::vector<double> e = edges; e[3] = e[2]; a = rok; a.edges = e.data(); EXPECT(rel(a), CP_ERR_INVALID); }
  { std::vector<double> e = edges; e[3] = e[4]; a = rok; a.edges = e.data(); EXPECT(rel(a), CP_ERR_INVALID); }
  { std::vector<double> e(edges.rbegin(), edges.rend()); a = rok; a.edges = e.data(); EXPECT(rel(a), CP_ERR_INVALID); }
  { std::vector<double> e = edges; e[0] = -INFINITY; e[M - 2] = INFINITY; a = rok; a.B = 0; a.edges = e.data(); EXPECT(rel(a), CP_OK); }      // legal ends
  { std::vector<double> e(63); for (int k = 0; k < 63; ++k) e[k] = k; a = rok; a.B = 0; a.M = 64; a.edges = e.data(); EXPECT(rel(a), CP_OK); }
  { std::vector<double> s61(61, 0.5); a = rok; a.B = 0; a.r = 30; a.rows = 61; a.gb = 30; a.bs = 61LL * N; a.scale = s61.data(); EXPECT(rel(a), CP_OK); }
  // alignment
  a = rok; a.bits = (const float*)(buf + 2); EXPECT(rel(a), CP_ERR_ALIGN);
  a = rok; a.roi = (const float*)(buf + 2); EXPECT(rel(a), CP_ERR_ALIGN);
  a = rok; a.gx = (const float*)(buf + 1); EXPECT(rel(a), CP_ERR_ALIGN);
  a = rok; a.gy = (const float*)(buf + 3); EXPECT(rel(a), CP_ERR_ALIGN);
  a = rok; a.ints = (long long*)(buf + 4); EXPECT(rel(a), CP_ERR_ALIGN);
  a = rok; a.sums = (double*)(buf + 4); EXPECT(rel(a), CP_ERR_ALIGN);
  a = rok; a.scratch = buf + 4; EXPECT(rel(a), CP_ERR_ALIGN);
  // B = 0: nothing to do, returns without a launch; one bin needs no table
  a = rok; a.B = 0; EXPECT(rel(a), CP_OK);
  a = rok; a.B = 0; a.M = 1; a.edges = nullptr; EXPECT(rel(a), CP_OK);
  EXPECT(cp_code_reliability_scratch_bytes(6, 15), 1024LL * 13 * (3 * 15 + 7) * 8);
  EXPECT(cp_code_reliability_scratch_bytes(30, 64), 1024LL * 61 * (3 * 64 + 7) * 8);
  EXPECT(cp_code_reliability_scratch_bytes(0, 15), 0);
  EXPECT(cp_code_reliability_scratch_bytes(31, 15), 0);
  EXPECT(cp_code_reliability_scratch_bytes(6, 0), 0);
  EXPECT(cp_code_reliability_scratch_bytes(6, 65), 0);

  // cp_fit_code_scale
  struct F {
    const float* bits; long long bs; int rows, r; const float* roi; const float* gx; const float* gy; int gb; const int32_t* group; int G, B, N;
    double s_min, s_max, tol; int iters; double* scale; double* info; void* scratch;
  };
  const F fok = {f, 13LL * N, 13, r, f, f, f, 6, group.data(), K, 2, N, 1.0 / 64, 64.0, 1e-8, 60, d, d, buf};
  auto fit = [](const F& a) {
    return cp_fit_code_scale(nullptr, a.bits, a.bs, a.rows, a.r, a.roi, a.gx, a.gy, a.gb, a.group, a.G, a.B, a.N, a.s_min, a.s_max, a.tol, a.iters,
                             a.scale, a.info, a.scratch);
  };
  F b;
  b = fok; b.bits = nullptr; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.roi = nullptr; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.gx = nullptr; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.gy = nullptr; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.group = nullptr; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.scale = nullptr; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.info = nullptr; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.scratch = nullptr; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.B = -1; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.N = 0; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.r = 0; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.r = 31; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.rows = 12; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.gb = 5; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.bs = 13LL * N - 1; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.G = 0; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.G = K + 1; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.G = K - 1; EXPECT(fit(b), CP_ERR_INVALID);                         // row 12 names group 12 of 12
  { std::vector<int32_t> g2 = group; g2[5] = -1; b = fok; b.group = g2.data(); EXPECT(fit(b), CP_ERR_INVALID); }
  { std::vector<int32_t> g2 = group; g2[K - 1] = K; b = fok; b.group = g2.data(); EXPECT(fit(b), CP_ERR_INVALID); }
  // the bracket: 0 < s_min <= 1 <= s_max < inf, s_min < s_max
  b = fok; b.s_min = 0.0; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.s_min = -1.0; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.s_min = NAN; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.s_min = 2.0; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.s_max = 0.5; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.s_max = INFINITY; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.s_max = NAN; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.s_min = 1.0; b.s_max = 1.0; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.tol = 0.0; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.tol = -1e-8; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.tol = NAN; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.tol = INFINITY; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.iters = 0; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.iters = -1; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.iters = CP_CALIB_MAX_ITERS + 1; EXPECT(fit(b), CP_ERR_INVALID);
  b = fok; b.bits = (const float*)(buf + 2); EXPECT(fit(b), CP_ERR_ALIGN);
  b = fok; b.scale = (double*)(buf + 4); EXPECT(fit(b), CP_ERR_ALIGN);
  b = fok; b.info = (double*)(buf + 4); EXPECT(fit(b), CP_ERR_ALIGN);
  b = fok; b.scratch = buf + 4; EXPECT(fit(b), CP_ERR_ALIGN);
  b = fok; b.B = 0; EXPECT(fit(b), CP_OK);
  b = fok; b.B = 0; b.s_min = 1.0; EXPECT(fit(b), CP_OK);                       // the bracket may start at 1
  b = fok; b.B = 0; b.iters = CP_CALIB_MAX_ITERS; EXPECT(fit(b), CP_OK);
  { std::vector<int32_t> g1(K, 0); b = fok; b.B = 0; b.G = 1; b.group = g1.data(); EXPECT(fit(b), CP_OK); }
  EXPECT(cp_fit_code_scale_info_doubles(), 12);
  EXPECT(cp_fit_code_scale_scratch_bytes(6), 1024LL * 13 * 4 * 8);
  EXPECT(cp_fit_code_scale_scratch_bytes(0), 0);
  EXPECT(cp_fit_code_scale_scratch_bytes(31), 0);

  // cp_sigma2_consistency
  std::vector<double> chi = {0.25, 1.0, 4.0, 5.99, 9.21};
  struct P {
    const float* p2d; const double* proj; const double* s2; const uint8_t* valid; int vs; const float* roi; const double* edges; int E, B, N;
    int32_t* counts; int32_t* nn; double* sums;
  };
  const P pok = {f, d, d, u8, 3, f, chi.data(), 5, 2, N, i32, i32, d};
  auto pit = [](const P& a) {
    return cp_sigma2_consistency(nullptr, a.p2d, a.proj, a.s2, a.valid, a.vs, a.roi, a.edges, a.E, a.B, a.N, a.counts, a.nn, a.sums);
  };
  P c;
  c = pok; c.p2d = nullptr; EXPECT(pit(c), CP_ERR_INVALID);
  c = pok; c.proj = nullptr; EXPECT(pit(c), CP_ERR_INVALID);
  c = pok; c.s2 = nullptr; EXPECT(pit(c), CP_ERR_INVALID);
  c = pok; c.valid = nullptr; EXPECT(pit(c), CP_ERR_INVALID);
  c = pok; c.roi = nullptr; EXPECT(pit(c), CP_ERR_INVALID);
  c = pok; c.edges = nullptr; EXPECT(pit(c), CP_ERR_INVALID);
  c = pok; c.counts = nullptr; EXPECT(pit(c), CP_ERR_INVALID);
  c = pok; c.nn = nullptr; EXPECT(pit(c), CP_ERR_INVALID);
  c = pok; c.sums = nullptr; EXPECT(pit(c), CP_ERR_INVALID);
  c = pok; c.B = -1; EXPECT(pit(c), CP_ERR_INVALID);
  c = pok; c.N = 0; EXPECT(pit(c), CP_ERR_INVALID);
  c = pok; c.vs = 0; EXPECT(pit(c), CP_ERR_INVALID);
  c = pok; c.vs = -3; EXPECT(pit(c), CP_ERR_INVALID);
  c = pok; c.E = -1; EXPECT(pit(c), CP_ERR_INVALID);
  c = pok; c.E = 64; EXPECT(pit(c), CP_ERR_INVALID);
  { std::vector<double> e = chi; e[2] = e[1]; c = pok; c.edges = e.data(); EXPECT(pit(c), CP_ERR_INVALID); }
  { std::vector<double> e = chi; e[4] = NAN; c = pok; c.edges = e.data(); EXPECT(pit(c), CP_ERR_INVALID); }
  { std::vector<double> e(chi.rbegin(), chi.rend()); c = pok; c.edges = e.data(); EXPECT(pit(c), CP_ERR_INVALID); }
  c = pok; c.p2d = (const float*)(buf + 2); EXPECT(pit(c), CP_ERR_ALIGN);
  c = pok; c.roi = (const float*)(buf + 2); EXPECT(pit(c), CP_ERR_ALIGN);
  c = pok; c.proj = (const double*)(buf + 4); EXPECT(pit(c), CP_ERR_ALIGN);
  c = pok; c.s2 = (const double*)(buf + 4); EXPECT(pit(c), CP_ERR_ALIGN);
  c = pok; c.sums = (double*)(buf + 4); EXPECT(pit(c), CP_ERR_ALIGN);
  c = pok; c.counts = (int32_t*)(buf + 2); EXPECT(pit(c), CP_ERR_ALIGN);
  c = pok; c.nn = (int32_t*)(buf + 2); EXPECT(pit(c), CP_ERR_ALIGN);
  c = pok; c.B = 0; EXPECT(pit(c), CP_OK);
  c = pok; c.B = 0; c.E = 0; c.edges = nullptr; EXPECT(pit(c), CP_OK);          // one bin needs no table
  c = pok; c.B = 0; c.valid = u8 + 2; EXPECT(pit(c), CP_OK);                    // a column of the (B,N,3) block: any byte address
  { std::vector<double> e(63); for (int k = 0; k < 63; ++k) e[k] = 0.5 * k; c = pok; c.B = 0; c.E = 63; c.edges = e.data(); EXPECT(pit(c), CP_OK); }
  printf("calib host check: %d refusal(s) as expected, %d failure(s)\n", refusals, failures);
  return failures ? 1 : 0;
}
