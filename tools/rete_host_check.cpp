// The host half of csrc/rete.hip -- argument checks and the walks over the host copies of the offsets, mesh ids and slots --
// exercised by a stand-alone program, so that it can be built under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C checkerpose_amd/csrc rete_host_check`, then run checkerpose_amd/csrc/rete_host_check).  Every call below returns before
// any launch or runtime call: no device is needed, nothing is loaded into Python.  Exit status 0 = every refusal as expected.
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
  double* d = (double*)buf;
  int32_t* i32 = (int32_t*)buf;
  // the host tables are heap blocks of exactly the sizes the entry points may read: a walk past them is the sanitizer's to find
  std::vector<int32_t> off = {0, 1, 3, 3}, ids = {0, 1, 2, 1, 0}, slots = {0, 12, 3, 3, 1};
  struct A {
    const double* a; const double* b; int P; const double* syms; const int32_t* off; const int32_t* off_h; int M;
    const int32_t* ids; const int32_t* ids_h; double* re; double* te; double* cs; int32_t* idx;
  };
  const A ok = {d, d, 5, d, i32, off.data(), 3, i32, ids.data(), d, d, d, i32};
  auto call = [](const A& x) {
    return cp_pose_rete(nullptr, x.a, x.b, x.P, x.syms, x.off, x.off_h, x.M, x.ids, x.ids_h, x.re, x.te, x.cs, x.idx);
  };
  A a;
  // null pointers (cos and index may be null; the table and its companions come together)
  a = ok; a.a = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.b = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.re = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.te = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.off = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.off_h = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.ids = nullptr; a.ids_h = nullptr; EXPECT(call(a), CP_ERR_INVALID);       // three sets need ids
  a = ok; a.P = 0; a.te = nullptr; EXPECT(call(a), CP_ERR_INVALID);                  // also with nothing to do
  a = ok; a.syms = nullptr; EXPECT(call(a), CP_ERR_INVALID);                         // companions without the table
  a = ok; a.syms = nullptr; a.off = nullptr; a.off_h = nullptr; a.ids_h = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.syms = nullptr; a.off = nullptr; a.off_h = nullptr; a.ids = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  // sizes
  a = ok; a.P = -1; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.M = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.M = -3; EXPECT(call(a), CP_ERR_INVALID);
  // offsets that do not start at 0 or do not ascend
  { std::vector<int32_t> o = {1, 2, 3, 4}; a = ok; a.off_h = o.data(); EXPECT(call(a), CP_ERR_INVALID); }
  { std::vector<int32_t> o = {0, 2, 1, 3}; a = ok; a.off_h = o.data(); EXPECT(call(a), CP_ERR_INVALID); }
  { std::vector<int32_t> o = {0, 2, 3, -1}; a = ok; a.off_h = o.data(); EXPECT(call(a), CP_ERR_INVALID); }
  // a mesh id out of range
  { std::vector<int32_t> m = {0, 1, 3, 1, 0}; a = ok; a.ids_h = m.data(); EXPECT(call(a), CP_ERR_INVALID); }
  { std::vector<int32_t> m = {0, 1, 2, 1, -1}; a = ok; a.ids_h = m.data(); EXPECT(call(a), CP_ERR_INVALID); }
  // alignment
  a = ok; a.P = 0; a.a = (const double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.P = 0; a.b = (const double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.P = 0; a.syms = (const double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.P = 0; a.re = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.P = 0; a.te = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.P = 0; a.cs = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.P = 0; a.off = (const int32_t*)(buf + 2); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.P = 0; a.ids = (const int32_t*)(buf + 2); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.P = 0; a.idx = (int32_t*)(buf + 2); EXPECT(call(a), CP_ERR_ALIGN);
  // nothing to do: returns without a launch -- with the table, without the optional outputs, without the host ids, without a table
  a = ok; a.P = 0; EXPECT(call(a), CP_OK);
  a = ok; a.P = 0; a.cs = nullptr; a.idx = nullptr; EXPECT(call(a), CP_OK);
  a = ok; a.P = 0; a.ids_h = nullptr; EXPECT(call(a), CP_OK);
  a = ok; a.P = 0; a.syms = nullptr; a.off = nullptr; a.off_h = nullptr; a.ids = nullptr; a.ids_h = nullptr; a.M = 0; EXPECT(call(a), CP_OK);
  { std::vector<int32_t> o = {0, 628}; a = ok; a.P = 0; a.M = 1; a.off_h = o.data(); a.ids = nullptr; a.ids_h = nullptr; EXPECT(call(a), CP_OK); }

  struct C {
    const double* re; const double* te; const double* adx; const double* diam; const int32_t* slot; const int32_t* slot_h; int P, n; int32_t* out;
  };
  const C okc = {d, d, d, d, i32, slots.data(), 5, 13, i32};
  auto counts = [](const C& x) { return cp_rete_pass_counts(nullptr, x.re, x.te, x.adx, x.diam, x.slot, x.slot_h, x.P, x.n, x.out); };
  C c;
  c = okc; c.re = nullptr; EXPECT(counts(c), CP_ERR_INVALID);
  c = okc; c.te = nullptr; EXPECT(counts(c), CP_ERR_INVALID);
  c = okc; c.adx = nullptr; EXPECT(counts(c), CP_ERR_INVALID);
  c = okc; c.diam = nullptr; EXPECT(counts(c), CP_ERR_INVALID);
  c = okc; c.slot = nullptr; EXPECT(counts(c), CP_ERR_INVALID);
  c = okc; c.out = nullptr; EXPECT(counts(c), CP_ERR_INVALID);
  c = okc; c.P = -1; EXPECT(counts(c), CP_ERR_INVALID);
  c = okc; c.n = 0; EXPECT(counts(c), CP_ERR_INVALID);
  c = okc; c.n = 257; EXPECT(counts(c), CP_ERR_INVALID);
  c = okc; c.n = 12; EXPECT(counts(c), CP_ERR_INVALID);                              // slot 12 needs 13 objects
  { std::vector<int32_t> s = {0, -1, 3, 3, 1}; c = okc; c.slot_h = s.data(); EXPECT(counts(c), CP_ERR_INVALID); }
  c = okc; c.re = (const double*)(buf + 4); EXPECT(counts(c), CP_ERR_ALIGN);
  c = okc; c.te = (const double*)(buf + 4); EXPECT(counts(c), CP_ERR_ALIGN);
  c = okc; c.adx = (const double*)(buf + 4); EXPECT(counts(c), CP_ERR_ALIGN);
  c = okc; c.diam = (const double*)(buf + 4); EXPECT(counts(c), CP_ERR_ALIGN);
  c = okc; c.slot = (const int32_t*)(buf + 2); EXPECT(counts(c), CP_ERR_ALIGN);
  c = okc; c.out = (int32_t*)(buf + 2); EXPECT(counts(c), CP_ERR_ALIGN);
  EXPECT(cp_rete_pass_columns(), 10);
  for (int code : {CP_ERR_INVALID, CP_ERR_ALIGN})
    if (!cp_strerror(code) || !cp_strerror(code)[0]) { printf("FAIL cp_strerror(%d)\n", code); ++failures; }
  printf("rete host check: %d refusal(s) as expected, %d failure(s)\n", refusals, failures);
  return failures ? 1 : 0;
}
