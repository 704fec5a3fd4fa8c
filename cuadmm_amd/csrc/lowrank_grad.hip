// Value and gradient at per-block factors (cuadmm_lowrank_grad): the multiplier pass between A x and A'ytilde, and the per-block terms.
// lowrank_grad.h has the formulas and the contracts; DESIGN.md, "Value and gradient at factors", the chain they stand in.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lowrank_grad.h"
#include "device_util.h"
#include "wave_reduce.h"

namespace cuadmm {
namespace {

struct LgCoef { double xunit, bscale, ics, sigma; };

// one constraint: every operation rounded once, nothing contracted; sigma == 0 passes y's bits through
__device__ __forceinline__ void lg_one(const LgCoef& c, double ax, double b, double na, double y, double& yt, double& r, double (&s)[2]) {
  const double rs = __dsub_rn(__dmul_rn(c.xunit, ax), b);
  r = __dmul_rn(__dmul_rn(na, rs), c.bscale);
  const double t = __dmul_rn(__dmul_rn(__dmul_rn(c.sigma, r), na), c.ics);
  yt = c.sigma == 0.0 ? y : __dsub_rn(y, t);
  s[0] = __dadd_rn(s[0], __dmul_rn(y, rs));
  s[1] = __dadd_rn(s[1], __dmul_rn(r, r));
}

// index i: constraint i (kVec = false) or the constraints 2 i, 2 i + 1 (kVec = true; the last index may hold one)
template <bool kVec>
struct LgMultiplier {
  const double *ax, *b, *normA, *y;
  double *ytilde, *r;
  long long m;
  LgCoef c;
  __device__ __forceinline__ void add(double (&s)[2], long long i) const {
    if (kVec && 2 * i + 1 < m) {
      const double2 a2 = reinterpret_cast<const double2*>(ax)[i], b2 = reinterpret_cast<const double2*>(b)[i];
      const double2 n2 = reinterpret_cast<const double2*>(normA)[i], y2 = reinterpret_cast<const double2*>(y)[i];
      double2 yt, rr;
      lg_one(c, a2.x, b2.x, n2.x, y2.x, yt.x, rr.x, s);
      lg_one(c, a2.y, b2.y, n2.y, y2.y, yt.y, rr.y, s);
      reinterpret_cast<double2*>(ytilde)[i] = yt;
      reinterpret_cast<double2*>(r)[i] = rr;
      return;
    }
    const long long e = kVec ? 2 * i : i;      // (kVec: the odd last constraint; e < m by the launcher's count)
    double yt, rr;
    lg_one(c, ax[e], b[e], normA[e], y[e], yt, rr, s);
    ytilde[e] = yt;
    r[e] = rr;
  }
};

struct LgBlockTerms {
  static constexpr int V = 3, N = kLgSums;
  static constexpr bool kFlag = true;
  static constexpr const char* kName = "lrg_block_terms";
  const double* p[V];      // C, x, M
  __device__ __forceinline__ void add(double (&a)[N], const double (&v)[V], bool free_blk) const {
    a[0] += v[0] * v[1];
    a[1] += free_blk ? v[2] * v[2] : 0.0;
  }
};

}  // namespace

int launch_lrg_multiplier(int m, const double* ax, const double* b, const double* normA, const double* y, double xunit, double bscale, double ics, double sigma,
                          double* ytilde, double* r, double* partials, hipStream_t st) {
  if (m < 0 || (m > 0 && (!ax || !b || !normA || !y || !ytilde || !r)) || !partials || ytilde == y) { set_error("lrg_multiplier: invalid argument"); return CUADMM_ERR_INVALID; }
  uintptr_t bits = 0;
  for (const void* q : {(const void*)ax, (const void*)b, (const void*)normA, (const void*)y, (const void*)ytilde, (const void*)r}) bits |= reinterpret_cast<uintptr_t>(q);
  const LgCoef c{xunit, bscale, ics, sigma};
  if ((bits & 15) == 0) return launch_slot_partials<2>(((long long)m + 1) / 2, LgMultiplier<true>{ax, b, normA, y, ytilde, r, m, c}, partials, st);
  return launch_slot_partials<2>((long long)m, LgMultiplier<false>{ax, b, normA, y, ytilde, r, m, c}, partials, st);
}

int launch_lrg_block_terms(const double* C, const double* x, const double* M, const BlockTasksView& t, double* cpart, double* sums, hipStream_t st) {
  return launch_block_reduce(LgBlockTerms{{C, x, M}}, t, cpart, sums, st);
}

}  // namespace cuadmm
