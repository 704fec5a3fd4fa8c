// cuadmm_quartic_min: the global minimiser of c0 + c1 t + c2 t^2 + c3 t^3 + c4 t^4 on [0, t_max] (include/cuadmm_amd.h; lowrank_line.h).
// Host only: no device, no solver handle.
//
// The derivative d(t) = c1 + 2 c2 t + 3 c3 t^2 + 4 c4 t^3 is monotone between its own stationary points, the roots of
// 2 c2 + 6 c3 t + 12 c4 t^2, which have a closed form (the stable quadratic formula; a linear or constant d' where leading coefficients
// vanish).  They cut [0, T] into at most three brackets; a bracket whose ends give d opposite signs holds exactly one root, refined by
// Newton steps that fall back to bisection whenever a step leaves the bracket.  T = t_max, or, for t_max = +inf, Cauchy's bound on the
// roots of d (every stationary point of the quartic lies below it, and the quartic grows beyond the last one).
// The candidates 0, the interior roots and a finite t_max are evaluated by Horner in ascending order; a later one wins only where it is
// strictly smaller, so ties go to the smallest t.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "cuadmm_amd.h"

namespace {

inline double horner(const double c[5], double t) { return (((c[4] * t + c[3]) * t + c[2]) * t + c[1]) * t + c[0]; }

}  // namespace

extern "C" int cuadmm_quartic_min(const double c[5], double t_max, double out4[4]) {
  using cuadmm::set_error;
  if (!c || !out4) { set_error("quartic_min: null argument"); return CUADMM_ERR_INVALID; }
  for (int i = 0; i < 5; ++i)
    if (!std::isfinite(c[i])) { set_error("quartic_min: c[%d] is not finite", i); return CUADMM_ERR_INVALID; }
  if (!(t_max >= 0.0)) { set_error("quartic_min: t_max = %g, allowed is t_max >= 0 (+inf included)", t_max); return CUADMM_ERR_INVALID; }
  const double d[4] = {c[1], 2 * c[2], 3 * c[3], 4 * c[4]};
  double T = t_max;
  if (std::isinf(t_max)) {
    if (c[4] > 0) T = 1 + std::max({std::fabs(d[0]), std::fabs(d[1]), std::fabs(d[2])}) / d[3];
    else if (c[4] == 0 && c[3] == 0 && c[2] > 0) T = 1 + std::fabs(d[0]) / d[1];
    else { set_error("quartic_min: unbounded below on [0, inf): c4 = %g, c3 = %g, c2 = %g", c[4], c[3], c[2]); return CUADMM_ERR_INVALID; }
    if (!std::isfinite(T)) { set_error("quartic_min: the bound on the stationary points overflows"); return CUADMM_ERR_INVALID; }
  }
  auto dv = [&](double t) { return ((d[3] * t + d[2]) * t + d[1]) * t + d[0]; };
  auto ddv = [&](double t) { return (3 * d[3] * t + 2 * d[2]) * t + d[1]; };
  // the stationary points of d inside (0, T), ascending
  double cut[4];
  int ncut = 0;
  cut[ncut++] = 0.0;
  {
    const double qa = 3 * d[3], qb = 2 * d[2], qc = d[1];
    double s[2];
    int ns = 0;
    if (qa == 0) {
      if (qb != 0) s[ns++] = -qc / qb;
    } else {
      const double disc = qb * qb - 4 * qa * qc;
      if (disc >= 0) {
        const double w = -0.5 * (qb + std::copysign(std::sqrt(disc), qb));
        s[ns++] = w / qa;
        if (w != 0) s[ns++] = qc / w;
      }
    }
    if (ns == 2 && s[0] > s[1]) std::swap(s[0], s[1]);
    for (int i = 0; i < ns; ++i)
      if (s[i] > cut[ncut - 1] && s[i] < T) cut[ncut++] = s[i];
  }
  if (T > cut[ncut - 1]) cut[ncut++] = T;
  double root[3];
  int nroot = 0;
  for (int i = 0; i + 1 < ncut; ++i) {
    double lo = cut[i], hi = cut[i + 1], flo = dv(lo), fhi = dv(hi);
    if (flo == 0 || fhi == 0 || (flo < 0) == (fhi < 0)) {      // a root at an end is the neighbour's, or a candidate below
      if (flo == 0 && lo > 0 && lo < T && (nroot == 0 || root[nroot - 1] < lo)) root[nroot++] = lo;
      continue;
    }
    double t = 0.5 * (lo + hi);
    for (int it = 0; it < 200 && lo < hi; ++it) {
      const double ft = dv(t);
      if (ft == 0) break;
      if ((ft < 0) == (flo < 0)) lo = t; else hi = t;
      const double g = ddv(t);
      double tn = g != 0 ? t - ft / g : 0.5 * (lo + hi);
      if (!(tn > lo && tn < hi)) tn = 0.5 * (lo + hi);
      if (tn == t || !(tn > lo && tn < hi)) break;      // the bracket holds no double between its ends
      t = tn;
    }
    if (t > 0 && t < T && (nroot == 0 || root[nroot - 1] < t)) root[nroot++] = t;
  }
  double best_t = 0.0, best_f = horner(c, 0.0);
  for (int i = 0; i < nroot; ++i) {
    const double f = horner(c, root[i]);
    if (f < best_f) { best_f = f; best_t = root[i]; }
  }
  if (std::isfinite(t_max) && t_max > 0) {
    const double f = horner(c, t_max);
    if (f < best_f) { best_f = f; best_t = t_max; }
  }
  out4[0] = best_t; out4[1] = best_f; out4[2] = best_f - c[0]; out4[3] = (double)nroot;
  return CUADMM_OK;
}
