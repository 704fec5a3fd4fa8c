// cuadmm_cg_update: the scalar step of Polak-Ribiere+ nonlinear conjugate gradients between a gradient and a direction
// (include/cuadmm_amd.h; lowrank_refine.h).  Host only: no device, no solver handle.  Plain doubles, every operation rounded once.
#include <cmath>

#include "common.h"
#include "cuadmm_amd.h"

extern "C" int cuadmm_cg_update(double gg, double go, double gd, double gg_prev, int first, double out3[3]) {
  using cuadmm::set_error;
  if (!out3) { set_error("cg_update: null argument"); return CUADMM_ERR_INVALID; }
  const double in[4] = {gg, go, gd, gg_prev};
  static const char* const name[4] = {"gg", "go", "gd", "gg_prev"};
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(in[i])) { set_error("cg_update: %s is not finite", name[i]); return CUADMM_ERR_INVALID; }
  double beta = 0.0;
  if (!first && gg_prev != 0.0) {
    const double num = gg - go;
    const double pr = num / gg_prev;
    beta = pr > 0.0 ? pr : 0.0;            // max(0, .): a NaN gives 0
  }
  const double bd = beta * gd;
  const double slope = bd - gg;
  const bool restart = first || !(slope < 0.0);
  out3[0] = restart ? 0.0 : beta;
  out3[1] = slope;
  out3[2] = restart ? 1.0 : 0.0;
  return CUADMM_OK;
}
