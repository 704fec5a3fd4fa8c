// Infeasibility detection from iterate differences (option "infeas_check"): launchers of the stream kernels (infeas.hip) and the
// decision on host numbers.  DESIGN.md, "Infeasibility certificates".
#pragma once
#include <hip/hip_runtime.h>

namespace cuadmm {

constexpr int kInfeasSlots = 1024;    // workgroups of the reductions = partial sums per scalar (fixed: the sums do not depend on the device)
constexpr int kInfeasThreads = 256;
constexpr size_t kInfeasPartials = (size_t)kInfeasSlots * 2;   // doubles of scratch the reductions need

// statistics of one check, as infeas_decide reads them (a test that was not evaluated leaves NaN in its projection entries)
enum { INF_DY2 = 0, INF_BDY = 1, INF_DX2 = 2, INF_CDX = 3, INF_PATY2 = 4, INF_ADX2 = 5, INF_PNEGDX2 = 6, INF_ATY2 = 7 /* ||A'dy||^2: not read by the rule */, INF_NSTATS = 8 };
constexpr double kInfeasProjErr = 1e-12;   // per-entry accuracy of the projection kernels relative to ||input||_F (their contract)

// One pass over n elements: d = cur - prev, prev <- cur, out <- d (negate: -d; elements inside one of the nz ranges
// [zoff[r], zoff[r] + zlen[r]): 0), sums2[0] = ||d||^2, sums2[1] = <w, d> (both of the plain d, over all n).  zoff / zlen: device
// arrays (nz = 0: none).  Two doubles per access when cur, prev, w and out are 16-byte aligned, else one.
int launch_infeas_roll(long long n, const double* cur, double* prev, const double* w, double* out, int negate, int nz, const long long* zoff,
                       const long long* zlen, double* partials, double* sums2, hipStream_t st);

// sum_out[0] = ||v||^2 on the device (no host wait), the same slot sums
int launch_infeas_norm2(long long n, const double* v, double* partials, double* sum_out, hipStream_t st);

// The rule on the statistics of a check: verdict 3 (primal infeasible) when beta = b'dy / ||dy|| > 0 and
// eta = ||P+(A'dy)|| / ||dy|| <= tol beta; else 4 (dual infeasible) when gamma = -C'dx / ||dx|| > 0 and
// max(||A dx||, ||P+(-dx)||) / ||dx|| <= tol gamma; else 0.  out3: [beta or gamma, eta, beta / eta or gamma / eta] of the verdict
// (scaled space; eta = 0 gives an infinite radius).  NaN anywhere in a test's numbers: no verdict from that test.  Host only.
int infeas_decide(const double stats[INF_NSTATS], double tol, int* verdict, double out3[3]);

}  // namespace cuadmm
