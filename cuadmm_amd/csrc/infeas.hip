// Infeasibility detection from iterate differences (option "infeas_check"): the HBM-bound stream kernels and the decision rule.
// infeas.h has the contracts; DESIGN.md, "Infeasibility certificates", the mathematics.
//
// Both kernels walk a vector with a FIXED stride of kInfeasSlots * kInfeasThreads work items, one item = two doubles (one 16-byte
// access per stream) when every pointer is 16-byte aligned, else one double; an odd last element of an aligned vector is taken by
// the first thread.  A launch starts only the workgroups that have work; the others would contribute exact zeros, so the sums do not
// depend on how many were started: one partial per workgroup and scalar (wave_sum, then the four waves in order), then one
// wavefront per scalar adds the slots in a fixed order.  No atomics: bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

#include "infeas.h"
#include "device_util.h"
#include "wave_reduce.h"

namespace cuadmm {
namespace {

constexpr long long kStride = (long long)kInfeasSlots * kInfeasThreads;

__device__ __forceinline__ long long inf_tid() { return (long long)blockIdx.x * kInfeasThreads + threadIdx.x; }

struct RollArgs {
  const double *cur, *w;
  double *prev, *out;
  const long long *zoff, *zlen;
  int nz, negate, vec;
};

__device__ __forceinline__ double roll_out(const RollArgs& a, long long i, double d) {
  for (int r = 0; r < a.nz; ++r)
    if (i >= a.zoff[r] && i - a.zoff[r] < a.zlen[r]) return 0.0;
  return a.negate ? -d : d;
}

__global__ __launch_bounds__(kInfeasThreads) void infeas_roll_kernel(long long n, RollArgs a, double* partials) {
  __shared__ double lds[4];
  double s_dd = 0, s_wd = 0;
  const long long t = inf_tid();
  if (a.vec) {
    const long long np = n >> 1;
    for (long long p = t; p < np; p += kStride) {
      const double2 c = reinterpret_cast<const double2*>(a.cur)[p], q = reinterpret_cast<const double2*>(a.prev)[p];
      const double2 w = reinterpret_cast<const double2*>(a.w)[p];
      const double dx = c.x - q.x, dy = c.y - q.y;
      reinterpret_cast<double2*>(a.prev)[p] = c;
      reinterpret_cast<double2*>(a.out)[p] = make_double2(roll_out(a, 2 * p, dx), roll_out(a, 2 * p + 1, dy));
      s_dd += dx * dx; s_dd += dy * dy;
      s_wd += w.x * dx; s_wd += w.y * dy;
    }
  }
  const long long first = a.vec ? (n & ~1LL) : 0;       // aligned: only the odd last element is left, for thread 0
  for (long long i = first + t; i < n; i += kStride) {
    const double c = a.cur[i];
    const double d = c - a.prev[i];
    a.prev[i] = c;
    a.out[i] = roll_out(a, i, d);
    s_dd += d * d;
    s_wd += a.w[i] * d;
  }
  s_dd = block_sum(s_dd, lds);
  s_wd = block_sum(s_wd, lds);
  if (threadIdx.x == 0) { partials[2 * (size_t)blockIdx.x] = s_dd; partials[2 * (size_t)blockIdx.x + 1] = s_wd; }
}

__global__ __launch_bounds__(kInfeasThreads) void infeas_norm2_kernel(long long n, const double* v, int vec, double* partials) {
  __shared__ double lds[4];
  double s = 0;
  const long long t = inf_tid();
  if (vec) {
    const long long np = n >> 1;
    for (long long p = t; p < np; p += kStride) {
      const double2 x = reinterpret_cast<const double2*>(v)[p];
      s += x.x * x.x; s += x.y * x.y;
    }
  }
  const long long first = vec ? (n & ~1LL) : 0;
  for (long long i = first + t; i < n; i += kStride) s += v[i] * v[i];
  s = block_sum(s, lds);
  if (threadIdx.x == 0) partials[2 * (size_t)blockIdx.x] = s;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// workgroups with work: one item per thread, an item = 2 doubles on the 16-byte path
int grid_for(long long n, bool vec) {
  const long long items = vec ? std::max<long long>(n >> 1, n & 1) : n;
  const long long nb = (items + kInfeasThreads - 1) / kInfeasThreads;
  return (int)std::max<long long>(1, std::min<long long>(nb, kInfeasSlots));
}

}  // namespace

int launch_infeas_roll(long long n, const double* cur, double* prev, const double* w, double* out, int negate, int nz, const long long* zoff,
                       const long long* zlen, double* partials, double* sums2, hipStream_t st) {
  if (n < 0 || !cur || !prev || !w || !out || !partials || !sums2 || nz < 0 || (nz > 0 && (!zoff || !zlen))) {
    set_error("infeas_roll: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  RollArgs a{cur, w, prev, out, zoff, zlen, nz, negate ? 1 : 0, 0};
  a.vec = aligned16(cur) && aligned16(prev) && aligned16(w) && aligned16(out);
  const int nb = grid_for(n, a.vec != 0);
  hipLaunchKernelGGL(infeas_roll_kernel, dim3(nb), dim3(kInfeasThreads), 0, st, n, a, partials);
  hipLaunchKernelGGL(slots_final_kernel<2>, dim3(2), dim3(64), 0, st, partials, nb, sums2);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int launch_infeas_norm2(long long n, const double* v, double* partials, double* sum_out, hipStream_t st) {
  if (n < 0 || !v || !partials || !sum_out) { set_error("infeas_norm2: invalid argument"); return CUADMM_ERR_INVALID; }
  const int vec = aligned16(v);
  const int nb = grid_for(n, vec != 0);
  hipLaunchKernelGGL(infeas_norm2_kernel, dim3(nb), dim3(kInfeasThreads), 0, st, n, v, vec, partials);
  hipLaunchKernelGGL(slots_final_kernel<2>, dim3(1), dim3(64), 0, st, partials, nb, sum_out);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int infeas_decide(const double stats[INF_NSTATS], double tol, int* verdict, double out3[3]) {
  if (!stats || !verdict || !out3) { set_error("infeas_decide: null"); return CUADMM_ERR_INVALID; }
  *verdict = 0;
  out3[0] = out3[1] = out3[2] = 0;
  const double inf = std::numeric_limits<double>::infinity();
  // every comparison is written so that a NaN makes it false
  const double ny = std::sqrt(stats[INF_DY2]);
  if (ny > 0 && ny < inf && tol >= 0) {
    const double beta = stats[INF_BDY] / ny, eta = std::sqrt(stats[INF_PATY2]) / ny;
    if (beta > 0 && beta < inf && eta >= 0 && eta <= tol * beta) {
      *verdict = 3;
      out3[0] = beta; out3[1] = eta; out3[2] = eta > 0 ? beta / eta : inf;
      return CUADMM_OK;
    }
  }
  const double nx = std::sqrt(stats[INF_DX2]);
  if (nx > 0 && nx < inf && tol >= 0) {
    const double gamma = -stats[INF_CDX] / nx, e1 = std::sqrt(stats[INF_ADX2]) / nx, e2 = std::sqrt(stats[INF_PNEGDX2]) / nx;
    const double eta = e1 >= e2 ? e1 : e2;
    if (gamma > 0 && gamma < inf && e1 >= 0 && e2 >= 0 && eta <= tol * gamma) {
      *verdict = 4;
      out3[0] = gamma; out3[1] = eta; out3[2] = eta > 0 ? gamma / eta : inf;
    }
  }
  return CUADMM_OK;
}

}  // namespace cuadmm
