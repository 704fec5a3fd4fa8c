// KKT and DIMACS report of any point (cuadmm_evaluate): the per-block statistics and the reductions behind them.  evaluate.h has the
// contracts; DESIGN.md, "Evaluation of a point", the definitions.
//
// The per-block statistics are block_reduce.h's skeleton with five vectors and six sums: X, S, PX, PS and Rd1 are read once (40 B per
// slot); ||A X - b||^2 is its slot-partial kernel.
#include <hip/hip_runtime.h>

#include "evaluate.h"
#include "device_util.h"
#include "wave_reduce.h"

namespace cuadmm {
namespace {

struct EvBlockStats {
  static constexpr int V = 5, N = kEvSums;
  static constexpr bool kFlag = true;
  static constexpr const char* kName = "ev_block_stats";
  const double* p[V];      // X, S, PX, PS, Rd1
  // free_blk: an unconstrained block (no cone violation of x, all of s is one)
  __device__ __forceinline__ void add(double (&a)[N], const double (&v)[V], bool free_blk) const {
    const double x = v[0], s = v[1], px = v[2], ps = v[3], r1 = v[4];
    const double dx = free_blk ? 0.0 : px - x;
    const double ds = free_blk ? s : ps - s;
    const double rd = r1 + s;
    a[0] += x * x;
    a[1] += dx * dx;
    a[2] += s * s;
    a[3] += ds * ds;
    a[4] += x * s;
    a[5] += rd * rd;
  }
};

struct RpTerm {
  const double *ax, *b, *normA;
  double bscale;
  __device__ __forceinline__ void add(double& s, long long i) const {
    const double ro = normA[i] * (b[i] - ax[i]) * bscale;      // the stopping test's ||Rp|| in the caller's units (engine.hip, Step 5)
    s += ro * ro;
  }
};

__global__ __launch_bounds__(kBrThreads) void ev_combine_kernel(int nblk, const double* __restrict__ sums, const double* cx_part, const double* by_part,
                                                                const double* rp_part, double* out8) {
  __shared__ double lds[4];
  static_assert(kBrSlots == kBrThreads, "one partial per thread");
  double vx = 0, vs = 0, xs = 0, rd = 0;
  for (int k = threadIdx.x; k < nblk; k += kBrThreads) {
    const double* q = sums + kEvSums * (size_t)k;
    vx += q[1]; vs += q[3]; xs += q[4]; rd += q[5];
  }
  vx = block_sum(vx, lds); vs = block_sum(vs, lds); xs = block_sum(xs, lds); rd = block_sum(rd, lds);
  const double cx = block_sum(cx_part[threadIdx.x], lds), by = block_sum(by_part[threadIdx.x], lds), rp = block_sum(rp_part[threadIdx.x], lds);
  if (threadIdx.x == 0) {
    out8[0] = vx; out8[1] = vs; out8[2] = xs; out8[3] = rd; out8[4] = cx; out8[5] = by; out8[6] = rp; out8[7] = 0.0;
  }
}

}  // namespace

int launch_ev_block_stats(const double* X, const double* S, const double* PX, const double* PS, const double* Rd1, const BlockTasksView& t,
                          double* cpart, double* sums, hipStream_t st) {
  return launch_block_reduce(EvBlockStats{{X, S, PX, PS, Rd1}}, t, cpart, sums, st);
}

int launch_ev_rp(int m, const double* ax, const double* b, const double* normA, double bscale, double* partials, hipStream_t st) {
  if (m < 0 || (m > 0 && (!ax || !b || !normA)) || !partials) { set_error("ev_rp: invalid argument"); return CUADMM_ERR_INVALID; }
  return launch_slot_partials(m, RpTerm{ax, b, normA, bscale}, partials, st);
}

int launch_ev_combine(int nblk, const double* sums, const double* cx_part, const double* by_part, const double* rp_part, double* out8, hipStream_t st) {
  if (nblk < 0 || (nblk > 0 && !sums) || !cx_part || !by_part || !rp_part || !out8) { set_error("ev_combine: invalid argument"); return CUADMM_ERR_INVALID; }
  hipLaunchKernelGGL(ev_combine_kernel, dim3(1), dim3(kBrThreads), 0, st, nblk, sums, cx_part, by_part, rp_part, out8);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

}  // namespace cuadmm
