// The three streaming kernels of cuadmm_lowrank_refine: lowrank_refine.h has the formulas and the contracts; DESIGN.md, "Refinement over
// factors", the step they stand in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "lowrank_refine.h"
#include "device_util.h"
#include "wave_reduce.h"

namespace cuadmm {
namespace {

constexpr int kRfThreads = 256;
constexpr int kRfGrid = 2048;            // workgroups of a streaming launch at most (grid-stride beyond)

// One rounding per operation.  This file is compiled with contraction on, and the toolchain's __dmul_rn / __dadd_rn / __dsub_rn are
// plain operators inside the header, which that contraction fuses into v_fma_f64 (seen in this file's assembly); operators written
// under the pragma below are not fused.
#pragma clang fp contract(off)
__device__ __forceinline__ double rf_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double rf_add(double a, double b) { return a + b; }
__device__ __forceinline__ double rf_sub(double a, double b) { return a - b; }

__device__ __forceinline__ double rf_grad(double w, double unit) { return rf_mul(2.0, rf_mul(w, unit)); }

__device__ __forceinline__ void rf_dot_one(double unit, double w, double go, double d, double (&s)[kRfParts]) {
  const double g = rf_grad(w, unit);
  s[0] = rf_add(s[0], rf_mul(g, g));
  s[1] = rf_add(s[1], rf_mul(g, go));
  s[2] = rf_add(s[2], rf_mul(g, d));
}

// index i: entry i (kVec = false) or the entries 2 i, 2 i + 1 (kVec = true; the last index may hold one)
template <bool kVec>
struct RfDots {
  const double *W, *Gold, *Dold;
  long long n;
  double unit;
  __device__ __forceinline__ void add(double (&s)[kRfParts], long long i) const {
    if (kVec && 2 * i + 1 < n) {
      const double2 w = reinterpret_cast<const double2*>(W)[i], g = reinterpret_cast<const double2*>(Gold)[i], d = reinterpret_cast<const double2*>(Dold)[i];
      rf_dot_one(unit, w.x, g.x, d.x, s);
      rf_dot_one(unit, w.y, g.y, d.y, s);
      return;
    }
    const long long e = kVec ? 2 * i : i;      // (kVec: the odd last entry; e < n by the launcher's count)
    rf_dot_one(unit, W[e], Gold[e], Dold[e], s);
  }
};

__device__ __forceinline__ void rf_dir_one(double unit, double beta, bool restart, double root, double w, double dold, double& d, double& ds, double& g) {
  g = rf_grad(w, unit);
  d = restart ? -g : rf_sub(rf_mul(beta, dold), g);
  ds = rf_mul(d, root);
}

template <bool kVec>
__global__ __launch_bounds__(kRfThreads) void lrr_direction_kernel(long long n, const double* __restrict__ W, double unit, double beta, int restart, double root,
                                                                   double* __restrict__ D, double* __restrict__ Ds, double* __restrict__ Gold) {
  const long long work = kVec ? (n + 1) / 2 : n, stride = (long long)gridDim.x * kRfThreads;
  const bool rs = restart != 0;
  for (long long i = (long long)blockIdx.x * kRfThreads + threadIdx.x; i < work; i += stride) {
    if (kVec && 2 * i + 1 < n) {
      const double2 w = reinterpret_cast<const double2*>(W)[i];
      double2 dold = double2{0.0, 0.0}, d, ds, g;
      if (!rs) dold = reinterpret_cast<const double2*>(D)[i];
      rf_dir_one(unit, beta, rs, root, w.x, dold.x, d.x, ds.x, g.x);
      rf_dir_one(unit, beta, rs, root, w.y, dold.y, d.y, ds.y, g.y);
      reinterpret_cast<double2*>(D)[i] = d;
      reinterpret_cast<double2*>(Ds)[i] = ds;
      reinterpret_cast<double2*>(Gold)[i] = g;
      continue;
    }
    const long long e = kVec ? 2 * i : i;      // e < n: i < work
    double d, ds, g;
    rf_dir_one(unit, beta, rs, root, W[e], rs ? 0.0 : D[e], d, ds, g);
    D[e] = d;
    Ds[e] = ds;
    Gold[e] = g;
  }
}

__device__ __forceinline__ void rf_step_one(double t, double root, double d, double& l, double& ls) {
  l = rf_add(l, rf_mul(t, d));
  ls = rf_mul(l, root);
}

template <bool kVec>
__global__ __launch_bounds__(kRfThreads) void lrr_step_kernel(long long n, double t, double root, const double* __restrict__ D, double* __restrict__ L,
                                                              double* __restrict__ Ls) {
  const long long work = kVec ? (n + 1) / 2 : n, stride = (long long)gridDim.x * kRfThreads;
  for (long long i = (long long)blockIdx.x * kRfThreads + threadIdx.x; i < work; i += stride) {
    if (kVec && 2 * i + 1 < n) {
      const double2 d = reinterpret_cast<const double2*>(D)[i];
      double2 l = reinterpret_cast<const double2*>(L)[i], ls;
      rf_step_one(t, root, d.x, l.x, ls.x);
      rf_step_one(t, root, d.y, l.y, ls.y);
      reinterpret_cast<double2*>(L)[i] = l;
      reinterpret_cast<double2*>(Ls)[i] = ls;
      continue;
    }
    const long long e = kVec ? 2 * i : i;      // e < n: i < work
    double l = L[e], ls;
    rf_step_one(t, root, D[e], l, ls);
    L[e] = l;
    Ls[e] = ls;
  }
}

inline bool rf_aligned(std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* q : ptrs) bits |= reinterpret_cast<uintptr_t>(q);
  return (bits & 15) == 0;
}
inline unsigned rf_grid(long long work) { return (unsigned)std::min<long long>((work + kRfThreads - 1) / kRfThreads, kRfGrid); }

}  // namespace

int launch_lrr_dots(long long n, const double* W, double unit, const double* G_old, const double* D_old, double* partials, hipStream_t st) {
  if (n < 0 || (n > 0 && (!W || !G_old || !D_old)) || !partials) { set_error("lrr_dots: invalid argument"); return CUADMM_ERR_INVALID; }
  if (rf_aligned({W, G_old, D_old})) return launch_slot_partials<kRfParts>((n + 1) / 2, RfDots<true>{W, G_old, D_old, n, unit}, partials, st);
  return launch_slot_partials<kRfParts>(n, RfDots<false>{W, G_old, D_old, n, unit}, partials, st);
}

int launch_lrr_direction(long long n, const double* W, double unit, double beta, int restart, double root, double* D, double* Ds, double* G_old, hipStream_t st) {
  if (n < 0 || (n > 0 && (!W || !D || !Ds || !G_old)) || (D && (D == Ds || D == G_old || D == W)) || (Ds && (Ds == G_old || Ds == W)) || (G_old && G_old == W)) {
    set_error("lrr_direction: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  if (n == 0) return CUADMM_OK;
  if (rf_aligned({W, D, Ds, G_old}))
    hipLaunchKernelGGL(lrr_direction_kernel<true>, dim3(rf_grid((n + 1) / 2)), dim3(kRfThreads), 0, st, n, W, unit, beta, restart, root, D, Ds, G_old);
  else
    hipLaunchKernelGGL(lrr_direction_kernel<false>, dim3(rf_grid(n)), dim3(kRfThreads), 0, st, n, W, unit, beta, restart, root, D, Ds, G_old);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int launch_lrr_step(long long n, double t, double root, const double* D, double* L, double* Ls, hipStream_t st) {
  if (n < 0 || (n > 0 && (!D || !L || !Ls)) || (L && (L == Ls || L == D)) || (Ls && Ls == D)) { set_error("lrr_step: invalid argument"); return CUADMM_ERR_INVALID; }
  if (n == 0) return CUADMM_OK;
  if (rf_aligned({D, L, Ls}))
    hipLaunchKernelGGL(lrr_step_kernel<true>, dim3(rf_grid((n + 1) / 2)), dim3(kRfThreads), 0, st, n, t, root, D, L, Ls);
  else
    hipLaunchKernelGGL(lrr_step_kernel<false>, dim3(rf_grid(n)), dim3(kRfThreads), 0, st, n, t, root, D, L, Ls);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

}  // namespace cuadmm
