// Safeguarded Anderson acceleration of the iteration (option "accel"): three HBM-bound stream kernels and the host solve of the
// small least-squares system.  accel.h has the contracts; DESIGN.md, "Acceleration", the algorithm.
//
// All three kernels walk the two halves of a state vector (X part, S part) with a FIXED stride of kAccelSlots * kAccelThreads work
// items, one item = two doubles (one 16-byte access per stream) when every pointer of that half is 16-byte aligned, else one double.
// An odd last element of an aligned half is taken by the first thread.  A launch starts only the workgroups that have work; the
// others would contribute exact zeros, so the reductions do not depend on how many were started: slot partials per workgroup
// (wave_sum, then the four waves in order), then one wavefront per dot product adds the slots in a fixed order.  No atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "accel.h"
#include "device_util.h"
#include "wave_reduce.h"

namespace cuadmm {
namespace {

constexpr long long kStride = (long long)kAccelSlots * kAccelThreads;
constexpr int kQ = 2 * kAccelMaxMem;     // partial sums per slot

__device__ __forceinline__ long long aa_tid() { return (long long)blockIdx.x * kAccelThreads + threadIdx.x; }

// ---- push ------------------------------------------------------------------------------------------------------------------
struct PushHalf {
  const double *u, *x, *fp, *gp;
  double *g, *f, *dF, *dG;
  double sc;
  int vec;
};

__device__ __forceinline__ double push_elem(double x, double u, double fp, double gp, double sc, double& dF, double& dG) {
  const double g = sc * (x - u);
  dF = sc * (x - fp);
  dG = g - gp;
  return g;
}

__device__ __forceinline__ double push_half(const PushHalf& h, long long n, int have_prev) {
  double acc = 0;
  const long long t = aa_tid();
  if (h.vec) {
    const long long np = n >> 1;
    for (long long p = t; p < np; p += kStride) {
      const double2 x = reinterpret_cast<const double2*>(h.x)[p], u = reinterpret_cast<const double2*>(h.u)[p];
      double2 fp = x, gp = make_double2(0, 0);
      if (have_prev) { fp = reinterpret_cast<const double2*>(h.fp)[p]; gp = reinterpret_cast<const double2*>(h.gp)[p]; }
      double2 g, dF, dG;
      g.x = push_elem(x.x, u.x, fp.x, gp.x, h.sc, dF.x, dG.x);
      g.y = push_elem(x.y, u.y, fp.y, gp.y, h.sc, dF.y, dG.y);
      reinterpret_cast<double2*>(h.g)[p] = g;
      reinterpret_cast<double2*>(h.f)[p] = x;
      if (have_prev) { reinterpret_cast<double2*>(h.dF)[p] = dF; reinterpret_cast<double2*>(h.dG)[p] = dG; }
      acc += g.x * g.x;
      acc += g.y * g.y;
    }
  }
  const long long first = h.vec ? (n & ~1LL) : 0;       // aligned half: only the odd last element is left, for thread 0
  for (long long i = first + t; i < n; i += kStride) {
    const double x = h.x[i], u = h.u[i];
    const double fp = have_prev ? h.fp[i] : x, gp = have_prev ? h.gp[i] : 0.0;
    double dF, dG;
    const double g = push_elem(x, u, fp, gp, h.sc, dF, dG);
    h.g[i] = g;
    h.f[i] = x;
    if (have_prev) { h.dF[i] = dF; h.dG[i] = dG; }
    acc += g * g;
  }
  return acc;
}

__global__ __launch_bounds__(kAccelThreads) void aa_push_kernel(long long L, PushHalf hx, PushHalf hs, int have_prev, double* partials) {
  __shared__ double lds[4];
  double acc = push_half(hx, L, have_prev);
  acc += push_half(hs, L, have_prev);
  acc = block_sum(acc, lds);
  if (threadIdx.x == 0) partials[(size_t)blockIdx.x * kQ] = acc;
}

// ---- gram ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kAccelThreads) void aa_gram_kernel(long long L, long long hs, long long col_stride, int cols, int newest, const double* ring,
                                                                 const double* g, int vec_x, int vec_s, double* partials) {
  __shared__ double lds[4];
  double an[kAccelMaxMem], ag[kAccelMaxMem];
#pragma unroll
  for (int j = 0; j < kAccelMaxMem; ++j) { an[j] = 0; ag[j] = 0; }
  const long long t = aa_tid();
  for (int half = 0; half < 2; ++half) {
    const long long off = half ? hs : 0;
    const int vec = half ? vec_s : vec_x;
    const double* gh = g + off;
    const double* nh = ring + (long long)newest * col_stride + off;
    const double* ch = ring + off;
    if (vec) {
      const long long np = L >> 1;
      for (long long p = t; p < np; p += kStride) {
        const double2 gv = reinterpret_cast<const double2*>(gh)[p], nv = reinterpret_cast<const double2*>(nh)[p];
#pragma unroll
        for (int j = 0; j < kAccelMaxMem; ++j)
          if (j < cols) {
            const double2 c = j == newest ? nv : reinterpret_cast<const double2*>(ch + (long long)j * col_stride)[p];
            an[j] += nv.x * c.x; an[j] += nv.y * c.y;
            ag[j] += c.x * gv.x; ag[j] += c.y * gv.y;
          }
      }
    }
    const long long first = vec ? (L & ~1LL) : 0;
    for (long long i = first + t; i < L; i += kStride) {
      const double gv = gh[i], nv = nh[i];
#pragma unroll
      for (int j = 0; j < kAccelMaxMem; ++j)
        if (j < cols) {
          const double c = j == newest ? nv : ch[(long long)j * col_stride + i];
          an[j] += nv * c;
          ag[j] += c * gv;
        }
    }
  }
#pragma unroll
  for (int j = 0; j < kAccelMaxMem; ++j)
    if (j < cols) {
      const double a = block_sum(an[j], lds), b = block_sum(ag[j], lds);
      if (threadIdx.x == 0) { partials[(size_t)blockIdx.x * kQ + j] = a; partials[(size_t)blockIdx.x * kQ + cols + j] = b; }
    }
}

// ---- combine ---------------------------------------------------------------------------------------------------------------
struct Gamma { double v[kAccelMaxMem]; };

// hi + lo = sum_j gamma_j d_j to about twice the working precision (two-product by fma, two-sum), then the result in one rounding
struct DD { double hi, lo; };
__device__ __forceinline__ void dd_add_prod(DD& a, double x, double y) {
#pragma clang fp contract(off)
  const double p = x * y;
  const double e = __builtin_fma(x, y, -p);
  const double s = a.hi + p;
  const double bb = s - a.hi;
  const double err = (a.hi - (s - bb)) + (p - bb);
  a.hi = s;
  a.lo += err + e;
}
// sc * x - (a.hi + a.lo), rounded once (sc * x exact as a two-product)
__device__ __forceinline__ double dd_finish(double sc, double x, const DD& a) {
#pragma clang fp contract(off)
  const double p = sc * x;
  const double e = __builtin_fma(sc, x, -p);
  const double q = -a.hi;
  const double s = p + q;
  const double bb = s - p;
  const double err = (p - (s - bb)) + (q - bb);
  return s + ((err + e) - a.lo);
}

__global__ __launch_bounds__(kAccelThreads) void aa_combine_kernel(long long L, long long hs, long long col_stride, int cols, const double* ring, Gamma gm,
                                                                    double sig, double* X, double* S, double* u_out, int vec_x, int vec_s) {
  const long long t = aa_tid();
  for (int half = 0; half < 2; ++half) {
    const long long off = half ? hs : 0;
    const int vec = half ? vec_s : vec_x;
    double* xs = half ? S : X;
    const double sc = half ? sig : 1.0;
    const double* ch = ring + off;
    double* uo = u_out ? u_out + off : nullptr;
    if (vec) {
      const long long np = L >> 1;
      for (long long p = t; p < np; p += kStride) {
        const double2 x = reinterpret_cast<const double2*>(xs)[p];
        DD a{0, 0}, b{0, 0};
#pragma unroll
        for (int j = 0; j < kAccelMaxMem; ++j)
          if (j < cols) {
            const double2 c = reinterpret_cast<const double2*>(ch + (long long)j * col_stride)[p];
            dd_add_prod(a, gm.v[j], c.x);
            dd_add_prod(b, gm.v[j], c.y);
          }
        double2 r;
        r.x = dd_finish(sc, x.x, a);
        r.y = dd_finish(sc, x.y, b);
        if (half) { r.x = r.x / sig; r.y = r.y / sig; }
        reinterpret_cast<double2*>(xs)[p] = r;
        if (uo) reinterpret_cast<double2*>(uo)[p] = r;
      }
    }
    const long long first = vec ? (L & ~1LL) : 0;
    for (long long i = first + t; i < L; i += kStride) {
      const double x = xs[i];
      DD a{0, 0};
#pragma unroll
      for (int j = 0; j < kAccelMaxMem; ++j)
        if (j < cols) dd_add_prod(a, gm.v[j], ch[(long long)j * col_stride + i]);
      double r = dd_finish(sc, x, a);
      if (half) r = r / sig;
      xs[i] = r;
      if (uo) uo[i] = r;
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int grid_for(long long L) {
  const long long nb = (L + kAccelThreads - 1) / kAccelThreads;
  return (int)std::max<long long>(1, std::min<long long>(nb, kAccelSlots));
}

}  // namespace

int launch_aa_push(long long L, long long hs, const double* u, const double* X, const double* S, double sig, const double* f_prev, const double* g_prev,
                   int have_prev, double* g_out, double* f_out, double* dF_out, double* dG_out, double* partials, double* gnorm2_out, hipStream_t st) {
  if (L < 0 || hs < L || !u || !X || !S || !g_out || !f_out || !partials || !gnorm2_out || (have_prev && (!f_prev || !g_prev || !dF_out || !dG_out))) {
    set_error("aa_push: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  PushHalf hx{u, X, f_prev, g_prev, g_out, f_out, dF_out, dG_out, 1.0, 0};
  PushHalf hh{u + hs, S, have_prev ? f_prev + hs : nullptr, have_prev ? g_prev + hs : nullptr, g_out + hs, f_out + hs, have_prev ? dF_out + hs : nullptr,
              have_prev ? dG_out + hs : nullptr, sig, 0};
  for (PushHalf* h : {&hx, &hh})
    h->vec = aligned16(h->u) && aligned16(h->x) && aligned16(h->g) && aligned16(h->f) &&
             (!have_prev || (aligned16(h->fp) && aligned16(h->gp) && aligned16(h->dF) && aligned16(h->dG)));
  const int nb = grid_for(L);
  hipLaunchKernelGGL(aa_push_kernel, dim3(nb), dim3(kAccelThreads), 0, st, L, hx, hh, have_prev, partials);
  hipLaunchKernelGGL(slots_final_kernel<kQ>, dim3(1), dim3(64), 0, st, partials, nb, gnorm2_out);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int launch_aa_gram(long long L, long long hs, long long col_stride, int cols, int newest, const double* ring_dG, const double* g, double* partials,
                   double* dots, hipStream_t st) {
  if (L < 0 || hs < L || col_stride < hs + L || cols < 1 || cols > kAccelMaxMem || newest < 0 || newest >= cols || !ring_dG || !g || !partials || !dots) {
    set_error("aa_gram: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  const bool stride_ok = (col_stride & 1) == 0;
  const int vec_x = stride_ok && aligned16(ring_dG) && aligned16(g);
  const int vec_s = stride_ok && aligned16(ring_dG + hs) && aligned16(g + hs);
  const int nb = grid_for(L);
  hipLaunchKernelGGL(aa_gram_kernel, dim3(nb), dim3(kAccelThreads), 0, st, L, hs, col_stride, cols, newest, ring_dG, g, vec_x, vec_s, partials);
  hipLaunchKernelGGL(slots_final_kernel<kQ>, dim3(2 * cols), dim3(64), 0, st, partials, nb, dots);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int launch_aa_combine(long long L, long long hs, long long col_stride, int cols, const double* ring_dF, const double* gamma, double sig, double* X,
                      double* S, double* u_out, hipStream_t st) {
  if (L < 0 || hs < L || col_stride < hs + L || cols < 1 || cols > kAccelMaxMem || !ring_dF || !gamma || !X || !S || !(sig > 0)) {
    set_error("aa_combine: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  Gamma gm{};
  for (int j = 0; j < cols; ++j) gm.v[j] = gamma[j];
  const bool stride_ok = (col_stride & 1) == 0;
  const int vec_x = stride_ok && aligned16(ring_dF) && aligned16(X) && (!u_out || aligned16(u_out));
  const int vec_s = stride_ok && aligned16(ring_dF + hs) && aligned16(S) && (!u_out || aligned16(u_out + hs));
  hipLaunchKernelGGL(aa_combine_kernel, dim3(grid_for(L)), dim3(kAccelThreads), 0, st, L, hs, col_stride, cols, ring_dF, gm, sig, X, S, u_out, vec_x, vec_s);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int accel_solve_ls(const double* gram, const double* rhs, int cols, double reg, double* gamma_out) {
  if (!gram || !rhs || !gamma_out || cols < 1 || cols > kAccelMaxMem) { set_error("accel_solve_ls: invalid argument"); return CUADMM_ERR_INVALID; }
  long double M[kAccelMaxMem][kAccelMaxMem], z[kAccelMaxMem];
  long double tr = 0;
  for (int i = 0; i < cols; ++i) tr += (long double)gram[i * cols + i];
  const long double shift = (long double)reg * tr / cols;
  for (int i = 0; i < cols; ++i)
    for (int j = 0; j < cols; ++j) M[i][j] = (long double)gram[i * cols + j] + (i == j ? shift : 0.0L);
  // M = R^T R, row by row of the lower triangle (stored in M's lower part)
  for (int j = 0; j < cols; ++j) {
    long double d = M[j][j];
    for (int k = 0; k < j; ++k) d -= M[j][k] * M[j][k];
    if (!(d > 0) || !std::isfinite((double)d)) { set_error("accel_solve_ls: pivot %d of the regularised Gram matrix is not positive", j); return CUADMM_ERR_FACTOR; }
    const long double r = sqrtl(d);
    M[j][j] = r;
    for (int i = j + 1; i < cols; ++i) {
      long double v = M[i][j];
      for (int k = 0; k < j; ++k) v -= M[i][k] * M[j][k];
      M[i][j] = v / r;
    }
  }
  for (int i = 0; i < cols; ++i) {
    long double v = rhs[i];
    for (int k = 0; k < i; ++k) v -= M[i][k] * z[k];
    z[i] = v / M[i][i];
  }
  for (int i = cols - 1; i >= 0; --i) {
    long double v = z[i];
    for (int k = i + 1; k < cols; ++k) v -= M[k][i] * z[k];
    z[i] = v / M[i][i];
  }
  for (int i = 0; i < cols; ++i) {
    gamma_out[i] = (double)z[i];
    if (!std::isfinite(gamma_out[i])) { set_error("accel_solve_ls: solution is not finite"); return CUADMM_ERR_FACTOR; }
  }
  return CUADMM_OK;
}

}  // namespace cuadmm
