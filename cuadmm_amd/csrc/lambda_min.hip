// Certified per-block lower bounds on lambda_min: one workgroup per block unpacks the svec block, brackets -lambda_min between a
// floor and a Gershgorin bound and bisects on the shift mu with Cholesky trials of M + mu I.  lambda_min.h has the contracts, DESIGN.md,
// "Certified lambda_min", the bound.
//
// The trial is plain fp64 VALU arithmetic (fma, IEEE division and square root): the bound is a theorem about those operations, in any
// order of summation, and must not rest on the rounding of a matrix instruction's accumulate steps.
// Every loop is bounded by n and by the step count; nothing waits on memory.
#include <hip/hip_runtime.h>

#include <cmath>

#include "lambda_min.h"
#include "device_util.h"

namespace cuadmm {
namespace {

constexpr double kLmInvSqrt2 = 0.7071067811865476;      // off-diagonal svec entries carry sqrt(2)

// f over a workgroup of NT threads, the same bits in every thread (f commutative: the xor butterfly gives every lane one value)
template <int NT, class F>
__device__ __forceinline__ double lm_reduce(double v, double* red, F f) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = f(v, __shfl_xor(v, o, 64));
  if (NT == 64) return v;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) r = f(r, red[w]);
  return r;
}

// Right-looking Cholesky of M + mu I on the packed lower triangle S (entry (i, j), j <= i, at i (i + 1) / 2 + j: the svec order), M read
// from the svec block x as sign * x.  false at the first pivot that is not positive and finite.  Every thread returns the same: the pivot
// is one word read behind a barrier.
template <int NT>
__device__ bool lm_trial(const double* __restrict__ x, double sign, int n, double mu, double* S) {
  constexpr int TX = NT == 64 ? 8 : 16, TY = NT / TX;
  const int tid = (int)threadIdx.x, tx = tid % TX, ty = tid / TX;
  const int len = n * (n + 1) / 2;
  __syncthreads();                 // every thread has read the pivot the last trial ended at
  for (int e = tid; e < len; e += NT) S[e] = (sign * x[e]) * kLmInvSqrt2;
  __syncthreads();
  for (int i = tid; i < n; i += NT) S[i * (i + 3) / 2] = sign * x[i * (i + 3) / 2] + mu;
  __syncthreads();
  for (int k = 0; k < n; ++k) {
    const double p = S[k * (k + 3) / 2];
    if (!(p > 0.0) || !(p < INFINITY)) return false;
    if (k == n - 1) break;
    const double r = sqrt(p);
    for (int i = k + 1 + tid; i < n; i += NT) {
      const int q = i * (i + 1) / 2 + k;
      S[q] = S[q] / r;
    }
    __syncthreads();
    for (int i = k + 1 + ty; i < n; i += TY) {
      const int ri = i * (i + 1) / 2;
      const double lik = S[ri + k];
      for (int j = k + 1 + tx; j <= i; j += TX) S[ri + j] = fma(-lik, S[j * (j + 1) / 2 + k], S[ri + j]);
    }
    __syncthreads();
  }
  return true;
}

template <int NT, bool LDS>
__global__ __launch_bounds__(NT) void lambda_min_kernel(const int* __restrict__ list, const double* __restrict__ v, double sign, const long long* __restrict__ off,
                                                        const int* __restrict__ blk, int steps, int cap, double* work, const long long* __restrict__ work_off, double* out) {
  extern __shared__ double lm_sm[];
  __shared__ double red[4];
  const int tid = (int)threadIdx.x;
  const int k = list[blockIdx.x];
  const int b = blk[k];
  const double* x = v + off[k];
  double* o = out + kLmOut * (size_t)k;
  auto add = [](double a, double c) { return a + c; };
  auto mn = [](double a, double c) { return a < c ? a : c; };
  auto mx = [](double a, double c) { return a > c ? a : c; };
  if (b <= 0) {                    // unconstrained: no cone, the 2-norm of the slice for the caller's sums
    double s = 0;
    for (long long i = tid; i < -(long long)b; i += NT) s = fma(x[i], x[i], s);
    s = lm_reduce<NT>(s, red, add);
    if (tid == 0) { o[0] = 0.0; o[1] = 0.0; o[2] = (double)kLmFree; o[3] = sqrt(s); }
    return;
  }
  const int n = b;
  // ---- one pass over the rows: trace, sum |m_ii|, ||M||_F^2, sum |m_ij|, the Gershgorin value, min m_ii, max |m_ij| (infinite for a NaN)
  double t = 0, tau = 0, f2 = 0, asum = 0, g = INFINITY, dmin = INFINITY, amax = 0;
  for (int i = tid; i < n; i += NT) {
    const long long ri = (long long)i * (i + 1) / 2;
    const double d = sign * x[ri + i];
    double r = 0, sq = d * d;
    auto take = [&](double a) {
      const double ax = fabs(a);
      r += ax;
      sq = fma(a, a, sq);
      if (!(ax <= amax)) amax = ax == ax ? ax : INFINITY;
    };
    for (int j = 0; j < i; ++j) take(x[ri + j] * kLmInvSqrt2);
    for (int j = i + 1; j < n; ++j) take(x[(long long)j * (j + 1) / 2 + i] * kLmInvSqrt2);
    const double ad = fabs(d);
    if (!(ad <= amax)) amax = ad == ad ? ad : INFINITY;
    t += d; tau += ad; f2 += sq; asum += ad + r;
    g = mn(g, d - r);
    dmin = mn(dmin, d);
  }
  t = lm_reduce<NT>(t, red, add); tau = lm_reduce<NT>(tau, red, add); f2 = lm_reduce<NT>(f2, red, add); asum = lm_reduce<NT>(asum, red, add);
  g = lm_reduce<NT>(g, red, mn); dmin = lm_reduce<NT>(dmin, red, mn); amax = lm_reduce<NT>(amax, red, mx);
  const double eps = (double)(n + 2) * 0x1p-52;
  const double f = sqrt(f2);
  const double nu_max = mx(0.0, -g) + eps * asum;          // M + nu_max I is diagonally dominant, the rounding of g and asum included
  const double nu_floor = eps * f;
  double* S = LDS ? lm_sm : (work ? work + work_off[blockIdx.x] : nullptr);
  const bool in_range = amax <= kLmRangeHi && (amax >= kLmRangeLo || amax == 0.0);
  double lo, hi, flag;
  if (n > kLmMax || n > cap || !in_range || !S) {       // (n > cap: never, by the host's classes; the scratch is sized by cap)
    lo = nu_max < INFINITY ? -nu_max : -INFINITY;          // (a NaN among the entries: nothing is known)
    hi = dmin == dmin ? dmin : INFINITY;
    flag = (double)kLmUnrefined;
  } else {
    // the margin of a success at mu: lm_margin, plus a second-order term for the rounding of the trace itself
    auto margin = [&](double mu) { return mx(lm_margin(n, t, mu), 0.0) + eps * eps * (tau + (double)n * mu); };
    double a = nu_floor, c = nu_max, won = -1.0;
    if (lm_trial<NT>(x, sign, n, a, S)) {
      lo = mx(-a - margin(a), -nu_max);
      hi = dmin;                                           // no shift failed: lambda_min <= min m_ii is all that is known from above
      flag = (double)kLmPsdAtFloor;
    } else {
      for (int s = 0; s < steps; ++s) {
        if (!(c > a)) break;
        const double mu = sqrt(a) * sqrt(c);               // (not sqrt(a c): the product leaves the range the entries are held to)
        if (!(mu > a && mu < c)) break;
        if (lm_trial<NT>(x, sign, n, mu, S)) { c = mu; won = mu; } else a = mu;
      }
      lo = won >= 0.0 ? mx(-won - margin(won), -nu_max) : -nu_max;
      hi = -a;
      flag = (double)kLmRefined;
    }
  }
  if (tid == 0) { o[0] = lo; o[1] = hi; o[2] = flag; o[3] = f; }
}

}  // namespace

int lm_build_classes(int nblk, const int* blk, LmClass (&cls)[kLmClasses], long long* work_doubles) {
  if (nblk < 0 || (nblk > 0 && !blk) || !work_doubles) { set_error("lambda_min: invalid argument"); return CUADMM_ERR_INVALID; }
  static const int top[kLmClasses - 1] = {kLmSmall, 64, 128, kLmLds, kLmMax};
  for (auto& c : cls) { c.blocks.clear(); c.work.clear(); c.nmax = 0; }
  long long w = 0;
  for (int k = 0; k < nblk; ++k) {
    const int n = blk[k];
    int q = kLmClasses - 1;
    for (int j = kLmClasses - 2; j >= 0; --j)
      if (n > 0 && n <= top[j]) q = j;
    cls[q].blocks.push_back(k);
    if (n > cls[q].nmax) cls[q].nmax = n;
    if (q == kLmClasses - 2) { cls[q].work.push_back(w); w += (long long)n * (n + 1) / 2; }
  }
  *work_doubles = w;
  return CUADMM_OK;
}

int launch_lambda_min(int cls, int count, int nmax, const int* list, const double* v, double sign, const long long* off, const int* blk, int steps,
                      double* work, const long long* work_off, double* out, hipStream_t st) {
  if (cls < 0 || cls >= kLmClasses || count < 0 || steps < 1 || steps > kLmStepsMax || !(sign == 1.0 || sign == -1.0) ||
      (count > 0 && (!list || !v || !off || !blk || !out)) || (cls == kLmClasses - 2 && count > 0 && (!work || !work_off)) ||
      (cls < kLmClasses - 2 && (nmax < 0 || nmax > kLmLds)) || (cls == 0 && nmax > kLmSmall)) {
    set_error("lambda_min: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  if (count == 0) return CUADMM_OK;
  const size_t lds = cls < kLmClasses - 2 ? sizeof(double) * (size_t)nmax * (size_t)(nmax + 1) / 2 : 0;
  if (cls == 0) {
    hipLaunchKernelGGL((lambda_min_kernel<64, true>), dim3((unsigned)count), dim3(64), lds, st, list, v, sign, off, blk, steps, nmax, nullptr, nullptr, out);
  } else if (cls < kLmClasses - 2) {
    static LdsCapOnce once;
    CUADMM_HIP_TRY(once(reinterpret_cast<const void*>(&lambda_min_kernel<256, true>)));
    hipLaunchKernelGGL((lambda_min_kernel<256, true>), dim3((unsigned)count), dim3(256), lds, st, list, v, sign, off, blk, steps, nmax, nullptr, nullptr, out);
  } else {
    const bool ws = cls == kLmClasses - 2;
    hipLaunchKernelGGL((lambda_min_kernel<256, false>), dim3((unsigned)count), dim3(256), 0, st, list, v, sign, off, blk, steps, kLmMax, ws ? work : nullptr,
                       ws ? work_off : nullptr, out);
  }
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

}  // namespace cuadmm

extern "C" double cuadmm_lambda_min_margin(int n, double trace, double mu) { return cuadmm::lm_margin(n, trace, mu); }
