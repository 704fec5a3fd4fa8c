// Per-block numerical rank and low-rank factor: one workgroup per block runs Cholesky with diagonal pivoting on the svec block where it
// lies, in the lazy left-looking form, until the largest residual diagonal entry falls to the threshold or the column cap is reached.
// lowrank.h has the contracts and the four statements about the factor, DESIGN.md, "Low-rank factors", their derivation.
//
// Plain fp64 VALU arithmetic (fma, IEEE division and square root): the statements are about those operations and must not rest on the
// rounding of a matrix instruction's accumulate steps.  The running diagonal and the pivot row live in LDS, L in the output buffer: a
// thread re-reads only the rows it wrote itself (coalesced over i, the pivot row an LDS broadcast), the pivot row crosses threads behind a
// barrier.  Every loop is bounded by n and the column cap; nothing waits on another workgroup.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "lowrank.h"
#include "factor_layout.h"
#include "device_util.h"

namespace cuadmm {
namespace {

constexpr double kLrInvSqrt2 = 0.7071067811865476;      // off-diagonal svec entries carry sqrt(2)

// f over a workgroup of NT threads, the same bits in every thread (f commutative: the xor butterfly gives every lane one value)
template <int NT, class F>
__device__ __forceinline__ double lr_reduce(double v, double* red, F f) {
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

// (a, i) before (c, j): the larger value, on a tie the smaller index -- a total order, so the reduction below is one pair in every thread
__device__ __forceinline__ bool lr_before(double a, int i, double c, int j) { return a > c || (a == c && i < j); }

// argmax of (v, i) over the workgroup under lr_before
template <int NT>
__device__ __forceinline__ void lr_argmax(double& v, int& i, double* red, int* redi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double c = __shfl_xor(v, o, 64);
    const int j = __shfl_xor(i, o, 64);
    if (lr_before(c, j, v, i)) { v = c; i = j; }
  }
  if (NT == 64) return;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = v; redi[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = red[0]; i = redi[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w)
    if (lr_before(red[w], redi[w], v, i)) { v = red[w]; i = redi[w]; }
}

template <int NT>
__global__ __launch_bounds__(NT) void lowrank_kernel(const int* __restrict__ list, const double* __restrict__ v, double sign, const long long* __restrict__ off,
                                                     const int* __restrict__ blk, double tol, int rmax, int cap, const long long* __restrict__ loff,
                                                     const long long* __restrict__ poff, double* Lbuf, int* __restrict__ pivbuf, double* __restrict__ out) {
  extern __shared__ double lr_sm[];      // d[n], then the pivot row [rc]
  __shared__ double red[4];
  __shared__ int redi[4];
  const int tid = (int)threadIdx.x;
  const int k = list[blockIdx.x];
  const int b = blk[k];
  double* o = out + kLrOut * (size_t)k;
  if (b <= 0) {                    // unconstrained: rank 0 and nothing else
    if (tid == 0) { o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = 0.0; o[4] = (double)kLrFree; o[5] = (double)loff[k]; }
    return;
  }
  const int n = b, rc = n < rmax ? n : rmax;
  const double* x = v + off[k];
  double* L = Lbuf + loff[k];      // column j at L + j n, rows in the block's order
  int* piv = pivbuf + poff[k];
  double* d = lr_sm;
  double* prow = lr_sm + n;
  auto add = [](double a, double c) { return a + c; };
  auto mn = [](double a, double c) { return a < c ? a : c; };
  auto mx = [](double a, double c) { return a > c ? a : c; };
  // ---- max |m_ij| (infinite for a NaN): every slot as an off-diagonal one, then the diagonal slots at their own weight
  const long long len = (long long)n * (n + 1) / 2;
  double amax = 0, t = 0, dmax0 = -INFINITY;
  for (long long e = tid; e < len; e += NT) {
    const double ax = fabs(x[e]) * kLrInvSqrt2;
    if (!(ax <= amax)) amax = ax == ax ? ax : INFINITY;
  }
  const bool fits = n <= cap;      // (always, by the host's classes: the LDS is sized by cap)
  for (int i = tid; i < n; i += NT) {
    const double di = sign * x[(long long)i * (i + 3) / 2];
    const double ax = fabs(di);
    if (!(ax <= amax)) amax = ax == ax ? ax : INFINITY;
    if (fits) d[i] = di;
    t += di;
    dmax0 = mx(dmax0, di);
  }
  amax = lr_reduce<NT>(amax, red, mx);
  t = lr_reduce<NT>(t, red, add);
  dmax0 = lr_reduce<NT>(dmax0, red, mx);
  if (!fits || !(amax <= kLrRangeHi && (amax >= kLrRangeLo || amax == 0.0))) {      // not factored
    for (long long e = tid; e < (long long)n * rc; e += NT) L[e] = 0.0;
    for (int j = tid; j < rc; j += NT) piv[j] = -1;
    if (tid == 0) { o[0] = 0.0; o[1] = NAN; o[2] = 0.0; o[3] = t; o[4] = (double)kLrNotFactored; o[5] = (double)loff[k]; }
    return;
  }
  const double thr = tol * mx(dmax0, 0.0);
  // a row leaves the running diagonal as -infinity: its entries are finite, so no row that is still in can hold that
  int r = 0;
  double flag = (double)kLrComplete;
  __syncthreads();
  for (;; ++r) {                   // at most rc + 1 turns
    double dp = -INFINITY;
    int p = INT_MAX;
    for (int i = tid; i < n; i += NT)
      if (d[i] > dp) { dp = d[i]; p = i; }      // (ascending i: the smallest index of a tie)
    lr_argmax<NT>(dp, p, red, redi);
    if (!(dp > thr)) break;
    if (r == rc) { flag = (double)kLrCapped; break; }
    const double s = sqrt(dp);
    for (int j = tid; j < r; j += NT) prow[j] = L[(size_t)j * n + p];
    if (tid == 0) piv[r] = p;
    __syncthreads();
    double* Lr = L + (size_t)r * n;
    for (int i = tid; i < n; i += NT) {
      const double di = d[i];
      if (di == -INFINITY) { Lr[i] = 0.0; continue; }
      if (i == p) { Lr[i] = s; d[i] = -INFINITY; continue; }
      const int hi = i > p ? i : p, lo = i > p ? p : i;
      double acc = (sign * x[(long long)hi * (hi + 1) / 2 + lo]) * kLrInvSqrt2;
      const double* Li = L + i;
#pragma unroll 4
      for (int j = 0; j < r; ++j) acc = fma(-Li[(size_t)j * n], prow[j], acc);
      const double l = acc / s;
      Lr[i] = l;
      d[i] = fma(-l, l, di);
    }
    __syncthreads();               // column r is in memory and the pivot row may be overwritten
  }
  // ---- where it stopped: the rows still in, the columns not taken
  double resid = 0, dneg = 0;
  for (int i = tid; i < n; i += NT) {
    const double di = d[i];
    if (di != -INFINITY) { resid += fabs(di); dneg = mn(dneg, di); }
  }
  resid = lr_reduce<NT>(resid, red, add);
  dneg = lr_reduce<NT>(dneg, red, mn);
  for (long long e = (long long)r * n + tid; e < (long long)n * rc; e += NT) L[e] = 0.0;
  for (int j = r + tid; j < rc; j += NT) piv[j] = -1;
  if (tid == 0) { o[0] = (double)r; o[1] = resid; o[2] = dneg; o[3] = t; o[4] = flag; o[5] = (double)loff[k]; }
}

}  // namespace

int lr_build_classes(int nblk, const int* blk, int rmax, LrClass (&cls)[kLrClasses], std::vector<long long>* loff, std::vector<long long>* poff) {
  if (!loff || !poff) { set_error("lowrank: invalid argument"); return CUADMM_ERR_INVALID; }
  int rc = factor_offsets("lowrank", nblk, blk, rmax, loff);
  if (rc) return rc;
  static const int top[kLrClasses] = {kLrSmall, 128, 1024, kMaxBlockSize};
  for (auto& c : cls) { c.blocks.clear(); c.nmax = 0; }
  poff->assign((size_t)nblk + 1, 0);
  for (int k = 0; k < nblk; ++k) {
    const int n = blk[k];
    int q = 0;
    while (n > top[q]) ++q;
    cls[q].blocks.push_back(k);
    if (n > cls[q].nmax) cls[q].nmax = n;
    (*poff)[k + 1] = (*poff)[k] + (n > 0 ? factor_cols(n, rmax) : 0);
  }
  return CUADMM_OK;
}

int launch_lowrank(int cls, int count, int nmax, const int* list, const double* v, double sign, const long long* off, const int* blk, double tol, int rmax,
                   const long long* loff, const long long* poff, double* Lbuf, int* piv, double* out, hipStream_t st) {
  if (cls < 0 || cls >= kLrClasses || count < 0 || !(tol >= 0.0 && tol < 1.0) || rmax < 1 || rmax > kMaxBlockSize || !(sign == 1.0 || sign == -1.0) ||
      nmax < 0 || nmax > kMaxBlockSize || (cls == 0 && nmax > kLrSmall) || (count > 0 && (!list || !v || !off || !blk || !loff || !poff || !Lbuf || !piv || !out))) {
    set_error("lowrank: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  if (count == 0) return CUADMM_OK;
  const size_t lds = sizeof(double) * (size_t)(nmax + (nmax < rmax ? nmax : rmax));      // <= 128 KiB
  if (cls == 0) {
    hipLaunchKernelGGL((lowrank_kernel<64>), dim3((unsigned)count), dim3(64), lds, st, list, v, sign, off, blk, tol, rmax, nmax, loff, poff, Lbuf, piv, out);
  } else {
    static LdsCapOnce once;
    CUADMM_HIP_TRY(once(reinterpret_cast<const void*>(&lowrank_kernel<256>)));
    hipLaunchKernelGGL((lowrank_kernel<256>), dim3((unsigned)count), dim3(256), lds, st, list, v, sign, off, blk, tol, rmax, nmax, loff, poff, Lbuf, piv, out);
  }
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

}  // namespace cuadmm
