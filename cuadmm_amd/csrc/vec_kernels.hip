// HBM-bound kernels of the ADMM iteration (gfx950): fused vector updates, the two SpMVs,
// deterministic reductions, plus the op-level kernels that mirror the reference's own
// element-wise CUDA kernels one to one (used by the parity tests through the C ABI).
//
// Fusion map (reference call sites in src/solver.cu):
//   aty_xb     : SpMV At*y (:514) + D2D copy (:518) + Rd1 -= C (:520) + Xb = X + sig*Rd1 (:527)
//   post_admm  : Xdiff (:652) + S (:656) + Rd (:746) + X update (:758) + ||Rd||^2 (:775-776)
//                + <C,X> (:774), one pass
//   post_S / post_X : the same split around the second sGS solve (:693-729)
//   spmv_rows  : -A*SmC (:478,:695) and -A*X (:764) in one pass over A (SmC = S - C formed on the fly,
//                :672-674 removed)
// All reductions are two-stage (per-workgroup partials, then one workgroup) => run-to-run
// deterministic, unlike atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "device_util.h"
#include "vec_kernels.h"
#include "psd_fuse.h"

namespace cuadmm {

constexpr int kVecThreads = 256;

static inline int grid_for(long long n, int per_block, int cap = 256 * 8) {
  long long g = (n + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// block-wide sums of up to 2 values; result valid in thread 0
template <int NT>
__device__ __forceinline__ void block_sum2(double& a, double& b) {
  __shared__ double sa[NT / 64], sb[NT / 64];
  a = wave_sum(a);
  b = wave_sum(b);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sa[w] = a; sb[w] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ta = 0, tb = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) { ta += sa[i]; tb += sb[i]; }
    a = ta; b = tb;
  }
}

// ------------------------------------------------------------------------------------------
// Rd1 = At*y - C ; Xb = X + sig*Rd1          (one thread per svec row; rows are mostly 0..few nnz)
// ------------------------------------------------------------------------------------------
// Rows with more than `skip_above` entries (> 0) are left to aty_xb_long_kernel: a moment relaxation has svec slots --
// the (1,1) entry of the moment matrix -- that appear in thousands of constraints (PushT_N=10: one row with 2720 of
// the 46 388 nonzeros made this kernel take 0.39 ms of a 0.89 ms iteration).
// FOUR rows per thread and pass (rows i, i + stride, ...: every access still coalesced across the wavefront): the row pointers, C
// and X of all four are in flight before the first data-dependent nonzero loop starts.  With one row per thread the kernel was
// bound by memory-level parallelism, not bandwidth: 3.3 TB/s at BASELINE configs[3] size (41 % of 8 TB/s).
template <bool WRITE_XB>
__global__ __launch_bounds__(kVecThreads) void aty_xb_kernel(long long L, const int* __restrict__ rp,
                                                             const int* __restrict__ ci, const double* __restrict__ av,
                                                             const double* __restrict__ y, const double* __restrict__ C,
                                                             const double* __restrict__ X, double sig,
                                                             double* __restrict__ Rd1, double* __restrict__ Xb, int skip_above) {
  constexpr int R = 4;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x; i0 < L; i0 += R * stride) {
    int p0[R], p1[R];
    double c[R], x[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const long long i = i0 + k * stride;
      const long long ii = i < L ? i : i0;                   // out of range: the thread's first row again (masked below)
      p0[k] = rp[ii]; p1[k] = rp[ii + 1]; c[k] = C[ii];
      x[k] = WRITE_XB ? X[ii] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const long long i = i0 + k * stride;
      if (i >= L || (skip_above > 0 && p1[k] - p0[k] > skip_above)) continue;
      double t = 0.0;
      for (int p = p0[k]; p < p1[k]; ++p) t += av[p] * y[ci[p]];
      const double r = t - c[k];
      Rd1[i] = r;
      if (WRITE_XB) Xb[i] = x[k] + r * sig;
    }
  }
}

// EIGHT lanes per row: a moment relaxation has svec rows of up to the long-row cap (128) entries among thousands of short ones
// (PlanarHand_N=1: mean 2.8, 7.7 % of the rows above 8), and one thread per row walks such a row one dependent gather after the
// other -- the longest row decides: 52 us for 55 k rows, latency, not bandwidth.  Lane s of a row takes entries s, s + 8, ...; three
// shuffles add the partial sums in a fixed order.  Taken when a row below the cap is longer than 24.
template <bool WRITE_XB>
__global__ __launch_bounds__(kVecThreads) void aty_xb_g8_kernel(long long L, const int* __restrict__ rp, const int* __restrict__ ci,
                                                                const double* __restrict__ av, const double* __restrict__ y,
                                                                const double* __restrict__ C, const double* __restrict__ X, double sig,
                                                                double* __restrict__ Rd1, double* __restrict__ Xb, int skip_above) {
  const long long gt = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long i = gt >> 3;
  const int sub = (int)(gt & 7);
  const bool in = i < L;
  const int p0 = in ? rp[i] : 0, p1 = in ? rp[i + 1] : 0;
  const bool skip = skip_above > 0 && p1 - p0 > skip_above;
  double t = 0.0;
  if (!skip)
    for (int p = p0 + sub; p < p1; p += 8) t += av[p] * y[ci[p]];
  t += __shfl_xor(t, 4, 64);
  t += __shfl_xor(t, 2, 64);
  t += __shfl_xor(t, 1, 64);
  if (in && !skip && sub == 0) {
    const double r = t - C[i];
    Rd1[i] = r;
    if (WRITE_XB) Xb[i] = X[i] + r * sig;
  }
}

// the same over a LIST of svec rows (fused iteration: the rows outside the blocks whose projection kernel does this itself)
__global__ __launch_bounds__(kVecThreads) void aty_xb_idx_kernel(long long nidx, const int* __restrict__ idx, const int* __restrict__ rp,
                                                                 const int* __restrict__ ci, const double* __restrict__ av,
                                                                 const double* __restrict__ y, const double* __restrict__ C,
                                                                 const double* __restrict__ X, double sig,
                                                                 double* __restrict__ Rd1, double* __restrict__ Xb) {
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < nidx; k += (long long)gridDim.x * blockDim.x) {
    const int i = idx[k];
    double t = 0.0;
    for (int p = rp[i]; p < rp[i + 1]; ++p) t += av[p] * y[ci[p]];
    const double r = t - C[i];
    Rd1[i] = r;
    Xb[i] = X[i] + r * sig;
  }
}

// Second half of an sGS iteration in ONE pass (solver.cu:707-729,746-758,774-776): Rd1 = A^T y - C with the new y, Rd = Rd1 + S,
// X += tau sigma Rd, sum Rd^2, <C, X> -- aty_xb_kernel<false> followed by post_kernel<2> wrote and re-read Rd1 (16 B per svec
// element of 76) and took two launches.  Same expressions; Rd1 is not stored (the next iteration forms its own).
__global__ __launch_bounds__(kVecThreads) void aty_post2_kernel(long long L, const int* __restrict__ rp, const int* __restrict__ ci,
                                                                const double* __restrict__ av, const double* __restrict__ y,
                                                                const double* __restrict__ C, const double* __restrict__ S,
                                                                double* __restrict__ X, double tau_sig, double* __restrict__ partials) {
  double s_rd = 0.0, s_cx = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < L; i += (long long)gridDim.x * blockDim.x) {
    double t = 0.0;
    for (int p = rp[i]; p < rp[i + 1]; ++p) t += av[p] * y[ci[p]];
    const double c = C[i];
    const double r1 = t - c;
    const double rd = r1 + S[i];
    const double xn = X[i] + tau_sig * rd;
    X[i] = xn;
    s_rd += rd * rd;
    s_cx += c * xn;
  }
  block_sum2<kVecThreads>(s_rd, s_cx);
  if (threadIdx.x == 0) { partials[2 * blockIdx.x] = s_rd; partials[2 * blockIdx.x + 1] = s_cx; }
}

// one workgroup per long row (two-stage sum in a fixed order: reproducible)
template <bool WRITE_XB>
__global__ __launch_bounds__(kVecThreads) void aty_xb_long_kernel(const int* __restrict__ long_rows, const int* __restrict__ rp,
                                                                  const int* __restrict__ ci, const double* __restrict__ av,
                                                                  const double* __restrict__ y, const double* __restrict__ C,
                                                                  const double* __restrict__ X, double sig,
                                                                  double* __restrict__ Rd1, double* __restrict__ Xb) {
  __shared__ double red[kVecThreads];
  const int i = long_rows[blockIdx.x];
  double t = 0.0;
  for (int p = rp[i] + (int)threadIdx.x; p < rp[i + 1]; p += kVecThreads) t += av[p] * y[ci[p]];
  red[threadIdx.x] = t;
  __syncthreads();
  for (int o = kVecThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double r = red[0] - C[i];
    Rd1[i] = r;
    if (WRITE_XB) Xb[i] = X[i] + r * sig;
  }
}

// ------------------------------------------------------------------------------------------
// after the projection
// ------------------------------------------------------------------------------------------
// mode 0 (ADMM): S = (Xproj - X)/sig - Rd1 ; Rd = Rd1 + S ; X += tau*sig*Rd ; sums
// mode 1 (sGS first half): S only
// mode 2 (sGS second half): Rd = Rd1 + S ; X += tau*sig*Rd ; sums        (S read, not written)
template <int MODE>
__global__ __launch_bounds__(kVecThreads) void post_kernel(long long L, const double* __restrict__ Xproj,
                                                           const double* __restrict__ Rd1, const double* __restrict__ C,
                                                           double* __restrict__ X, double* __restrict__ S,
                                                           double inv_sig, double tau_sig, double* __restrict__ partials) {
  double s_rd = 0.0, s_cx = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < L; i += (long long)gridDim.x * blockDim.x) {
    const double x = X[i];
    const double r1 = Rd1[i];
    double s;
    if (MODE == 2) {
      s = S[i];
    } else {
      const double xdiff = Xproj[i] - x;
      s = inv_sig * xdiff - r1;
      S[i] = s;
    }
    if (MODE != 1) {
      const double rd = r1 + s;
      const double xn = x + tau_sig * rd;
      X[i] = xn;
      s_rd += rd * rd;
      s_cx += C[i] * xn;
    }
  }
  if (MODE != 1) {
    block_sum2<kVecThreads>(s_rd, s_cx);
    if (threadIdx.x == 0) { partials[2 * blockIdx.x] = s_rd; partials[2 * blockIdx.x + 1] = s_cx; }
  }
}

// post_kernel<0|1> over a LIST of svec rows (fused iteration); partial sums at partials[2 * blockIdx.x]
template <int MODE>
__global__ __launch_bounds__(kVecThreads) void post_idx_kernel(long long nidx, const int* __restrict__ idx, const double* __restrict__ Xproj,
                                                               const double* __restrict__ Rd1, const double* __restrict__ C,
                                                               double* __restrict__ X, double* __restrict__ S,
                                                               double inv_sig, double tau_sig, double* __restrict__ partials) {
  double s_rd = 0.0, s_cx = 0.0;
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < nidx; k += (long long)gridDim.x * blockDim.x) {
    const int i = idx[k];
    const double x = X[i];
    const double r1 = Rd1[i];
    const double xdiff = Xproj[i] - x;
    const double s = inv_sig * xdiff - r1;
    S[i] = s;
    if (MODE == 0) {
      const double rd = r1 + s;
      const double xn = x + tau_sig * rd;
      X[i] = xn;
      s_rd += rd * rd;
      s_cx += C[i] * xn;
    }
  }
  if (MODE == 0) {
    block_sum2<kVecThreads>(s_rd, s_cx);
    if (threadIdx.x == 0) { partials[2 * blockIdx.x] = s_rd; partials[2 * blockIdx.x + 1] = s_cx; }
  }
}

// sums `nparts` (a,b) pairs into out[0], out[1]: one workgroup of 1024 threads, four independent partial sums per thread
// (the fused iteration leaves one pair per block: 10 000 pairs took 13 us with 256 threads and one dependent chain each);
// fixed assignment and order: bit-reproducible
constexpr int kReduceThreads = 1024;
__global__ __launch_bounds__(kReduceThreads) void reduce_pairs_kernel(const double* __restrict__ partials, int nparts,
                                                                      double* __restrict__ out) {
  double a0 = 0.0, b0 = 0.0, a1 = 0.0, b1 = 0.0, a2 = 0.0, b2 = 0.0, a3 = 0.0, b3 = 0.0;
  const double2* __restrict__ pp = reinterpret_cast<const double2*>(partials);
  int i = threadIdx.x;
  for (; i + 3 * kReduceThreads < nparts; i += 4 * kReduceThreads) {
    const double2 v0 = pp[i], v1 = pp[i + kReduceThreads], v2 = pp[i + 2 * kReduceThreads], v3 = pp[i + 3 * kReduceThreads];
    a0 += v0.x; b0 += v0.y; a1 += v1.x; b1 += v1.y; a2 += v2.x; b2 += v2.y; a3 += v3.x; b3 += v3.y;
  }
  for (; i < nparts; i += kReduceThreads) { const double2 v = pp[i]; a0 += v.x; b0 += v.y; }
  double a = (a0 + a1) + (a2 + a3), b = (b0 + b1) + (b2 + b3);
  block_sum2<kReduceThreads>(a, b);
  if (threadIdx.x == 0) { out[0] = a; out[1] = b; }
}

// Fused iteration with closed blocks (psd_fuse.h): the projection kernels left BOTH partial pairs per block -- (sum Rd^2,
// <C, X>) in p1 (followed by the pairs of the stand-alone post step) and (||Rp org||^2, b^T y) in p2 -- and this one
// workgroup forms all four scalars of the stopping test: out4 = [||Rp||^2, b.y, sum Rd^2, <C,X>], sums_out = out4[2..3].
// The sums are formed per SEGMENT of kQuadSeg consecutive pairs (one workgroup per segment: thread t adds pairs t, t + 1024, ... of
// its segment into two alternating accumulators, then the workgroup's tree) and the segment sums are added in segment order.  Up to
// kQuadSeg pairs (BASELINE configs[1]: 10 000 blocks) that is the single-workgroup reduction of round 2, bit for bit; beyond (configs[3]:
// 100 000 blocks, 57 us through one CU) the segments run on as many workgroups.  Every variant -- one launch per iteration, several
// iterations per launch -- uses this association: the same bits.
constexpr int kQuadSeg = 16384;
__device__ __forceinline__ void quad_segment_sum(const double2* __restrict__ q, int n, int seg, double& a, double& b) {
  const int beg = seg * kQuadSeg, end = n < beg + kQuadSeg ? n : beg + kQuadSeg;
  double a0 = 0.0, b0 = 0.0, a1 = 0.0, b1 = 0.0;
  int i = beg + (int)threadIdx.x;
  for (; i + kReduceThreads < end; i += 2 * kReduceThreads) { const double2 u = q[i], v = q[i + kReduceThreads]; a0 += u.x; b0 += u.y; a1 += v.x; b1 += v.y; }
  for (; i < end; i += kReduceThreads) { const double2 u = q[i]; a0 += u.x; b0 += u.y; }
  a = a0 + a1; b = b0 + b1;
  block_sum2<kReduceThreads>(a, b);      // valid in thread 0
  __syncthreads();
}
__global__ __launch_bounds__(kReduceThreads) void reduce_quads_kernel(const double* __restrict__ p1, int n1, const double* __restrict__ p2, int n2,
                                                                     double* __restrict__ out4, double* __restrict__ sums_out, double* __restrict__ seg_out) {
  const double2* __restrict__ q1 = reinterpret_cast<const double2*>(p1);
  const double2* __restrict__ q2 = reinterpret_cast<const double2*>(p2);
  const int sg = (int)blockIdx.x;
  double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
  if (sg * kQuadSeg < n1 || sg == 0) quad_segment_sum(q1, n1, sg, a, b);
  if (sg * kQuadSeg < n2 || sg == 0) quad_segment_sum(q2, n2, sg, c, d);
  if (threadIdx.x == 0) {
    if (gridDim.x == 1) { out4[0] = c; out4[1] = d; out4[2] = a; out4[3] = b; sums_out[0] = a; sums_out[1] = b; }
    else { double* o = seg_out + 4 * (size_t)sg; o[0] = c; o[1] = d; o[2] = a; o[3] = b; }
  }
}
__global__ void reduce_quads_final_kernel(const double* __restrict__ seg_out, int nseg, double* __restrict__ out4, double* __restrict__ sums_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double v[4] = {seg_out[0], seg_out[1], seg_out[2], seg_out[3]};
  for (int s = 1; s < nseg; ++s)
    for (int k = 0; k < 4; ++k) v[k] += seg_out[4 * (size_t)s + k];
  for (int k = 0; k < 4; ++k) out4[k] = v[k];
  sums_out[0] = v[2]; sums_out[1] = v[3];
}

// Several iterations per launch (SignFuse::iters): workgroup k forms the four scalars of iteration k from that iteration's partial
// arrays (p1 + k stride, p2 + k stride; n pairs each) with the assignment and order of reduce_quads_kernel -- the same bits as
// one launch per iteration.
__global__ __launch_bounds__(kReduceThreads) void reduce_quads_batch_kernel(const double* __restrict__ p1, const double* __restrict__ p2, int n,
                                                                           long long stride, double* __restrict__ out4) {
  const double2* __restrict__ q1 = reinterpret_cast<const double2*>(p1 + (long long)blockIdx.x * stride);
  const double2* __restrict__ q2 = reinterpret_cast<const double2*>(p2 + (long long)blockIdx.x * stride);
  const int nseg = n > 0 ? (n + kQuadSeg - 1) / kQuadSeg : 1;
  double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
  for (int sg = 0; sg < nseg; ++sg) {
    double sa, sb, sc, sd;
    quad_segment_sum(q1, n, sg, sa, sb);
    quad_segment_sum(q2, n, sg, sc, sd);
    if (sg == 0) { a = sa; b = sb; c = sc; d = sd; } else { a += sa; b += sb; c += sc; d += sd; }
  }
  if (threadIdx.x == 0) { double* o = out4 + 4 * (size_t)blockIdx.x; o[0] = c; o[1] = d; o[2] = a; o[3] = b; }
}

int launch_reduce_quads_batch(const double* p1, const double* p2, int n, long long stride, int iters, double* out4, hipStream_t st) {
  hipLaunchKernelGGL(reduce_quads_batch_kernel, dim3(iters), dim3(kReduceThreads), 0, st, p1, p2, n, stride, out4);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

// closed blocks keep a per-block copy of their rows of [A X | A (S - C)] (psd_sign_closed.h); after a stand-alone kernel wrote
// those vectors by row (init, restart, the sGS half step's A X) the copy is refreshed from them
__global__ __launch_bounds__(kVecThreads) void closed_gather_out_kernel(const ClosedRec* __restrict__ rec, int nslots, const double* __restrict__ ax,
                                                                      const double* __restrict__ as, double* __restrict__ cl_out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int slot = (int)(i / kClosedMaxRows), k = (int)(i % kClosedMaxRows);
  if (slot >= nslots || k >= rec[slot].nk) return;
  const int row = rec[slot].rows[k];
  cl_out[16 * (long long)slot + k] = ax[row];
  cl_out[16 * (long long)slot + 8 + k] = as[row];
}
int launch_closed_gather_out(const ClosedRec* rec, int nslots, const double* ax, const double* as, double* cl_out, hipStream_t st) {
  if (nslots <= 0) return CUADMM_OK;
  const long long n = (long long)nslots * kClosedMaxRows;
  hipLaunchKernelGGL(closed_gather_out_kernel, dim3((unsigned)((n + kVecThreads - 1) / kVecThreads)), dim3(kVecThreads), 0, st, rec, nslots, ax, as, cl_out);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int reduce_quads_segments(int n1, int n2) {
  const int nmax = n1 > n2 ? n1 : n2;
  return nmax > 0 ? (nmax + kQuadSeg - 1) / kQuadSeg : 1;
}
// seg_scratch: 4 doubles per segment (reduce_quads_segments), only touched when there is more than one segment
int launch_reduce_quads(const double* p1, int n1, const double* p2, int n2, double* out4, double* sums_out, double* seg_scratch, hipStream_t st) {
  const int nseg = reduce_quads_segments(n1, n2);
  if (nseg > 1 && !seg_scratch) { set_error("reduce_quads: no scratch for %d segments", nseg); return CUADMM_ERR_INVALID; }
  hipLaunchKernelGGL(reduce_quads_kernel, dim3(nseg), dim3(kReduceThreads), 0, st, p1, n1, p2, n2, out4, sums_out, seg_scratch);
  if (nseg > 1) hipLaunchKernelGGL(reduce_quads_final_kernel, dim3(1), dim3(64), 0, st, seg_scratch, nseg, out4, sums_out);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

// Owned-constraints sharding: the two constraint-space sums of the stopping test, formed on the device from A*X so that
// all four scalars of an iteration travel in ONE small all-reduce enqueued on the stream (no host round trip):
//   out4[0] = sum_i (normA_i (b_i - (A X)_i) bscale)^2   (|| Rp org ||^2, solver.cu:768-772)
//   out4[1] = sum_i b_i y_i                               (solver.cu:781)
//   out4[2..3] = sums[0..1] (sum Rd^2, <C, X>: copied next to them)
// Two stages over a fixed grid, fixed summation order: bit-reproducible.
__global__ __launch_bounds__(kVecThreads) void rp_stats_partial_kernel(int m, const double* __restrict__ ax, const double* __restrict__ b,
                                                                       const double* __restrict__ normA, const double* __restrict__ y,
                                                                       double bscale, double* __restrict__ partials) {
  double a = 0.0, c = 0.0;
  for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < m; i += (int)(gridDim.x * blockDim.x)) {
    const double ro = normA[i] * (b[i] - ax[i]) * bscale;
    a += ro * ro;
    c += b[i] * y[i];
  }
  block_sum2<kVecThreads>(a, c);
  if (threadIdx.x == 0) { partials[2 * blockIdx.x] = a; partials[2 * blockIdx.x + 1] = c; }
}
__global__ __launch_bounds__(kVecThreads) void rp_stats_final_kernel(const double* __restrict__ partials, int nparts, const double* __restrict__ sums,
                                                                     double* __restrict__ out4) {
  double a = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) { a += partials[2 * i]; c += partials[2 * i + 1]; }
  block_sum2<kVecThreads>(a, c);
  if (threadIdx.x == 0) { out4[0] = a; out4[1] = c; out4[2] = sums[0]; out4[3] = sums[1]; }
}
// two-stage, fixed grid (64 workgroups) and fixed summation order: bit-reproducible; `partials` holds 128 doubles
int launch_rp_stats(int m, const double* ax, const double* b, const double* normA, const double* y, double bscale,
                    const double* sums, double* partials, double* out4, hipStream_t st) {
  constexpr int kGrid = 64;
  hipLaunchKernelGGL(rp_stats_partial_kernel, dim3(kGrid), dim3(kVecThreads), 0, st, m, ax, b, normA, y, bscale, partials);
  hipLaunchKernelGGL(rp_stats_final_kernel, dim3(1), dim3(kVecThreads), 0, st, partials, kGrid, sums, out4);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// The y-solve of a block-diagonal A A^T on the device (engine option: automatic when the elimination forest of the factor
// consists of many small trees): y = (L D L^T)^-1 rhs with rhs = -A(S-C) + (b - A X) / sigma (solver.cu:478-500), one
// THREAD per tree.  The sweeps of a solve never leave a tree, and inside a tree this is the serial host algorithm
// (aat_ldlt.cpp: columns ascending, x[i] -= L[i][j] x[j]; then x[j] / D[j] and the transposed sweep) with unfused
// multiply-subtract, so y is bit-identical to the host solve.  y stays in HBM: no m-vector crosses PCIe in an iteration.
// (Contraction is switched off for the kernel's body by pragma: __dmul_rn / __dsub_rn are plain operators to this compiler and were
// fused into v_fma_f64 / v_fmac_f64 after inlining -- tests/test_gpu_iter_kernels.py compares with the host solve bit for bit.)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kVecThreads) void forest_solve_kernel(int ntrees, const int* __restrict__ tree_ptr, const int* __restrict__ tree_cols,
                                                                   const long long* __restrict__ Lp, const int* __restrict__ Li,
                                                                   const double* __restrict__ Lx, const double* __restrict__ D,
                                                                   const double* __restrict__ ax, const double* __restrict__ asmc,
                                                                   const double* __restrict__ b, double isig, double* __restrict__ x) {
#pragma clang fp contract(off)
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= ntrees) return;
  const int c0 = tree_ptr[t], c1 = tree_ptr[t + 1];
  for (int q = c0; q < c1; ++q) {
    const int j = tree_cols[q];
    const double rp = -ax[j] + b[j];                                 // Rp = -A X + b
    const double scaled = isig * rp;
    x[j] = -asmc[j] + scaled;                                        // rhs = -A(S-C) + Rp / sigma
  }
  for (int q = c0; q < c1; ++q) {                                    // L z = rhs
    const int j = tree_cols[q];
    const double xj = x[j];
    if (xj != 0.0)
      for (long long p = Lp[j]; p < Lp[j + 1]; ++p) { const double u = Lx[p] * xj; x[Li[p]] = x[Li[p]] - u; }
  }
  for (int q = c1 - 1; q >= c0; --q) {                               // D^-1, then L^T y = z
    const int j = tree_cols[q];
    double s = x[j] / D[j];
    for (long long p = Lp[j]; p < Lp[j + 1]; ++p) { const double u = Lx[p] * x[Li[p]]; s = s - u; }
    x[j] = s;
  }
}
int launch_forest_solve(int ntrees, const int* tree_ptr, const int* tree_cols, const long long* Lp, const int* Li, const double* Lx,
                        const double* D, const double* ax, const double* asmc, const double* b, double isig, double* x, hipStream_t st) {
  if (ntrees <= 0) return CUADMM_OK;
  hipLaunchKernelGGL(forest_solve_kernel, dim3((ntrees + kVecThreads - 1) / kVecThreads), dim3(kVecThreads), 0, st, ntrees, tree_ptr, tree_cols, Lp,
                     Li, Lx, D, ax, asmc, b, isig, x);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// rows of A (constraints, already in the solver's permuted order): T lanes per row.
//   outX[row]  = sum a * X[col]            (if outX)
//   outS[row]  = sum a * (S[col] - C[col]) (if outS)
// ------------------------------------------------------------------------------------------
// `cap` > 0: only the first `cap` nonzeros of a row are summed here; the rest of such LONG rows (a trace or all-ones
// constraint can hold as many nonzeros as the whole svec) is cut into segments summed by spmv_segments_kernel and
// added in segment order by spmv_finish_kernel -- one row must not serialise the launch (swissroll: one row with
// 320 000 of the 330 537 nonzeros made this kernel take 4.8 ms).
template <int T>
__global__ __launch_bounds__(kVecThreads) void spmv_rows_kernel(int rows, const int* __restrict__ rp,
                                                                const int* __restrict__ ci, const double* __restrict__ av,
                                                                const double* __restrict__ X, const double* __restrict__ S,
                                                                const double* __restrict__ C, double* __restrict__ outX,
                                                                double* __restrict__ outS, int cap, const int* __restrict__ rowmap) {
  const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int sub = (int)(threadIdx.x & (T - 1));
  const long long nsub = (long long)gridDim.x * blockDim.x / T;
  const bool doX = outX != nullptr, doS = outS != nullptr;
  for (long long row = gtid / T; row < rows; row += nsub) {
    const int p0 = rp[row];
    int p1 = rp[row + 1];
    if (cap > 0 && p1 - p0 > cap) p1 = p0 + cap;
    double ax = 0.0, as = 0.0;
    for (int p = p0 + sub; p < p1; p += T) {
      const int c = ci[p];
      const double a = av[p];
      if (doX) ax += a * X[c];
      if (doS) as += a * (S[c] - C[c]);
    }
#pragma unroll
    for (int o = T >> 1; o > 0; o >>= 1) {
      ax += __shfl_xor(ax, o, 64);
      as += __shfl_xor(as, o, 64);
    }
    if (sub == 0) {
      const long long orow = rowmap ? rowmap[row] : row;     // compact row list (fused iteration): the constraint's own slot
      if (doX) outX[orow] = ax;
      if (doS) outS[orow] = as;
    }
  }
}

// one workgroup per segment [seg_begin, seg_end) of a long row: partial[2*seg] (A X), partial[2*seg+1] (A (S - C))
__global__ __launch_bounds__(kVecThreads) void spmv_segments_kernel(const int* __restrict__ seg_begin, const int* __restrict__ seg_end,
                                                                    const int* __restrict__ ci, const double* __restrict__ av,
                                                                    const double* __restrict__ X, const double* __restrict__ S,
                                                                    const double* __restrict__ C, bool doX, bool doS,
                                                                    double* __restrict__ partial) {
  __shared__ double rx[kVecThreads], rs[kVecThreads];
  const int p0 = seg_begin[blockIdx.x], p1 = seg_end[blockIdx.x];
  double ax = 0.0, as = 0.0;
  for (int p = p0 + (int)threadIdx.x; p < p1; p += kVecThreads) {
    const int c = ci[p];
    const double a = av[p];
    if (doX) ax += a * X[c];
    if (doS) as += a * (S[c] - C[c]);
  }
  rx[threadIdx.x] = ax; rs[threadIdx.x] = as;
  __syncthreads();
  for (int o = kVecThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { rx[threadIdx.x] += rx[threadIdx.x + o]; rs[threadIdx.x] += rs[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { partial[2 * blockIdx.x] = rx[0]; partial[2 * blockIdx.x + 1] = rs[0]; }
}
// out[row] += its segments' partials, in segment order (one thread per long row)
__global__ void spmv_finish_kernel(int nlong, const int* __restrict__ long_row, const int* __restrict__ long_seg0,
                                   const double* __restrict__ partial, double* __restrict__ outX, double* __restrict__ outS) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= nlong) return;
  double ax = 0.0, as = 0.0;
  for (int sgi = long_seg0[i]; sgi < long_seg0[i + 1]; ++sgi) { ax += partial[2 * sgi]; as += partial[2 * sgi + 1]; }
  if (outX) outX[long_row[i]] += ax;
  if (outS) outS[long_row[i]] += as;
}

int launch_aty_xb(bool write_xb, long long L, const int* rp, const int* ci, const double* av, const double* y,
                  const double* C, const double* X, double sig, double* Rd1, double* Xb, hipStream_t st, const AtyLongRows* lr) {
  const int grid = grid_for((L + 3) / 4, kVecThreads, 256 * 16);
  const int skip = (lr && lr->nlong > 0) ? lr->cap : 0;
  if (lr && lr->max_short > 24) {                       // rows of dozens of entries below the long-row cap: eight lanes per row
    const long long g8 = (L * 8 + kVecThreads - 1) / kVecThreads;
    if (write_xb) hipLaunchKernelGGL(aty_xb_g8_kernel<true>, dim3((unsigned)g8), dim3(kVecThreads), 0, st, L, rp, ci, av, y, C, X, sig, Rd1, Xb, skip);
    else hipLaunchKernelGGL(aty_xb_g8_kernel<false>, dim3((unsigned)g8), dim3(kVecThreads), 0, st, L, rp, ci, av, y, C, X, sig, Rd1, Xb, skip);
  } else if (write_xb)
    hipLaunchKernelGGL(aty_xb_kernel<true>, dim3(grid), dim3(kVecThreads), 0, st, L, rp, ci, av, y, C, X, sig, Rd1, Xb, skip);
  else
    hipLaunchKernelGGL(aty_xb_kernel<false>, dim3(grid), dim3(kVecThreads), 0, st, L, rp, ci, av, y, C, X, sig, Rd1, Xb, skip);
  if (skip > 0) {
    if (write_xb)
      hipLaunchKernelGGL(aty_xb_long_kernel<true>, dim3(lr->nlong), dim3(kVecThreads), 0, st, lr->rows, rp, ci, av, y, C, X, sig, Rd1, Xb);
    else
      hipLaunchKernelGGL(aty_xb_long_kernel<false>, dim3(lr->nlong), dim3(kVecThreads), 0, st, lr->rows, rp, ci, av, y, C, X, sig, Rd1, Xb);
  }
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int launch_aty_xb_idx(long long nidx, const int* idx, const int* rp, const int* ci, const double* av, const double* y, const double* C,
                      const double* X, double sig, double* Rd1, double* Xb, hipStream_t st) {
  if (nidx <= 0) return CUADMM_OK;
  hipLaunchKernelGGL(aty_xb_idx_kernel, dim3(grid_for(nidx, kVecThreads, 256 * 16)), dim3(kVecThreads), 0, st, nidx, idx, rp, ci, av, y, C, X, sig, Rd1, Xb);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int launch_aty_post2(long long L, const int* rp, const int* ci, const double* av, const double* y, const double* C, const double* S, double* X,
                     double tau_sig, double* partials, double* sums_out, hipStream_t st) {
  const int grid = post_grid(L);
  hipLaunchKernelGGL(aty_post2_kernel, dim3(grid), dim3(kVecThreads), 0, st, L, rp, ci, av, y, C, S, X, tau_sig, partials);
  hipLaunchKernelGGL(reduce_pairs_kernel, dim3(1), dim3(kReduceThreads), 0, st, partials, grid, sums_out);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int AtyLongRows::build(long long L, const int* rp_host) {
  release();
  std::vector<int> lr;
  for (long long i = 0; i < L; ++i)
    if (rp_host[i + 1] - rp_host[i] > cap) lr.push_back((int)i);
  max_short = 0;
  for (long long i = 0; i < L; ++i) { const int len = rp_host[i + 1] - rp_host[i]; if (len <= cap && len > max_short) max_short = len; }
  nlong = (int)lr.size();
  if (nlong == 0) return CUADMM_OK;
  CUADMM_HIP_TRY(hipMalloc(&rows, sizeof(int) * lr.size()));
  { int rc_ = staged_h2d(rows, lr.data(), sizeof(int) * lr.size()); if (rc_) return rc_; }
  return CUADMM_OK;
}
void AtyLongRows::release() {
  if (rows) { hipError_t e = hipFree(rows); (void)e; }
  rows = nullptr;
  nlong = 0;
}

int post_grid(long long L) { return grid_for(L, kVecThreads * 4, 256 * 8); }

int launch_post(int mode, long long L, const double* Xproj, const double* Rd1, const double* C, double* X, double* S,
                double inv_sig, double tau_sig, double* partials, double* sums_out, hipStream_t st) {
  const int grid = post_grid(L);
  switch (mode) {
    case 0: hipLaunchKernelGGL(post_kernel<0>, dim3(grid), dim3(kVecThreads), 0, st, L, Xproj, Rd1, C, X, S, inv_sig, tau_sig, partials); break;
    case 1: hipLaunchKernelGGL(post_kernel<1>, dim3(grid), dim3(kVecThreads), 0, st, L, Xproj, Rd1, C, X, S, inv_sig, tau_sig, partials); break;
    default: hipLaunchKernelGGL(post_kernel<2>, dim3(grid), dim3(kVecThreads), 0, st, L, Xproj, Rd1, C, X, S, inv_sig, tau_sig, partials); break;
  }
  CUADMM_HIP_TRY(hipGetLastError());
  if (mode != 1) {
    hipLaunchKernelGGL(reduce_pairs_kernel, dim3(1), dim3(kReduceThreads), 0, st, partials, grid, sums_out);
    CUADMM_HIP_TRY(hipGetLastError());
  }
  return CUADMM_OK;
}

// Fused iteration: the projection kernels left one partial pair per fused block in partials[0, 2 nfused); the rows of `idx`
// add their grid's pairs behind them, and (mode 0) everything is summed in slot order.
int launch_post_rest(int mode, long long nidx, const int* idx, int nfused, const double* Xproj, const double* Rd1, const double* C, double* X,
                     double* S, double inv_sig, double tau_sig, double* partials, double* sums_out, hipStream_t st, int* nparts_out) {
  const int grid = nidx > 0 ? post_grid(nidx) : 0;
  if (nidx > 0) {
    double* part = partials + 2 * (size_t)nfused;
    if (mode == 0) hipLaunchKernelGGL(post_idx_kernel<0>, dim3(grid), dim3(kVecThreads), 0, st, nidx, idx, Xproj, Rd1, C, X, S, inv_sig, tau_sig, part);
    else hipLaunchKernelGGL(post_idx_kernel<1>, dim3(grid), dim3(kVecThreads), 0, st, nidx, idx, Xproj, Rd1, C, X, S, inv_sig, tau_sig, part);
    CUADMM_HIP_TRY(hipGetLastError());
  }
  if (nparts_out) { *nparts_out = nfused + grid; return CUADMM_OK; }    // the caller reduces (launch_reduce_quads)
  if (mode == 0) {
    hipLaunchKernelGGL(reduce_pairs_kernel, dim3(1), dim3(kReduceThreads), 0, st, partials, nfused + grid, sums_out);
    CUADMM_HIP_TRY(hipGetLastError());
  }
  return CUADMM_OK;
}

int launch_spmv_rows(int rows, double avg_nnz, const int* rp, const int* ci, const double* av, const double* X,
                     const double* S, const double* C, double* outX, double* outS, hipStream_t st, const SpmvLongRows* lr, const int* rowmap) {
  if (rows <= 0) return CUADMM_OK;
  const int cap = (lr && lr->nlong > 0) ? lr->cap : 0;
  int T = 1;
  while (T < 64 && T < avg_nnz) T <<= 1;
  const int grid = grid_for((long long)rows * T, kVecThreads, 256 * 16);
#define CUADMM_SPMV_CASE(TT) \
  case TT: hipLaunchKernelGGL(spmv_rows_kernel<TT>, dim3(grid), dim3(kVecThreads), 0, st, rows, rp, ci, av, X, S, C, outX, outS, cap, rowmap); break;
  switch (T) {
    CUADMM_SPMV_CASE(1) CUADMM_SPMV_CASE(2) CUADMM_SPMV_CASE(4) CUADMM_SPMV_CASE(8)
    CUADMM_SPMV_CASE(16) CUADMM_SPMV_CASE(32) CUADMM_SPMV_CASE(64)
  }
#undef CUADMM_SPMV_CASE
  CUADMM_HIP_TRY(hipGetLastError());
  if (cap > 0) {
    hipLaunchKernelGGL(spmv_segments_kernel, dim3(lr->nseg), dim3(kVecThreads), 0, st, lr->seg_begin, lr->seg_end, ci, av, X, S, C,
                       outX != nullptr, outS != nullptr, lr->partial);
    hipLaunchKernelGGL(spmv_finish_kernel, dim3((lr->nlong + 63) / 64), dim3(64), 0, st, lr->nlong, lr->long_row, lr->long_seg0, lr->partial,
                       outX, outS);
    CUADMM_HIP_TRY(hipGetLastError());
  }
  return CUADMM_OK;
}

// rows with more than `cap` nonzeros: segments of `seg_len` nonzeros beyond the first `cap`
int SpmvLongRows::build(int rows, const int* rp_host) {
  release();
  // "long" is relative: 8x the average row, at least 256 nonzeros (a matrix of uniformly long rows has no long rows)
  cap = (int)std::max<long long>(256, rows > 0 ? 8LL * rp_host[rows] / rows : 0);
  std::vector<int> lrow, lseg0{0}, sb, se;
  for (int r = 0; r < rows; ++r) {
    const int len = rp_host[r + 1] - rp_host[r];
    if (len <= cap) continue;
    lrow.push_back(r);
    for (int p = rp_host[r] + cap; p < rp_host[r + 1]; p += seg_len) { sb.push_back(p); se.push_back(std::min(p + seg_len, rp_host[r + 1])); }
    lseg0.push_back((int)sb.size());
  }
  nlong = (int)lrow.size();
  nseg = (int)sb.size();
  if (nlong == 0) return CUADMM_OK;
  CUADMM_HIP_TRY(hipMalloc(&long_row, sizeof(int) * lrow.size()));
  CUADMM_HIP_TRY(hipMalloc(&long_seg0, sizeof(int) * lseg0.size()));
  CUADMM_HIP_TRY(hipMalloc(&seg_begin, sizeof(int) * sb.size()));
  CUADMM_HIP_TRY(hipMalloc(&seg_end, sizeof(int) * se.size()));
  CUADMM_HIP_TRY(hipMalloc(&partial, sizeof(double) * 2 * sb.size()));
  { int rc_ = staged_h2d(long_row, lrow.data(), sizeof(int) * lrow.size()); if (rc_) return rc_; }
  { int rc_ = staged_h2d(long_seg0, lseg0.data(), sizeof(int) * lseg0.size()); if (rc_) return rc_; }
  { int rc_ = staged_h2d(seg_begin, sb.data(), sizeof(int) * sb.size()); if (rc_) return rc_; }
  { int rc_ = staged_h2d(seg_end, se.data(), sizeof(int) * se.size()); if (rc_) return rc_; }
  return CUADMM_OK;
}
// average row length that picks the lanes per row of spmv_rows_kernel: with long rows only the part the main kernel sums counts
// (their capped tails go to the segment kernels)
double spmv_avg_nnz(int rows, const int* rp_host, const SpmvLongRows& lr) {
  if (rows <= 0) return 1.0;
  if (lr.nlong == 0) return (double)(rp_host[rows] - rp_host[0]) / rows;
  long long capped = 0;
  for (int i = 0; i < rows; ++i) capped += std::min(rp_host[i + 1] - rp_host[i], lr.cap);
  return (double)capped / rows;
}
void SpmvLongRows::release() {
  for (void* p : {(void*)long_row, (void*)long_seg0, (void*)seg_begin, (void*)seg_end, (void*)partial}) if (p) { hipError_t e = hipFree(p); (void)e; }
  long_row = long_seg0 = seg_begin = seg_end = nullptr;
  partial = nullptr;
  nlong = nseg = 0;
}

// ------------------------------------------------------------------------------------------
// small helpers used by the engine
// ------------------------------------------------------------------------------------------
__global__ void scale_kernel(double* v, long long n, double s) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) v[i] *= s;
}
// dst <- src (device to device), as a kernel on the caller's stream: the runtime's own device-to-device copy measured at 0.3 ms
// for 42 MB on this driver (a copy-engine path); 16 bytes per lane, two in flight
__global__ __launch_bounds__(kVecThreads) void copy_kernel(double* __restrict__ dst, const double* __restrict__ src, long long n) {
  const long long n2 = n / 2, stride = (long long)gridDim.x * blockDim.x;
  const double2* __restrict__ s2 = reinterpret_cast<const double2*>(src);
  double2* __restrict__ d2 = reinterpret_cast<double2*>(dst);
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + stride < n2; i += 2 * stride) { const double2 a = s2[i], b = s2[i + stride]; d2[i] = a; d2[i + stride] = b; }
  for (; i < n2; i += stride) d2[i] = s2[i];
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) dst[n - 1] = src[n - 1];
}
int launch_copy(double* dst, const double* src, long long n, hipStream_t st) {
  if (n <= 0) return CUADMM_OK;
  hipLaunchKernelGGL(copy_kernel, dim3(grid_for(n / 2 + 1, kVecThreads, 256 * 8)), dim3(kVecThreads), 0, st, dst, src, n);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

typedef unsigned sl_copy16 __attribute__((ext_vector_type(4)));
// several device-to-device copies in ONE launch (the checkpoint of a batch: X, S, y, [A X | sums | A (S - C)], the schedule hints):
// 16-byte words where the length allows, 4-byte words for the tail; pointers 16-byte aligned (hipMalloc)
__global__ __launch_bounds__(kVecThreads) void copy_multi_kernel(CopyJobs j) {
  const long long stride = (long long)gridDim.x * kVecThreads;
  for (int q = 0; q < j.count; ++q) {
    const sl_copy16* __restrict__ s = reinterpret_cast<const sl_copy16*>(j.src[q]);
    sl_copy16* __restrict__ d = reinterpret_cast<sl_copy16*>(j.dst[q]);
    const long long n16 = j.nbytes[q] >> 4;
    for (long long i = (long long)blockIdx.x * kVecThreads + threadIdx.x; i < n16; i += stride) d[i] = s[i];
    const int tail4 = (int)((j.nbytes[q] & 15) >> 2);
    if (blockIdx.x == 0 && (int)threadIdx.x < tail4)
      reinterpret_cast<unsigned*>(j.dst[q])[4 * n16 + threadIdx.x] = reinterpret_cast<const unsigned*>(j.src[q])[4 * n16 + threadIdx.x];
  }
}
int launch_copy_multi(const CopyJobs& jobs, hipStream_t st) {
  long long most = 0;
  for (int q = 0; q < jobs.count; ++q) {
    if (jobs.nbytes[q] & 3) { set_error("copy_multi: length %lld is not a multiple of 4 bytes", jobs.nbytes[q]); return CUADMM_ERR_INVALID; }
    most = std::max(most, jobs.nbytes[q] >> 4);
  }
  if (jobs.count <= 0 || most <= 0) {
    bool any = false;
    for (int q = 0; q < jobs.count; ++q) any = any || jobs.nbytes[q] > 0;
    if (!any) return CUADMM_OK;
  }
  hipLaunchKernelGGL(copy_multi_kernel, dim3(grid_for(most + 1, kVecThreads, 256 * 8)), dim3(kVecThreads), 0, st, jobs);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int launch_scale(double* v, long long n, double s, hipStream_t st) {
  if (n <= 0) return CUADMM_OK;
  hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n, kVecThreads)), dim3(kVecThreads), 0, st, v, n, s);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// cuadmm_update_bC (engine_update.hip): new b / C on a factored solver.  Every element goes through the rounded operations of
// materialise() followed by init's scaling, in that order, so the updated solver holds the bits a fresh init would hold.
// ------------------------------------------------------------------------------------------
// One streaming pass over the rank's svec: X <- (X x1) x2, S <- (S s1) s2 (ZERO: both <- 0, a cold start), C <- 0 when it is
// replaced (its entries are scattered behind this launch).  16 bytes per lane and access, two elements of every vector in flight;
// 32 L bytes of traffic (+ 8 L with C); the pad behind the L elements is not touched.
typedef double up_d2 __attribute__((ext_vector_type(2)));
template <bool WRITE_C, bool ZERO>
__global__ __launch_bounds__(kVecThreads) void update_svec_kernel(double* __restrict__ X, double* __restrict__ S, double* __restrict__ C, long long n,
                                                                double x1, double x2, double s1, double s2) {
  const long long n2 = n / 2, stride = (long long)gridDim.x * kVecThreads;
  up_d2* __restrict__ X2 = reinterpret_cast<up_d2*>(X);
  up_d2* __restrict__ S2 = reinterpret_cast<up_d2*>(S);
  up_d2* __restrict__ C2 = reinterpret_cast<up_d2*>(C);
  const up_d2 zero = {0.0, 0.0};
  long long i = (long long)blockIdx.x * kVecThreads + threadIdx.x;
  if (ZERO) {
    for (; i < n2; i += stride) { X2[i] = zero; S2[i] = zero; if (WRITE_C) C2[i] = zero; }
  } else {
    for (; i + stride < n2; i += 2 * stride) {
      const up_d2 xa = X2[i], xb = X2[i + stride], sa = S2[i], sb = S2[i + stride];
      X2[i] = (xa * x1) * x2; X2[i + stride] = (xb * x1) * x2;
      S2[i] = (sa * s1) * s2; S2[i + stride] = (sb * s1) * s2;
      if (WRITE_C) { C2[i] = zero; C2[i + stride] = zero; }
    }
    for (; i < n2; i += stride) {
      const up_d2 xa = X2[i], sa = S2[i];
      X2[i] = (xa * x1) * x2; S2[i] = (sa * s1) * s2;
      if (WRITE_C) C2[i] = zero;
    }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    X[n - 1] = ZERO ? 0.0 : (X[n - 1] * x1) * x2;
    S[n - 1] = ZERO ? 0.0 : (S[n - 1] * s1) * s2;
    if (WRITE_C) C[n - 1] = 0.0;
  }
}
int launch_update_svec(double* X, double* S, double* C, long long n, bool zero, double x1, double x2, double s1, double s2, hipStream_t st) {
  if (n <= 0) return CUADMM_OK;
  const dim3 grid(grid_for(n / 2 + 1, kVecThreads * 2, 256 * 8)), block(kVecThreads);
  if (C && zero) hipLaunchKernelGGL((update_svec_kernel<true, true>), grid, block, 0, st, X, S, C, n, x1, x2, s1, s2);
  else if (C) hipLaunchKernelGGL((update_svec_kernel<true, false>), grid, block, 0, st, X, S, C, n, x1, x2, s1, s2);
  else if (zero) hipLaunchKernelGGL((update_svec_kernel<false, true>), grid, block, 0, st, X, S, C, n, x1, x2, s1, s2);
  else hipLaunchKernelGGL((update_svec_kernel<false, false>), grid, block, 0, st, X, S, C, n, x1, x2, s1, s2);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}
// One pass over the m constraints (the factor's order): b <- 0 when it is replaced (entries scattered behind this launch);
// y by ymode: 0 leave, 1 <- 0, 2 <- ((y / normA cs_old) normA) ics_new  (materialise(), then init's y0 normA / Cscale)
__global__ __launch_bounds__(kVecThreads) void update_cons_kernel(int m, double* __restrict__ b, double* __restrict__ y, const double* __restrict__ normA,
                                                                int ymode, double cs_old, double ics_new) {
  for (int i = blockIdx.x * kVecThreads + threadIdx.x; i < m; i += gridDim.x * kVecThreads) {
    if (b) b[i] = 0.0;
    if (ymode == 1) y[i] = 0.0;
    else if (ymode == 2) { const double na = normA[i]; y[i] = ((y[i] / na * cs_old) * na) * ics_new; }
  }
}
int launch_update_cons(int m, double* b, double* y, const double* normA, int ymode, double cs_old, double ics_new, hipStream_t st) {
  if (m <= 0 || (!b && ymode == 0)) return CUADMM_OK;
  hipLaunchKernelGGL(update_cons_kernel, dim3(grid_for(m, kVecThreads)), dim3(kVecThreads), 0, st, m, b, y, normA, ymode, cs_old, ics_new);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}
// dst[idx[k]] = val[k] * s: the entries of a sparse vector into its zero-filled dense form (distinct indices: no two lanes meet)
__global__ __launch_bounds__(kVecThreads) void scatter_scaled_kernel(double* __restrict__ dst, const int* __restrict__ idx, const double* __restrict__ val, int n, double s) {
  for (int k = blockIdx.x * kVecThreads + threadIdx.x; k < n; k += gridDim.x * kVecThreads) dst[idx[k]] = val[k] * s;
}
int launch_scatter_scaled(double* dst, const int* idx, const double* val, int n, double s, hipStream_t st) {
  if (n <= 0) return CUADMM_OK;
  hipLaunchKernelGGL(scatter_scaled_kernel, dim3(grid_for(n, kVecThreads)), dim3(kVecThreads), 0, st, dst, idx, val, n, s);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}
// closed blocks: the b entries of the per-block records from the by-row vector (nothing else in a record depends on b)
__global__ __launch_bounds__(kVecThreads) void closed_patch_b_kernel(ClosedRec* __restrict__ rec, int nslots, const double* __restrict__ b) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int slot = (int)(i / kClosedMaxRows), k = (int)(i % kClosedMaxRows);
  if (slot >= nslots || k >= rec[slot].nk) return;
  rec[slot].b[k] = b[rec[slot].rows[k]];
}
int launch_closed_patch_b(ClosedRec* rec, int nslots, const double* b, hipStream_t st) {
  if (nslots <= 0) return CUADMM_OK;
  const long long n = (long long)nslots * kClosedMaxRows;
  hipLaunchKernelGGL(closed_patch_b_kernel, dim3((unsigned)((n + kVecThreads - 1) / kVecThreads)), dim3(kVecThreads), 0, st, rec, nslots, b);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// cuadmm_update_A (engine_update.hip): new values of A on the pattern of init.  The host normalises this rank's values with init's arithmetic
// and uploads them once, in the caller's order; this kernel writes the value arrays of both device matrices from them through two index
// maps (CSR slot -> position in the upload, built at the first update).  Stores are streaming and 16 bytes wide wherever the target is
// 16-byte aligned (a leading element of a misaligned array and an odd last one go alone); the loads are the gather.  The long-row and
// compact-row SpMV variants read these arrays too, so nothing else has to move.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void gather_vals_range(double* __restrict__ dst, const int* __restrict__ from, long long n, const double* __restrict__ src,
                                                  long long tid, long long stride) {
  if (n <= 0) return;
  const long long head = (reinterpret_cast<unsigned long long>(dst) & 8ull) ? 1 : 0;      // elements in front of the first 16-byte boundary
  const long long n2 = (n - head) / 2;
  up_d2* __restrict__ d2 = reinterpret_cast<up_d2*>(dst + head);
  const int* __restrict__ f2 = from + head;
  for (long long i = tid; i < n2; i += stride) {
    up_d2 v;
    v.x = src[f2[2 * i]]; v.y = src[f2[2 * i + 1]];
    d2[i] = v;
  }
  if (tid == 0) {
    if (head) dst[0] = src[from[0]];
    if ((n - head) & 1) dst[n - 1] = src[from[n - 1]];
  }
}
__global__ __launch_bounds__(kVecThreads) void gather_vals_kernel(double* __restrict__ vA, const int* __restrict__ fromA, long long nA, double* __restrict__ vAt,
                                                                const int* __restrict__ fromAt, long long nAt, const double* __restrict__ src) {
  const long long tid = (long long)blockIdx.x * kVecThreads + threadIdx.x, stride = (long long)gridDim.x * kVecThreads;
  gather_vals_range(vA, fromA, nA, src, tid, stride);
  gather_vals_range(vAt, fromAt, nAt, src, tid, stride);
}
int launch_gather_vals(double* vA, const int* fromA, long long nA, double* vAt, const int* fromAt, long long nAt, const double* src, hipStream_t st) {
  if (nA <= 0 && nAt <= 0) return CUADMM_OK;
  hipLaunchKernelGGL(gather_vals_kernel, dim3(grid_for(std::max(nA, nAt) / 2 + 1, kVecThreads, 256 * 8)), dim3(kVecThreads), 0, st, vA, fromA, nA, vAt, fromAt, nAt, src);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// op-level kernels: one per reference kernel (same element-wise semantics)
// ------------------------------------------------------------------------------------------
// src/kernels/vec_mat_conversion.cu:11-34
__global__ void v2m_kernel(const double* Xb, double* large_mat, double* small_mat, const int* mB, const int* m1,
                           const int* m2, int vec_len) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < vec_len) {
    const int a = m1[idx], b = m2[idx];
    const double v = (a == b) ? Xb[idx] : Xb[idx] * 0x1.6a09e667f3bcdp-1;
    double* dst = (mB[idx] == 0) ? large_mat : small_mat;
    dst[a] = v;
    dst[b] = v;
  }
}
// src/kernels/vec_mat_conversion.cu:36-57
__global__ void m2v_kernel(double* Xb, const double* large_mat, const double* small_mat, const int* mB, const int* m1,
                           const int* m2, int vec_len) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < vec_len) {
    const int a = m1[idx], b = m2[idx];
    const double* src = (mB[idx] == 0) ? large_mat : small_mat;
    const double v = src[a];
    Xb[idx] = (a == b) ? v : v * 0x1.6a09e667f3bccp+0;
  }
}
// src/kernels/dense_scalar.cu:41-47
__global__ void max_zero_kernel(double* w, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) w[i] = fmax(w[i], 0.0);
}
// src/kernels/diagonal_batch.cu:11-23 (column-major: scales column j of matrix k by w[k*n+j])
__global__ void mul_diag_kernel(double* out, const double* in, const double* w, int n, long long total) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < total) {
    const long long n2 = (long long)n * n;
    const long long k = idx / n2;
    const int col = (int)((idx - k * n2) / n);
    out[idx] = in[idx] * w[k * n + col];
  }
}
// src/kernels/permutation.cu:12-18 (scatter)
__global__ void permute_kernel(double* v1, const double* v2, const int* perm, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v1[perm[i]] = v2[i];
}
// src/kernels/sparse_matrix_norm.cu:11-31
__global__ void normA_kernel(const int* cp, double* vals, double* normA, int con_num) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < con_num) {
    double nrm = 0.0;
    for (int p = cp[j]; p < cp[j + 1]; ++p) nrm += vals[p] * vals[p];
    nrm = fmax(1.0, sqrt(nrm));
    normA[j] = nrm;
    for (int p = cp[j]; p < cp[j + 1]; ++p) vals[p] /= nrm;
  }
}
// src/kernels/dense_dense.cu:15-24 / :28-37
__global__ void axpby2_kernel(double* v1, const double* v2, double a, double b, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v1[i] = a * v1[i] + b * v2[i];
}
__global__ void axpby3_kernel(double* v1, const double* v2, const double* v3, double a, double b, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v1[i] = a * v2[i] + b * v3[i];
}
// general CSR SpMV y = alpha*A*x + beta*y (include/cuadmm/cusparse.h:70-83), one wavefront-quarter per row
__global__ void spmv_csr_kernel(int rows, const int* rp, const int* ci, const double* av, const double* x, double* y,
                                double alpha, double beta) {
  constexpr int T = 16;
  const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int sub = (int)(threadIdx.x & (T - 1));
  const long long nsub = (long long)gridDim.x * blockDim.x / T;
  for (long long row = gtid / T; row < rows; row += nsub) {
    double acc = 0.0;
    for (int p = rp[row] + sub; p < rp[row + 1]; p += T) acc += av[p] * x[ci[p]];
#pragma unroll
    for (int o = T >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (sub == 0) y[row] = (beta == 0.0) ? alpha * acc : alpha * acc + beta * y[row];
  }
}
__global__ __launch_bounds__(kVecThreads) void sumsq_partial_kernel(const double* v, long long n, double* partials) {
  double a = 0.0, b = 0.0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) a += v[i] * v[i];
  block_sum2<kVecThreads>(a, b);
  if (threadIdx.x == 0) { partials[2 * blockIdx.x] = a; partials[2 * blockIdx.x + 1] = 0.0; }
}

// P = T * V^T per n x n column-major matrix on the FP64 matrix cores
// (the reference's cublasDgemmStridedBatched(N,T), include/cuadmm/cublas.h:18-35).
// One wavefront per 16x16 tile of P; v_mfma_f64_16x16x4_f64: lane l feeds A[i=l&15][k=l>>4],
// B[k=l>>4][j=l&15]; D[row=(l>>4)+4*reg][col=l&15].
typedef double v4f64 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void mul_trans_mfma_kernel(double* __restrict__ P, const double* __restrict__ T,
                                                             const double* __restrict__ V, int n, int count,
                                                             int tiles_per_dim) {
  const int wave = (int)((blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6);
  const int lane = (int)(threadIdx.x & 63);
  const int tiles = tiles_per_dim * tiles_per_dim;
  const int mat = wave / tiles;
  if (mat >= count) return;
  const int tile = wave - mat * tiles;
  const int ti = tile % tiles_per_dim, tj = tile / tiles_per_dim;
  const double* Tm = T + (long long)mat * n * n;
  const double* Vm = V + (long long)mat * n * n;
  double* Pm = P + (long long)mat * n * n;
  const int i = ti * 16 + (lane & 15);   // row of T feeding A
  const int j = tj * 16 + (lane & 15);   // row of V feeding B (B[k][j] = V[j][k])
  const int kk = lane >> 4;
  v4f64 acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < n; k0 += 4) {
    const int k = k0 + kk;
    const double a = (i < n && k < n) ? Tm[(long long)k * n + i] : 0.0;
    const double b = (j < n && k < n) ? Vm[(long long)k * n + j] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  const int col = tj * 16 + (lane & 15);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = ti * 16 + (lane >> 4) + 4 * r;
    if (row < n && col < n) Pm[(long long)col * n + row] = acc[r];
  }
}

}  // namespace cuadmm

using namespace cuadmm;

#define ST(s) ((hipStream_t)(s))
#define LAUNCH1D(kern, n, st, ...)                                                          \
  do {                                                                                      \
    long long _n = (n);                                                                     \
    if (_n > 0) {                                                                           \
      hipLaunchKernelGGL(kern, dim3((unsigned)((_n + 255) / 256)), dim3(256), 0, ST(st), __VA_ARGS__); \
      CUADMM_HIP_TRY(hipGetLastError());                                                    \
    }                                                                                       \
  } while (0)

namespace {
template <class T>
struct HookBuf {
  T* p = nullptr;
  int from(const T* h, size_t n) {
    CUADMM_HIP_TRY(hipMalloc(&p, sizeof(T) * std::max<size_t>(n, 1)));
    return (n && h) ? staged_h2d(p, h, sizeof(T) * n) : CUADMM_OK;
  }
  int to(T* h, size_t n) const { return n ? staged_d2h(h, p, sizeof(T) * n) : CUADMM_OK; }
  ~HookBuf() { if (p) { hipError_t e = hipFree(p); (void)e; } }
};
bool csr_ok(long long rows, long long cols, const int* rp, const int* ci) {
  if (rows < 0 || !rp || rp[0] != 0) return false;
  for (long long i = 0; i < rows; ++i) if (rp[i + 1] < rp[i]) return false;
  if (rp[rows] > 0 && !ci) return false;
  for (int p = 0; p < rp[rows]; ++p) if (ci[p] < 0 || ci[p] >= cols) return false;
  return true;
}
}  // namespace

extern "C" {

int cuadmm_op_vector_to_matrices(const double* Xb, double* large_mat, double* small_mat, const int* map_B,
                                 const int* map_M1, const int* map_M2, int vec_len, void* stream) {
  LAUNCH1D(v2m_kernel, vec_len, stream, Xb, large_mat, small_mat, map_B, map_M1, map_M2, vec_len);
  return CUADMM_OK;
}
int cuadmm_op_matrices_to_vector(double* Xb, const double* large_mat, const double* small_mat, const int* map_B,
                                 const int* map_M1, const int* map_M2, int vec_len, void* stream) {
  LAUNCH1D(m2v_kernel, vec_len, stream, Xb, large_mat, small_mat, map_B, map_M1, map_M2, vec_len);
  return CUADMM_OK;
}
int cuadmm_op_max_zero(double* w, int64_t n, void* stream) {
  LAUNCH1D(max_zero_kernel, n, stream, w, (long long)n);
  return CUADMM_OK;
}
int cuadmm_op_mul_diag_batch(double* out, const double* in, const double* w, int n, int count, void* stream) {
  const long long total = (long long)n * n * count;
  LAUNCH1D(mul_diag_kernel, total, stream, out, in, w, n, total);
  return CUADMM_OK;
}
int cuadmm_op_mul_trans_batch(double* P, const double* T, const double* V, int n, int count, void* stream) {
  if (n <= 0 || count <= 0) return CUADMM_OK;
  const int tpd = (n + 15) / 16;
  const long long waves = (long long)tpd * tpd * count;
  const long long blocks = (waves + 3) / 4;
  hipLaunchKernelGGL(mul_trans_mfma_kernel, dim3((unsigned)blocks), dim3(256), 0, ST(stream), P, T, V, n, count, tpd);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}
int cuadmm_op_permute(double* v1, const double* v2, const int* perm, int n, void* stream) {
  LAUNCH1D(permute_kernel, n, stream, v1, v2, perm, n);
  return CUADMM_OK;
}
int cuadmm_op_get_normA(const int* col_ptrs, double* vals, double* normA, int con_num, void* stream) {
  LAUNCH1D(normA_kernel, con_num, stream, col_ptrs, vals, normA, con_num);
  return CUADMM_OK;
}
int cuadmm_op_spmv_csr(int rows, const int* row_ptrs, const int* col_ids, const double* vals, const double* x, double* y,
                       double alpha, double beta, void* stream) {
  if (rows <= 0) return CUADMM_OK;
  const int grid = grid_for((long long)rows * 16, 256, 256 * 16);
  hipLaunchKernelGGL(spmv_csr_kernel, dim3(grid), dim3(256), 0, ST(stream), rows, row_ptrs, col_ids, vals, x, y, alpha, beta);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}
int cuadmm_op_axpby2(double* v1, const double* v2, double alpha, double beta, int64_t n, void* stream) {
  LAUNCH1D(axpby2_kernel, n, stream, v1, v2, alpha, beta, (long long)n);
  return CUADMM_OK;
}
int cuadmm_op_axpby3(double* v1, const double* v2, const double* v3, double alpha, double beta, int64_t n, void* stream) {
  LAUNCH1D(axpby3_kernel, n, stream, v1, v2, v3, alpha, beta, (long long)n);
  return CUADMM_OK;
}
int cuadmm_op_norm2(const double* v, int64_t n, double* host_out, void* stream) {
  if (!host_out) { set_error("norm2: null output"); return CUADMM_ERR_INVALID; }
  *host_out = 0.0;
  if (n <= 0) return CUADMM_OK;
  const int grid = grid_for(n, kVecThreads * 4, 1024);
  double* buf = nullptr;
  CUADMM_HIP_TRY(hipMalloc(&buf, sizeof(double) * (2 * (size_t)grid + 2)));
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(grid), dim3(kVecThreads), 0, ST(stream), v, (long long)n, buf);
  hipLaunchKernelGGL(reduce_pairs_kernel, dim3(1), dim3(kReduceThreads), 0, ST(stream), buf, grid, buf + 2 * grid);
  double h[2] = {0, 0};
  hipError_t e = hipMemcpyAsync(h, buf + 2 * grid, sizeof(h), hipMemcpyDeviceToHost, ST(stream));
  if (e == hipSuccess) e = hipStreamSynchronize(ST(stream));
  hipError_t e2 = hipFree(buf);
  (void)e2;
  CUADMM_HIP_TRY(e);
  *host_out = sqrt(h[0]);
  return CUADMM_OK;
}

// ------------------------------------------------------------------------------------------
// Test hooks only: the iteration's own kernels as ops (host pointers; copies through the staged buffers).  Every index array is
// checked before anything is launched, so a malformed input is an error code, never an out-of-range access.
// ------------------------------------------------------------------------------------------

int cuadmm_op_aty_xb(int64_t L, int m, const int* rp, const int* ci, const double* av, const double* y, const double* C, const double* X,
                     double sig, int write_xb, double* Rd1, double* Xb, int* info2) {
  if (L < 1 || m < 1 || !av || !y || !C || !X || !Rd1 || !Xb || !info2 || !csr_ok(L, m, rp, ci)) { set_error("op_aty_xb: bad arguments"); return CUADMM_ERR_INVALID; }
  const size_t nnz = (size_t)rp[L];
  AtyLongRows lr;
  int rc = lr.build(L, rp);
  if (rc) return rc;
  HookBuf<int> d_rp, d_ci;
  HookBuf<double> d_av, d_y, d_C, d_X, d_Rd1, d_Xb;
  if ((rc = d_rp.from(rp, (size_t)L + 1)) || (rc = d_ci.from(ci, nnz)) || (rc = d_av.from(av, nnz)) || (rc = d_y.from(y, (size_t)m)) || (rc = d_C.from(C, (size_t)L)) ||
      (rc = d_X.from(X, (size_t)L)) || (rc = d_Rd1.from(Rd1, (size_t)L)) || (rc = d_Xb.from(Xb, (size_t)L)))
    return rc;
  if ((rc = launch_aty_xb(write_xb != 0, L, d_rp.p, d_ci.p, d_av.p, d_y.p, d_C.p, d_X.p, sig, d_Rd1.p, d_Xb.p, nullptr, &lr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  if ((rc = d_Rd1.to(Rd1, (size_t)L)) || (rc = d_Xb.to(Xb, (size_t)L))) return rc;
  info2[0] = lr.nlong; info2[1] = lr.max_short;
  return CUADMM_OK;
}

int cuadmm_op_post(int mode, int64_t L, const double* Xproj, const double* Rd1, const double* C, double* X, double* S, double inv_sig, double tau_sig,
                   double* sums2, int m, const int* rp, const int* ci, const double* av, const double* y, int* nparts_out) {
  if (mode < 0 || mode > 3 || L < 1 || !C || !X || !S || !sums2) { set_error("op_post: bad arguments"); return CUADMM_ERR_INVALID; }
  if (mode < 3 && (!Xproj || !Rd1)) { set_error("op_post: modes 0 - 2 take Xproj and Rd1"); return CUADMM_ERR_INVALID; }
  if (mode == 3 && (m < 1 || !av || !y || !csr_ok(L, m, rp, ci))) { set_error("op_post: mode 3 takes A^T by svec rows and y"); return CUADMM_ERR_INVALID; }
  const int grid = post_grid(L);
  int rc;
  HookBuf<double> d_Xp, d_Rd1, d_C, d_X, d_S, d_part, d_sums, d_av, d_y;
  HookBuf<int> d_rp, d_ci;
  if ((rc = d_C.from(C, (size_t)L)) || (rc = d_X.from(X, (size_t)L)) || (rc = d_S.from(S, (size_t)L)) || (rc = d_part.from(nullptr, 2 * (size_t)grid)) ||
      (rc = d_sums.from(sums2, 2)))
    return rc;
  if (mode < 3) {
    if ((rc = d_Xp.from(Xproj, (size_t)L)) || (rc = d_Rd1.from(Rd1, (size_t)L))) return rc;
    rc = launch_post(mode, L, d_Xp.p, d_Rd1.p, d_C.p, d_X.p, d_S.p, inv_sig, tau_sig, d_part.p, d_sums.p, nullptr);
  } else {
    const size_t nnz = (size_t)rp[L];
    if ((rc = d_rp.from(rp, (size_t)L + 1)) || (rc = d_ci.from(ci, nnz)) || (rc = d_av.from(av, nnz)) || (rc = d_y.from(y, (size_t)m))) return rc;
    rc = launch_aty_post2(L, d_rp.p, d_ci.p, d_av.p, d_y.p, d_C.p, d_S.p, d_X.p, tau_sig, d_part.p, d_sums.p, nullptr);
  }
  if (rc) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  if ((rc = d_X.to(X, (size_t)L)) || (rc = d_S.to(S, (size_t)L)) || (rc = d_sums.to(sums2, 2))) return rc;
  if (nparts_out) *nparts_out = grid;
  return CUADMM_OK;
}

int cuadmm_op_spmv_rows(int rows, int ncols, const int* rp, const int* ci, const double* av, const double* X, const double* S, const double* C,
                        int want_x, int want_s, const int* rowmap, int out_len, double* outX, double* outS, int* info4) {
  if (rows < 1 || ncols < 1 || !av || !X || !S || !C || !outX || !outS || !info4 || out_len < 1 || !csr_ok(rows, ncols, rp, ci) || (!rowmap && out_len != rows)) {
    set_error("op_spmv_rows: bad arguments");
    return CUADMM_ERR_INVALID;
  }
  if (rowmap)
    for (int r = 0; r < rows; ++r) if (rowmap[r] < 0 || rowmap[r] >= out_len) { set_error("op_spmv_rows: rowmap[%d] out of range", r); return CUADMM_ERR_INVALID; }
  const size_t nnz = (size_t)rp[rows];
  int rc;
  SpmvLongRows lr;
  // a compact row list has no long rows (engine: the rows left over by the fused blocks; the finish kernel writes by row number)
  if (!rowmap && (rc = lr.build(rows, rp))) return rc;
  const double avg = spmv_avg_nnz(rows, rp, lr);
  HookBuf<int> d_rp, d_ci, d_map;
  HookBuf<double> d_av, d_X, d_S, d_C, d_oX, d_oS;
  if ((rc = d_rp.from(rp, (size_t)rows + 1)) || (rc = d_ci.from(ci, nnz)) || (rc = d_av.from(av, nnz)) || (rc = d_X.from(X, (size_t)ncols)) ||
      (rc = d_S.from(S, (size_t)ncols)) || (rc = d_C.from(C, (size_t)ncols)) || (rc = d_oX.from(outX, (size_t)out_len)) || (rc = d_oS.from(outS, (size_t)out_len)) ||
      (rowmap && (rc = d_map.from(rowmap, (size_t)rows))))
    return rc;
  if ((rc = launch_spmv_rows(rows, avg, d_rp.p, d_ci.p, d_av.p, d_X.p, d_S.p, d_C.p, want_x ? d_oX.p : nullptr, want_s ? d_oS.p : nullptr, nullptr,
                             rowmap ? nullptr : &lr, rowmap ? d_map.p : nullptr)))
    return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  if ((rc = d_oX.to(outX, (size_t)out_len)) || (rc = d_oS.to(outS, (size_t)out_len))) return rc;
  int T = 1;
  while (T < 64 && T < avg) T <<= 1;                 // launch_spmv_rows' own choice
  info4[0] = T; info4[1] = lr.cap; info4[2] = lr.nlong; info4[3] = lr.nseg;
  return CUADMM_OK;
}

int cuadmm_op_rp_stats(int m, const double* ax, const double* b, const double* normA, const double* y, double bscale, const double* sums2, double* out4) {
  if (m < 1 || !ax || !b || !normA || !y || !sums2 || !out4) { set_error("op_rp_stats: bad arguments"); return CUADMM_ERR_INVALID; }
  int rc;
  HookBuf<double> d_ax, d_b, d_n, d_y, d_sums, d_part, d_out;
  if ((rc = d_ax.from(ax, (size_t)m)) || (rc = d_b.from(b, (size_t)m)) || (rc = d_n.from(normA, (size_t)m)) || (rc = d_y.from(y, (size_t)m)) ||
      (rc = d_sums.from(sums2, 2)) || (rc = d_part.from(nullptr, 128)) || (rc = d_out.from(out4, 4)))
    return rc;
  if ((rc = launch_rp_stats(m, d_ax.p, d_b.p, d_n.p, d_y.p, bscale, d_sums.p, d_part.p, d_out.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  return d_out.to(out4, 4);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// Test hooks only: the fused step's list kernels, the quad sums, the copies and the update passes (tests/test_gpu_step_kernels.py).
// Same rules as above: host pointers, everything checked before a launch, the default stream, synchronised before the return.
// ------------------------------------------------------------------------------------------
namespace {
// n entries, each in [0, len), no entry twice
bool list_ok(long long n, const int* idx, long long len) {
  if (n < 0 || n > len || (n > 0 && !idx)) return false;
  std::vector<unsigned char> seen((size_t)std::max<long long>(len, 1), 0);
  for (long long k = 0; k < n; ++k) {
    if (idx[k] < 0 || idx[k] >= len || seen[(size_t)idx[k]]) return false;
    seen[(size_t)idx[k]] = 1;
  }
  return true;
}
const double kHookNaN = __builtin_nan("");
// `n` doubles of h (may be null: none) followed by `pad` NaNs
std::vector<double> nan_padded(const double* h, size_t n, size_t pad) {
  std::vector<double> v(n + pad, kHookNaN);
  if (h && n) std::copy(h, h + n, v.begin());
  return v;
}
int hook_invalid(const char* who) { set_error("%s: bad arguments", who); return CUADMM_ERR_INVALID; }
}  // namespace

extern "C" {

int cuadmm_op_aty_xb_idx(int64_t L, int m, const int* rp, const int* ci, const double* av, const double* y, const double* C, const double* X, double sig,
                         int64_t nidx, const int* idx, double* Rd1, double* Xb) {
  if (L < 1 || m < 1 || !av || !y || !C || !X || !Rd1 || !Xb || !csr_ok(L, m, rp, ci) || !list_ok(nidx, idx, L)) return hook_invalid("op_aty_xb_idx");
  const size_t nnz = (size_t)rp[L];
  int rc;
  HookBuf<int> d_rp, d_ci, d_idx;
  HookBuf<double> d_av, d_y, d_C, d_X, d_Rd1, d_Xb;
  if ((rc = d_rp.from(rp, (size_t)L + 1)) || (rc = d_ci.from(ci, nnz)) || (rc = d_av.from(av, nnz)) || (rc = d_y.from(y, (size_t)m)) || (rc = d_C.from(C, (size_t)L)) ||
      (rc = d_X.from(X, (size_t)L)) || (rc = d_Rd1.from(Rd1, (size_t)L)) || (rc = d_Xb.from(Xb, (size_t)L)) || (rc = d_idx.from(idx, (size_t)nidx)))
    return rc;
  if ((rc = launch_aty_xb_idx(nidx, d_idx.p, d_rp.p, d_ci.p, d_av.p, d_y.p, d_C.p, d_X.p, sig, d_Rd1.p, d_Xb.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  if ((rc = d_Rd1.to(Rd1, (size_t)L)) || (rc = d_Xb.to(Xb, (size_t)L))) return rc;
  return CUADMM_OK;
}

int cuadmm_op_post_rest(int mode, int64_t L, int64_t nidx, const int* idx, int nfused, const double* fused_pairs, const double* Xproj, const double* Rd1,
                        const double* C, double* X, double* S, double inv_sig, double tau_sig, int use_quads, double* sums2, double* partials_out,
                        int* nparts_out) {
  if (mode < 0 || mode > 1 || L < 1 || nfused < 0 || nfused > (1 << 24) || (nidx == 0 && nfused == 0) || (nfused > 0 && !fused_pairs) || !Xproj || !Rd1 || !C || !X ||
      !S || !sums2 || !partials_out || !nparts_out || !list_ok(nidx, idx, L))
    return hook_invalid("op_post_rest");
  const int grid = nidx > 0 ? post_grid(nidx) : 0;
  const std::vector<double> part = nan_padded(fused_pairs, 2 * (size_t)nfused, 2 * (size_t)grid);
  int rc, nparts = -1;
  HookBuf<int> d_idx;
  HookBuf<double> d_Xp, d_Rd1, d_C, d_X, d_S, d_part, d_sums;
  if ((rc = d_idx.from(idx, (size_t)nidx)) || (rc = d_Xp.from(Xproj, (size_t)L)) || (rc = d_Rd1.from(Rd1, (size_t)L)) || (rc = d_C.from(C, (size_t)L)) ||
      (rc = d_X.from(X, (size_t)L)) || (rc = d_S.from(S, (size_t)L)) || (rc = d_part.from(part.data(), part.size())) || (rc = d_sums.from(sums2, 2)))
    return rc;
  if ((rc = launch_post_rest(mode, nidx, d_idx.p, nfused, d_Xp.p, d_Rd1.p, d_C.p, d_X.p, d_S.p, inv_sig, tau_sig, d_part.p, d_sums.p, nullptr,
                             use_quads ? &nparts : nullptr)))
    return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  if ((rc = d_X.to(X, (size_t)L)) || (rc = d_S.to(S, (size_t)L)) || (rc = d_sums.to(sums2, 2)) || (rc = d_part.to(partials_out, part.size()))) return rc;
  *nparts_out = nparts;
  return CUADMM_OK;
}

int cuadmm_op_reduce_quads(const double* p1, int n1, const double* p2, int n2, int pad_pairs, int with_scratch, double* out4, double* sums2) {
  if (n1 < 0 || n2 < 0 || (n1 > 0 && !p1) || (n2 > 0 && !p2) || pad_pairs < 0 || pad_pairs > 1024 || !out4 || !sums2) return hook_invalid("op_reduce_quads");
  const std::vector<double> h1 = nan_padded(p1, 2 * (size_t)n1, 2 * (size_t)pad_pairs), h2 = nan_padded(p2, 2 * (size_t)n2, 2 * (size_t)pad_pairs);
  const std::vector<double> hs = nan_padded(nullptr, 0, 4 * (size_t)reduce_quads_segments(n1, n2)), ho = nan_padded(nullptr, 0, 6);
  int rc;
  HookBuf<double> d_1, d_2, d_scr, d_out, d_sums;
  if ((rc = d_1.from(h1.data(), h1.size())) || (rc = d_2.from(h2.data(), h2.size())) || (with_scratch && (rc = d_scr.from(hs.data(), hs.size()))) ||
      (rc = d_out.from(ho.data(), 4)) || (rc = d_sums.from(ho.data() + 4, 2)))
    return rc;
  const int rc_launch = launch_reduce_quads(d_1.p, n1, d_2.p, n2, d_out.p, d_sums.p, with_scratch ? d_scr.p : nullptr, nullptr);
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  if ((rc = d_out.to(out4, 4)) || (rc = d_sums.to(sums2, 2))) return rc;      // (a refusal leaves both as they were filled)
  return rc_launch;
}

int cuadmm_op_reduce_quads_batch(const double* p1, const double* p2, int n, int64_t stride, int iters, double* out4) {
  if (!p1 || !p2 || !out4 || n < 0 || stride < 2 || (stride & 1) || stride < 2 * (int64_t)n || stride > ((int64_t)1 << 26) || iters < 1 || iters > 64)
    return hook_invalid("op_reduce_quads_batch");
  const size_t len = (size_t)stride * (size_t)iters, nout = 4 * (size_t)iters + 4;
  int rc;
  HookBuf<double> d_1, d_2, d_out;
  if ((rc = d_1.from(p1, len)) || (rc = d_2.from(p2, len)) || (rc = d_out.from(out4, nout))) return rc;
  if ((rc = launch_reduce_quads_batch(d_1.p, d_2.p, n, stride, iters, d_out.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  return d_out.to(out4, nout);
}

int cuadmm_op_closed_rows(int nslots, const int* nk, const int* rows, int m, const double* ax, const double* as, const double* b, double* cl_out, double* b_out,
                          int64_t* changed_out) {
  if (nslots < 1 || nslots > (1 << 20) || m < 1 || !nk || !rows || !ax || !as || !b || !cl_out || !b_out || !changed_out) return hook_invalid("op_closed_rows");
  for (int s = 0; s < nslots; ++s) {
    if (nk[s] < 1 || nk[s] > kClosedMaxRows) return hook_invalid("op_closed_rows");
    for (int k = 0; k < nk[s]; ++k)
      if (rows[kClosedMaxRows * (size_t)s + k] < 0 || rows[kClosedMaxRows * (size_t)s + k] >= m) return hook_invalid("op_closed_rows");
  }
  std::vector<ClosedRec> up((size_t)nslots), down((size_t)nslots);
  memset(static_cast<void*>(up.data()), 0xA5, sizeof(ClosedRec) * up.size());
  for (int s = 0; s < nslots; ++s) {
    up[s].nk = nk[s];
    for (int k = 0; k < nk[s]; ++k) up[s].rows[k] = rows[kClosedMaxRows * (size_t)s + k];
  }
  int rc;
  HookBuf<ClosedRec> d_rec;
  HookBuf<double> d_ax, d_as, d_b, d_cl;
  if ((rc = d_rec.from(up.data(), up.size())) || (rc = d_ax.from(ax, (size_t)m)) || (rc = d_as.from(as, (size_t)m)) || (rc = d_b.from(b, (size_t)m)) ||
      (rc = d_cl.from(cl_out, 16 * (size_t)nslots)))
    return rc;
  if ((rc = launch_closed_gather_out(d_rec.p, nslots, d_ax.p, d_as.p, d_cl.p, nullptr)) || (rc = launch_closed_patch_b(d_rec.p, nslots, d_b.p, nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  if ((rc = d_cl.to(cl_out, 16 * (size_t)nslots)) || (rc = d_rec.to(down.data(), down.size()))) return rc;
  int64_t changed = 0;
  for (int s = 0; s < nslots; ++s) {
    const unsigned char* u = reinterpret_cast<const unsigned char*>(&up[s]);
    const unsigned char* d = reinterpret_cast<const unsigned char*>(&down[s]);
    const size_t b0 = offsetof(ClosedRec, b), b1 = b0 + sizeof(double) * (size_t)nk[s];
    for (size_t q = 0; q < sizeof(ClosedRec); ++q)
      if ((q < b0 || q >= b1) && u[q] != d[q]) ++changed;
    memcpy(b_out + kClosedMaxRows * (size_t)s, down[s].b, sizeof(double) * kClosedMaxRows);
  }
  *changed_out = changed;
  return CUADMM_OK;
}

int cuadmm_op_copy(const double* src, int64_t n, double* dst) {
  if (n < 1 || n > ((int64_t)1 << 28) || !src || !dst) return hook_invalid("op_copy");
  int rc;
  HookBuf<double> d_src, d_dst;
  if ((rc = d_src.from(src, (size_t)n)) || (rc = d_dst.from(dst, (size_t)n + 4))) return rc;
  if ((rc = launch_copy(d_dst.p, d_src.p, n, nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  return d_dst.to(dst, (size_t)n + 4);
}

int cuadmm_op_copy_multi(int count, const int64_t* nbytes, const void* const* src, void* const* dst) {
  if (count < 1 || count > 6 || !nbytes || !src || !dst) return hook_invalid("op_copy_multi");
  for (int q = 0; q < count; ++q)
    if (nbytes[q] < 0 || nbytes[q] > ((int64_t)1 << 30) || (nbytes[q] > 0 && !src[q]) || !dst[q]) return hook_invalid("op_copy_multi");
  int rc;
  HookBuf<unsigned char> d_src[6], d_dst[6];
  CopyJobs jobs{};
  jobs.count = count;
  for (int q = 0; q < count; ++q) {
    if ((rc = d_src[q].from(static_cast<const unsigned char*>(src[q]), (size_t)nbytes[q])) ||
        (rc = d_dst[q].from(static_cast<const unsigned char*>(dst[q]), (size_t)nbytes[q] + 32)))
      return rc;
    jobs.dst[q] = d_dst[q].p; jobs.src[q] = d_src[q].p; jobs.nbytes[q] = nbytes[q];
  }
  if ((rc = launch_copy_multi(jobs, nullptr))) return rc;                    // (a length that is no multiple of 4 is refused there, before the launch)
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  for (int q = 0; q < count; ++q)
    if ((rc = d_dst[q].to(static_cast<unsigned char*>(dst[q]), (size_t)nbytes[q] + 32))) return rc;
  return CUADMM_OK;
}

int cuadmm_op_scale(double* v, int64_t n, double s) {
  if (n < 1 || n > ((int64_t)1 << 28) || !v) return hook_invalid("op_scale");
  int rc;
  HookBuf<double> d_v;
  if ((rc = d_v.from(v, (size_t)n + 4))) return rc;
  if ((rc = launch_scale(d_v.p, n, s, nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  return d_v.to(v, (size_t)n + 4);
}

int cuadmm_op_update_svec(int64_t n, double* X, double* S, double* C, int zero, double x1, double x2, double s1, double s2) {
  if (n < 1 || n > ((int64_t)1 << 28) || !X || !S) return hook_invalid("op_update_svec");
  int rc;
  HookBuf<double> d_X, d_S, d_C;
  if ((rc = d_X.from(X, (size_t)n + 2)) || (rc = d_S.from(S, (size_t)n + 2)) || (C && (rc = d_C.from(C, (size_t)n + 2)))) return rc;
  if ((rc = launch_update_svec(d_X.p, d_S.p, C ? d_C.p : nullptr, n, zero != 0, x1, x2, s1, s2, nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  if ((rc = d_X.to(X, (size_t)n + 2)) || (rc = d_S.to(S, (size_t)n + 2)) || (C && (rc = d_C.to(C, (size_t)n + 2)))) return rc;
  return CUADMM_OK;
}

int cuadmm_op_update_cons(int m, double* b, double* y, const double* normA, int ymode, double cs_old, double ics_new) {
  if (m < 1 || ymode < 0 || ymode > 2 || (ymode != 0 && !y) || (ymode == 2 && !normA)) return hook_invalid("op_update_cons");
  int rc;
  HookBuf<double> d_b, d_y, d_n;
  if ((b && (rc = d_b.from(b, (size_t)m + 2))) || (y && (rc = d_y.from(y, (size_t)m + 2))) || (normA && (rc = d_n.from(normA, (size_t)m)))) return rc;
  if ((rc = launch_update_cons(m, b ? d_b.p : nullptr, y ? d_y.p : nullptr, normA ? d_n.p : nullptr, ymode, cs_old, ics_new, nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  if ((b && (rc = d_b.to(b, (size_t)m + 2))) || (y && (rc = d_y.to(y, (size_t)m + 2)))) return rc;
  return CUADMM_OK;
}

int cuadmm_op_scatter_scaled(int len, double* dst, int n, const int* idx, const double* val, double s) {
  if (len < 1 || !dst || (n > 0 && !val) || !list_ok(n, idx, len)) return hook_invalid("op_scatter_scaled");
  int rc;
  HookBuf<int> d_idx;
  HookBuf<double> d_dst, d_val;
  if ((rc = d_dst.from(dst, (size_t)len)) || (rc = d_idx.from(idx, (size_t)n)) || (rc = d_val.from(val, (size_t)n))) return rc;
  if ((rc = launch_scatter_scaled(d_dst.p, d_idx.p, d_val.p, n, s, nullptr))) return rc;
  CUADMM_HIP_TRY(hipStreamSynchronize(nullptr));
  return d_dst.to(dst, (size_t)len);
}

}  // extern "C"
