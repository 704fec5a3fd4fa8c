// The quartic along a line in factor space (cuadmm_lowrank_line): svec of L L', L D' + D L' and D D' per block in one pass on the fp64
// matrix cores, the streaming pass behind the three A x, and the per-block objective terms.  lowrank_line.h has the formulas and the
// contracts; DESIGN.md, "Line search along factor steps", the chain they stand in.
//
// The outer products keep the lane layout of lowrank_apply.hip.  v_mfma_f64_16x16x4_f64: lane l feeds A[i = l & 15][k = l >> 4] and
// B[k = l >> 4][j = l & 15] and holds D[row = (l >> 4) + 4 reg][col = l & 15], so a register is four rows of 16 consecutive svec slots.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lowrank_line.h"
#include "device_util.h"
#include "wave_reduce.h"

namespace cuadmm {
namespace {

typedef double ll_v4f64 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void block_outer3_kernel(const LoTask* __restrict__ tasks, const double* __restrict__ L, const double* __restrict__ D,
                                                           const long long* __restrict__ loff, const int* __restrict__ ranks, const long long* __restrict__ off,
                                                           const int* __restrict__ blk, double* __restrict__ v0, double* __restrict__ v1,
                                                           double* __restrict__ v2) {
  const int lane = (int)threadIdx.x & 63;
  const LoTask t = tasks[blockIdx.x * 4 + ((int)threadIdx.x >> 6)];
  if (t.k < 0) return;
  const int n = blk[t.k], r = ranks[t.k];
  if (n <= 0) return;                        // (the host lists PSD blocks only)
  const double* Lk = L + loff[t.k];          // column c at Lk + c n
  const double* Dk = D + loff[t.k];
  const long long o = off[t.k];
  const int r16 = lane & 15, kk = lane >> 4;
  for (int tile = t.t0; tile < t.t1; tile += t.step) {
    const int ti = lo_tile_row(tile), tj = tile - ti * (ti + 1) / 2;
    const int ia = kLoTile * ti + r16, ib = kLoTile * tj + r16;
    ll_v4f64 acc0 = ll_v4f64{0.0, 0.0, 0.0, 0.0}, acc1 = acc0, acc2 = acc0;
    for (int k0 = 0; k0 < r; k0 += 4) {      // wave-uniform trip count
      const int k = k0 + kk;
      const bool ua = k < r && ia < n, ub = k < r && ib < n;
      const double la = ua ? Lk[(size_t)k * n + ia] : 0.0;
      const double lb = ub ? Lk[(size_t)k * n + ib] : 0.0;
      const double da = ua ? Dk[(size_t)k * n + ia] : 0.0;
      const double db = ub ? Dk[(size_t)k * n + ib] : 0.0;
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(la, lb, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(la, db, acc1, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(da, lb, acc1, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(da, db, acc2, 0, 0, 0);
    }
    const int col = ib;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = kLoTile * ti + kk + 4 * q;
      if (row < n && col <= row) {
        const long long at = o + (long long)row * (row + 1) / 2 + col;
        v0[at] = col == row ? acc0[q] : acc0[q] * kLoSqrt2;
        v1[at] = col == row ? acc1[q] : acc1[q] * kLoSqrt2;
        v2[at] = col == row ? acc2[q] : acc2[q] * kLoSqrt2;
      }
    }
  }
}

struct LlCoef { double xunit, bscale; };

// one constraint: every operation rounded once, nothing contracted
__device__ __forceinline__ void ll_one(const LlCoef& c, double a0, double a1, double a2, double b, double na, double y, double& r0, double& p, double& q,
                                       double (&s)[kLlParts]) {
  const double rs = __dsub_rn(__dmul_rn(c.xunit, a0), b), ps = __dmul_rn(c.xunit, a1), qs = __dmul_rn(c.xunit, a2);
  r0 = __dmul_rn(__dmul_rn(na, rs), c.bscale);
  p = __dmul_rn(__dmul_rn(na, ps), c.bscale);
  q = __dmul_rn(__dmul_rn(na, qs), c.bscale);
  s[0] = __dadd_rn(s[0], __dmul_rn(y, rs));
  s[1] = __dadd_rn(s[1], __dmul_rn(y, ps));
  s[2] = __dadd_rn(s[2], __dmul_rn(y, qs));
  s[3] = __dadd_rn(s[3], __dmul_rn(r0, r0));
  s[4] = __dadd_rn(s[4], __dmul_rn(r0, p));
  s[5] = __dadd_rn(s[5], __dmul_rn(p, p));
  s[6] = __dadd_rn(s[6], __dmul_rn(r0, q));
  s[7] = __dadd_rn(s[7], __dmul_rn(p, q));
  s[8] = __dadd_rn(s[8], __dmul_rn(q, q));
}

// index i: constraint i (kVec = false) or the constraints 2 i, 2 i + 1 (kVec = true; the last index may hold one)
template <bool kVec>
struct LlSums {
  const double *ax0, *ax1, *ax2, *b, *normA, *y;
  double *r0, *p, *q;
  long long m;
  LlCoef c;
  __device__ __forceinline__ void add(double (&s)[kLlParts], long long i) const {
    if (kVec && 2 * i + 1 < m) {
      const double2 a0 = reinterpret_cast<const double2*>(ax0)[i], a1 = reinterpret_cast<const double2*>(ax1)[i], a2 = reinterpret_cast<const double2*>(ax2)[i];
      const double2 b2 = reinterpret_cast<const double2*>(b)[i], n2 = reinterpret_cast<const double2*>(normA)[i], y2 = reinterpret_cast<const double2*>(y)[i];
      double2 rr, pp, qq;
      ll_one(c, a0.x, a1.x, a2.x, b2.x, n2.x, y2.x, rr.x, pp.x, qq.x, s);
      ll_one(c, a0.y, a1.y, a2.y, b2.y, n2.y, y2.y, rr.y, pp.y, qq.y, s);
      reinterpret_cast<double2*>(r0)[i] = rr;
      reinterpret_cast<double2*>(p)[i] = pp;
      reinterpret_cast<double2*>(q)[i] = qq;
      return;
    }
    const long long e = kVec ? 2 * i : i;      // (kVec: the odd last constraint; e < m by the launcher's count)
    double rr, pp, qq;
    ll_one(c, ax0[e], ax1[e], ax2[e], b[e], normA[e], y[e], rr, pp, qq, s);
    r0[e] = rr;
    p[e] = pp;
    q[e] = qq;
  }
};

struct LlBlockTerms {
  static constexpr int V = 4, N = kLlSums;
  static constexpr bool kFlag = false;
  static constexpr const char* kName = "lrl_block_terms";
  const double* p[V];      // C, x0, x1, x2
  __device__ __forceinline__ void add(double (&a)[N], const double (&v)[V], bool) const {
    a[0] += v[0] * v[1];
    a[1] += v[0] * v[2];
    a[2] += v[0] * v[3];
  }
};

}  // namespace

int launch_block_outer3(int nslots, const LoTask* tasks, const double* L, const double* D, const long long* loff, const int* ranks, const long long* off,
                        const int* blk, double* x0, double* x1, double* x2, hipStream_t st) {
  if (nslots < 0 || nslots % 4 || (nslots > 0 && (!tasks || !L || !D || !loff || !ranks || !off || !blk || !x0 || !x1 || !x2)) || (x0 && (x0 == x1 || x0 == x2)) ||
      (x1 && x1 == x2)) {
    set_error("block_outer3: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  if (nslots == 0) return CUADMM_OK;
  hipLaunchKernelGGL(block_outer3_kernel, dim3((unsigned)(nslots / 4)), dim3(256), 0, st, tasks, L, D, loff, ranks, off, blk, x0, x1, x2);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

int launch_lrl_sums(int m, const double* ax0, const double* ax1, const double* ax2, const double* b, const double* normA, const double* y, double xunit,
                    double bscale, double* r0, double* p, double* q, double* partials, hipStream_t st) {
  if (m < 0 || (m > 0 && (!ax0 || !ax1 || !ax2 || !b || !normA || !y || !r0 || !p || !q)) || !partials) { set_error("lrl_sums: invalid argument"); return CUADMM_ERR_INVALID; }
  uintptr_t bits = 0;
  for (const void* v : {(const void*)ax0, (const void*)ax1, (const void*)ax2, (const void*)b, (const void*)normA, (const void*)y, (const void*)r0, (const void*)p,
                        (const void*)q})
    bits |= reinterpret_cast<uintptr_t>(v);
  const LlCoef c{xunit, bscale};
  if ((bits & 15) == 0) return launch_slot_partials<kLlParts>(((long long)m + 1) / 2, LlSums<true>{ax0, ax1, ax2, b, normA, y, r0, p, q, m, c}, partials, st);
  return launch_slot_partials<kLlParts>((long long)m, LlSums<false>{ax0, ax1, ax2, b, normA, y, r0, p, q, m, c}, partials, st);
}

int launch_lrl_block_terms(const double* C, const double* x0, const double* x1, const double* x2, const BlockTasksView& t, double* cpart, double* sums,
                           hipStream_t st) {
  return launch_block_reduce(LlBlockTerms{{C, x0, x1, x2}}, t, cpart, sums, st);
}

}  // namespace cuadmm
