// W_k = M_k V_k per block on the fp64 matrix cores, M_k read as it lies in an svec vector: block_mult.h has the task list and the
// rounding contract, factor_layout.h the layout of V and W, DESIGN.md, "Blocks times factors", the sizes and what was measured.
//
// One wavefront owns 16 rows of W.  v_mfma_f64_16x16x4_f64: lane l feeds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] and holds
// D[row = (l >> 4) + 4 reg][col = l & 15].  A is the panel's 16 x 4 piece of M (raw slots, the diagonal lane 0.0), B the 4 x 16 piece of V.
// For k < i the four lanes of a row read 32 consecutive bytes of its packed row, for k > i the 16 lanes of a k read 128 consecutive bytes
// of row k.  No LDS, no barrier, nothing waits on another wavefront; the loops are bounded by n and r.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "block_mult.h"
#include "factor_layout.h"
#include "device_util.h"

namespace cuadmm {
namespace {

typedef double bm_v4f64 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void block_mult_kernel(const BmTask* __restrict__ tasks, const double* __restrict__ v, double sign, const double* __restrict__ V,
                                                         double* __restrict__ W, const long long* __restrict__ loff, const int* __restrict__ ranks,
                                                         const long long* __restrict__ off, const int* __restrict__ blk) {
  const int lane = (int)threadIdx.x & 63;
  const BmTask t = tasks[blockIdx.x * 4 + ((int)threadIdx.x >> 6)];
  if (t.k < 0) return;
  const int n = blk[t.k], r = ranks[t.k];
  if (n <= 0 || r <= 0) return;              // (the host lists PSD blocks only; r = 0 writes nothing)
  const double* x = v + off[t.k];
  const double* Vk = V + loff[t.k];          // column c at Vk + c n
  double* Wk = W + loff[t.k];
  const int l16 = lane & 15, kk = lane >> 4;
  const int i = kBmPanel * t.p + l16;        // the row of M this lane feeds
  const long long rowi = (long long)i * (i + 1) / 2;
  for (int c0 = 0; c0 < r; c0 += kBmPanel * kBmGroups) {      // wave-uniform trip counts throughout
    bm_v4f64 acc[kBmGroups];
#pragma unroll
    for (int g = 0; g < kBmGroups; ++g) acc[g] = bm_v4f64{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < n; k0 += 4) {
      const int j = k0 + kk;
      double a = 0.0;
      if (i < n && j < n && j != i) a = j < i ? x[rowi + j] : x[(long long)j * (j + 1) / 2 + i];
#pragma unroll
      for (int g = 0; g < kBmGroups; ++g) {
        const int c = c0 + kBmPanel * g;
        if (c < r) {
          const int col = c + l16;
          const double b = (j < n && col < r) ? Vk[(size_t)col * n + j] : 0.0;
          acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[g], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < kBmGroups; ++g) {
      const int col = c0 + kBmPanel * g + l16;
      if (col >= r) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = kBmPanel * t.p + kk + 4 * q;
        if (row < n) {
          const size_t e = (size_t)col * n + row;
          const double diag = __dmul_rn(x[(long long)row * (row + 1) / 2 + row], Vk[e]);
          Wk[e] = sign * __fma_rn(kInvSqrt2, acc[g][q], diag);
        }
      }
    }
  }
}

}  // namespace

int bm_build_tasks(int nblk, const int* blk, int rmax, std::vector<BmTask>* tasks, std::vector<long long>* loff) {
  std::vector<long long> own;
  if (!tasks) { set_error("block_mult: invalid argument"); return CUADMM_ERR_INVALID; }
  int rc = factor_offsets("block_mult", nblk, blk, rmax, loff ? loff : &own);
  if (rc) return rc;
  tasks->clear();
  std::vector<int> big;
  for (int k = 0; k < nblk; ++k)
    if (blk[k] > kBmPanel) big.push_back(k);
  std::stable_sort(big.begin(), big.end(), [&](int a, int b) { return blk[a] > blk[b]; });
  for (int k : big) {
    for (int p = 0, P = bm_panels(blk[k]); p < P; ++p) tasks->push_back(BmTask{k, p});
    while (tasks->size() % 4) tasks->push_back(BmTask{-1, 0});
  }
  for (int k = 0; k < nblk; ++k)
    if (blk[k] > 0 && blk[k] <= kBmPanel) tasks->push_back(BmTask{k, 0});
  while (tasks->size() % 4) tasks->push_back(BmTask{-1, 0});
  return CUADMM_OK;
}

int launch_block_mult(int nslots, const BmTask* tasks, const double* v, double sign, const double* V, double* W, const long long* loff, const int* ranks,
                      const long long* off, const int* blk, hipStream_t st) {
  if (nslots < 0 || nslots % 4 || (nslots > 0 && (!tasks || !v || !V || !W || !loff || !ranks || !off || !blk))) {
    set_error("block_mult: invalid argument");
    return CUADMM_ERR_INVALID;
  }
  if (nslots == 0) return CUADMM_OK;
  hipLaunchKernelGGL(block_mult_kernel, dim3((unsigned)(nslots / 4)), dim3(256), 0, st, tasks, v, sign, V, W, loff, ranks, off, blk);
  CUADMM_HIP_TRY(hipGetLastError());
  return CUADMM_OK;
}

}  // namespace cuadmm
