// Wave-wide deterministic sums on the DPP crossbar (shared by the matrix-sign kernels).
#pragma once
#include <hip/hip_runtime.h>

namespace cuadmm {

// ---------------------------------------------------------------------------------------------------------------
// Wave-wide sums for the schedule statistics (sign_sched.h): xor-butterfly inside each row of 16 lanes on the DPP
// crossbar (quad_perm, row_half_mirror, row_mirror -- no LDS traffic, fixed association order, so every lane of a row
// holds bit-identical sums), then the four row sums through v_readlane.  The result is wave-uniform (SGPR operands),
// so the schedule's branches are scalar.
// ---------------------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double sw_dpp(double v) {
  // bound_ctrl: every lane has a valid source under these controls, and the destination needs no initialisation (without it the
  // compiler zeroes both halves first: two v_mov per step -- VALU slots the fp64 matrix pipe pays for)
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double sw_readlane(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double wave_sum(double v) {
  v += sw_dpp<0xB1>(v);    // quad_perm [1,0,3,2]
  v += sw_dpp<0x4E>(v);    // quad_perm [2,3,0,1]
  v += sw_dpp<0x141>(v);   // row_half_mirror
  v += sw_dpp<0x140>(v);   // row_mirror
  return (sw_readlane(v, 0) + sw_readlane(v, 16)) + (sw_readlane(v, 32) + sw_readlane(v, 48));
}

// ---------------------------------------------------------------------------------------------------------------
// The pieces of wave_sum for the per-block reductions (block_reduce.h): a row of 16 lanes or the
// wavefront owns a block, a workgroup of 256 threads a chunk of a long one.
// ---------------------------------------------------------------------------------------------------------------
// the sum over each row of 16 lanes, in every lane of the row (the first four steps of wave_sum)
__device__ __forceinline__ double row_sum(double v) {
  v += sw_dpp<0xB1>(v);
  v += sw_dpp<0x4E>(v);
  v += sw_dpp<0x141>(v);
  v += sw_dpp<0x140>(v);
  return v;
}
__device__ __forceinline__ double rows_to_wave(double v) {
  return (sw_readlane(v, 0) + sw_readlane(v, 16)) + (sw_readlane(v, 32) + sw_readlane(v, 48));
}
// sum over a workgroup of 256 threads in a fixed order; valid in every thread
__device__ __forceinline__ double block_sum(double v, double* lds /* 4 doubles */) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[w] = v;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// second stage of the stream kernels' reductions (accel.hip, infeas.hip): with STRIDE partial sums per slot, workgroup q (one
// wavefront) adds partials[slot * STRIDE + q] over the slots, lane l the slots l, l + 64, ...
template <int STRIDE>
__global__ __launch_bounds__(64) void slots_final_kernel(const double* partials, int nslots, double* out) {
  const int q = blockIdx.x;
  double v = 0;
  for (int s = threadIdx.x; s < nslots; s += 64) v += partials[(size_t)s * STRIDE + q];
  v = wave_sum(v);
  if (threadIdx.x == 0) out[q] = v;
}

}  // namespace cuadmm
