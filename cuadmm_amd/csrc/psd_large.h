// PSD projection of blocks with n > 64 through the matrix sign function on the fp64 matrix cores (psd_large.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "psd_options.h"

namespace cuadmm {

struct ClusterMulti;

struct SignPsd {
  // pred: steps the previous projection needed.  mem_off: the group's own range of members in d_state / d_done / d_bar / scale (every
  // group one, in group order).  merged: the group runs its whole sign iteration in ONE launch shared with the other merged groups
  // (lg_sign_cluster_kernel over several padded sizes), so it has a workspace of its own too (ws_off: elements into X0 / S / Y / T;
  // part_off: into each half of d_part; slot: which [2] of d_group and which table of d_xcc); the others run on the caller's stream one
  // after the other and share the workspace at offset 0
  struct Group { int N = 0, begin = 0, count = 0, pred = 0, mem_off = 0, slot = 0; bool merged = false; size_t ws_off = 0, part_off = 0, cs_off = 0;
                 mutable int bar_par = 0; };      // cs_off: into colsum_f; bar_par: which of the group's two barrier-counter sets the next fused projection uses
  PsdOptions opt;                            // the owner's switches (PsdPlan::build copies its own)
  std::vector<Group> groups;                 // same padded size N, bounded workspace
  int* d_ids = nullptr;                      // block ids, group after group
  int* d_steps = nullptr;                    // not owned; when set: Newton-Schulz steps taken per block
  int* d_hint = nullptr;                     // not owned; schedule warm start per block (lift steps of the previous projection)
  int hint_max_n = 512;                      // ... for the groups padded to at most this size: mid-size blocks gain (PlanarHand_N=10's 81 blocks of
                                             // 66 ... 120: projection 1.03 -> 0.98 ms, taha1a 1.08 -> 1.02), one n = 2 000 block loses a step (C3 17 -> 18).
                                             // A property of the group, not of the path: launches and one-launch kernel stay bit-identical
  double *X0 = nullptr, *S = nullptr, *Y = nullptr, *T = nullptr, *colsum = nullptr, *scale = nullptr;
  double* colsum_f = nullptr;                // fused one-launch prologue: [group][member][LG_CS_ROWS][N] column-sum chunks (every group its own: merged groups run together)
  void* d_state = nullptr;                   // 2 x SignDevState per member (adaptive schedule, sign_sched.h)
  void* d_done = nullptr;                    // SignDone per member
  double* d_part = nullptr;                  // per-tile partial sums of the schedule statistics (p1 | p2)
  size_t part_half = 0;
  int* d_group = nullptr;                    // [members not finished, largest step count] of the group in flight
  int* h_group = nullptr;                    // pinned host copy (polled between chunks of steps)
  unsigned* d_bar = nullptr;                 // per member, two sets (members_cap apart): barrier counter of the one-launch variant.  A fused group
                                             // alternates between its two sets and zeroes the other one for its next projection; a run that is
                                             // not fused counts in set 0 and zeroes it at its start
  size_t bar_stride = 0;                     // members_cap (all groups' counts): distance between the two counter sets
  int* d_xcc = nullptr;                      // [member][tile]: XCD of every workgroup of the one-launch variant (run-time check)
  // what build() allocates, as build_host() worked it out
  struct Sizes { size_t elems = 1, members_cap = 1, max_cols = 1, cs_total = 1; int n_merged = 0; };
  // the part of build() that needs no device: the groups (padding, the psd_lg_pad32 shrink, chunks of psd_sign_ws_mb, which of them share
  // one launch, every offset), the members group after group, and the sizes of the buffers
  void build_host(const int* blk, const std::vector<int>& members, std::vector<int>& ids, Sizes& sz);
  int build(const int* blk, const std::vector<int>& members);
  // test hook (cuadmm_psd_sign_groups): N, count, merged, slot, tile, ntiles, decide_kernel, cluster, spread, cluster_wgs, superblock, fused --
  // from the functions the launches themselves ask
  static constexpr int kGroupInfo = 12;
  void group_info(const Group& g, int* out) const;
  int launch_group(Group& g, const double* in, double* out, const long long* boff, const int* bn, int* d_fail, hipStream_t st, bool poll);
  void cluster_add(ClusterMulti& cm, const Group& g, int* d_fail, int max_steps) const;     // appends g to a one-launch set
  int cluster_run(ClusterMulti& cm, bool prologue, const double* in, double* out, const long long* boff, const int* bn, int* d_fail, hipStream_t st);
  void release();
  int project(const double* in, double* out, const long long* boff, const int* bn, int* d_fail, hipStream_t st);
  bool empty() const { return groups.empty(); }
  ~SignPsd() { release(); }
};

// C = alpha * A*B + beta * E, n x n row-major, A symmetric, n a multiple of 64 (E may be null)
int large_gemm_sym(int N, const double* A, const double* B, double alpha, double beta, const double* E, double* C, hipStream_t st);

}  // namespace cuadmm
