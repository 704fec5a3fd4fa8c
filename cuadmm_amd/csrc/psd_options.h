// Switches of the projection planner and its kernels.  ONE INSTANCE PER PLAN (PsdPlan::opt): two solvers in a process can
// choose differently, and every variant is reachable by a test through cuadmm_set_option (keys "psd_*").  Nothing here is
// cached process-wide; from_env() gives the defaults and reads the developer-aid variables.  The keys, their environment variables and
// their clamps are the rows of psd_option_table() below.
// PsdPlan::build() resolves every option that selects a kernel or an instantiation into the plan's launch table (psd_plan.h) and
// into SignPsd::opt: set on a built plan, such an option is kept for the plans built afterwards and changes nothing in this one.
// Only psd_overlap and psd_debug are read at every projection.
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>

#include "option_table.h"

namespace cuadmm {

struct PsdOptions {
  int n16_sign = 1;        // psd_n16: 9 <= n <= 16 on the one-wavefront sign kernel (0: register eigensolver)
  int n32_sign = 1;        // psd_n32: 17 <= n <= 32 likewise
  int mid = 0;             // psd_mid: 33 <= n <= 64: 0 = by count (psd_wave4_min), 1 = register eigensolver, 2 = one workgroup per block
  int wave4_min = 1024;    // psd_wave4_min: blocks of a 33 <= n <= 64 class from which one wavefront per block wins over one workgroup
  int w32_occ = 4;         // psd_w32_occ: wavefronts per SIMD of the n <= 32 one-wavefront kernels (3 | 4)
  int cu_occ = 4;          // psd_cu_occ: the same for the launches that run several iterations (psd_sign_closed_cu_kernel)
  int lds_triple = 1;      // psd_lds_triple: one-workgroup kernels of 33 <= n <= 64 with a third LDS matrix when the class has <= 256 blocks
  int sign_min = 65;       // psd_sign_min: blocks from this size on take the batched-GEMM matrix-sign path
  int overlap = 1;         // psd_overlap: size classes on their own streams
  // batched-GEMM path (psd_large.hip)
  int lg_tile = 0;         // psd_lg_tile: 0 = by size, 32 | 64 forces the tile
  int lg_pad32 = 1;        // psd_lg_pad32: groups on 32 x 32 tiles pad to a multiple of 32
  int lg_decide = 0;       // psd_lg_decide: 0 = by tile count, 1 = decisions inside the product kernels, 2 = a separate kernel
  int lg_merge = 1;        // psd_lg_merge: one-launch groups of different padded sizes share ONE launch (workspaces of their own)
  int lg_fuse = 1;         // psd_lg_fuse: the one-launch kernel does its own prologue (svec -> X0, column sums, S, state) and epilogue (svec store): one launch instead of three
  int lg_cluster_wgs = 224;  // psd_lg_cluster_wgs: the largest grid the one-launch sign kernel takes (its workgroups must be co-resident: three of them fit a CU, 119 VGPRs + 16 AGPRs)
  int lg_cluster = 1;      // psd_lg_cluster: a handful of mid-size blocks run their whole sign iteration in one launch (per-member barriers)
  int sign_maxsteps = 0;   // psd_sign_maxsteps: cap of the schedule (0: SignSched::kCap)
  int sign_sync = 1;       // psd_sign_sync: poll "members not finished" between chunks of steps
  int sign_ws_mb = 8192;   // psd_sign_ws_mb: workspace bound of a group
  int debug = 0;           // developer aid: CUADMM_PSD_DEBUG (phase ticks of the kernels on stderr; serialises the classes)

  // the defaults: each option's environment variable (round 1 / 2 names) is consulted ONCE here, per plan -- never cached -- and
  // goes through set() like a value from cuadmm_set_option
  static PsdOptions from_env();
  // false when the key is not one of this struct's or the value is refused; *why (optional): kOptOk for an unknown key, else the refusal
  bool set(const std::string& k, double value, OptCheck* why = nullptr);
};

// The table of the keys (option_table.h: adding an option is adding its row and its field), in the order INTEGRATION.md section 6 lists them.
inline OptionTable<PsdOptions> psd_option_table() {
  using O = OptionSpec<PsdOptions>;
#define F(member) CUADMM_OPT_FIELD(PsdOptions, member)
  static const O rows[] = {
      O("psd_n16", F(n16_sign), kOptInt, 1, "9 <= n <= 16 on the one-wavefront sign kernel (0: register eigensolver)").from_env("CUADMM_PSD_N16", kEnvEig0).read(kAtPlanBuild),
      O("psd_n32", F(n32_sign), kOptInt, 1, "17 <= n <= 32 likewise").from_env("CUADMM_PSD_N32", kEnvEig0).read(kAtPlanBuild),
      O("psd_mid", F(mid), kOptInt, 0, "33 <= n <= 64: 0 by count, 1 register eigensolver, 2 one workgroup per block").from_env("CUADMM_PSD_MID", kEnvEig1).read(kAtPlanBuild),
      O("psd_wave4_min", F(wave4_min), kOptInt, 1024, "blocks of a 33 <= n <= 64 class from which one wavefront per block wins").from_env("CUADMM_PSD_WAVE4_MIN").read(kAtPlanBuild),
      O("psd_sign_min", F(sign_min), kOptInt, 65, "blocks from this size on take the batched-GEMM matrix-sign path").from_env("CUADMM_PSD_SIGN_MIN").at_least(65).read(kAtPlanBuild),
      O("psd_lds_triple", F(lds_triple), kOptInt, 1, "one-workgroup kernels of 33 <= n <= 64 with a third LDS matrix (classes of <= 256 blocks)").from_env("CUADMM_PSD_LDS_TRIPLE").read(kAtPlanBuild),
      O("psd_w32_occ", F(w32_occ), kOptInt, 4, "wavefronts per SIMD of the n <= 32 one-wavefront kernels (3 | 4)").from_env("CUADMM_PSD_W32_OCC").normalised(kNorm3or4).read(kAtPlanBuild),
      O("psd_cu_occ", F(cu_occ), kOptInt, 4, "the same for the launches that run several iterations").from_env("CUADMM_PSD_CU_OCC").normalised(kNorm3or4).read(kAtPlanBuild),
      O("psd_overlap", F(overlap), kOptInt, 1, "size classes on their own streams").from_env("CUADMM_PSD_OVERLAP").read(kLive),
      O("psd_lg_tile", F(lg_tile), kOptInt, 0, "sign path: 0 = tile by size, 32 | 64 forces it").read(kAtPlanBuild),
      O("psd_lg_pad32", F(lg_pad32), kOptInt, 1, "sign path: groups on 32 x 32 tiles pad to a multiple of 32").read(kAtPlanBuild),
      O("psd_lg_decide", F(lg_decide), kOptInt, 0, "sign path: 0 by tile count, 1 decisions inside the product kernels, 2 a separate kernel").read(kAtPlanBuild),
      O("psd_lg_cluster", F(lg_cluster), kOptInt, 1, "sign path: a handful of mid-size blocks run their whole iteration in one launch").from_env("CUADMM_PSD_LG_CLUSTER").read(kAtPlanBuild),
      O("psd_lg_merge", F(lg_merge), kOptInt, 1, "sign path: one-launch groups of different padded sizes share one launch").from_env("CUADMM_PSD_LG_MERGE").read(kAtPlanBuild),
      O("psd_sign_sync", F(sign_sync), kOptInt, 1, "sign path: poll \"members not finished\" between chunks of steps").read(kAtPlanBuild),
      O("psd_sign_maxsteps", F(sign_maxsteps), kOptInt, 0, "sign path: cap of the schedule (0: SignSched::kCap)").read(kAtPlanBuild),
      O("psd_sign_ws_mb", F(sign_ws_mb), kOptInt, 8192, "sign path: workspace bound of a group").at_least(1).read(kAtPlanBuild),
      O("psd_lg_cluster_wgs", F(lg_cluster_wgs), kOptInt, 224, "sign path: the largest grid the one-launch kernel takes").from_env("CUADMM_PSD_LG_CLUSTER_WGS").clamp(8, 960).read(kAtPlanBuild),
      O("psd_lg_fuse", F(lg_fuse), kOptInt, 1, "sign path: the one-launch kernel does its own prologue and epilogue").from_env("CUADMM_PSD_LG_FUSE").read(kAtPlanBuild),
      O("psd_debug", F(debug), kOptInt, 0, "developer aid: phase ticks of the kernels on stderr; serialises the classes").from_env("CUADMM_PSD_DEBUG").at_least(0).read(kLive),
  };
#undef F
  return {rows, (int)(sizeof(rows) / sizeof(rows[0]))};
}
inline PsdOptions PsdOptions::from_env() {
  PsdOptions o;
  options_from_env(psd_option_table(), o);
  return o;
}
inline bool PsdOptions::set(const std::string& k, double value, OptCheck* why) {
  const OptionSpec<PsdOptions>* o = psd_option_table().find(k.c_str());
  const OptCheck c = o ? option_store(*o, *this, value) : kOptOk;
  if (why) *why = c;
  return o && c == kOptOk;
}

}  // namespace cuadmm
