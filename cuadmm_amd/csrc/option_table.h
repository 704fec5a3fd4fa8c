// The options of cuadmm_set_option as DATA: one row per key with its environment variable, default, kind, normalisation, validity rule,
// when it is read, what an in-process group does with it, and a one-line description.  Two tables are built from the row type: the
// engine's (below; its fields live in struct cuadmm_solver) and the projection planner's (psd_options.h; struct PsdOptions).
// ADDING AN OPTION IS ADDING ONE ROW (and its field): cuadmm_set_option, cuadmm_get_option, cuadmm_option_info, the environment
// defaults and the group's forwarding and replay all walk the tables.  DESIGN.md, "The option tables".
// Host only, no HIP include: plain g++ compiles it (tests/option_table_selftest.cpp runs every row under ASan + UBSan).
#pragma once
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace cuadmm {

enum OptKind { kOptInt, kOptLong, kOptReal };      // int: truncated toward zero, as (int)value; long: the same into a long long
enum OptNorm { kNormNone, kNormClamp, kNormAtLeast, kNorm3or4, kNormBool };      // [lo, hi] | >= lo | 3 or else 4 | value != 0
// the row's own refusal: an integer in [lo, hi] | 0 or an integer in [lo, hi] | not negative (NaN fails each of them)
enum OptValid { kValidAny, kValidIntIn, kValidPeriod, kValidNonNeg };
// kBeforeInit is ENFORCED (refused on an initialised solver); the others are documentation: kAtInit is read by cuadmm_init, kAtPlanBuild is
// resolved into a projection plan when it is built (a later set is kept for the plans built afterwards), kLive is read while solving
enum OptWhen { kBeforeInit, kAtInit, kAtPlanBuild, kLive };
// an in-process group (duo_group.hip): kGroupShared is replayed on new ranks and forwarded to the existing ones; kGroupPerRank is the
// group's own business on every rank (neither); kGroupInject is replayed but not forwarded, and a leader arms its group's hook with it
enum OptGroup { kGroupShared, kGroupPerRank, kGroupInject };
enum : unsigned { kEnvNegated = 1, kEnvEig0 = 2, kEnvEig1 = 4 };      // VAR != 0 means 0 | the spelling "eig" means 0 / 1, and "lds" means 2
enum OptCheck { kOptOk, kOptInvalid, kOptNotFinite, kOptOutOfRange };

constexpr int kOptAccelMaxMem = 16;      // = kAccelMaxMem (accel.h; engine.hip asserts it): the refusal of "accel" names it

struct OptionRow {
  const char* key = nullptr;
  const char* doc = nullptr;
  double def = 0;
  OptKind kind = kOptInt;
  const char* env = nullptr;
  unsigned env_flags = 0;
  OptNorm norm = kNormNone;
  OptValid valid = kValidAny;
  double lo = 0, hi = 0;
  const char* refusal = nullptr;      // the whole message of the validity rule
  OptWhen when = kAtInit;
  OptGroup group = kGroupShared;
  // cuadmm_option_info: kind | when << 2 | group << 4 | env negated << 6 | env takes eig / lds << 7 (bit 8: the planner's table)
  unsigned flags() const {
    return (unsigned)kind | (unsigned)when << 2 | (unsigned)group << 4 | (env_flags & kEnvNegated ? 64u : 0u) | (env_flags & (kEnvEig0 | kEnvEig1) ? 128u : 0u);
  }
};

// T: the struct that holds the fields.  field(obj, v): stores *v when v is given, returns what the field holds.
template <class T>
struct OptionSpec : OptionRow {
  using Field = double (*)(T&, const double*);
  Field field = nullptr;
  OptionSpec(const char* k, Field f, OptKind kd, double d, const char* text) { key = k; field = f; kind = kd; def = d; doc = text; }
  // the columns most rows leave at their defaults
  OptionSpec from_env(const char* name, unsigned fl = 0) const { OptionSpec o = *this; o.env = name; o.env_flags = fl; return o; }
  OptionSpec clamp(double l, double h) const { OptionSpec o = *this; o.norm = kNormClamp; o.lo = l; o.hi = h; return o; }
  OptionSpec at_least(double l) const { OptionSpec o = *this; o.norm = kNormAtLeast; o.lo = l; return o; }
  OptionSpec normalised(OptNorm n) const { OptionSpec o = *this; o.norm = n; return o; }
  OptionSpec checked(OptValid v, double l, double h, const char* msg) const { OptionSpec o = *this; o.valid = v; o.lo = l; o.hi = h; o.refusal = msg; return o; }
  OptionSpec read(OptWhen w) const { OptionSpec o = *this; o.when = w; return o; }
  OptionSpec in_group(OptGroup g) const { OptionSpec o = *this; o.group = g; return o; }
};
// (a captureless lambda per row: the fields have four types and sit in nested structs, which a pointer to member does not reach)
#define CUADMM_OPT_FIELD(T, member) \
  [](T& o, const double* v) -> double { if (v) o.member = static_cast<decltype(o.member)>(*v); return (double)o.member; }

template <class T>
struct OptionTable {
  const OptionSpec<T>* rows;
  int n;
  const OptionSpec<T>* begin() const { return rows; }
  const OptionSpec<T>* end() const { return rows + n; }
  const OptionSpec<T>* find(const char* key) const {
    for (const OptionSpec<T>& o : *this)
      if (!std::strcmp(o.key, key)) return &o;
    return nullptr;
  }
};

// check -> normalise: what the row stores for `value` (in *stored), or why it is refused.  The row's own rule goes first (its message
// is the older one: "infeas_tol must not be negative" answers a NaN); then no value that is not finite, and no integer beyond its type.
inline OptCheck option_check(const OptionRow& o, double value, double* stored) {
  const bool whole_in_range = value >= o.lo && value <= o.hi && value == std::floor(value);
  if ((o.valid == kValidIntIn && !whole_in_range) || (o.valid == kValidPeriod && !(value == 0 || whole_in_range)) || (o.valid == kValidNonNeg && !(value >= 0)))
    return kOptInvalid;
  if (!std::isfinite(value)) return kOptNotFinite;
  if (o.norm == kNormBool) { *stored = value != 0; return kOptOk; }
  if (o.kind == kOptReal) { *stored = value; return kOptOk; }
  double v = std::trunc(value);
  if (o.kind == kOptInt ? !(v >= (double)INT_MIN && v <= (double)INT_MAX) : !(v >= -0x1p63 && v < 0x1p63)) return kOptOutOfRange;
  if (o.norm == kNormClamp || o.norm == kNormAtLeast) v = v < o.lo ? o.lo : (o.norm == kNormClamp && v > o.hi ? o.hi : v);
  if (o.norm == kNorm3or4) v = v == 3 ? 3 : 4;
  *stored = v;
  return kOptOk;
}
template <class T>
OptCheck option_store(const OptionSpec<T>& o, T& obj, double value) {
  double v = 0;
  const OptCheck c = option_check(o, value, &v);
  if (c == kOptOk) o.field(obj, &v);
  return c;
}
template <class T>
double option_get(const OptionSpec<T>& o, const T& obj) { return o.field(const_cast<T&>(obj), nullptr); }

// The defaults from the environment: every row that names a variable consults it HERE, once per call (one call per solver, one per
// plan; nothing is cached), and the value goes through the row's checks like one from cuadmm_set_option.
template <class T>
void options_from_env(const OptionTable<T>& table, T& obj) {
  for (const OptionSpec<T>& o : table) {
    const char* e = o.env ? std::getenv(o.env) : nullptr;
    if (!e) continue;
    int v;
    if ((o.env_flags & (kEnvEig0 | kEnvEig1)) && !std::strcmp(e, "eig")) v = o.env_flags & kEnvEig1 ? 1 : 0;      // the register eigensolver
    else if ((o.env_flags & (kEnvEig0 | kEnvEig1)) && !std::strcmp(e, "lds")) v = 2;                              // one workgroup per block
    else v = std::atoi(e);
    if (o.env_flags & kEnvNegated) v = v ? 0 : 1;
    option_store(o, obj, (double)v);
  }
}

// The engine's table.  S is struct cuadmm_solver (engine_state.h); a template only so that this header stays free of HIP and a host
// program can run the rows over a stand-in with the same members.
template <class S>
OptionTable<S> engine_option_table() {
  using O = OptionSpec<S>;
#define F(member) CUADMM_OPT_FIELD(S, member)
  static const O rows[] = {
      O("device", F(device), kOptInt, 0, "HIP device ordinal").in_group(kGroupPerRank),
      O("verbose", F(verbose), kOptInt, 1, "1: the census and the iteration table on stdout").read(kLive).in_group(kGroupPerRank),
      O("rank", F(rank), kOptInt, 0, "this engine's index among the `world` engines that share the blocks").in_group(kGroupPerRank),
      O("world", F(world), kOptInt, 1, "engines that share the blocks by index (cuadmm_set_allreduce)").in_group(kGroupPerRank),
      O("profile", F(profile), kOptInt, 0, "1: time every kernel class with HIP events; 2: only the projection").read(kLive),
      O("force_comm", F(force_comm), kOptInt, 0, "call the collective hook even when world == 1 (transport tests)"),
      O("eig_rank", F(eig_rank), kOptInt, 0, "r > 0: only the r largest eigenvalues of every PSD block survive the projection"),
      O("eig_rank_begin_iter", F(eig_rank_begin_iter), kOptInt, 0, "eig_rank is active from this iteration on").read(kLive),
      O("eig_rank_maxfeas", F(eig_rank_maxfeas), kOptReal, 0.0, "... or once maxfeas is below this (0: never)").read(kLive),
      O("psd_steps", F(psd_steps), kOptInt, 0, "record the sign kernels' step count per block (cuadmm_get_psd_steps)"),
      O("batch", F(bt.max_iters), kOptInt, 64, "most ADMM iterations per launch, closed blocks (0 / 1: off)").clamp(0, 256).read(kLive),
      O("batch_mixed", F(bt.allow_mixed), kOptReal, 0, "batches although several tile geometries share the work (tests)").normalised(kNormBool).read(kLive),
      O("fuse", F(sw.fuse), kOptInt, 1, "the vector work of 9 <= n <= 64 blocks inside their projection kernels").from_env("CUADMM_FUSE"),
      O("fuse_rows", F(sw.fuse_rows), kOptInt, 1, "constraint rows local to one fused block evaluated there").from_env("CUADMM_FUSE_ROWS"),
      O("fuse_solve", F(sw.fuse_solve), kOptInt, -1, "closed blocks solve for their own multipliers (-1: whenever possible)").from_env("CUADMM_FUSE_SOLVE"),
      O("tiny_sign", F(opt_tiny_sign), kOptInt, 1, "n <= 8 on the sign kernel: 0 never, 1 closed candidates, 2 always"),
      O("psd_hint", F(opt_hint), kOptInt, 1, "schedule warm start: 0 off, 1 one-wavefront kernels + mid-size sign groups, 2 all, 3 one-wavefront kernels only")
          .from_env("CUADMM_PSD_HINT"),
      O("lpt", F(sw.lpt), kOptInt, 1, "longest block first"),
      O("host_solve", F(sw.host_solve), kOptInt, 0, "keep the y-solve on the host (no forest / lead / tail on the device)").from_env("CUADMM_HOST_SOLVE"),
      O("tail_k", F(sw.tail_k), kOptInt, -1, "-1 cost model, 0 host-only factor, k > 0 forces the GPU tail size").from_env("CUADMM_TAIL_K"),
      O("lead_stream", F(sw.lead_stream), kOptInt, 0, "the leading sweeps on the streaming kernels only (no LDS-resident trees)"),
      O("tail_one_pass", F(sw.tail_one_pass), kOptInt, 1, "the GPU tail applied in one pass over inv(L22) (0: two triangular GEMVs)"),
      O("lead_tops", F(sw.lead_tops), kOptInt, -1, "dense tree tops: -1 when the forest is too deep for the sweeps, 0 never, L always, cut at height L"),
      O("lead_small_kb", F(sw.lead_small_kb), kOptInt, 0, "LDS bound of the trees that share a workgroup in fours (0: chosen at build from 4 / 8 / 16)"),
      O("l21_device", F(sw.l21_device), kOptInt, 1, "hybrid y-solve allowed (0: host, 2: whenever the sweeps stay on the host)"),
      O("local_constraints", F(sw.local_constraints), kOptInt, 1, "owned-constraints sharding when the problem allows it")
          .from_env("CUADMM_NO_LOCAL_CONSTRAINTS", kEnvNegated),
      O("host_scalars", F(sw.host_scalars), kOptInt, 0, "owned constraints: the four scalars through the host").from_env("CUADMM_HOST_SCALARS"),
      O("mapped_out", F(sw.mapped_out), kOptInt, 1, "results through a mapped pinned buffer when no collective is needed")
          .from_env("CUADMM_NO_MAPPED_OUT", kEnvNegated),
      O("aty_post2", F(sw.aty_post2), kOptInt, 1, "the sGS second half in one pass"),
      O("lazy_unscale", F(lazy_unscale), kOptInt, 1, "0: unscale X, y, S at the end of every solve").read(kLive),
      O("duo_cpu_eig_on_gpu", F(duo_cpu_eig_on_gpu), kOptInt, 0, "accept cuadmm_duo_init(if_gpu_eig_mom = false) and project on the GPU"),
      O("duo_share_device", F(duo_share_device), kOptInt, 0, "in-process group: all N engines on this solver's device"),
      O("duo_exchange", F(duo_exchange), kOptInt, -1, "in-process group: -1 choose, 0 host-staged, 1 device-side exchange"),
      O("tail_max_k", F(sw.tail_max_k), kOptInt, 32768, "cap of the planner's GPU tail (<= 65 536)"),
      O("solve_next", F(sw.solve_next), kOptInt, 1, "the y-solve of iteration k + 1 is enqueued before the host waits for iteration k").read(kLive),
      O("accel", F(aa.mem), kOptInt, 0, "memory of the Anderson acceleration (0: off)")
          .checked(kValidIntIn, 0, kOptAccelMaxMem, "set_option: accel must be an integer from 0 (off) to 16"),
      O("accel_safeguard", F(aa.safeguard), kOptReal, 2.0, "a candidate is rejected when ||g|| grows by more than this factor (<= 0: always)").read(kLive),
      O("accel_reg", F(aa.reg), kOptReal, 1e-10, "relative Tikhonov term of the least-squares solve").read(kLive),
      O("infeas_check", F(inf.period), kOptInt, 0, "period of the infeasibility check (0: off)")
          .checked(kValidPeriod, 2, 1e6, "set_option: infeas_check must be 0 (off) or an integer period from 2 to 1000000").read(kBeforeInit),
      O("infeas_tol", F(inf.tol), kOptReal, 1e-6, "a ray is a certificate when its violation is at most this times its scalar")
          .checked(kValidNonNeg, 0, 0, "set_option: infeas_tol must not be negative").read(kLive),
      O("gap_check", F(lb.period), kOptInt, 0, "period of the certified-gap check (0: off)")
          .checked(kValidPeriod, 2, 1e6, "set_option: gap_check must be 0 (off) or an integer period from 2 to 1000000").read(kBeforeInit),
      O("gap_tol", F(lb.tol), kOptReal, 0.0, "tolerance of the certified-gap verdict (0: the solve's stop_tol)")
          .checked(kValidNonNeg, 0, 0, "set_option: gap_tol must not be negative").read(kLive),
      O("tail_shard", F(sw.tail_shard), kOptInt, 1, "world > 1, replicated solve: every rank applies 1 / world of the tail's rows"),
      O("tail_pivot", F(sw.tail_pivot), kOptInt, 1, "the tail's dense LDL^T with diagonal pivoting (0: unpivoted)"),
      O("tail_refine", F(sw.tail_refine), kOptInt, 0, "accuracy mode of the tail: one refinement step of each triangular solve"),
      O("lead_debug", F(sw.lead_debug), kOptInt, 0, "developer aid: statistics of the leading elimination forest on stderr at init"),
      O("debug_eig", F(sw.debug_eig), kOptInt, 0, "developer aid: dump of a projection input that hits the QL cap").read(kLive),
      O("update_A_inject_fail", F(upa.inject_fail), kOptInt, 0, "test hook: the next cuadmm_update_A fails as a broken factorisation would").read(kLive),
      O("duo_inject_fail", F(duo_inject), kOptLong, 0, "test hook of the in-process group's exchange").read(kLive).in_group(kGroupInject),
  };
#undef F
  static_assert(kOptAccelMaxMem == 16, "the refusal of accel spells the bound");
  return {rows, (int)(sizeof(rows) / sizeof(rows[0]))};
}

}  // namespace cuadmm
