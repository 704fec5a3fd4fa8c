// Stand-alone host program (its own main; no device, no library): every row of the two option tables through store and get, the
// normalisations written out by hand, the values no key takes, and the defaults from the environment.  Built with
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I cuadmm_amd/csrc -I include
// and run by tests/test_options_host.py; ASan / UBSan end it on the first finding (a double beyond int converted to one, say).
// struct cuadmm_solver needs the HIP headers, so the engine's rows run over a stand-in with the same members.
#include <cstdio>
#include <limits>
#include <set>
#include <string>

#include "psd_options.h"

using namespace cuadmm;

struct StandIn {
  int device, verbose, rank, world, profile, force_comm, psd_steps, eig_rank, eig_rank_begin_iter;
  double eig_rank_maxfeas;
  int duo_share_device, duo_exchange, duo_cpu_eig_on_gpu, lazy_unscale, opt_tiny_sign, opt_hint;
  long long duo_inject;
  struct { int max_iters; bool allow_mixed; } bt;
  struct { int inject_fail; } upa;
  struct {
    int fuse, fuse_rows, fuse_solve, host_solve, host_scalars, tail_k, local_constraints, mapped_out, lpt, aty_post2, lead_stream, tail_one_pass, solve_next,
        tail_max_k, tail_refine, tail_pivot, tail_shard, l21_device, lead_debug, lead_small_kb, lead_tops, debug_eig;
  } sw;
  struct { int mem; double safeguard, reg; } aa;
  struct { int period; double tol; } inf, lb;
};

static int failures = 0;
#define CHECK(cond, ...) \
  do { if (!(cond)) { ++failures; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <class T>
static void every_row(const OptionTable<T>& table, T& obj, std::set<std::string>& keys, std::set<std::string>& envs) {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (const OptionSpec<T>& o : table) {
    CHECK(keys.insert(o.key).second, "key %s twice", o.key);
    if (o.env) CHECK(envs.insert(o.env).second, "variable %s twice", o.env);
    CHECK(table.find(o.key) == &o, "%s", o.key);
    CHECK(o.doc && o.doc[0], "%s has no description", o.key);
    CHECK((o.valid == kValidAny) == (o.refusal == nullptr), "%s: a rule and its message go together", o.key);
    CHECK(o.valid == kValidAny || o.norm == kNormNone || o.norm == kNorm3or4 || o.norm == kNormBool, "%s: a clamp and a rule would share lo / hi", o.key);
    CHECK(option_store(o, obj, o.def) == kOptOk && option_get(o, obj) == o.def, "%s refuses or changes its default %g", o.key, o.def);
    const double before = option_get(o, obj);
    for (double bad : {nan, inf, -inf}) {
      const OptCheck c = option_store(o, obj, bad);
      CHECK(c == kOptNotFinite || (o.valid != kValidAny && c == kOptInvalid), "%s took %g (%d)", o.key, bad, (int)c);      // (or the row's own refusal)
    }
    for (double big : {1e300, -1e300, 2147483648.0, -2147483649.0, 9.3e18, -9.3e18}) {
      const bool beyond = o.kind == kOptInt || (o.kind == kOptLong && std::fabs(big) > 9e18);
      const OptCheck c = option_store(o, obj, big);
      if (o.valid != kValidAny && c == kOptInvalid) continue;      // the row's own refusal
      CHECK(c == (beyond ? kOptOutOfRange : kOptOk), "%s: %g gives %d", o.key, big, (int)c);
      if (c == kOptOk) option_store(o, obj, before);
    }
    CHECK(option_get(o, obj) == before, "%s: a refused value was stored", o.key);
    CHECK(option_store(o, obj, 2147483647.9) == (o.valid == kValidIntIn || o.valid == kValidPeriod ? kOptInvalid : kOptOk), "%s: INT_MAX + 0.9 truncates into range", o.key);
    option_store(o, obj, before);
  }
}

template <class T>
static void stores(const OptionTable<T>& table, T& obj, const char* key, double in, double want) {
  const OptionSpec<T>* o = table.find(key);
  CHECK(o != nullptr, "no key %s", key);
  if (!o) return;
  const OptCheck c = option_store(*o, obj, in);
  CHECK(c == kOptOk && option_get(*o, obj) == want, "%s: %g -> %g (status %d), expected %g", key, in, option_get(*o, obj), (int)c, want);
}

int main() {
  const OptionTable<StandIn> eng = engine_option_table<StandIn>();
  const OptionTable<PsdOptions> psd = psd_option_table();
  StandIn s{};
  PsdOptions p;
  for (const OptionSpec<PsdOptions>& o : psd) CHECK(option_get(o, p) == o.def, "%s: the table says %g, the struct %g", o.key, o.def, option_get(o, p));
  std::set<std::string> keys, envs;
  every_row(eng, s, keys, envs);
  every_row(psd, p, keys, envs);
  CHECK(eng.n == 49 && psd.n == 20, "%d + %d keys", eng.n, psd.n);

  // what the chain of cuadmm_set_option and PsdOptions::set stored before the tables
  stores(eng, s, "batch", 300, 256); stores(eng, s, "batch", -5, 0); stores(eng, s, "batch", 2.9, 2);
  stores(psd, p, "psd_w32_occ", 5, 4); stores(psd, p, "psd_w32_occ", 3, 3);
  stores(psd, p, "psd_cu_occ", 3, 3); stores(psd, p, "psd_cu_occ", 0, 4);
  stores(psd, p, "psd_sign_min", 10, 65); stores(psd, p, "psd_sign_min", 200, 200);
  stores(psd, p, "psd_lg_cluster_wgs", 5, 8); stores(psd, p, "psd_lg_cluster_wgs", 2000, 960);
  stores(psd, p, "psd_sign_ws_mb", 0, 1);
  stores(psd, p, "psd_debug", -1, 0);
  stores(eng, s, "tail_k", -1.5, -1);
  stores(eng, s, "lead_small_kb", 99, 99);
  stores(eng, s, "batch_mixed", 7, 1); stores(eng, s, "batch_mixed", 0.5, 1); stores(eng, s, "batch_mixed", 1e300, 1); stores(eng, s, "batch_mixed", 0, 0);
  stores(eng, s, "accel_safeguard", -1.0, -1.0);
  stores(eng, s, "fuse_solve", -7.9, -7); stores(eng, s, "eig_rank_maxfeas", 1e-3, 1e-3);
  stores(psd, p, "psd_wave4_min", 17.5, 17);
  stores(eng, s, "duo_inject_fail", 4e12, 4e12); stores(eng, s, "duo_inject_fail", -2.5, -2);
  stores(eng, s, "accel", 16, 16); stores(eng, s, "infeas_check", 2, 2); stores(eng, s, "gap_check", 1e6, 1e6); stores(eng, s, "infeas_tol", 0, 0);
  for (double bad : {-1.0, 17.0, 2.5}) CHECK(option_store(*eng.find("accel"), s, bad) == kOptInvalid && s.aa.mem == 16, "accel %g", bad);
  for (double bad : {1.0, -2.0, 1000001.0, 2.5}) CHECK(option_store(*eng.find("infeas_check"), s, bad) == kOptInvalid && s.inf.period == 2, "infeas_check %g", bad);
  CHECK(option_store(*eng.find("gap_tol"), s, -1e-9) == kOptInvalid, "gap_tol");

  // the defaults from the environment
  const char* vars[][2] = {{"CUADMM_FUSE", "0"}, {"CUADMM_NO_MAPPED_OUT", "1"}, {"CUADMM_NO_LOCAL_CONSTRAINTS", "1"}, {"CUADMM_TAIL_K", "512"},
                           {"CUADMM_PSD_HINT", "3"}, {"CUADMM_PSD_MID", "lds"}, {"CUADMM_PSD_N16", "eig"}, {"CUADMM_PSD_LG_CLUSTER_WGS", "5000"}};
  for (const auto& v : vars) setenv(v[0], v[1], 1);
  StandIn e{};
  for (const OptionSpec<StandIn>& o : eng) o.field(e, &o.def);
  options_from_env(eng, e);
  const PsdOptions pe = PsdOptions::from_env();
  CHECK(e.sw.fuse == 0 && e.sw.mapped_out == 0 && e.sw.local_constraints == 0 && e.sw.tail_k == 512 && e.opt_hint == 3 && e.sw.fuse_rows == 1, "engine defaults from the environment");
  CHECK(pe.mid == 2 && pe.n16_sign == 0 && pe.lg_cluster_wgs == 960 && pe.n32_sign == 1, "psd defaults from the environment: %d %d %d", pe.mid, pe.n16_sign, pe.lg_cluster_wgs);
  setenv("CUADMM_PSD_MID", "eig", 1); setenv("CUADMM_NO_MAPPED_OUT", "0", 1);
  options_from_env(eng, e);
  CHECK(PsdOptions::from_env().mid == 1 && e.sw.mapped_out == 1, "eig on psd_mid is 1; NO_MAPPED_OUT=0 leaves it on");
  CHECK(PsdOptions().mid == 0 && PsdOptions().lg_cluster_wgs == 224, "PsdOptions() never reads the environment");

  std::printf("option tables: %d keys, %d failures\n", eng.n + psd.n, failures);
  return failures ? 1 : 0;
}
