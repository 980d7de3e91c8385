#include "settings.h"

#include <cstdlib>

namespace dpgo {
namespace {

// one overload per kind of field (integers, double, flag, string), each by the parse rule of settings.h
void get(const char *name, long long &v) { if (const char *e = getenv(name)) v = atoll(e); }
void get(const char *name, int &v) { if (const char *e = getenv(name)) v = (int)atoll(e); }
void get(const char *name, double &v) { if (const char *e = getenv(name)) v = atof(e); }
void get(const char *name, bool &v) { if (const char *e = getenv(name)) v = atoll(e) != 0; }
void get(const char *name, std::optional<int> &v) { if (const char *e = getenv(name)) v = (int)atoll(e); }
void get(const char *name, std::string &v) { if (const char *e = getenv(name)) v = e; }

Settings read() {
  Settings s;
  get("DPGO_SPD_FUSE_ROOT", s.spd_fuse_root);
  get("DPGO_SPD_FUSE_ROOT_DYNAMIC", s.spd_fuse_root_dynamic);
  get("DPGO_SPD_FUSE_ROOT_MAXLOG", s.spd_fuse_root_maxlog);
  get("DPGO_SPD_ROOT_SYM", s.spd_root_sym);
  get("DPGO_SPD_ROOT_SYM_MB", s.spd_root_sym_mb);
  get("DPGO_SPD_ROOT_SYM_BLOCKS", s.spd_root_sym_blocks);
  get("DPGO_SPD_FINE_FWD", s.spd_fine_fwd);
  get("DPGO_SPD_FINE_BWD", s.spd_fine_bwd);
  get("DPGO_SPD_FINE_BWD_TALL", s.spd_fine_bwd_tall);
  get("DPGO_SPD_FINE_ROOT", s.spd_fine_root);
  get("DPGO_SPD_FINE_ROOT8", s.spd_fine_root8);
  get("DPGO_SPD_KEEP_MB", s.spd_keep_mb);
  get("DPGO_SPD_PANEL_PAIRS", s.spd_panel_pairs);
  get("DPGO_SPD_LEAF_RR", s.spd_leaf_rr);
  get("DPGO_SPD_COLLAPSE_RR", s.spd_collapse_rr);
  get("DPGO_SPD_LEAF_TT", s.spd_leaf_tt);
  get("DPGO_SPD_COLLAPSE_TT", s.spd_collapse_tt);
  get("DPGO_SPD_COLLAPSE", s.spd_collapse);
  get("DPGO_SPD_QUOTIENT", s.spd_quotient);
  get("DPGO_SPD_DEVICE_PANELS", s.spd_device_panels);
  get("DPGO_SPD_HOST_FACTOR", s.spd_host_factor);
  get("DPGO_SPD_LEFT_LOOKING", s.spd_left_looking);
  get("DPGO_SPD_FUSE_POTRF_WGS", s.spd_fuse_potrf_wgs);
  get("DPGO_SPD_EXTEND_SLOTS", s.spd_extend_slots);
  get("DPGO_ND_WINDOW", s.nd_window);
  get("DPGO_ND_ROOTS", s.nd_roots);
  get("DPGO_ND_SPECTRAL", s.nd_spectral);
  std::string depths = "40,60,90,120";
  get("DPGO_ND_LANCZOS", depths);
  for (size_t p = 0; p < depths.size();) {
    size_t c = depths.find(',', p);
    if (c == std::string::npos) c = depths.size();
    s.nd_lanczos.push_back(atoi(depths.substr(p, c - p).c_str()));
    p = c + 1;
  }

  get("DPGO_FUSED", s.fused);
  get("DPGO_SPEC_UPDATE", s.spec_update);
  get("DPGO_SPEC_REFINE", s.spec_refine);
  get("DPGO_LAZY_UPDATE_REDUCE", s.lazy_update_reduce);
  get("DPGO_LAZY_UNPACK", s.lazy_unpack);
  get("DPGO_DEFER_UPDATE", s.defer_update);
  get("DPGO_ITER_GRAPH", s.iter_graph);
  get("DPGO_CG_GRAPH", s.cg_graph);
  get("DPGO_RESCALE_HOST", s.rescale_host);
  get("DPGO_EXCHANGE", s.exchange);

  get("DPGO_COMM_TIMEOUT", s.comm_timeout);
  get("DPGO_HOST_THREADS", s.host_threads);

  get("DPGO_SPD_DUMP", s.spd_dump);
  get("DPGO_SPD_DUMP_FRONTS", s.spd_dump_fronts);
  get("DPGO_SETUP_TIMING", s.setup_timing);
  get("DPGO_HOST_TIMING", s.host_timing);
  get("DPGO_SPD_TRACE", s.spd_trace);

  get("DPGO_DEBUG_FAIL_REFACTOR", s.debug_fail_refactor);
  get("DPGO_DEBUG_FAIL_EXCHANGE", s.debug_fail_exchange);
  get("DPGO_DEBUG_LATE_HOST_US", s.debug_late_host_us);
  get("DPGO_HOST_BOUND_BELOW", s.host_bound_below);
  return s;
}

}  // namespace

const Settings &settings() {
  static const Settings s = read();
  return s;
}

}  // namespace dpgo
