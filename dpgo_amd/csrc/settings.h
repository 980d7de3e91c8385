// The library's DPGO_* environment settings: tuning knobs, mechanism switches, diagnostics, deadlines and test hooks.
// None is needed to run.  The comments below are the authoritative table (DESIGN 8 names them by purpose).
//
// Parse rule.  Every setting is read once per process, on the first call of settings(); changing the environment
// afterwards has no effect.
//  - A number (int / long long / double) is atoll / atof of the value whenever the variable is set, 0 included.
//  - A flag (bool) is on when the variable is set to a non-zero integer: "1" is on; "0", "" and words are off.
//  - A std::optional is empty when the variable is unset: the call site applies a default that depends on context.
//  - A string is the value as given, "" when unset.
// (The driver's RANK / WORLD_SIZE / ... / DPGO_FORCE_COMM are read in dist_pgo.cpp, DPGO_RDV_TIMEOUT in rdv.h.)
#pragma once

#include <optional>
#include <string>
#include <vector>

namespace dpgo {

struct Settings {
  // ---- solver plan and ordering
  bool spd_fuse_root = true;              // DPGO_SPD_FUSE_ROOT (1): roots applied through the explicit inverse of their complement; 0: two sweeps
  bool spd_fuse_root_dynamic = false;     // DPGO_SPD_FUSE_ROOT_DYNAMIC (0): fused roots also for a factor re-done every iteration (Dynamic)
  int spd_fuse_root_maxlog = 9;           // DPGO_SPD_FUSE_ROOT_MAXLOG (9): roots keep the two sweeps beyond a pivot range of 10^this
  std::optional<int> spd_root_sym;        // DPGO_SPD_ROOT_SYM (auto): 1 / 0 forces the fused roots as one triangle on / off
  int spd_root_sym_mb = 32;               // DPGO_SPD_ROOT_SYM_MB (32): auto: one triangle from a root of this many MB
  std::optional<int> spd_root_sym_blocks; // DPGO_SPD_ROOT_SYM_BLOCKS (block count / 768): 64x64 blocks per item of the triangle
  int spd_fine_fwd = 192;                 // DPGO_SPD_FINE_FWD (192): forward solve levels below this many wide tiles take 16-row tiles
  int spd_fine_bwd = 256;                 // DPGO_SPD_FINE_BWD (256): the same for backward levels
  int spd_fine_bwd_tall = 800;            // DPGO_SPD_FINE_BWD_TALL (800): ... and below this many where a front is >= 1000 rows tall
  int spd_fine_root = 192;                // DPGO_SPD_FINE_ROOT (192): fused roots below this many 64-row tiles take 16-row tiles
  int spd_fine_root8 = 64;                // DPGO_SPD_FINE_ROOT8 (64): ... and below this many, 8-row tiles
  long long spd_keep_mb = 200;            // DPGO_SPD_KEEP_MB (200): panels up to this many MiB stay in the Infinity Cache between solves
  bool spd_panel_pairs = true;            // DPGO_SPD_PANEL_PAIRS (1): panels of the 64- and 16-row tiles paired for 16-byte loads (spd_panel.h); 0: plain
  int spd_leaf_rr = 96;                  // DPGO_SPD_LEAF_RR (96): leaf size of the nested dissection of G_RR + lambda I
  int spd_collapse_rr = 0;                // DPGO_SPD_COLLAPSE_RR (0): merged tree levels of G_RR; 0: by the solve's cost model
  std::optional<int> spd_leaf_tt;         // DPGO_SPD_LEAF_TT (128; 64 for a Dynamic group): leaf size of G_tt
  std::optional<int> spd_collapse_tt;     // DPGO_SPD_COLLAPSE_TT (0 = cost model; 1 for a Dynamic group): merged tree levels of G_tt
  std::optional<int> spd_collapse;        // DPGO_SPD_COLLAPSE (the caller's): merged tree levels of every factor
  bool spd_quotient = true;               // DPGO_SPD_QUOTIENT (1): G_RR ordered on its quotient graph (blocks of d); 0: scalar
  bool spd_device_panels = true;          // DPGO_SPD_DEVICE_PANELS (1): solve panels packed on the device; 0: on the host
  bool spd_host_factor = false;           // DPGO_SPD_HOST_FACTOR (0): 1: the numeric factorisation on the host, also for Dynamic
  bool spd_left_looking = true;           // DPGO_SPD_LEFT_LOOKING (1): small levels of the device factorisation left-looking
  long long spd_fuse_potrf_wgs = 768;     // DPGO_SPD_FUSE_POTRF_WGS (768): right-looking levels of up to this many workgroups factor
                                          //   the diagonal block beside their rows' loads
  bool spd_extend_slots = false;          // DPGO_SPD_EXTEND_SLOTS (0): 1: the assembly with a launch per child slot (same bits)
  double nd_window = 0.45;                // DPGO_ND_WINDOW (0.45): nested dissection: least share of the vertices on either side
  int nd_roots = 2;                       // DPGO_ND_ROOTS (2): BFS level structures tried per separator
  bool nd_spectral = true;                // DPGO_ND_SPECTRAL (1): spectral (Fiedler vector) separator candidates
  std::vector<int> nd_lanczos;            // DPGO_ND_LANCZOS ("40,60,90,120"): Lanczos depths of the Fiedler vectors

  // ---- mechanism switches (each 0 selects an earlier round's exact equivalent)
  bool fused = true;                      // DPGO_FUSED (1): fused passes; 0: round 5's launch sequence
  bool spec_update = true;                // DPGO_SPEC_UPDATE (1): the GPU decides update() before the host has read it back
  bool spec_refine = true;                // DPGO_SPEC_REFINE (1): the refinement started ahead of update()'s read-back
  bool lazy_update_reduce = true;         // DPGO_LAZY_UPDATE_REDUCE (1): update()'s reduction left to the next refinement
  bool lazy_unpack = true;                // DPGO_LAZY_UNPACK (1): a group-stream exchange unpacked inside the inter-edge pass
  bool defer_update = true;               // DPGO_DEFER_UPDATE (1): update()'s closing read-back deferred to the next reader
  std::optional<int> iter_graph;          // DPGO_ITER_GRAPH (auto): segments replayed by measurement; 0: never; 1: always
  bool cg_graph = true;                   // DPGO_CG_GRAPH (1): CG steps of small multi-node groups replayed; 0: eager
  bool rescale_host = false;              // DPGO_RESCALE_HOST (0): 1: Dynamic rescale on the host (no device values kept)
  std::string exchange;                   // DPGO_EXCHANGE (""): "allgather": never the neighbour-to-neighbour exchange

  // ---- deadlines and threads
  double comm_timeout = 120.0;            // DPGO_COMM_TIMEOUT (120, at least 1): seconds a communication stream may take
  int host_threads = 0;                   // DPGO_HOST_THREADS (0 = the CPUs this process may use, at most 64): set-up threads

  // ---- diagnostics (stderr unless named)
  bool spd_dump = false;                  // DPGO_SPD_DUMP (0): factor, panel and per-launch tables of both solves
  std::string spd_dump_fronts;            // DPGO_SPD_DUMP_FRONTS (""): file for "w u height depth" per front (spd_stats)
  bool setup_timing = false;              // DPGO_SETUP_TIMING (0): wall time of the set-up phases
  bool host_timing = false;               // DPGO_HOST_TIMING (0): where the host's time goes, when the group goes
  bool spd_trace = false;                 // DPGO_SPD_TRACE (0): per-tile phase timestamps (a -DSPD_TRACE build)

  // ---- test hooks
  bool debug_fail_refactor = false;       // DPGO_DEBUG_FAIL_REFACTOR (0): 1: a refactorisation's verdict is "not positive definite"
  int debug_fail_exchange = 0;            // DPGO_DEBUG_FAIL_EXCHANGE (0): the n-th exchange of this process fails
  int debug_late_host_us = 0;             // DPGO_DEBUG_LATE_HOST_US (0): the host comes n us late to every read-back
  double host_bound_below = 0.40;         // DPGO_HOST_BOUND_BELOW (0.40): share of waiting below which the host is the slower side
};

const Settings &settings();

}  // namespace dpgo
