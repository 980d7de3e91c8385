// The device side of the multifrontal solve (spd.h): the factor's panels, the tile plan of both sweeps and of the fused
// roots (spd_solve.cpp), and the launches of one solve (k_spd_level, k_root_sym / k_root_combine in kernels.hip).
#pragma once
#include <memory>
#include <vector>

#include "devbuf.h"
#include "kernels.h"
#include "spd.h"

namespace dpgo {

class SpdSolverDev;

// out <- scale * A^-1 in on the unknowns' entries of the records (everything else in `out` is left alone); in != out
// class_of: the node set the roots' tile class is chosen for, if not mask.v (SpdSolverDev::fine_root_for)
void spd_run(int d, hipStream_t st, SpdSolverDev &S, NodeMask mask, double *in, double *out, double scale, const NodeBits *class_of = nullptr);
// DPGO_SPD_DUMP=1: the tile plan's per-launch table on stderr, every launch timed on `vec` (a zero vector; overwritten)
void spd_profile(int d, hipStream_t st, SpdSolverDev &S, double *vec);
// a warning on stderr when F's pivots span so many orders of magnitude that its solves lose digits
void warn_conditioning(const char *what, const SpdFactor &F);

// The descriptor's layout fields (ld, pair_kq, mat_off) of a tile with `count` rows in the class of `rows`-high tiles, as
// upload() sets them; the doubles its panel of `len` entries per row takes; and upload()'s host packer for one tile (what
// k_pack_panels does on the device): the entries of `factor` that `ps` names, to panels + it.mat_off
SpdItem spd_panel_item(int rows, int count, bool pairs, int64_t mat_off);
int64_t spd_panel_doubles(const SpdItem &it, int64_t len);
void spd_pack_panel_host(const SpdItem &it, const PanelSrc &ps, const double *factor, double *panels);

// What upload() decided, for the tests to read back (dpgo_debug_spd_solver_plan): a launch's tile class and counts
struct SpdPlanInfo {
  struct Level { int rows = 0, nwide = 0, nnarrow = 0; std::vector<int> wcount, ncount; };   // (wcount / ncount: per local node)
  bool fused_root = false, root_sym = false, stream_once = false;
  int dof = 0, nnodes = 0, root_fine_rows = 0, root_fine_below = 0;
  std::vector<Level> fwd, bwd;
  Level root, root_fine, root_rows;   // the fused roots' launch, its finer class, the triangle's block rows (k_root_combine)
};

class SpdSolverDev {
 public:
  SpdFactor F;   // host copy kept for sizes / host solves
  SpdSolverDev();
  ~SpdSolverDev();
  // F's panels and tile plan on the device; F's host copy of the factor goes.  dof: unknowns per record (1: the
  // translation, d: the rotation rows); dcols: columns of a right-hand side; node_of_unknown: local node of every row of A
  void upload(int dof, int dcols, const std::vector<int> &node_of_unknown);
  int repack(hipStream_t st);   // the panels again from F.dev_W / F.dev_WT (same pattern, new values)
  // the finer tile class of the fused roots for a launch over the nodes `v` (few live roots)
  bool fine_root_for(NodeBits v) const;
  SpdPlanInfo plan_info() const;

 private:
  struct Plan;   // device buffers and tile plan (spd_solve.cpp)
  std::unique_ptr<Plan> plan_;
  friend void spd_run(int, hipStream_t, SpdSolverDev &, NodeMask, double *, double *, double, const NodeBits *);
  friend void spd_profile(int, hipStream_t, SpdSolverDev &, double *);
};

}  // namespace dpgo
