// The lists and buffers of the robust objective on one (group, graph): what robust.cpp and gnc.cpp share.
#pragma once
#include "gnc.h"
#include "group.h"
#include "robust.h"

namespace dpgo {

struct Group::RobustState {
  RobustPlan plan;
  bool on_device = false;
  long long bytes = 0;   // what robust_alloc allocates for the plan
  DevBuf<double> rec, out, rows, partials, Mw, sum, grad;   // grad: dof per own row, for robust_hessian's hand-out
  DevBuf<int64_t> counts;
  DevBuf<int> inc_ptr, inc, blk_ptr, blk;
  EdgeSummaryDev *sum_dev() const { return reinterpret_cast<EdgeSummaryDev *>(sum.p); }
  // graduated non-convexity (gnc.cpp): the partials of k_gnc_edge and its summary; its weights live in out + 3 m, where
  // the robust objective keeps its own, so that every launcher behind them is called as robust.cpp calls it
  bool gnc_on_device = false;
  DevBuf<double> gnc_partials, gnc_sum;
  DevBuf<int64_t> gnc_counts;
  long long gnc_bytes() const { return gnc_reduce_bytes(plan.nb, GNC_COUNT_SLOTS, 1); }
  GncSummaryDev *gnc_sum_dev() const { return reinterpret_cast<GncSummaryDev *>(gnc_sum.p); }
};

}  // namespace dpgo
