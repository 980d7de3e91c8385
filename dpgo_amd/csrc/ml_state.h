// The lists and buffers of the maximum-likelihood objective on one (group, graph): what ml.cpp and ml_gnc.cpp share.
#pragma once
#include "group.h"
#include "ml.h"
#include "ml_gnc.h"
#include "robust.h"

namespace dpgo {

struct Group::MlState {
  RobustPlan plan;             // the records and the lists (robust.h)
  std::vector<double> omega;   // m x dof^2: the graph's, or Omega_iso
  bool on_device = false;
  long long bytes = 0;         // what ml_alloc allocates for the plan
  DevBuf<double> rec, om, r, wr, chi2, ge, jw, partials, sum, grad;
  DevBuf<int64_t> counts;
  DevBuf<int> inc_ptr, inc, blk_ptr, blk;
  // two summaries: [0] of the last full edge pass (a point), [1] of the last trial pass, which must not overwrite it
  MlSummaryDev *sum_dev(bool full = true) const { return reinterpret_cast<MlSummaryDev *>(sum.p) + (full ? 0 : 1); }
  MlEdgeOut out() const { return {r.p, wr.p, chi2.p, ge.p, jw.p}; }
  // graduated non-convexity (ml_gnc.cpp): the weights, the robust set (one int per edge, uploaded per call: the records' inter
  // word stays as ml_begin compares it), the partials of k_ml_gnc_edge and its two summaries, by the same rule as above
  bool gnc_on_device = false;
  DevBuf<double> gnc_w, gnc_partials, gnc_sum;
  DevBuf<int> gnc_in_R;
  DevBuf<int64_t> gnc_counts;
  long long gnc_bytes() const { return 12ll * plan.m + gnc_reduce_bytes(plan.nb, ML_GNC_COUNT_SLOTS, 2); }
  long long gnc_remain() const { return gnc_on_device ? 0 : gnc_bytes(); }
  MlGncSummaryDev *gnc_sum_dev(bool full = true) const { return reinterpret_cast<MlGncSummaryDev *>(gnc_sum.p) + (full ? 0 : 1); }
};

}  // namespace dpgo
