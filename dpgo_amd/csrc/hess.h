// What every consumer of the anchored tangent-space Hessian's factor (CovState::F, cov_state.h) shares: covariance,
// pair_covariance, joint_marginal, candidate_set, sensitivity, robust_sensitivity, edge_reliability, polish / robust_polish / gnc, hessian_modes, robust_covariance and the
// read-backs cov_hessian / robust_hessian.  Stated once, in hess.cpp:
//
//  * the analysis' numbers (HessAnalysis, the base of every result struct; Group::cov_analyse in cov.cpp fills it);
//  * the refusal (Group::hess_reserve): what a call may allocate on a shared device, as a list of parts;
//  * the verdict (Group::hess_factor, and the part of it polish_loop's own loop shares, Group::hess_refactor).
//
// The callers differ in their parts only -- see the "still to allocate" terms at cov_setup, polish_setup, pairs_setup,
// edge_reliability, joint_marginal, candidate_set and modes_loop.
#pragma once

namespace dpgo {

// unknowns ... max_front, device_bytes and symbolic_s come from the symbolic analysis (and the sizes of the call) and are filled
// for SKIPPED too; symbolic_s: host seconds of the analysis, 0 after the first call of a group.  pivot_min / pivot_max: of the
// last factorisation (0 where no front was factored).  factor_ms: host milliseconds from the launch that writes H to the
// factorisation's verdict (polish: see polish.h).
struct HessAnalysis {
  int unknowns = 0, fronts = 0, levels = 0, max_front = 0;
  long long device_bytes = 0;
  double symbolic_s = 0, pivot_min = 0, pivot_max = 0, factor_ms = 0;
};

// One term of a refusal: all of its bytes (they count against max_bytes and are reported as device_bytes), and those of them
// this call would still have to allocate (they count against half of the free memory).
struct HessPart {
  long long bytes, remain;
};

}  // namespace dpgo
