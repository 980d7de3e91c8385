// What the two translation units of the C ABI share (capi.cpp: the public entry points; capi_debug.cpp: the test hooks):
// the exception barrier, the handle structs, and one converter per struct that crosses the boundary.  Private: nothing
// outside those two files includes it.
#pragma once
#include "../../include/dpgo_amd.h"

#include <cstdio>
#include <exception>
#include <vector>

#include "comm.h"
#include "edges.h"
#include "group.h"

// No exception leaves the library: a failed HIP call (dpgo::DeviceError) or an allocation failure becomes the
// reference's `return -1` (+ a line on stderr), never abort() / terminate() in the host process.
template <class F>
static int guarded(F &&f) {
  try {
    return f();
  } catch (const std::exception &e) {
    fprintf(stderr, "[dpgo_amd] ERROR: %s\n", e.what());
    return -1;
  } catch (...) {
    fprintf(stderr, "[dpgo_amd] ERROR: unknown exception\n");
    return -1;
  }
}

struct dpgo_graph {
  dpgo::Graph g;
};
struct dpgo_group {
  dpgo::Group *grp = nullptr;
  std::vector<int> all;
};
struct dpgo_comm {
  dpgo::Comm *c = nullptr;
};

inline int node_info(const dpgo_graph_t *g, int node, dpgo::DataInfo &info) {
  if (!g || node < 0 || node >= g->g.num_nodes) return -1;
  return dpgo::generate_data_info(node, g->g.d, g->g.measurements[node], info);
}

inline dpgo::Options to_cpp(const dpgo_options_t &o) {
  dpgo::Options r;
  r.scheme = o.scheme; r.regularizer = o.regularizer; r.accepted_delta = o.accepted_delta;
  r.eta[0] = o.eta[0]; r.eta[1] = o.eta[1]; r.psi = o.psi; r.phi = o.phi;
  r.max_soft_restart_hits[0] = o.max_soft_restart_hits[0]; r.max_soft_restart_hits[1] = o.max_soft_restart_hits[1];
  r.oscillation_cnt_period = o.oscillation_cnt_period; r.max_oscillations = o.max_oscillations;
  r.loss = o.loss; r.loss_reg = o.loss_reg; r.rescale = o.rescale; r.max_rescale_count = o.max_rescale_count;
  r.grad_norm_tol = o.grad_norm_tol;
  r.rel_func_decrease_tol = o.rel_func_decrease_tol; r.stepsize_tol = o.stepsize_tol;
  r.max_iterations = o.max_iterations; r.max_iterations_accepted = o.max_iterations_accepted;
  r.reg_Cholesky_precon_max_condition_number = o.reg_Cholesky_precon_max_condition_number;
  r.preconditioned_grad_norm_tol = o.preconditioned_grad_norm_tol; r.max_tCG_iterations = o.max_tCG_iterations;
  r.STPCG_kappa = o.STPCG_kappa; r.STPCG_theta = o.STPCG_theta; r.preconditioner = o.preconditioner;
  r.verbose = o.verbose;
  return r;
}

// the polish options without the anchor, which the C struct carries and the C++ calls take as an argument; null: the defaults
inline dpgo::PolishOptions to_cpp(const dpgo_polish_options_t *opt) {
  dpgo::PolishOptions o;
  if (opt) { o.max_steps = opt->max_steps; o.max_tries = opt->max_tries; o.rel_tol = opt->rel_tol; o.grad_tol = opt->grad_tol; }
  return o;
}

inline void to_c(const dpgo::EdgeSummary &s, dpgo_edge_summary_t *o) {
  o->F = s.F; o->F_intra = s.F_intra; o->F_inter = s.F_inter; o->weight_min = s.weight_min;
  o->num_inter = s.num_inter; o->num_downweighted = s.num_downweighted;
}

// the analysis' numbers (hess.h), which the eight result structs below carry under the same names
template <class C>
inline void analysis_to_c(const dpgo::HessAnalysis &r, C *o) {
  o->unknowns = r.unknowns; o->fronts = r.fronts; o->levels = r.levels; o->max_front = r.max_front;
  o->device_bytes = r.device_bytes; o->symbolic_s = r.symbolic_s; o->pivot_min = r.pivot_min;
  o->pivot_max = r.pivot_max; o->factor_ms = r.factor_ms;
}

inline void to_c(const dpgo::CovResult &r, dpgo_cov_result_t *o) {
  analysis_to_c(r, o);
  o->outcome = r.outcome; o->stationarity = r.stationarity; o->numeric_ms = r.numeric_ms;
  o->selinv_ms = r.selinv_ms; o->selinv_flops = r.selinv_flops;
}

inline void to_c(const dpgo::PairsResult &r, dpgo_pairs_result_t *o) {
  analysis_to_c(r, o);
  o->outcome = r.outcome; o->columns = r.columns; o->batches = r.batches; o->reserved = 0;
  o->stationarity = r.stationarity; o->solve_ms = r.solve_ms; o->gate_ms = r.gate_ms;
  o->solve_flops = r.solve_flops; o->factor_bytes = r.factor_bytes;
}

inline void to_c(const dpgo::MargResult &r, dpgo_marg_result_t *o) {
  analysis_to_c(r, o);
  o->outcome = r.outcome; o->info_not_pd = r.info_not_pd; o->n = r.n; o->columns = r.columns; o->batches = r.batches;
  o->reserved = 0; o->stationarity = r.stationarity; o->solve_ms = r.solve_ms; o->dense_ms = r.dense_ms;
  o->dense_pivot_min = r.dense_pivot_min; o->dense_pivot_max = r.dense_pivot_max;
}

inline void to_c(const dpgo::CandResult &r, dpgo_cand_result_t *o) {
  analysis_to_c(r, o);
  o->outcome = r.outcome; o->joint_not_pd = r.joint_not_pd; o->n = r.n; o->poses = r.poses; o->columns = r.columns;
  o->batches = r.batches; o->n_selected = r.n_selected; o->reserved = 0; o->stationarity = r.stationarity;
  o->solve_ms = r.solve_ms; o->dense_ms = r.dense_ms; o->select_ms = r.select_ms;
  o->dense_pivot_min = r.dense_pivot_min; o->dense_pivot_max = r.dense_pivot_max;
}

inline void to_c(const dpgo::SensResult &r, dpgo_sens_result_t *o) {
  analysis_to_c(r, o);
  o->outcome = r.outcome; o->columns = r.columns; o->batches = r.batches; o->edges = r.edges;
  o->stationarity = r.stationarity; o->solve_ms = r.solve_ms; o->edge_ms = r.edge_ms;
}

inline void to_c(const dpgo::RelyResult &r, dpgo_rely_result_t *o) {
  analysis_to_c(r, o);
  o->outcome = r.outcome; o->method_used = r.method_used; o->edges = r.edges; o->flagged = r.flagged;
  o->unweighted = r.unweighted; o->columns = r.columns; o->batches = r.batches; o->reserved = 0;
  o->device_bytes_selinv = r.device_bytes_selinv; o->device_bytes_solve = r.device_bytes_solve;
  o->redundancy_sum = r.redundancy_sum; o->stationarity = r.stationarity;
  o->inverse_ms = r.inverse_ms; o->edge_ms = r.edge_ms;
}

inline void to_c(const dpgo::PolishResult &r, dpgo_polish_result_t *o) {
  analysis_to_c(r, o);
  o->outcome = r.outcome; o->steps = r.steps; o->factorisations = r.factorisations;
  o->indefinite = r.indefinite; o->F_initial = r.F_initial; o->F_final = r.F_final;
  o->grad_initial = r.grad_initial; o->grad_final = r.grad_final; o->hmax = r.hmax;
  o->mu_final = r.mu_final; o->total_ms = r.total_ms; o->solve_ms = r.solve_ms; o->other_ms = r.other_ms;
}

inline dpgo::ModesOptions to_cpp(const dpgo_modes_options_t *opt) {
  dpgo::ModesOptions o;
  if (opt) {
    o.guard = opt->guard; o.max_iters = opt->max_iters; o.max_tries = opt->max_tries; o.want_escape = opt->want_escape;
    o.rel_tol = opt->rel_tol; o.shift = opt->shift; o.seed = opt->seed;
  }
  return o;
}

inline void to_c(const dpgo::ModesResult &r, dpgo_modes_result_t *o) {
  analysis_to_c(r, o);
  o->outcome = r.outcome; o->iterations = r.iterations; o->factorisations = r.factorisations; o->shift_tries = r.shift_tries;
  o->block = r.block; o->negative = r.negative; o->escaped = r.escaped; o->reserved = 0;
  o->mu = r.mu; o->hmax = r.hmax; o->stationarity = r.stationarity; o->escape_alpha = r.escape_alpha; o->F = r.F;
  o->F_escape = r.F_escape; o->solve_ms = r.solve_ms; o->gram_ms = r.gram_ms; o->ritz_ms = r.ritz_ms;
  o->update_ms = r.update_ms; o->total_ms = r.total_ms;
}
