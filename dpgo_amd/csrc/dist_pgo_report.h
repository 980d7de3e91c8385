// dist_pgo_report.h -- what the dist_pgo driver prints besides numbers: the names of the C ABI's outcomes and the writers its
// report files share.  Included by dist_pgo.cpp only; needs include/dpgo_amd.h and <cstdio>, no GPU and no state.
#pragma once
#include <cstdio>

#include "../../include/dpgo_amd.h"

namespace report {

// ---- one name function per printed enum of include/dpgo_amd.h
inline const char *polish_name(int o) {
  return o == DPGO_POLISH_CONVERGED ? "CONVERGED" : o == DPGO_POLISH_MAX_STEPS ? "MAX_STEPS" : o == DPGO_POLISH_STALLED ? "STALLED" : "SKIPPED";
}
inline const char *modes_name(int o) {
  return o == DPGO_MODES_CONVERGED ? "CONVERGED" : o == DPGO_MODES_MAX_ITERS ? "MAX_ITERS" : o == DPGO_MODES_STALLED ? "STALLED" : "SKIPPED";
}
inline const char *staircase_name(int o) {
  return o == DPGO_STAIR_SOLVED ? "SOLVED" : o == DPGO_STAIR_MAX_RANK ? "MAX_RANK" : o == DPGO_STAIR_SADDLE ? "SADDLE" : "SKIPPED";
}
inline const char *gnc_name(int o) {
  return o == DPGO_GNC_CONVERGED ? "CONVERGED" : o == DPGO_GNC_ALL_INLIERS ? "ALL_INLIERS" : o == DPGO_GNC_MAX_LEVELS ? "MAX_LEVELS"
         : o == DPGO_GNC_INNER_FAILED ? "INNER_FAILED" : "SKIPPED";
}
// (PROVEN comes from dpgo_group_verify and dpgo_graph_verify_reweighted only: dpgo_group_certify never returns it)
inline const char *cert_status_name(int s) {
  return s == DPGO_CERT_PROVEN ? "PROVEN" : s == DPGO_CERT_NEGATIVE ? "NEGATIVE" : s == DPGO_CERT_NONNEGATIVE ? "NONNEGATIVE" : "UNDECIDED";
}
inline const char *cert_factor_name(int o) { return o == DPGO_CERT_FACTOR_PD ? "PD" : o == DPGO_CERT_FACTOR_NOT_PD ? "NOT_PD" : "SKIPPED"; }
inline const char *cov_name(int o) { return o == DPGO_COV_OK ? "OK" : o == DPGO_COV_NOT_PD ? "NOT_PD" : "SKIPPED"; }
inline const char *pairs_name(int o) { return o == DPGO_PAIRS_OK ? "OK" : o == DPGO_PAIRS_NOT_PD ? "NOT_PD" : "SKIPPED"; }
inline const char *sens_name(int o) { return o == DPGO_SENS_OK ? "OK" : o == DPGO_SENS_NOT_PD ? "NOT_PD" : "SKIPPED"; }
inline const char *rely_name(int o) { return o == DPGO_RELY_OK ? "OK" : o == DPGO_RELY_NOT_PD ? "NOT_PD" : "SKIPPED"; }
inline const char *rely_method_name(int m) { return m == DPGO_RELY_SELINV ? "SELINV" : m == DPGO_RELY_SOLVE ? "SOLVE" : "AUTO"; }
inline const char *marg_name(int o) { return o == DPGO_MARG_OK ? "OK" : o == DPGO_MARG_NOT_PD ? "NOT_PD" : "SKIPPED"; }
inline const char *cand_name(int o) { return o == DPGO_CAND_OK ? "OK" : o == DPGO_CAND_NOT_PD ? "NOT_PD" : "SKIPPED"; }

// ---- the writers (17 digits throughout)
// open a report for writing, or say on stderr that it cannot be written
inline FILE *open_report(const char *path) {
  FILE *f = fopen(path, "w");
  if (!f) fprintf(stderr, "Cannot write %s.\n", path);
  return f;
}

// the upper triangle of one dof x dof block, row by row, every value behind a blank
inline void write_upper(FILE *f, const double *B, int dof) {
  for (int a = 0; a < dof; a++)
    for (int b = a; b < dof; b++) fprintf(f, " %.17g", B[(size_t)a * dof + b]);
}

// a dense n x n matrix, one line per row
inline void write_matrix(FILE *f, const double *M, int n) {
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < n; j++) fprintf(f, "%s%.17g", j ? " " : "", M[(size_t)i * n + j]);
    fprintf(f, "\n");
  }
}

// one line per edge: e i j inter, then rows x width values out of sens[(a * m + e) * width + b]
inline void write_sensitivity_rows(FILE *f, int m, const int *I, const int *J, const unsigned char *inter, const double *sens, int rows,
                                   int width) {
  for (int e = 0; e < m; e++) {
    fprintf(f, "%d %d %d %d", e, I[e], J[e], (int)inter[e]);
    for (int a = 0; a < rows; a++)
      for (int b = 0; b < width; b++) fprintf(f, " %.17g", sens[((size_t)a * m + e) * width + b]);
    fprintf(f, "\n");
  }
}

}   // namespace report
