// The certificate's buffers (cert.cpp), allocated by a group's first certificate call; cov.cpp reads the pattern, M's
// values, Lambda and the records of X from it.
#pragma once
#include <vector>

#include "group.h"
#include "spd.h"

namespace dpgo {

struct Group::CertState {
  DevBuf<double> X, V, W, P;            // P0 + P1 rows: what a product with M reads (neighbour rows by the halo copy)
  DevBuf<double> MX, SV, SW, SP, tmp;   // P0 rows
  DevBuf<double> Lam, Tp, partials;
  double *h_sums = nullptr;             // pinned: what k_cert_reduce writes
  bool have_Tp = false;
  std::vector<int> gid;                 // unified own row -> global pose
  std::vector<int> row_of;              // ... and back (Group::own_row), with the pattern (cert_build_pattern)
  // STEP 1: the pattern of S on the unknowns (d+1) p + r (p the unified own row), M's values in that order, the factor
  CsrMatrix A;                          // ptr / col only: the values are written on the device
  std::vector<int> bptr_h;
  DevBuf<int> bptr, diag_pose;
  DevBuf<double> Mval;
  SpdFactor F;
  bool have_pattern = false, have_symbolic = false;
  double symbolic_s = 0;                // of the analysis, reported by the call that ran it
  long long factor_bytes = 0;
  ~CertState() {
    if (h_sums) (void)hipHostFree(h_sums);
    spd_release_numeric(F);
    spd_release_device(F);
  }
};

}  // namespace dpgo
