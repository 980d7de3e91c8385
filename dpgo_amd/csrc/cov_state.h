// The covariance's pattern, factor and maps (cov.cpp), allocated by a group's first covariance or polish call; polish.cpp
// factors the same matrix in the same numeric context and keeps its vectors here.
#pragma once
#include <vector>

#include "group.h"
#include "spd.h"

namespace dpgo {

struct Group::CovState {
  CsrMatrix A;                 // ptr / col only, unknowns dof p + a (p the unified own row): the values are written on the device
  std::vector<int> bcol_h;     // per block of the certificate's pattern: the unified own row of its columns
  DevBuf<int> bcol;
  SpdFactor F;
  std::vector<int> piv_front, piv_loc;   // per unknown: the front that eliminates it, its position among that front's pivots
  bool have_symbolic = false;
  double symbolic_s = 0;
  // what the refusals count (hess.h: HessPart): the numeric phase with its W / WT panels and the block-column map, which the
  // first call that is not refused leaves on the device; the blocks of the selected inversion
  long long numeric_bytes = 0, selinv_bytes = 0;
  HessPart numeric_part() const { return {numeric_bytes, F.numeric ? 0 : numeric_bytes}; }
  // the Newton polish (polish.cpp): the tangent gradient, the right-hand side / solution of a step, the unshifted diagonal of
  // H -- dof doubles per own row each; the Hessian modes (modes.cpp) shift with the same diagonal and escape along g
  DevBuf<double> pol_g, pol_sol, pol_hdiag;
  ~CovState() {
    spd_release_numeric(F);
    spd_release_device(F);
  }
};

}  // namespace dpgo
