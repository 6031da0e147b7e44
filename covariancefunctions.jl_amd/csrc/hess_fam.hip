// hess_fam.hip — compiled once per family that has a Hessian MVM (-DCOVGRAM_FAM=<covgram_family>: EQ, RQ, Cauchy, IMQ, Dot,
// ExponentialDot); exports launch_hess_family_<FAM>.
#include "hess_mvm.hpp"

#ifndef COVGRAM_FAM
#error "compile with -DCOVGRAM_FAM=<0, 2, 4, 5, 7, 8>"
#endif

namespace covgram {
#define CG_CAT2(a, b) a##b
#define CG_CAT(a, b) CG_CAT2(a, b)
int CG_CAT(launch_hess_family_, COVGRAM_FAM)(const HessArgs& a, int dtype) {
    return launch_hess_family<COVGRAM_FAM>(a, dtype);
}
}  // namespace covgram
