// vgh_fam.hip — compiled once per family that has a value-gradient-Hessian MVM (-DCOVGRAM_FAM=<covgram_family>: EQ, RQ, Cauchy, IMQ,
// Dot, ExponentialDot: the families of hess_fam.hip); exports launch_vgh_family_<FAM>.
#include "vgh_mvm.hpp"

#ifndef COVGRAM_FAM
#error "compile with -DCOVGRAM_FAM=<0, 2, 4, 5, 7, 8>"
#endif

namespace covgram {
#define CG_CAT2(a, b) a##b
#define CG_CAT(a, b) CG_CAT2(a, b)
int CG_CAT(launch_vgh_family_, COVGRAM_FAM)(const VghArgs& a, int dtype) {
    return launch_vgh_family<COVGRAM_FAM>(a, dtype);
}
}  // namespace covgram
