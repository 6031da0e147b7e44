// hess_fam.hip — compiled once per family of COVGRAM_HESS_FAMILIES (hess_mvm.hpp; -DCOVGRAM_FAM=<covgram_family>); exports
// launch_hess_family_<FAM> (Hessian MVM) and launch_vgh_family_<FAM> (value-gradient-Hessian MVM).
#include "hess_mvm.hpp"

#ifndef COVGRAM_FAM
#error "compile with -DCOVGRAM_FAM=<0, 2, 4, 5, 7, 8>"
#endif

namespace covgram {
#define CG_CAT2(a, b) a##b
#define CG_CAT(a, b) CG_CAT2(a, b)
int CG_CAT(launch_hess_family_, COVGRAM_FAM)(const HessArgs& a, int dtype) {
    return launch_hess_family<COVGRAM_FAM, false>(a, dtype);
}
int CG_CAT(launch_vgh_family_, COVGRAM_FAM)(const HessArgs& a, int dtype) {
    return launch_hess_family<COVGRAM_FAM, true>(a, dtype);
}
}  // namespace covgram
