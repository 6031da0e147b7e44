// block_fam.hip — compiled once per family (-DCOVGRAM_FAM=<covgram_family>, 11 / 12 = the composite pseudo-families): exports
// launch_bm_family_<FAM> (gradient / value-gradient blocks) and, for the families with a Hessian MVM (COVGRAM_HESS_FAMILIES,
// hess_mvm.hpp), launch_bmh_family_<FAM> (Hessian / value-gradient-Hessian blocks).
#include "block_matrix.hpp"

#ifndef COVGRAM_FAM
#error "compile with -DCOVGRAM_FAM=<0..12>"
#endif

namespace covgram {
#define CG_CAT2(a, b) a##b
#define CG_CAT(a, b) CG_CAT2(a, b)
int CG_CAT(launch_bm_family_, COVGRAM_FAM)(const BlockMatArgs& a, int dtype) {
    return launch_bm_family<COVGRAM_FAM, false>(a, dtype);
}
#define CG_OR_FAM(name, n, arg) || COVGRAM_FAM == n
#if 0 COVGRAM_HESS_FAMILIES(CG_OR_FAM, )
int CG_CAT(launch_bmh_family_, COVGRAM_FAM)(const BlockMatArgs& a, int dtype) {
    return launch_bm_family<COVGRAM_FAM, true>(a, dtype);
}
#endif
}  // namespace covgram
