// block_fam.hip — compiled once per family (-DCOVGRAM_FAM=<covgram_family>, 11 / 12 = the composite pseudo-families): exports
// launch_bm_family_<FAM> (gradient / value-gradient blocks) and, for the families with a Hessian MVM (EQ, RQ, Cauchy, IMQ, Dot,
// ExponentialDot), launch_bmh_family_<FAM> (Hessian / value-gradient-Hessian blocks).
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
#if COVGRAM_FAM == 0 || COVGRAM_FAM == 2 || COVGRAM_FAM == 4 || COVGRAM_FAM == 5 || COVGRAM_FAM == 7 || COVGRAM_FAM == 8
int CG_CAT(launch_bmh_family_, COVGRAM_FAM)(const BlockMatArgs& a, int dtype) {
    return launch_bm_family<COVGRAM_FAM, true>(a, dtype);
}
#endif
}  // namespace covgram
