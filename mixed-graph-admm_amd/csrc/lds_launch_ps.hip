// LDS-resident fused ADMM path: the k_admm_lds instances with the per-sample stop test of the outer loop
// (MGADMM_ADMM_PER_SAMPLE), as kernels k_admm_lds_ps.  Own translation unit: it compiles beside lds_launch.hip, whose
// instances stay what they were.
#define MGADMM_LDS_PER_SAMPLE_STOP 1
#define MG_LDS_UNIT 1     // MGADMM_Q_LDS_UNIT: this unit's launches report the kernels k_admm_lds_ps
#include "lds_dispatch.h"

int mg_lds_iteration_ps(const LdsLaunch& L, const LdsArgs& a, int B, hipStream_t st) { return lds_dispatch(L, a, B, st); }
