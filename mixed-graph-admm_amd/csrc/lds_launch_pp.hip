// LDS-resident fused ADMM path: the k_admm_lds instances with per-sample ADMM weights (mgadmm_solver_set_sample_params), as
// kernels k_admm_lds_pp; with a schedule of weights (mgadmm_solver_set_param_schedule) a trip reads the record of its iteration's
// row as well (lds_param_table.h), and a BAND instance the band table of its sample's set (mgadmm_solver_set_sample_bands).  The
// per-sample stop test is compiled in as well and runs when the launch carries stop words.  Own translation unit: it compiles
// beside lds_launch.hip and lds_launch_ps.hip, whose instances stay what they were.
#define MGADMM_LDS_PER_SAMPLE_PARAMS 1
#define MG_LDS_UNIT 2     // MGADMM_Q_LDS_UNIT: this unit's launches report the kernels k_admm_lds_pp
#include "lds_dispatch.h"

int mg_lds_iteration_pp(const LdsLaunch& L, const LdsArgs& a, int B, hipStream_t st) { return lds_dispatch(L, a, B, st); }
