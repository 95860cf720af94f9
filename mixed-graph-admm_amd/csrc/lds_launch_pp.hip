// LDS-resident fused ADMM path: the k_admm_lds instances with per-sample ADMM weights (mgadmm_solver_set_sample_params), as
// kernels k_admm_lds_pp; with a schedule of weights (mgadmm_solver_set_param_schedule) a trip reads the record of its iteration's
// row as well (lds_param_table.h).  The per-sample stop test is compiled in as well and runs when the launch carries stop words.  Own
// translation unit: it compiles beside lds_launch.hip and lds_launch_ps.hip, whose instances stay what they were.
#define MGADMM_LDS_PER_SAMPLE_PARAMS 1
#define MG_LDS_UNIT 2     // MGADMM_Q_LDS_UNIT: this unit's launches report the kernels k_admm_lds_pp
#include "lds_args.h"

// Per-sample temporal band weights (mgadmm_solver_set_sample_bands, band_sets.h): LdsArgs::band_w holds the tables of S sets
// back to back, T * skip floats each, and workgroup b of a BAND instance reads the one of set bset[b] -- one workgroup-uniform
// base, formed once per trip from a scalar load of the set number through the constant address space (as MG_LDS_IMG forms the
// image base of a graph set); band_back / band_fwd read through LdsCtx::band_w as they read the graph's own table.  Instances
// without BAND never read band_w: for them the call is empty.
//
// Where the base is formed.  lds_kernels.h is the source of all three compilations and stays byte for byte what it is (the
// kernels k_admm_lds and k_admm_lds_ps are compiled from it, and tests/test_lds_adapt_cpu.py pins its hash), so this unit adds
// the statement from outside: the trip body sets LdsCtx::band_w from the launch arguments and then, before any operator runs,
// calls its local lambda fetch_t(); here that call is `mg_lds_band_of_sample(c, kp, b), fetch_t()`.  (c, kp and b are the
// trip body's context, pointer to the launch arguments and workgroup number; the lambda's own definition is followed by `=`,
// not `(`, and is left alone.)
template <int TPG, bool BAND, int NU, int ND, int TP>
struct LdsCtx;
template <class Ctx, class Args>
__device__ __forceinline__ void mg_lds_band_of_sample(Ctx&, Args, int) {}
template <int TPG, int NU, int ND, int TP, class Args>
__device__ __forceinline__ void mg_lds_band_of_sample(LdsCtx<TPG, true, NU, ND, TP>& c, Args a, int b) {
    if (a->bset == nullptr) return;
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned set = (unsigned)((const int __attribute__((address_space(4)))*)a->bset)[b];
#else
    const unsigned set = (unsigned)a->bset[b];
#endif
    c.band_w = a->band_w + (size_t)(unsigned)(a->T * a->skip) * (size_t)set;
}
#define fetch_t() (mg_lds_band_of_sample(c, kp, b), fetch_t())
#include "lds_dispatch.h"
#undef fetch_t

int mg_lds_iteration_pp(const LdsLaunch& L, const LdsArgs& a, int B, hipStream_t st) { return lds_dispatch(L, a, B, st); }
