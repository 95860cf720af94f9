// LDS-resident fused ADMM path: kernel instantiations and launches (own translation unit: the library builds in parallel).
#define MG_LDS_UNIT 0     // MGADMM_Q_LDS_UNIT: this unit's launches report the kernels k_admm_lds
#include "lds_dispatch.h"

int mg_lds_iteration(const LdsLaunch& L, const LdsArgs& a, int B, hipStream_t st) {
    // a launch that carries per-sample weights takes the instances that read them (lds_launch_pp.hip),
    // a launch that carries per-sample stop words the instances with the stop test (lds_launch_ps.hip)
    if (a.sp != nullptr) return mg_lds_iteration_pp(L, a, B, st);
    return a.pstop != nullptr ? mg_lds_iteration_ps(L, a, B, st) : lds_dispatch(L, a, B, st);
}

int mg_lds_init(bool masked, int T, int t_in, int N, int TPG, int B, float tm, float den, const float* y, const float* mask, float* x,
                float* zu, float* zd, float* gam, float* gu, float* gd, int* nonfinite, const int* row_of_node, hipStream_t st) {
    dim3 grid((N + 255) / 256, B);
    if (masked) hipLaunchKernelGGL((k_init_lds<true>), grid, dim3(256), 0, st, T, t_in, N, TPG, B, tm, den, y, mask, x, zu, zd, gam, gu, gd, nonfinite, row_of_node);
    else hipLaunchKernelGGL((k_init_lds<false>), grid, dim3(256), 0, st, T, t_in, N, TPG, B, tm, den, y, (const float*)nullptr, x, zu, zd, gam, gu, gd, nonfinite, row_of_node);
    MG_HIP(hipGetLastError());
    return MGADMM_OK;
}

int mg_lds_state_layout(bool to_thread_major, int T, int N, int TPG, int B, const float* src, float* dst, const int* row_of_node, hipStream_t st) {
    dim3 grid((T * N + 255) / 256, B);
    if (to_thread_major) hipLaunchKernelGGL((k_state_layout<true>), grid, dim3(256), 0, st, T, N, TPG, src, dst, row_of_node);
    else hipLaunchKernelGGL((k_state_layout<false>), grid, dim3(256), 0, st, T, N, TPG, src, dst, row_of_node);
    MG_HIP(hipGetLastError());
    return MGADMM_OK;
}

int mg_lds_dxps(int T, int N, int B, const float* x, const float* xo, double* scratch, double* out, const int* stop, hipStream_t st) {
    const int TN = T * N, nsl = (B + 63) / 64;
    if (TN % 4 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)xo % 16) == 0)
        hipLaunchKernelGGL(k_dxps_sm4, dim3((TN / 4 + 63) / 64, nsl), dim3(64), 0, st, TN, B, x, xo, scratch + TN, stop);
    else
        hipLaunchKernelGGL(k_dxps_sm, dim3((TN + 255) / 256, nsl), dim3(256), 0, st, TN, B, x, xo, scratch + TN, stop);
    hipLaunchKernelGGL(k_dxps_sm_mean, dim3((TN + 255) / 256), dim3(256), 0, st, TN, B, nsl, (const double*)(scratch + TN), scratch, stop);
    hipLaunchKernelGGL(k_dxps_sm_final, dim3(T), dim3(256), 0, st, T, N, (const double*)scratch, out, stop);
    MG_HIP(hipGetLastError());
    return MGADMM_OK;
}

int mg_lds_stop_test(const double* metrics_row, const int* nonfinite, int has_phi, int has_zd, double tol, int it, int* stop, hipStream_t st) {
    hipLaunchKernelGGL(k_lds_stop_test, dim3(1), dim3(64), 0, st, metrics_row, nonfinite, has_phi, has_zd, tol, it, stop);
    MG_HIP(hipGetLastError());
    return MGADMM_OK;
}

int mg_lds_ps_history(const double* ps, const int* pstop, int n_it, int max_it, int B, int Bp, int* n_per_sample, double* metrics,
                      double* out_ps, hipStream_t st) {
    hipLaunchKernelGGL(k_lds_ps_history, dim3(n_it, MGADMM_NMETRIC), dim3(256), 0, st, ps, pstop, max_it, B, Bp, n_per_sample, metrics, out_ps);
    MG_HIP(hipGetLastError());
    return MGADMM_OK;
}

__global__ __launch_bounds__(256) void k_lds_adapt(const LdsAdaptArgs a) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= a.B) return;
    if (a.pstop != nullptr && a.pstop[b] != 0) return;      // a stopped sample keeps its history NaN from here on
    static_assert(MGADMM_M_DUAL_ZD == MGADMM_M_PRI_ZU + 5, "the six residual sums are consecutive metrics");
    double res[6], w[ldsparam::NW];
    for (int k = 0; k < 6; ++k) res[k] = a.ps[(size_t)(MGADMM_M_PRI_ZU + k) * a.Bp + b];
    for (int f = 0; f < ldsparam::NW; ++f) w[f] = a.w[(size_t)f * a.B + b];
    ldsadapt::step(w, res, a.has_phi, a.has_zd, a.q);
    for (int f = 0; f < 3; ++f) {
        a.w[(size_t)f * a.B + b] = w[f];
        a.hist[(size_t)f * a.B + b] = w[f];
    }
    const LdsSampleParams rec = ldsparam::record_of(a.ablation, w);
    for (int row = a.row_first; row < a.row_last; ++row) a.table[(size_t)row * a.B + b] = rec;
}

int mg_lds_adapt(const LdsAdaptArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_lds_adapt, dim3((a.B + 255) / 256), dim3(256), 0, st, a);
    MG_HIP(hipGetLastError());
    return MGADMM_OK;
}
