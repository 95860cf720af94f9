// LDS-resident fused ADMM path: kernel instantiations and launches (own translation unit: the library builds in parallel).
#define MG_LDS_UNIT 0     // MGADMM_Q_LDS_UNIT: this unit's launches report the kernels k_admm_lds
#include "lds_dispatch.h"
#include "lds_metric_kernels.h"

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

template <int NT>
static void lds_metrics_launch(const LdsMetricArgs& a, int wgs, hipStream_t st) {
    const int TN = a.T * a.N, nsl = (a.B + 63) / 64;
    const bool vec4 = TN % 4 == 0 && ((uintptr_t)a.x % 16) == 0 && ((uintptr_t)a.xo % 16) == 0;
    const long long tasks = (long long)(vec4 ? TN / 4 : TN) * nsl;
    const long long full = (tasks + NT - 1) / NT;
    const int grid = (int)(wgs > 0 && wgs < full ? wgs : full);
    if (vec4) hipLaunchKernelGGL((k_lds_metric_pass<4, NT>), dim3(grid), dim3(NT), 0, st, TN, a.B, a.x, a.xo, a.scratch, a.stop);
    else hipLaunchKernelGGL((k_lds_metric_pass<1, NT>), dim3(grid), dim3(NT), 0, st, TN, a.B, a.x, a.xo, a.scratch, a.stop);
    constexpr int NF = NT < 256 ? NT : 256;      // (the tree of the final has 256 leaves)
    hipLaunchKernelGGL((k_lds_metric_final<NF>), dim3(a.T + MGADMM_NMETRIC), dim3(NF), 0, st, a.T, a.N, a.B, a.Bp, nsl,
                       (const double*)a.scratch, a.dxps, a.stop, a.ps, a.out, a.out_ps);
}

int mg_lds_metrics(const LdsMetricArgs& a, const LdsMetricShape& shape, hipStream_t st) {
    switch (shape.threads) {
        case 64: lds_metrics_launch<64>(a, shape.wgs, st); break;
        case 256: lds_metrics_launch<256>(a, shape.wgs, st); break;
        case 512: lds_metrics_launch<512>(a, shape.wgs, st); break;
        default: mg_set_error("lds: metric pass with workgroups of %d threads (64, 256 or 512)", shape.threads); return MGADMM_ERR_INVALID;
    }
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
