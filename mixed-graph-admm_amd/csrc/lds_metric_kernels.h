// Whole-batch metric kernels of the LDS path (launched by lds_launch.hip, mg_lds_metrics; driven by LdsEngine::lds_batch_metrics):
// the whole-batch metrics of one ADMM iteration on the sample-major layout in two launches, k_lds_metric_pass and
// k_lds_metric_final, with the operations and the order of additions of the five they replace -- k_dxps_sm4 / k_dxps_sm,
// k_dxps_sm_mean, k_dxps_sm_final (lds_kernels.h, no longer launched) and k_batch_metrics (stream_kernels.h, still the streaming
// path's): every value is the same bit for bit.
#pragma once
#include "lds_kernels.h"

// Pass: task (b-slice, column of V consecutive elements) sums x - x_old over the 64 samples of its slice in ascending order,
// in double -> part[slice][e].  V = 4: 16-byte loads (T*N a multiple of 4 and 16-byte aligned vectors), eight samples of
// either vector in flight per lane; V = 1: any T*N.  The tasks are spread over the grid with a grid stride, so the launch
// decides how many workgroups of NT threads carry the pass: in the overlapped schedule of the outer loop (LdsEngine::
// lds_run_chunks) it runs beside the k_admm_lds launch of the next chunks, whose 15-wave workgroup leaves room for single
// waves of at most 128 VGPRs only (three of the four SIMDs of a CU are full; a workgroup of several waves waits for a CU
// without a k_admm_lds workgroup, 1.35 ms on average at cfg2: profiles/r17), and after the last chunk on an idle GPU.
template <int V, int NT>
__global__ __launch_bounds__(NT) void k_lds_metric_pass(int TN, int B, const float* __restrict__ x, const float* __restrict__ xo,
                                                        double* __restrict__ part, const int* __restrict__ stop) {
    if (stop != nullptr && *stop != 0) return;
    const int ncol = TN / V, nsl = (B + 63) / 64;
    const long long total = (long long)ncol * nsl;
    for (long long q = (long long)blockIdx.x * NT + threadIdx.x; q < total; q += (long long)gridDim.x * NT) {
        const int sl = (int)(q / ncol), e = (int)(q - (long long)sl * ncol) * V;
        const int b0 = sl * 64, b1 = min(B, b0 + 64);
        double* const dst = part + (size_t)sl * TN + e;
        if constexpr (V == 4) {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            int b = b0;
            for (; b + 8 <= b1; b += 8) {
                lds_f4 a[8], o[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    a[u] = *reinterpret_cast<const lds_f4*>(x + (size_t)(b + u) * TN + e);
                    o[u] = *reinterpret_cast<const lds_f4*>(xo + (size_t)(b + u) * TN + e);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    s0 += (double)a[u].x - (double)o[u].x;
                    s1 += (double)a[u].y - (double)o[u].y;
                    s2 += (double)a[u].z - (double)o[u].z;
                    s3 += (double)a[u].w - (double)o[u].w;
                }
            }
            for (; b < b1; ++b) {
                const lds_f4 a = *reinterpret_cast<const lds_f4*>(x + (size_t)b * TN + e);
                const lds_f4 o = *reinterpret_cast<const lds_f4*>(xo + (size_t)b * TN + e);
                s0 += (double)a.x - (double)o.x;
                s1 += (double)a.y - (double)o.y;
                s2 += (double)a.z - (double)o.z;
                s3 += (double)a.w - (double)o.w;
            }
            dst[0] = s0; dst[1] = s1; dst[2] = s2; dst[3] = s3;
        } else {
            double s = 0.0;
            for (int b = b0; b < b1; ++b) s += (double)x[(size_t)b * TN + e] - (double)xo[(size_t)b * TN + e];
            dst[0] = s;
        }
    }
}

// Final: workgroup t < T forms delta_x_per_step[t] -- per node the sum of the slices in ascending order, the mean over the
// samples and its square, then the norm over the nodes of time step t; workgroup T + m the whole-batch value of metric m from
// the per-sample sums ps[m][.] (norms -> sqrt(sum_b), regularisers -> mean_b; out_ps: a copy of the sums, [NMETRIC][B], or
// nullptr).  Either sum is the one over 256 strided partial sums and a binary tree that k_dxps_sm_final and k_batch_metrics
// took with 256 threads: NT threads (64: a single wave beside k_admm_lds, 256) each form the partial sums j = thread,
// thread + NT, ... and take the same tree.  The square was stored to memory between two kernels and must not contract with
// the sum that follows (contract(off); __dmul_rn is a plain product here, and one delta_x_per_step value in 384 moved by an
// ulp at cfg2 / B = 96).
template <int NT>
__global__ __launch_bounds__(NT) void k_lds_metric_final(int T, int N, int B, int Bp, int nslices, const double* __restrict__ part,
                                                         double* __restrict__ dxps, const int* __restrict__ stop,
                                                         const double* __restrict__ ps, double* __restrict__ out,
                                                         double* __restrict__ out_ps) {
#pragma clang fp contract(off)
    __shared__ double sm[256];
    const int t = blockIdx.x, TN = T * N;
    const bool is_dx = t < T;
    if (is_dx && stop != nullptr && *stop != 0) return;          // uniform
    const int m = t - T;
    for (int j = threadIdx.x; j < 256; j += NT) {
        double acc = 0.0;
        if (is_dx) {
            for (int i = j; i < N; i += 256) {
                const int e = t * N + i;
                double s = 0.0;
                int k = 0;
                for (; k + 8 <= nslices; k += 8) {        // eight slices per trip in flight; same order of additions
                    double v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(k + u) * TN + e];
#pragma unroll
                    for (int u = 0; u < 8; ++u) s += v[u];
                }
                for (; k < nslices; ++k) s += part[(size_t)k * TN + e];
                s /= (double)B;
                acc += s * s;
            }
        } else {
            for (int c = j; c < B; c += 256) {
                const double v = ps[(size_t)m * Bp + c];
                acc += v;
                if (out_ps) out_ps[(size_t)m * B + c] = v;
            }
        }
        sm[j] = acc;
    }
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        for (int j = threadIdx.x; j < w; j += NT) sm[j] += sm[j + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (is_dx) dxps[t] = sqrt(sm[0]);
        else {
            const double tot = sm[0];
            const bool is_mean = (m == MGADMM_M_GLR || m == MGADMM_M_DGTV || m == MGADMM_M_DGLR);
            out[m] = is_mean ? tot / (double)B : sqrt(tot);
        }
    }
}
