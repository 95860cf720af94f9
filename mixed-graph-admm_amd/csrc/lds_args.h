// Launch interface of the LDS-resident fused path (kernels in lds_kernels.h, compiled in lds_launch.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "lds_consts.h"     // LDS_NLEAD, LDS_MAXJ, lds_instance_key
#include "lds_param_table.h"   // LdsSampleParams, sched_row
#include "lds_adapt.h"         // ldsadapt::Params

// scalar part of the launch arguments: a trip of the loop inside k_admm_lds reads it from the kernarg segment
struct LdsArgsCore {
    int T, N, TN, TS, t_in, G, B, Bp;   // TS: LDS row stride (floats) of a node's time row, >= T
    int nthreads;          // N * G threads own elements; the other threads of the workgroup are GHOSTS: they own an LDS row
                           // of zeros (rows N .. NR-1) and table rows of zero weights, and run the same instruction stream
    int NR;                // LDS rows of an image: N + ghosts
    int has_phi, has_zd, first;
    int J;                 // ADMM iterations this launch runs on every sample (trips of the loop inside k_admm_lds), 1 .. LDS_MAXJ
    int lhsx_kind;         // 1: LHS_x contains cLdr, 0: diagonal ('DGTV'/'UT')
    int band, skip, q1;
    int max_cg;
    int record;            // alpha/beta history
    int stagger_wgs, stagger_ticks;   // the first `stagger_wgs` workgroups start up to `stagger_ticks` (10 ns) late, see k_admm_lds
    int tail_pairs;        // W_d^T rows: entries beyond the LDS_NLEAD leading ones, padded to 2 * tail_pairs per row
    float rho, rho_u, rho_d, mu_u, mu_d1, mu_d2;
    float cx1, cx2;        // LHS_x = HtH + cx1*I + cx2*cLdr
    double cg_tol2;        // CG_tol squared: a solve stops when r.r < CG_tol^2 (ADMM.py:360 without the square root)
    // graph image (global), ints: [rp_u NR+1][rp_d NR+1][pad][ent_u][ent_d][lead_t NR*LDS_NLEAD][tail_t NR*2*tail_pairs][diag 2 NR][pad];
    // entries are {LDS float offset of the neighbour's row, weight}.  The part [lds_img0, lds_img0 + lds_img_ints) is copied
    // to LDS by every workgroup (all of it, or -- instances that read the fixed-length rows from the global image once per
    // solve -- the tail table alone); off_* are offsets into the global image
    const int* csr;
    int lds_img0, lds_img_ints;
    int off_rp_u, off_rp_d, off_en_u, off_en_d, off_lead_t, off_tail_t;
    int off_diag;          // [NR] diagonal of W_d (uniform instances: their W_d rows hold the other entries; else 0) and [NR] of W_d^T, floats
    const float* band_w;   // [T*skip] (band mode)
    // state, sample-major (B, TN)
    float *zu, *zd, *phi, *gam, *gu, *gd;
    const float* y;        // (B, t_in, N) prediction / (B, T, N) mask mode
    const float* mask;     // (B, T, N) or nullptr
    // outputs
    double* ps;            // [J][NMETRIC][Bp] per-sample metric sums
    int* cg_iters;         // [J][3][Bp]
    float* alpha_hist;     // [3][max_cg][Bp] or nullptr
    float* beta_hist;
    int* nonfinite;
    const int* stop;       // device stop word of the ADMM outer loop (nullptr: none): a launch enqueued speculatively after the
                           // stop test of an earlier iteration passed returns at its first instruction
};
struct LdsArgs : LdsArgsCore {
    float* xs[LDS_MAXJ + 1];   // trip k reads the iterate xs[k] and writes xs[k + 1] (every iterate is kept: delta_x_per_step);
                               // indexed by the trip number straight from the kernarg segment
    // Per-sample stop of the outer loop (MGADMM_ADMM_PER_SAMPLE with check_stop; read by the kernels k_admm_lds_ps only, which a
    // launch takes when pstop != nullptr; behind xs: the offsets of everything k_admm_lds reads stay what they were): the workgroup tests its own sample after every trip
    int* pstop;            // [Bp] stop word of every sample: 0 = running, n_b = iterations it ran once it has stopped; a workgroup
                           // whose word is set returns at its first instruction
    int* pstop_count;      // number of samples that have stopped (the host ends the solve when it reads B)
    float* x_final;        // (B, TN): a sample that stops stores its iterate here itself (the iterate buffers of a chunk rotate)
    double admm_tol;       // ADMM_tol
    int it0;               // number of the launch's first iteration in this solve (n_b = it0 + trip + 1; the row of a weight schedule)
    // Per-sample weights (read by the kernels k_admm_lds_pp only, which a launch takes when sp != nullptr; behind everything the
    // other kernels read): workgroup b takes rho .. cx2 from sp[b] instead of the scalars above.  In these kernels the
    // per-sample stop test runs when pstop != nullptr
    const LdsSampleParams* sp;   // [B] device table ([sp_rows][sp_stride] with a schedule of weights, below)
    // Row plan of the uniform-row instances with a compile-time tail (lds_rows.h; read by those instances only; behind everything
    // else: no offset that existing code reads moves)
    unsigned long long npos;     // 4-bit field w: positions of the W_d^T table (leading entries + tail) wave w gathers -- the largest
                                 // in-degree among its rows; the table width when the rows are in node order
    int off_node;                // offset in the global image of node_of_row[NR]: the node in HBM of LDS row r (ghost rows: 0)
    // Per-sample graph weights (mgadmm_solver_set_sample_graphs; read by the kernels k_admm_lds_pp only; behind everything else):
    // csr then holds the images of S weight sets of one topology, set s at csr + s * img_stride, and workgroup b reads the
    // weights of set gset[b] (lds_graph_sets.h)
    int img_stride;              // ints between two images
    const int* gset;             // [Bp] device table, or nullptr: every workgroup reads set 0
    // Per-iteration weights (mgadmm_solver_set_param_schedule, lds_param_table.h; read by the kernels k_admm_lds_pp only; behind
    // everything else): sp then holds sp_rows rows of records, record row * sp_stride + b, and trip k of the launch reads row
    // sched_row(it0 + k, sp_row0, sp_rows).  Zero (no schedule): every trip reads sp[b]
    int sp_rows{}, sp_row0{}, sp_stride{};   // rows of the table, row of the solve's first iteration, records between two rows
    // Per-sample temporal band weights (mgadmm_solver_set_sample_bands, band_sets.h; read by the BAND instances of the kernels
    // k_admm_lds_pp only; behind everything else): band_w then holds the tables of S sets back to back, T * skip floats each, and
    // workgroup b reads the one of set bset[b]
    const int* bset{nullptr};    // [Bp] device table, or nullptr: band_w is the graph's own table
};

// Execution plan of k_admm_lds chosen by ldsplan::make (lds_plan.h)
struct LdsLaunch {
    int64_t key;    // lds_instance_key of the instance: time steps per thread, band mode, workgroup-size class (640 / 1024),
                    // single LDS vector, uniform rows (4 entries per W_u row, 5 per W_d row: unrolled gathers, entries read
                    // from the global image once per solve), slot vectors for per-thread operands, compile-time tail pairs
    int block;      // threads per workgroup
    size_t lds_bytes;
    int64_t* instance;  // receives the packed template arguments of the instance launched (MGADMM_Q_LDS_INSTANCE), or nullptr
    int* unit;          // receives the translation unit whose kernel was launched (MGADMM_Q_LDS_UNIT: 0 k_admm_lds, 1 k_admm_lds_ps,
                        // 2 k_admm_lds_pp), or nullptr
};

// J ADMM iterations for B samples (one workgroup per sample); returns a mgadmm_status
int mg_lds_iteration(const LdsLaunch& L, const LdsArgs& a, int B, hipStream_t st);
// the same with the per-sample stop test (a.pstop != nullptr; mg_lds_iteration forwards to it)
int mg_lds_iteration_ps(const LdsLaunch& L, const LdsArgs& a, int B, hipStream_t st);
// the same with per-sample weights (a.sp != nullptr; mg_lds_iteration forwards to it), with or without the stop test
int mg_lds_iteration_pp(const LdsLaunch& L, const LdsArgs& a, int B, hipStream_t st);
// initial state (ADMM.py:528-544): x in the reference's sample-major layout, zu / zd / gamma* thread-major for time groups of TPG steps
// (in row order: row_of_node as in mg_lds_state_layout)
int mg_lds_init(bool masked, int T, int t_in, int N, int TPG, int B, float tm, float den, const float* y, const float* mask, float* x,
                float* zu, float* zd, float* gam, float* gu, float* gd, int* nonfinite, const int* row_of_node, hipStream_t st);
// one state vector (B, T, N) <-> thread-major layout of the LDS path (lds_kernels.h, lds_state_index); src != dst
// row_of_node (device, [N]; nullptr = identity): the thread-major vectors are in ROW order (the thread of row r owns node
// node_of_row[r]), what a caller imports / exports stays in node order
int mg_lds_state_layout(bool to_thread_major, int T, int N, int TPG, int B, const float* src, float* dst, const int* row_of_node, hipStream_t st);
// The whole-batch metrics of one ADMM iteration in two launches (k_lds_metric_pass, k_lds_metric_final): delta_x_per_step on
// the sample-major layout (ADMM.py:614) and the whole-batch value of every metric from the per-sample sums (ADMM.py:612-637)
struct LdsMetricArgs {
    int T, N, B, Bp;
    const float *x, *xo;       // iterate k + 1 and iterate k, (B, T*N)
    double* scratch;           // double[T*N * ceil(B/64)]: the sums of every 64-sample slice
    double* dxps;              // double[T]
    const int* stop;           // device stop word (the delta_x_per_step half returns at once when it is set) or nullptr
    const double* ps;          // [NMETRIC][Bp] per-sample sums
    double* out;               // [NMETRIC]
    double* out_ps;            // [NMETRIC][B] copy of the sums, or nullptr
};
// How the two launches are cut into workgroups.  Beside a k_admm_lds launch (busy) only single waves find room on a CU, and
// the fewer CUs they touch the better; on an idle GPU the pass takes one task per thread and the whole device
struct LdsMetricShape {
    int threads;               // per workgroup: 64, 256 or 512
    int wgs;                   // workgroups of the pass, 0: one task per thread
};
int mg_lds_metrics(const LdsMetricArgs& a, const LdsMetricShape& shape, hipStream_t st);
// History of a solve that stopped per sample, from the stop words and the per-sample metric sums ps = [n_it][NMETRIC][Bp] of
// all n_it iterations enqueued: n_per_sample[b] = n_b (max_it for a sample that never stopped); metrics[n_it][NMETRIC] = the
// whole-batch values as if a stopped sample stood still (difference terms 0, the others as at its last iteration);
// out_ps (or nullptr) = [n_it][NMETRIC][B] the sums, NaN for the rows past n_b
int mg_lds_ps_history(const double* ps, const int* pstop, int n_it, int max_it, int B, int Bp, int* n_per_sample, double* metrics,
                      double* out_ps, hipStream_t st);
// stop test of one ADMM iteration on the device (ADMM.py:645-646 + the NaN asserts): *stop = it + 1 when both residual maxima
// are below tol, -(it + 1) when a metric or the iterate is not finite; leaves a stop word that is already set alone
int mg_lds_stop_test(const double* metrics_row, const int* nonfinite, int has_phi, int has_zd, double tol, int it, int* stop, hipStream_t st);
// One adaptation step of the penalties (lds_adapt.h), one thread per sample, between two launches of k_admm_lds_pp on the same
// stream.  A sample whose stop word is set is left alone; every other sample balances its three penalties on the six residual
// sums of the period's last iteration, keeps them in `w`, writes its records of rows [row_first, row_last) of the weight table
// through ldsparam::record_of and appends the penalties to the history.  Plain vector stores only
struct LdsAdaptArgs {
    const double* ps;          // [NMETRIC][Bp] per-sample sums of the period's last iteration
    const int* pstop;          // [Bp] per-sample stop words, or nullptr
    double* w;                 // [6][B] the six weights of every sample, as doubles (the three mus never change)
    LdsSampleParams* table;    // [rows][B] records, row = iteration of the solve
    double* hist;              // [3][B] row of the history this step appends
    int B, Bp, row_first, row_last, ablation, has_phi, has_zd;
    ldsadapt::Params q;
};
int mg_lds_adapt(const LdsAdaptArgs& a, hipStream_t st);
