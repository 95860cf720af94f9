// Internal declarations shared by the HIP translation units of libmgadmm.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <utility>
#include <vector>

#include "mgadmm.h"

void mg_set_error(const char* fmt, ...);

#define MG_HIP(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            mg_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_));    \
            return MGADMM_ERR_HIP;                                                             \
        }                                                                                      \
    } while (0)

#define MG_REQUIRE(cond, ...)                                                                  \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            mg_set_error(__VA_ARGS__);                                                         \
            return MGADMM_ERR_INVALID;                                                         \
        }                                                                                      \
    } while (0)

#define MG_TRY(x)                                                                              \
    do {                                                                                       \
        int rc_ = (x);                                                                         \
        if (rc_ != MGADMM_OK) return rc_;                                                      \
    } while (0)

// a Buf's error code (dev_buf.h: what DevMem / PinnedMem returned, or BUF_TOO_LARGE) as the status MG_HIP gives a failed HIP call
#define MG_BUF(x)                                                                              \
    do {                                                                                       \
        int e_ = (x);                                                                          \
        if (e_ != 0) {                                                                         \
            mg_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #x, mg_buf_error(e_));         \
            return MGADMM_ERR_HIP;                                                             \
        }                                                                                      \
    } while (0)

#include "dev_buf.h"
#include "host_csr.h"

// ---- who owns device memory: Buf (dev_buf.h) over these two policies, and the two handles below.  Every owner releases in
// its destructor; the destructors of the engines and mgadmm_graph_destroy select the device first.
struct DevMem {
    static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static int to_device(void* dst, const void* src, size_t bytes) { return (int)hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
    static void release(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
    static int alloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static int to_device(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
    static void release(void* p) { (void)hipHostFree(p); }
};
template <class T> using DevBuf = Buf<T, DevMem>;
template <class T> using PinnedBuf = Buf<T, PinnedMem>;
inline const char* mg_buf_error(int e) { return e == BUF_TOO_LARGE ? "size overflows size_t" : hipGetErrorString((hipError_t)e); }

// move-only owner of an event or a stream: created through put(), read as the plain handle
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
    Handle& operator=(Handle&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Handle() { if (h) (void)Destroy(h); }
    H* put() { return &h; }
    operator H() const { return h; }
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

struct DevCsr {
    int n = 0, nnz = 0, max_row = 0, avg_row_ceil = 0;
    DevBuf<int> rowptr, col;
    DevBuf<float> val;
};

// How a row-operator is evaluated by the row kernels (see k_rows in stream_kernels.h).
enum OpKind { OPK_NONE = 0, OPK_SPATIAL = 1, OPK_BAND = 2 };
enum SelfMode { SELF_ONE = 0, SELF_LDR = 1, SELF_LDRT = 2, SELF_LN_FATHER = 3 };   // LN_FATHER: 1 for t <= T-2, else 0

struct OpDesc {
    int kind;             // OpKind
    const int* rowptr;    // SPATIAL: CSR of the neighbour weights (internal node order)
    const int* col;
    const float* val;
    int shift;            // SPATIAL: time offset of the gathered rows (0, -1, +1)
    const float* band_w;  // BAND: [T*skip]
    int skip;
    int band_dir;         // BAND: -1 = Ldr (looks back), +1 = Ldr_T (looks forward)
    int self_mode;        // SelfMode
    int q1;               // SELF_LDRT: keep the identity on the t=0 block (quirk Q1)
    const double* self_w; // optional per-row factor of the self coefficient (apply_op_Ln: row sums of d_ew); plain row kernel only
    const float* band_wb; // BAND, optional: [T*skip][Bp] a weight per batch column (mgadmm_solver_set_sample_bands) instead of band_w
    // SPATIAL, optional: time-varying weights (mgadmm_graph_set_time_weights, tv_values.h).  No kernel but k_rows_tv reads them
    const float* val_t;   // [n_slices][slice_stride] values per time slice on the pattern rowptr / col, then CSR_PAD entries
    int slice_stride;     // entries of a slice (= nnz)
    int n_slices;         // T (Lu) or T-1 (Ldr, Ldr^T)
};

struct mgadmm_graph {
    int N = 0, T = 0, mode = 0, device = 0;
    int transpose_by_gather = 0, q1 = 0, skip = 0;
    bool has_perm = false;
    int reorder = 0;              // 0 none, 1 RCM, 2 greedy cluster order (enables the LDS-tiled row kernel)
    HostCsr hWu, hWd, hWdT;       // API node order (hWdT: exact transpose, or hWd when transpose_by_gather)
    std::vector<int> perm, iperm;  // perm[i] = API node at internal row i; iperm = inverse
    std::vector<int> cluster_starts;  // reorder = 2: first internal row of every cluster of the node order
    DevCsr Wu, Wd, WdT;            // internal node order, device
    DevBuf<float> band_w;          // device
    DevBuf<double> ln_rowsum;      // device, internal order: sum_j d_ew[i,j] (self coefficient of apply_op_Ln), built on first use
    DevBuf<int> d_perm;            // device (empty when identity)
    // time-varying weights (mgadmm_graph_set_time_weights): per-slice value tables in the internal node order on the patterns
    // of Wu / Wd / WdT, device; empty: that matrix is time-invariant.  WdT_t stays empty under transpose_by_gather (Wd_t serves)
    bool time_varying = false;
    int solvers = 0;               // solvers created on this graph so far (the tables must be set before the first one)
    DevBuf<float> Wu_t, Wd_t, WdT_t;
    int max_row_all = 0;

    OpDesc op_lu() const;
    OpDesc op_ldr() const;
    OpDesc op_ldrt() const;
};

// graph.hip
int mg_transpose_csr(const HostCsr& A, HostCsr& At);
int mg_rcm_order(const HostCsr& A, const HostCsr* B, std::vector<int>& perm);
int mg_cluster_order(const HostCsr& A, const HostCsr* B, int csize, std::vector<int>& perm, std::vector<int>* starts = nullptr);
int mg_permute_csr(const HostCsr& A, const std::vector<int>& perm, const std::vector<int>& iperm, HostCsr& out);

struct EngineBase;
struct mgadmm_solver {
    mgadmm_graph* g = nullptr;
    mgadmm_params p;
    int Bmax = 0;
    EngineBase* eng = nullptr;
};

struct EngineBase {
    virtual ~EngineBase() {}
    virtual int init() = 0;
    virtual int set_params(const mgadmm_params& p) = 0;
    virtual int set_sample_params(const mgadmm_sample_params* sp, int B) = 0;
    virtual int set_sample_graphs(int n_sets, mgadmm_graph* const* graphs, const int32_t* set_of_sample, int B) = 0;
    virtual int set_param_schedule(const mgadmm_param_schedule* sch, int n_rows, int B, int first_row) = 0;
    virtual int set_adaptive_rho(const mgadmm_adaptive_rho* ar, int start) = 0;
    virtual int set_sample_bands(int n_sets, const float* band_w, const int32_t* set_of_sample, int B) = 0;
    virtual int get_adaptive_history(int B, double* rho_hist, int max_periods, int* n_periods) = 0;
    virtual int64_t workspace_bytes() const = 0;
    virtual int path_for(int B) const = 0;
    virtual int query(int what, int64_t* out) const = 0;
    virtual int apply(int op, const void* x, void* y, int B, hipStream_t st) = 0;
    virtual int lhs(int which, const void* x, const void* mask, void* y, int B, hipStream_t st) = 0;
    virtual int phi_direct(const void* x, const void* gamma, void* phi, int B, hipStream_t st) = 0;
    virtual int initial_guess(const void* y, void* x, int B, hipStream_t st) = 0;
    virtual int initial_interpolation(const void* y, const void* mask, int mask_f32, void* x, int B,
                                      hipStream_t st) = 0;
    virtual int cg(int which, const void* rhs, const void* x0, const void* mask, void* x, int32_t* iters,
                   double* alpha, double* beta, int B, hipStream_t st) = 0;
    virtual int solve(const void* y, const void* mask, int mask_f32, int B, const void* x0, const mgadmm_state* state_in,
                      void* x_out, const mgadmm_state* state_out, mgadmm_history* hist, hipStream_t st) = 0;
    virtual int two_loops(const void* y, const void* mask, int mask_f32, int B, void* x_out, const mgadmm_state* state_out,
                          mgadmm_history* hist, hipStream_t st) = 0;
    virtual int prof_begin() = 0;
    virtual int prof_end(int64_t* counts, double* total_ms, double* bytes) = 0;
};

EngineBase* mg_make_engine_f32(mgadmm_solver* s);
EngineBase* mg_make_engine_f64(mgadmm_solver* s);
