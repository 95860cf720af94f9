// Table of ADMM weights by (iteration row, sample): the records the kernels k_admm_lds_pp read through MG_LDS_W
// (lds_kernels.h), and the per-iteration weights of the streaming path's host loop.  Three sources, in this order of
// precedence for each of the six weights: the per-iteration schedule (mgadmm_solver_set_param_schedule), the per-sample
// table (mgadmm_solver_set_sample_params), the scalar of mgadmm_params.  Plain C++ like lds_graph_sets.h, no HIP and no
// environment reads: compiled into libmgadmm.so (Engine) and into the CPU check tests/cpu/lds_param_table_check.cpp.
#pragma once
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "mgadmm.h"
#include "mg_hd.h"      // MG_HD: lhs_def_of and record_of also run on the device (k_lds_adapt, lds_adapt.h)

// One record of the device table: the eight values a trip of k_admm_lds reads from LdsArgsCore, formed by the host from six
// doubles with the expressions of the scalars (lds_fill_args)
struct LdsSampleParams {
    float rho, rho_u, rho_d, mu_u, mu_d1, mu_d2;
    float cx1, cx2;
};

struct LhsDef {
    int kind;  // 0 diagonal only, 1 cLdr = Ldr^T Ldr, 2 Lu
    int hth;   // include the observation operator H^T H
    double c1, c2;
};

// the three left-hand sides of ADMM.py:366-399 from the weights, in double
MG_HD inline LhsDef lhs_def_of(int which, int ablation, double rho, double rho_u, double rho_d, double mu_u, double mu_d2) {
    switch (which) {
        case MGADMM_LHS_X:
            if (ablation == MGADMM_ABL_NONE) return {1, 1, (rho_u + rho_d) / 2, rho / 2};
            if (ablation == MGADMM_ABL_DGLR) return {1, 1, rho_u / 2, rho / 2};
            return {0, 1, (rho_u + rho_d) / 2, 0.0};
        case MGADMM_LHS_ZU: return {2, 0, rho_u / 2, mu_u};
        default: return {1, 0, rho_d / 2, mu_d2};
    }
}

// Row of a schedule of `rows` rows that iteration `it` of a solve reads when the solve starts at row `row0`: the last row
// holds for the rest of the solve; no schedule (rows <= 1) is row 0.  constexpr: the kernel macro, the engine and the
// streaming loop call the same function.
constexpr int sched_row(int it, int row0, int rows) { return it + row0 < rows ? it + row0 : (rows > 0 ? rows - 1 : 0); }

namespace ldsparam {

constexpr int NW = 6;
constexpr const char* const NAMES[NW] = {"rho", "rho_u", "rho_d", "mu_u", "mu_d1", "mu_d2"};

// where the six weights of a (row, sample) come from; a null pointer hands on to the next source
struct Source {
    double scalar[NW] = {0, 0, 0, 0, 0, 0};
    const double* sample[NW] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // [B]
    const double* sched[NW] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};    // [n_rows][sched_B], or [n_rows] when sched_B == 0
    int n_rows = 1;       // rows of the schedule (1 without one)
    int sched_B = 0;      // columns of the schedule arrays; 0 = the shared form: every sample reads the same row
};

inline double weight_of(const Source& s, int f, int row, int b) {
    if (s.sched[f]) return s.sched_B > 0 ? s.sched[f][(size_t)row * s.sched_B + b] : s.sched[f][row];
    if (s.sample[f]) return s.sample[f][b];
    return s.scalar[f];
}

// the record of six doubles: lhs_def_of in double, then the casts
MG_HD inline LdsSampleParams record_of(int ablation, const double w[NW]) {
    const LhsDef dx = lhs_def_of(MGADMM_LHS_X, ablation, w[0], w[1], w[2], w[3], w[5]);
    LdsSampleParams r;
    r.cx1 = (float)dx.c1; r.cx2 = (float)dx.c2;
    r.rho = (float)w[0]; r.rho_u = (float)w[1]; r.rho_d = (float)w[2];
    r.mu_u = (float)w[3]; r.mu_d1 = (float)w[4]; r.mu_d2 = (float)w[5];
    return r;
}

// records [s.n_rows][B], row-major: record row * B + b is what workgroup b reads in an iteration of that row
inline void fill_records(const Source& s, int ablation, int B, std::vector<LdsSampleParams>& rec) {
    rec.resize((size_t)s.n_rows * B);
    for (int row = 0; row < s.n_rows; ++row)
        for (int b = 0; b < B; ++b) {
            double w[NW];
            for (int f = 0; f < NW; ++f) w[f] = weight_of(s, f, row, b);
            rec[(size_t)row * B + b] = record_of(ablation, w);
        }
}

// the six weights of iteration `it` in the shared form (streaming path: no per-sample source)
inline void row_weights(const Source& s, int it, int row0, double w[NW]) {
    const int row = sched_row(it, row0, s.n_rows);
    for (int f = 0; f < NW; ++f) w[f] = weight_of(s, f, row, 0);
}

// Values of a table `who` ([n_rows][B] row-major, B == 0: [n_rows]): finite, the three rhos > 0, the mus >= 0.  false: `why`
// names the offending [row][b] ([row] in the shared form)
inline bool validate(const char* who, const double* const src[NW], int n_rows, int B, std::string& why) {
    const int cols = B > 0 ? B : 1;
    char at[48], buf[200];
    for (int f = 0; f < NW; ++f) {
        if (!src[f]) continue;
        for (int row = 0; row < n_rows; ++row)
            for (int b = 0; b < cols; ++b) {
                const double v = src[f][(size_t)row * cols + b];
                if (B > 0) snprintf(at, sizeof(at), "[%d][%d]", row, b);
                else snprintf(at, sizeof(at), "[%d]", row);
                if (!std::isfinite(v)) snprintf(buf, sizeof(buf), "%s: %s%s is not finite", who, NAMES[f], at);
                else if (f < 3 && !(v > 0.0)) snprintf(buf, sizeof(buf), "%s: %s%s = %g, should be > 0", who, NAMES[f], at, v);
                else if (f >= 3 && !(v >= 0.0)) snprintf(buf, sizeof(buf), "%s: %s%s = %g, should be >= 0", who, NAMES[f], at, v);
                else continue;
                why = buf;
                return false;
            }
    }
    return true;
}

// first weight that both the schedule and the per-sample table name (nullptr: none)
template <typename A, typename B>
inline const char* given_twice(const A& sched_given, const B& sample_given) {
    for (int f = 0; f < NW; ++f)
        if (sched_given[f] && sample_given[f]) return NAMES[f];
    return nullptr;
}

}  // namespace ldsparam
