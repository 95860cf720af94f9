// What a solver refuses, and the host state of its two weight tables.  The per-sample features of the LDS-resident path
// (admm_convergence per_sample, sample_params, sample_graphs, param_schedule, adaptive_rho) share one decision -- "this solve
// cannot take the LDS-resident float32 path, because ..." -- and one rule about the whole-batch stop test: both are written
// once here, the wording of every feature is data, and the engine hands the message to mg_set_error.  Plain C++ like
// lds_plan.h, no HIP and no environment reads: compiled into libmgadmm.so (Engine) and into tests/cpu/solve_gate_check.cpp,
// which compares every answer with the engine's before the decisions moved here (tests/golden/solve_gate_parent.json).
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "mgadmm.h"
#include "lds_param_table.h"

namespace solvegate {

struct Result { int rc = MGADMM_OK; std::string msg; };      // msg: what mgadmm_last_error() reports when rc != MGADMM_OK
__attribute__((format(printf, 2, 3))) inline Result refuse(int rc, const char* fmt, ...) {
    char buf[1024];        // (the size of mg_set_error's own buffer)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return {rc, buf};
}

// What a decision reads of the solver and of the parameters in force (or about to be set): the scalar type is float, four
// fields of mgadmm_params, LdsPlan::ok, MGADMM_TEMPORAL_BAND, the graph's size.  The engine fills it once per call
struct Facts { bool f32; int path, cg_convergence, admm_convergence, check_stop; bool lds_ok, band; int N, T; };
// What is set on the solver: samples of the weights table and of the graph table, rows and columns of the schedule (0: none
// set; rows with sch_B = 0: the shared form), adaptive penalties
struct SetState { int sp_B, sg_B, sch_rows, sch_B; bool ad_on; };

// Why a solve cannot take the LDS-resident float32 path (nullptr: it can).  path_rungs: the two rungs about the parameters
// (set_sample_graphs decides when the table is set, before the parameters of the solve are known, and skips them);
// band_rung: the graph table's own last rung
inline const char* why_not_lds(const Facts& f, bool path_rungs, bool band_rung) {
    if (!f.f32) return "float64 arithmetic runs on the streaming path";
    if (path_rungs && f.path == MGADMM_PATH_STREAM) return "path is MGADMM_PATH_STREAM";
    if (path_rungs && f.cg_convergence == MGADMM_CG_BATCH_MAX) return "cg_convergence batch_max runs on the streaming path";
    if (!f.lds_ok) return "the LDS-resident path cannot hold this graph (it needs T*N*8 B + tables <= 160 KiB and N*G <= 1024)";
    if (band_rung && f.band) return "a band graph (line graph) has no W_d tables to vary";
    return nullptr;
}

// The wording of a feature: "<name><gloss> <be> implemented by ...: <why><suffix>", "<name> with check_stop <need> ...
// (<stop_gloss>the whole_batch stop test ...", "the <table> table holds <n> samples<per> ..."
struct Feature { const char *name, *gloss, *be, *need, *suffix, *stop_gloss, *table, *per; bool band_rung; };
constexpr Feature ADMM_PER_SAMPLE = {"admm_convergence per_sample", "", "is", "", "", "", "", "", false};
constexpr Feature ADAPTIVE_RHO = {"adaptive_rho", " (penalties adapted on the device)", "is", "needs", "", "every sample carries its own penalties: ", "", "", false};
constexpr Feature SAMPLE_PARAMS = {"sample_params", " (per-sample ADMM weights)", "are", "need", "", "", "sample_params", "", false};
constexpr Feature SAMPLE_GRAPHS = {"sample_graphs", " (per-sample graph weights)", "are", "need", "", "", "sample_graphs", "", true};
constexpr Feature PARAM_SCHEDULE = {"the per-sample form of param_schedule", " (one column per sample)", "is", "needs",
                                    "; the shared form (B = 0) runs on both paths", "", "param_schedule", " per row", false};

// the feature runs on the LDS-resident float32 path only
inline Result lds_only(const char* who, const Feature& ft, const Facts& f, bool path_rungs = true) {
    const char* why = why_not_lds(f, path_rungs, ft.band_rung);
    if (!why) return {};
    return refuse(MGADMM_ERR_UNSUPPORTED, "%s: %s%s %s implemented by the LDS-resident float32 path only: %s%s", who, ft.name, ft.gloss, ft.be, why, ft.suffix);
}
// every sample solves a problem of its own: one stop test over the whole batch means nothing
inline Result own_stop_only(const Feature& ft, const Facts& f) {
    if (!f.check_stop || f.admm_convergence != MGADMM_ADMM_WHOLE_BATCH) return {};
    return refuse(MGADMM_ERR_UNSUPPORTED, "solve: %s with check_stop %s admm_convergence per_sample (%sthe whole_batch stop test would sum "
                  "the residuals of different problems); or run a fixed count with check_stop = 0", ft.name, ft.need, ft.stop_gloss);
}
// a solve of B samples with a table of table_B samples set
inline Result table_gate(const Feature& ft, int table_B, const Facts& f, int B) {
    if (B != table_B) return refuse(MGADMM_ERR_INVALID, "solve: the %s table holds %d samples%s, the solve has B = %d", ft.table, table_B, ft.per, B);
    Result r = lds_only("solve", ft, f);
    return r.rc != MGADMM_OK ? r : own_stop_only(ft, f);
}

// The per-sample stop test of the outer loop lives in the LDS-resident kernel (one workgroup owns a sample); the streaming
// kernels are batch-innermost and would need per-sample masks throughout (like MGADMM_CG_BATCH_MAX is streaming-only).
// who: solver_create, set_params, solve
inline Result admm_convergence_gate(const Facts& f, const char* who) {
    if (f.admm_convergence != MGADMM_ADMM_WHOLE_BATCH && f.admm_convergence != MGADMM_ADMM_PER_SAMPLE)
        return refuse(MGADMM_ERR_INVALID, "%s: admm_convergence should be whole_batch (0) or per_sample (1), got %d", who, f.admm_convergence);
    return f.admm_convergence == MGADMM_ADMM_PER_SAMPLE ? lds_only(who, ADMM_PER_SAMPLE, f) : Result();
}
inline Result set_params_gate(const Facts& f) {
    if (f.path != MGADMM_PATH_LDS || f.cg_convergence != MGADMM_CG_BATCH_MAX) return {};
    return {MGADMM_ERR_UNSUPPORTED, "set_params: the LDS-resident path implements per-sample CG convergence only (batch_max: streaming path)"};
}
// set_sample_graphs, after its argument checks
inline Result set_sample_graphs_gate(const Facts& f) { return lds_only("set_sample_graphs", SAMPLE_GRAPHS, f, false); }

// A solve of B samples with `s` set: decided when the solve starts (tables and parameters arrive in separate calls, in any
// order), before anything is enqueued.  The ORDER is part of the interface: with several things set and several refusals
// due, the caller reads the first of
//   1. adaptive_rho: the path, the stop test, "both set" with a param_schedule, the B of the sample_params table it starts from
//   2. sample_params: B, the path, the stop test
//   3. sample_graphs: B, the path (a band graph last), the stop test
//   4. the per-sample form of param_schedule: B, the path, the stop test (the shared form runs on both paths and with the
//      whole-batch stop test: every sample solves the same problem)
//   5. path is MGADMM_PATH_LDS and the graph does not fit
inline Result solve_gate(const Facts& f, const SetState& s, int B) {
    Result r;
    auto refused = [&r](Result x) { r = std::move(x); return r.rc != MGADMM_OK; };
    if (s.ad_on) {
        if (refused(lds_only("solve", ADAPTIVE_RHO, f)) || refused(own_stop_only(ADAPTIVE_RHO, f))) return r;
        if (s.sch_rows > 0)
            return {MGADMM_ERR_UNSUPPORTED, "solve: adaptive_rho and a param_schedule are both set: the adaptation writes the table a schedule would fill"};
        if (s.sp_B != 0 && B != s.sp_B)
            return refuse(MGADMM_ERR_INVALID, "solve: adaptive_rho takes its start values from the sample_params table of %d samples, the solve has B = %d", s.sp_B, B);
    }
    if (s.sp_B > 0 && refused(table_gate(SAMPLE_PARAMS, s.sp_B, f, B))) return r;
    if (s.sg_B > 0 && refused(table_gate(SAMPLE_GRAPHS, s.sg_B, f, B))) return r;
    if (s.sch_rows > 0 && s.sch_B > 0 && refused(table_gate(PARAM_SCHEDULE, s.sch_B, f, B))) return r;
    if (f.path != MGADMM_PATH_LDS || f.lds_ok) return {};
    return refuse(MGADMM_ERR_UNSUPPORTED, "solve: the LDS-resident path needs float32, T*N*8 B + CSR <= 160 KiB and N*G <= 1024 (N=%d, T=%d)", f.N, f.T);
}

// Which table of records (LdsArgs::sp) the launches of a solve on the LDS path read, for every state solve_gate lets through:
// the table the adaptive steps write (max_it rows) before the schedule's records (sch_rows rows, the solve starts at sch_row0)
// before the per-sample records (one row).  stride_B: LdsArgs::sp_stride is the solve's B, not 0.  A graph table without a
// weights table reads per-sample records too (the same kernels): records of the scalars, which the engine then has to form
enum Table { TABLE_NONE, TABLE_SAMPLE, TABLE_SCHEDULE, TABLE_ADAPTIVE };
struct TableChoice { Table table; int sp_rows, sp_row0; bool stride_B, scalar_records; };
inline TableChoice table_of(const SetState& s, int sch_row0, int max_it) {
    if (s.ad_on) return {TABLE_ADAPTIVE, max_it, 0, true, false};
    if (s.sch_rows > 0) return {TABLE_SCHEDULE, s.sch_rows, sch_row0, true, false};
    return {s.sp_B > 0 || s.sg_B > 0 ? TABLE_SAMPLE : TABLE_NONE, 0, 0, false, s.sp_B == 0 && s.sg_B > 0};
}

// The caller's arrays of mgadmm_solver_set_sample_params ([sp_B]) and mgadmm_solver_set_param_schedule ([sch_rows][sch_B], or
// [sch_rows] in the shared form sch_B = 0; iteration k of a solve reads row min(sch_row0 + k, sch_rows - 1)).  An empty array:
// the weight follows the next source (lds_param_table.h).  A set_* that refuses leaves the state as it was
struct WeightTables {
    static constexpr int NW = ldsparam::NW;
    int sp_B = 0;                        // samples of the table; 0 = none set
    int sch_rows = 0, sch_B = 0, sch_row0 = 0;      // sch_rows = 0: none set
    std::vector<double> sp_val[NW], sch_val[NW];    // rho, rho_u, rho_d, mu_u, mu_d1, mu_d2

    void clear_sample() { sp_B = 0; for (auto& v : sp_val) v.clear(); }
    void clear_schedule() { sch_rows = sch_B = sch_row0 = 0; for (auto& v : sch_val) v.clear(); }
    // the two setters as the ABI has them: a null pointer or a count of 0 clears
    Result set_sample(const mgadmm_sample_params* spp, int B, int max_batch) {
        if (spp == nullptr || B == 0) { clear_sample(); return {}; }
        const mgadmm_sample_params& sp = *spp;
        if (B < 1 || B > max_batch) return refuse(MGADMM_ERR_INVALID, "set_sample_params: batch %d outside [1, max_batch=%d]", B, max_batch);
        const double* const src[NW] = {sp.rho, sp.rho_u, sp.rho_d, sp.mu_u, sp.mu_d1, sp.mu_d2};
        if (const char* twice = ldsparam::given_twice(source(true, {}).sched, src))
            return refuse(MGADMM_ERR_INVALID, "set_sample_params: %s is given twice, in the param_schedule that is set and in sample_params", twice);
        std::string why;
        if (!ldsparam::validate("set_sample_params", src, B, 0, why)) return {MGADMM_ERR_INVALID, why};      // (as a column of B rows)
        for (int f = 0; f < NW; ++f) sp_val[f].assign(src[f], src[f] ? src[f] + B : src[f]);
        sp_B = B;
        return {};
    }
    Result set_schedule(const mgadmm_param_schedule* schp, int n_rows, int B, int first_row, int max_batch) {
        if (schp == nullptr || n_rows == 0) { clear_schedule(); return {}; }
        const mgadmm_param_schedule& sch = *schp;
        if (n_rows < 1 || n_rows > (1 << 20)) return refuse(MGADMM_ERR_INVALID, "set_param_schedule: n_rows %d outside [1, 2^20]", n_rows);
        if (B < 0 || B > max_batch) return refuse(MGADMM_ERR_INVALID, "set_param_schedule: batch %d outside [0 (shared form), max_batch=%d]", B, max_batch);
        if (first_row < 0) return refuse(MGADMM_ERR_INVALID, "set_param_schedule: first_row %d is negative", first_row);
        if ((int64_t)n_rows * max_batch > (int64_t)1 << 27)
            return refuse(MGADMM_ERR_INVALID, "set_param_schedule: n_rows %d x max_batch %d records exceed 2^27", n_rows, max_batch);
        const double* const src[NW] = {sch.rho, sch.rho_u, sch.rho_d, sch.mu_u, sch.mu_d1, sch.mu_d2};
        std::string why;
        if (!ldsparam::validate("set_param_schedule: param_schedule", src, n_rows, B, why)) return {MGADMM_ERR_INVALID, why};
        if (const char* twice = ldsparam::given_twice(src, source(false, {}).sample))
            return refuse(MGADMM_ERR_INVALID, "set_param_schedule: %s is given twice, in param_schedule and in the sample_params table that is set", twice);
        for (int f = 0; f < NW; ++f) sch_val[f].assign(src[f], src[f] ? src[f] + (size_t)n_rows * (B > 0 ? B : 1) : src[f]);
        sch_rows = n_rows; sch_B = B; sch_row0 = first_row;
        return {};
    }
    // where a (row, sample) takes its six weights from: the schedule if `with_schedule`, the per-sample table, the scalars of `p`
    ldsparam::Source source(bool with_schedule, const mgadmm_params& p) const {
        ldsparam::Source src;
        const double scalar[NW] = {p.rho, p.rho_u, p.rho_d, p.mu_u, p.mu_d1, p.mu_d2};
        for (int f = 0; f < NW; ++f) {
            src.scalar[f] = scalar[f];
            src.sample[f] = sp_B > 0 && !sp_val[f].empty() ? sp_val[f].data() : nullptr;
            src.sched[f] = with_schedule && sch_rows > 0 && !sch_val[f].empty() ? sch_val[f].data() : nullptr;
        }
        if (with_schedule && sch_rows > 0) { src.n_rows = sch_rows; src.sched_B = sch_B; }
        return src;
    }
};

}  // namespace solvegate
