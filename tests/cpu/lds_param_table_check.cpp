// CPU run of the weight-table builder of the LDS-resident path (mixed-graph-admm_amd/csrc/lds_param_table.h).
//   lds_param_table_check
// Checks, each with an exit status of its own when it fails:
//   * sched_row: clamping to the last row, first_row, no schedule (rows 0 and 1), against a loop written out here;
//   * fill_records: the fallbacks schedule -> per-sample table -> scalar, in both forms of the schedule, for every ablation;
//   * a one-row schedule, and no schedule at all, give the records the engine formed before schedules existed (the code of
//     Engine::upload_sample_params, kept here as `legacy_records`), byte for byte;
//   * row_weights (the streaming loop) reads what record (row, 0) was formed from;
//   * validate / given_twice refuse by name: the field and [row][b] ([row] in the shared form).
// Prints one JSON object with the messages of the refusals.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "lds_param_table.h"

using ldsparam::NW;

#define CHECK(cond, code) do { if (!(cond)) { fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #cond); return code; } } while (0)

// Engine::upload_sample_params as it was before lds_param_table.h: sample b's six doubles, lhs_def_of in double, the casts
static std::vector<LdsSampleParams> legacy_records(int ablation, const double scalar[NW], const std::vector<double> sp_val[NW], int n) {
    std::vector<LdsSampleParams> rec((size_t)n);
    for (int b = 0; b < n; ++b) {
        double w[6];
        for (int f = 0; f < 6; ++f) w[f] = sp_val[f].empty() ? scalar[f] : sp_val[f][(size_t)b];
        double c1, c2;
        if (ablation == MGADMM_ABL_NONE) { c1 = (w[1] + w[2]) / 2; c2 = w[0] / 2; }
        else if (ablation == MGADMM_ABL_DGLR) { c1 = w[1] / 2; c2 = w[0] / 2; }
        else { c1 = (w[1] + w[2]) / 2; c2 = 0.0; }
        LdsSampleParams& r = rec[(size_t)b];
        r.cx1 = (float)c1; r.cx2 = (float)c2;
        r.rho = (float)w[0]; r.rho_u = (float)w[1]; r.rho_d = (float)w[2];
        r.mu_u = (float)w[3]; r.mu_d1 = (float)w[4]; r.mu_d2 = (float)w[5];
    }
    return rec;
}

static bool same_bytes(const std::vector<LdsSampleParams>& a, const std::vector<LdsSampleParams>& b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), sizeof(LdsSampleParams) * a.size()) == 0;
}

static double value(int f, int row, int b) { return 0.25 + 0.37 * f + 0.011 * row * (f + 1) + 0.0031 * b * (row + 2); }

int main() {
    static_assert(sizeof(LdsSampleParams) == 32, "a record is eight floats");
    // ---- sched_row
    for (int rows = 0; rows <= 5; ++rows)
        for (int row0 = 0; row0 <= 7; ++row0)
            for (int it = 0; it <= 9; ++it) {
                int want = it + row0;
                if (want > rows - 1) want = rows - 1;
                if (want < 0) want = 0;
                CHECK(sched_row(it, row0, rows) == want, 2);
            }
    CHECK(sched_row(0, 0, 12) == 0 && sched_row(11, 0, 12) == 11 && sched_row(12, 0, 12) == 11 && sched_row(19, 0, 12) == 11, 2);
    CHECK(sched_row(0, 8, 12) == 8 && sched_row(3, 8, 12) == 11 && sched_row(4, 8, 12) == 11, 2);
    CHECK(sched_row(5, 3, 0) == 0 && sched_row(5, 0, 1) == 0, 2);

    const double scalar[NW] = {1.5, 2.25, 0.75, 1.0, 3.0, 0.5};
    const int B = 5, R = 4;
    std::vector<double> samp[NW], sched_ps[NW], sched_sh[NW];
    for (int f = 0; f < NW; ++f) {
        for (int b = 0; b < B; ++b) samp[f].push_back(value(f, 17, b));
        for (int row = 0; row < R; ++row) {
            sched_sh[f].push_back(value(f, row, 40));
            for (int b = 0; b < B; ++b) sched_ps[f].push_back(value(f, row, b));
        }
    }
    // ---- fallbacks: weight f comes from the schedule (f = 0, 4), the per-sample table (f = 1, 5) or the scalar (f = 2, 3)
    for (int ablation = 0; ablation <= 3; ++ablation)
        for (int form = 0; form < 2; ++form) {
            ldsparam::Source s;
            for (int f = 0; f < NW; ++f) s.scalar[f] = scalar[f];
            s.sample[1] = samp[1].data(); s.sample[5] = samp[5].data();
            s.n_rows = R; s.sched_B = form ? B : 0;
            s.sched[0] = form ? sched_ps[0].data() : sched_sh[0].data();
            s.sched[4] = form ? sched_ps[4].data() : sched_sh[4].data();
            std::vector<LdsSampleParams> rec;
            ldsparam::fill_records(s, ablation, B, rec);
            CHECK(rec.size() == (size_t)R * B, 3);
            for (int row = 0; row < R; ++row)
                for (int b = 0; b < B; ++b) {
                    double w[NW] = {form ? value(0, row, b) : value(0, row, 40), value(1, 17, b), scalar[2], scalar[3],
                                    form ? value(4, row, b) : value(4, row, 40), value(5, 17, b)};
                    // the record of (row, b) is the record of a B = 1 table holding these six doubles as scalars
                    const std::vector<double> none[NW];
                    const std::vector<LdsSampleParams> one = legacy_records(ablation, w, none, 1);
                    CHECK(memcmp(&rec[(size_t)row * B + b], &one[0], sizeof(LdsSampleParams)) == 0, 3);
                    for (int f = 0; f < NW; ++f) CHECK(ldsparam::weight_of(s, f, row, b) == w[f], 3);
                }
            if (!form) {      // the streaming loop's weights of iteration it: the row, clamped
                for (int it = 0; it < 7; ++it) {
                    double w[NW];
                    ldsparam::row_weights(s, it, 1, w);
                    const int row = it + 1 < R ? it + 1 : R - 1;
                    CHECK(w[0] == value(0, row, 40) && w[4] == value(4, row, 40) && w[2] == scalar[2] && w[1] == value(1, 17, 0), 4);
                }
            }
        }
    // ---- no schedule, and a one-row schedule: the records of Engine::upload_sample_params as it was, byte for byte
    for (int ablation = 0; ablation <= 3; ++ablation) {
        std::vector<double> given[NW];
        given[0] = samp[0]; given[3] = samp[3]; given[4] = samp[4];       // a table that names three weights
        const std::vector<LdsSampleParams> want = legacy_records(ablation, scalar, given, B);
        ldsparam::Source s;
        for (int f = 0; f < NW; ++f) { s.scalar[f] = scalar[f]; s.sample[f] = given[f].empty() ? nullptr : given[f].data(); }
        std::vector<LdsSampleParams> rec;
        ldsparam::fill_records(s, ablation, B, rec);
        CHECK(same_bytes(rec, want), 5);
        // the same values as a one-row schedule in the per-sample form, nothing in the per-sample table
        ldsparam::Source t;
        for (int f = 0; f < NW; ++f) { t.scalar[f] = scalar[f]; t.sched[f] = given[f].empty() ? nullptr : given[f].data(); }
        t.n_rows = 1; t.sched_B = B;
        ldsparam::fill_records(t, ablation, B, rec);
        CHECK(same_bytes(rec, want), 5);
        // scalars alone (a solve with a graph table and no weights table): B copies of the scalars' record
        const std::vector<double> none[NW];
        ldsparam::fill_records(ldsparam::Source{{scalar[0], scalar[1], scalar[2], scalar[3], scalar[4], scalar[5]}}, ablation, B, rec);
        CHECK(same_bytes(rec, legacy_records(ablation, scalar, none, B)), 5);
    }
    // ---- refusals by name
    std::string why, msgs[6];
    const double* src[NW] = {sched_ps[0].data(), nullptr, sched_ps[2].data(), sched_ps[3].data(), nullptr, sched_ps[5].data()};
    CHECK(ldsparam::validate("t", src, R, B, why) && why.empty(), 6);
    std::vector<double> bad = sched_ps[2];
    bad[(size_t)2 * B + 3] = std::numeric_limits<double>::quiet_NaN();
    src[2] = bad.data();
    CHECK(!ldsparam::validate("t", src, R, B, why) && why == "t: rho_d[2][3] is not finite", 6);
    msgs[0] = why;
    bad = sched_ps[2]; bad[(size_t)3 * B + 4] = std::numeric_limits<double>::infinity();
    CHECK(!ldsparam::validate("t", src, R, B, why) && why == "t: rho_d[3][4] is not finite", 6);
    msgs[1] = why;
    bad = sched_ps[2]; bad[(size_t)1 * B + 0] = 0.0;
    CHECK(!ldsparam::validate("t", src, R, B, why) && why == "t: rho_d[1][0] = 0, should be > 0", 6);
    msgs[2] = why;
    src[2] = sched_ps[2].data();
    bad = sched_ps[5]; bad[(size_t)0 * B + 2] = -0.5;
    src[5] = bad.data();
    CHECK(!ldsparam::validate("t", src, R, B, why) && why == "t: mu_d2[0][2] = -0.5, should be >= 0", 6);
    msgs[3] = why;
    bad = sched_ps[5]; bad[(size_t)0 * B + 2] = 0.0;          // a mu of 0 is allowed
    CHECK(ldsparam::validate("t", src, R, B, why), 6);
    const double* shared[NW] = {nullptr, sched_sh[1].data(), nullptr, nullptr, nullptr, nullptr};
    CHECK(ldsparam::validate("t", shared, R, 0, why), 6);
    bad = sched_sh[1]; bad[3] = -1.0;
    shared[1] = bad.data();
    CHECK(!ldsparam::validate("t", shared, R, 0, why) && why == "t: rho_u[3] = -1, should be > 0", 6);
    msgs[4] = why;
    {
        const bool in_table[NW] = {false, true, false, false, true, false};
        const double* a[NW] = {sched_ps[0].data(), nullptr, nullptr, nullptr, sched_ps[4].data(), nullptr};
        const char* twice = ldsparam::given_twice(a, in_table);
        CHECK(twice && std::string(twice) == "mu_d1", 7);
        msgs[5] = twice;
        a[4] = nullptr;
        CHECK(ldsparam::given_twice(a, in_table) == nullptr, 7);
    }
    printf("{\"refusals\": [");
    for (int k = 0; k < 6; ++k) printf("%s\"%s\"", k ? ", " : "", msgs[k].c_str());
    printf("], \"record_bytes\": %d}\n", (int)sizeof(LdsSampleParams));
    return 0;
}
