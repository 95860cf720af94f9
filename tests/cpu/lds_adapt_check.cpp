// CPU run of the adaptive-penalty rule and its planning (mixed-graph-admm_amd/csrc/lds_adapt.h).
//   lds_adapt_check                     the checks below; prints one JSON object with the messages of the refusals
//   lds_adapt_check rule IN OUT         applies ldsadapt::step to every record of the file IN (19 doubles: rho, rho_u, rho_d,
//                                       the six residual sums, has_phi, has_zd, mu, tau, rho_min[3], rho_max[3]) and writes the
//                                       three penalties of every record to OUT (tests/test_lds_adapt_cpu.py compares with numpy)
// Checks, each with an exit status of its own when it fails:
//   * the three branches of the rule per pair, the clamps, NaN and 0 / 0 leaving the value alone, ablations skipping their pair;
//   * adapt_J and the set of iterations followed by a step, for every `every` <= 16 x start x until x max_it <= 40, against
//     loops written out here; the rows a step writes, against the penalties in force at every iteration;
//   * validate refuses by name;
//   * a rule that never steps leaves every row's record equal, byte for byte, to fill_records of the start weights.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "lds_adapt.h"

using ldsadapt::Params;
using ldsparam::NW;

#define CHECK(cond, code) do { if (!(cond)) { fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #cond); return code; } } while (0)

static Params params(int every, int until, double mu, double tau, double lo, double hi) {
    Params q;
    q.every = every; q.until = until; q.mu = mu; q.tau = tau; q.tau_inv = 1.0 / tau;
    for (int f = 0; f < 3; ++f) { q.rho_min[f] = lo; q.rho_max[f] = hi; }
    return q;
}

// What Engine::adapt_begin, Engine::adapt_step and k_lds_adapt do to the table of one solve, for B samples whose residual sums
// of iteration `it` are res(it, b, k).  Returns the table [max_it][B]; `in_force` receives the three penalties every
// iteration of every sample should read, from a loop over the iterations that knows nothing of rows_after
template <typename Res>
static std::vector<LdsSampleParams> replay(const ldsparam::Source& src, int ablation, int B, int max_it, int start, const Params& q,
                                           int has_phi, int has_zd, Res res, std::vector<double>& in_force) {
    std::vector<LdsSampleParams> row, tab;
    ldsparam::fill_records(src, ablation, B, row);
    for (int k = 0; k < max_it; ++k) tab.insert(tab.end(), row.begin(), row.end());
    std::vector<double> w((size_t)NW * B);
    for (int f = 0; f < NW; ++f)
        for (int b = 0; b < B; ++b) w[(size_t)f * B + b] = ldsparam::weight_of(src, f, 0, b);
    in_force.assign((size_t)max_it * 3 * B, 0.0);
    std::vector<double> cur(w);
    for (int it = 0; it < max_it; ++it) {
        for (int b = 0; b < B; ++b)
            for (int f = 0; f < 3; ++f) in_force[((size_t)it * 3 + f) * B + b] = cur[(size_t)f * B + b];
        const int n = start + it + 1;                     // iterations the problem has run after this one
        const bool steps = n % q.every == 0 && (q.until <= 0 || n <= q.until);
        if (steps != ldsadapt::step_after(it, start, q.every, q.until)) { in_force.clear(); return tab; }
        if (!steps) continue;
        const ldsadapt::Rows rows = ldsadapt::rows_after(it, start, q.every, q.until, max_it);
        if (rows.first < 0 || rows.last > max_it || rows.first > rows.last) { in_force.clear(); return tab; }
        for (int b = 0; b < B; ++b) {
            double r6[6], wb[NW];
            for (int k = 0; k < 6; ++k) r6[k] = res(it, b, k);
            for (int f = 0; f < NW; ++f) wb[f] = w[(size_t)f * B + b];
            ldsadapt::step(wb, r6, has_phi, has_zd, q);
            for (int f = 0; f < 3; ++f) cur[(size_t)f * B + b] = w[(size_t)f * B + b] = wb[f];
            const LdsSampleParams rec = ldsparam::record_of(ablation, wb);
            for (int r = rows.first; r < rows.last; ++r) tab[(size_t)r * B + b] = rec;
        }
    }
    return tab;
}

static int run_rule(const char* in, const char* out) {
    FILE* fi = fopen(in, "rb");
    FILE* fo = fopen(out, "wb");
    if (!fi || !fo) return 20;
    double v[19];
    while (fread(v, sizeof(double), 19, fi) == 19) {
        Params q;
        q.every = 1; q.mu = v[11]; q.tau = v[12]; q.tau_inv = 1.0 / v[12];
        for (int f = 0; f < 3; ++f) { q.rho_min[f] = v[13 + f]; q.rho_max[f] = v[16 + f]; }
        double w[3] = {v[0], v[1], v[2]};
        ldsadapt::step(w, v + 3, v[9] != 0.0, v[10] != 0.0, q);
        if (fwrite(w, sizeof(double), 3, fo) != 3) return 21;
    }
    fclose(fi);
    return fclose(fo) == 0 ? 0 : 22;
}

int main(int argc, char** argv) {
    if (argc == 4 && strcmp(argv[1], "rule") == 0) return run_rule(argv[2], argv[3]);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // ---- one pair: r = 2, mu = 10 (m2 = 100), tau = 2
    {
        using ldsadapt::balance;
        CHECK(balance(2.0, 401.0, 1.0, 10, 2, 0.5, 0.1, 100) == 4.0, 2);        // pri2 > 100 * 4 * dual2: up
        CHECK(balance(2.0, 400.0, 1.0, 10, 2, 0.5, 0.1, 100) == 2.0, 2);        // equal: not greater
        CHECK(balance(2.0, 1.0, 26.0, 10, 2, 0.5, 0.1, 100) == 1.0, 2);         // s2 = 104 > 100 * pri2: down
        CHECK(balance(2.0, 1.0, 25.0, 10, 2, 0.5, 0.1, 100) == 2.0, 2);
        CHECK(balance(2.0, 5.0, 1.0, 10, 2, 0.5, 0.1, 100) == 2.0, 2);          // balanced
        CHECK(balance(2.0, 401.0, 1.0, 10, 2, 0.5, 0.1, 3.0) == 3.0, 2);        // the clamps
        CHECK(balance(2.0, 1.0, 26.0, 10, 2, 0.5, 1.5, 100) == 1.5, 2);
        CHECK(balance(2.0, nan, 1.0, 10, 2, 0.5, 0.1, 100) == 2.0 && balance(2.0, 1.0, nan, 10, 2, 0.5, 0.1, 100) == 2.0, 2);
        CHECK(balance(2.0, 0.0, 0.0, 10, 2, 0.5, 0.1, 100) == 2.0, 2);
        CHECK(balance(2.0, 1.0, 0.0, 10, 2, 0.5, 0.1, 100) == 4.0 && balance(2.0, 0.0, 1.0, 10, 2, 0.5, 0.1, 100) == 1.0, 2);
    }
    // ---- the pairs and the ablations
    {
        const Params q = params(4, 0, 10, 2, 0.01, 100);
        const double res[6] = {1e6, 1.0, 1.0, 1e6, 1e6, 1.0};      // zu: up; phi: down; zd: up
        for (int has_phi = 0; has_phi <= 1; ++has_phi)
            for (int has_zd = 0; has_zd <= 1; ++has_zd) {
                double w[3] = {2.0, 3.0, 5.0};
                ldsadapt::step(w, res, has_phi, has_zd, q);
                CHECK(w[ldsadapt::RHO_U] == 6.0, 3);
                CHECK(w[ldsadapt::RHO] == (has_phi ? 1.0 : 2.0), 3);
                CHECK(w[ldsadapt::RHO_D] == (has_zd ? 10.0 : 5.0), 3);
            }
    }
    // ---- adapt_J
    for (int every = 1; every <= LDS_MAXJ; ++every)
        for (int chunk = 1; chunk <= LDS_MAXJ; ++chunk) {
            int want = 1;
            for (int j = 1; j <= chunk; ++j) if (every % j == 0) want = j;
            CHECK(ldsadapt::adapt_J(every, chunk) == want, 4);
        }
    // ---- the steps of a solve and the rows they write, against the penalties in force at every iteration
    static_assert(sizeof(LdsSampleParams) == 32, "a record is eight floats");
    ldsparam::Source src;
    const int B = 3;
    const double scal[NW] = {1.5, 2.5, 0.75, 1.0, 2.0, 0.5};
    std::vector<double> rho_u_b = {0.5, 2.0, 8.0};
    for (int f = 0; f < NW; ++f) src.scalar[f] = scal[f];
    src.sample[1] = rho_u_b.data();
    // residual sums that move the penalties up and down with the iteration and the sample
    auto res = [](int it, int b, int k) { return std::ldexp(1.0, ((it * 7 + b * 3 + k * 5) % 23) - 11); };
    long n_cases = 0, n_steps = 0;
    for (int every = 1; every <= LDS_MAXJ; ++every)
        for (int start = 0; start <= 2 * every; start += every)
            for (int until = 0; until <= 40; until += (until < 6 ? 1 : 5))
                for (int max_it = 1; max_it <= 40; max_it += (max_it < 18 ? 1 : 11)) {
                    const Params q = params(every, until, 1.5, 2, 1e-3, 1e3);
                    std::vector<double> in_force;
                    const std::vector<LdsSampleParams> tab = replay(src, MGADMM_ABL_NONE, B, max_it, start, q, 1, 1, res, in_force);
                    CHECK(!in_force.empty(), 5);
                    for (int it = 0; it < max_it; ++it)
                        for (int b = 0; b < B; ++b) {
                            double w[NW];
                            for (int f = 0; f < NW; ++f) w[f] = f < 3 ? in_force[((size_t)it * 3 + f) * B + b] : ldsparam::weight_of(src, f, 0, b);
                            const LdsSampleParams want = ldsparam::record_of(MGADMM_ABL_NONE, w);
                            CHECK(memcmp(&want, &tab[(size_t)it * B + b], sizeof(want)) == 0, 6);
                        }
                    for (int it = 0; it < max_it; ++it) n_steps += ldsadapt::step_after(it, start, every, until);
                    ++n_cases;
                }
    CHECK(n_steps > 1000, 7);
    // ---- a rule that never steps: every row is fill_records of the start weights
    for (int abl = 0; abl <= 3; ++abl) {
        const Params q = params(4, 0, 1e30, 2, 1e-3, 1e3);
        std::vector<double> in_force;
        const std::vector<LdsSampleParams> tab = replay(src, abl, B, 20, 0, q, 1, 1, res, in_force);
        std::vector<LdsSampleParams> row;
        ldsparam::fill_records(src, abl, B, row);
        CHECK(tab.size() == (size_t)20 * B, 8);
        for (int it = 0; it < 20; ++it) CHECK(memcmp(&tab[(size_t)it * B], row.data(), sizeof(LdsSampleParams) * B) == 0, 8);
    }
    // ---- refusals
    std::vector<std::string> msgs;
    auto refuse = [&](Params q, int start) {
        std::string why;
        if (ldsadapt::validate(q, start, why)) return false;
        msgs.push_back(why);
        return true;
    };
    std::string why;
    CHECK(ldsadapt::validate(params(4, 0, 10, 2, 1e-3, 1e3), 8, why) && ldsadapt::validate(params(16, 8, 1.5, 1.1, 1, 1), 0, why), 9);
    CHECK(refuse(params(0, 0, 10, 2, 1e-3, 1e3), 0) && refuse(params(17, 0, 10, 2, 1e-3, 1e3), 0), 9);
    CHECK(refuse(params(4, 0, 1.0, 2, 1e-3, 1e3), 0) && refuse(params(4, 0, nan, 2, 1e-3, 1e3), 0), 9);
    CHECK(refuse(params(4, 0, 10, 1.0, 1e-3, 1e3), 0), 9);
    CHECK(refuse(params(4, 0, 10, 2, 0.0, 1e3), 0) && refuse(params(4, 0, 10, 2, 2.0, 1.0), 0), 9);
    CHECK(refuse(params(4, 0, 10, 2, 1e-3, 1e3), -4) && refuse(params(4, 0, 10, 2, 1e-3, 1e3), 6), 9);
    CHECK(refuse(params(4, -1, 10, 2, 1e-3, 1e3), 0), 9);
    printf("{\"cases\": %ld, \"steps\": %ld, \"refusals\": [", n_cases, n_steps);
    for (size_t i = 0; i < msgs.size(); ++i) printf("%s\"%s\"", i ? ", " : "", msgs[i].c_str());
    printf("]}\n");
    return 0;
}
