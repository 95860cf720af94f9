// CPU check of csrc/band_sets.h (per-sample temporal band weights), a program of its own built with AddressSanitizer + UBSan:
//   - every refusal of the setter and of the solve-time gate, with its return code and its message;
//   - a call that refuses leaves the table as it was, n_sets == 0 or a null pointer clears it;
//   - the expansion the streaming kernels read: column b the table of set_of[b], the padded columns zero;
//   - a narrow table padded to the solver's width equals the native one on every entry an operator reads, and the stencils
//     formed with either (the loops of band_back / band_fwd and of op_apply_band, floats, accumulator from +0) agree bit for bit;
//   - the records a band table alone takes on the LDS path.
// Prints one JSON object and exits 0, or names what failed and exits 1.
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "solve_gate.h"
#include "band_sets.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond); \
                                             fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static void expect(const solvegate::Result& r, int rc, const char* msg) {
    CHECK(r.rc == rc && r.msg == msg, "rc %d \"%s\", expected %d \"%s\"", r.rc, r.msg.c_str(), rc, msg);
}

// rows 1 / min(t, s) on the hops an operator reads, zero beyond (utils.skip_connection_tables), in a table of `width` hops
static std::vector<float> uniform_table(int T, int s, int width) {
    std::vector<float> w((size_t)T * width, 0.0f);
    for (int t = 1; t < T; ++t) {
        const int m = t < s ? t : s;
        for (int h = 0; h < m; ++h) w[(size_t)t * width + h] = 1.0f / (float)m;
    }
    return w;
}

// Ldr-like and Ldr^T-like stencils of one node's time series with a band table, as the kernels form them
static std::vector<float> stencils(const std::vector<float>& w, int T, int skip, const std::vector<float>& x) {
    std::vector<float> out((size_t)2 * T);
    for (int t = 0; t < T; ++t) {
        float back = 0.f, fwd = 0.f;
        for (int s = 0; s < skip; ++s) {
            const int tt = t - 1 - s;
            if (tt < 0) break;
            back += w[(size_t)t * skip + s] * x[(size_t)tt];
        }
        for (int s = 0; s < skip; ++s) {
            const int tt = t + 1 + s;
            if (tt >= T) break;
            fwd += w[(size_t)tt * skip + s] * x[(size_t)tt];
        }
        out[(size_t)t] = back;
        out[(size_t)T + t] = fwd;
    }
    return out;
}

int main() {
    using bandsets::BandSets;
    const int T = 24, W = 6, MAXB = 300;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<float> tabs;
    for (int s : {1, 2, 3, 6}) { const auto u = uniform_table(T, s, W); tabs.insert(tabs.end(), u.begin(), u.end()); }
    const int S = 4, B = 70;
    std::vector<int32_t> set_of((size_t)B);
    for (int b = 0; b < B; ++b) set_of[(size_t)b] = (3 * b + b / 64) % S;

    // ---- the setter: refusals in their order, each leaving the state as it was
    BandSets bs;
    expect(bs.set(true, T, W, S, tabs.data(), set_of.data(), B, MAXB), MGADMM_OK, "");
    CHECK(bs.B == B && bs.n_sets == S && bs.T == T && bs.skip == W && bs.w == tabs && bs.set_of == set_of, "state after set");
    const BandSets before = bs;
    auto unchanged = [&]() { return bs.B == before.B && bs.n_sets == before.n_sets && bs.w == before.w && bs.set_of == before.set_of; };
    expect(bs.set(false, T, W, S, tabs.data(), set_of.data(), B, MAXB), MGADMM_ERR_UNSUPPORTED,
           "set_sample_bands: the solver's graph is not MGADMM_TEMPORAL_BAND: a spatial temporal graph has no band table to vary "
           "(sample_graphs varies its W_d)");
    expect(bs.set(true, T, W, S, tabs.data(), set_of.data(), 0, MAXB), MGADMM_ERR_INVALID, "set_sample_bands: batch 0 outside [1, max_batch=300]");
    expect(bs.set(true, T, W, S, tabs.data(), set_of.data(), 301, MAXB), MGADMM_ERR_INVALID, "set_sample_bands: batch 301 outside [1, max_batch=300]");
    expect(bs.set(true, T, W, -1, tabs.data(), set_of.data(), B, MAXB), MGADMM_ERR_INVALID, "set_sample_bands: n_sets -1 outside [1, max_batch=300]");
    expect(bs.set(true, T, W, 301, tabs.data(), set_of.data(), B, MAXB), MGADMM_ERR_INVALID, "set_sample_bands: n_sets 301 outside [1, max_batch=300]");
    // the order: the graph before B before n_sets before the index before the entries
    expect(bs.set(false, T, W, -1, tabs.data(), set_of.data(), 0, MAXB).rc == MGADMM_ERR_UNSUPPORTED ? solvegate::Result() : solvegate::Result{1, "order"}, 0, "");
    expect(bs.set(true, T, W, -1, tabs.data(), set_of.data(), 0, MAXB), MGADMM_ERR_INVALID, "set_sample_bands: batch 0 outside [1, max_batch=300]");
    {
        std::vector<int32_t> bad = set_of;
        bad[65] = S;
        std::vector<float> badw = tabs;
        badw[(size_t)(2 * T + 5) * W + 1] = nan;
        expect(bs.set(true, T, W, S, badw.data(), bad.data(), B, MAXB), MGADMM_ERR_INVALID, "set_sample_bands: set_of_sample[65] = 4 outside [0, n_sets=4)");
        bad[65] = -1;
        expect(bs.set(true, T, W, S, tabs.data(), bad.data(), B, MAXB), MGADMM_ERR_INVALID, "set_sample_bands: set_of_sample[65] = -1 outside [0, n_sets=4)");
        expect(bs.set(true, T, W, S, badw.data(), set_of.data(), B, MAXB), MGADMM_ERR_INVALID, "set_sample_bands: band_w[2][5][1] is not finite");
        badw = tabs;
        badw[(size_t)(3 * T + 23) * W + 5] = inf;
        expect(bs.set(true, T, W, S, badw.data(), set_of.data(), B, MAXB), MGADMM_ERR_INVALID, "set_sample_bands: band_w[3][23][5] is not finite");
        // entries no operator reads are ignored: s >= min(t, skip) -- row 0 whole, [1][1 ..], [2][2 ..], ...
        badw = tabs;
        for (int j = 0; j < S; ++j)
            for (int t = 0; t < T; ++t)
                for (int s = 0; s < W; ++s)
                    if (!bandsets::is_read(t, s, W)) badw[((size_t)j * T + t) * W + s] = (t + s) % 2 ? nan : inf;
        CHECK(unchanged(), "a refused call changed the table");
        expect(bs.set(true, T, W, S, badw.data(), set_of.data(), B, MAXB), MGADMM_OK, "");
        CHECK(bs.B == B, "non-finite entries that are never read must be accepted");
    }
    int n_read = 0;
    for (int t = 0; t < T; ++t)
        for (int s = 0; s < W; ++s) n_read += bandsets::is_read(t, s, W);
    CHECK(n_read == 0 + 1 + 2 + 3 + 4 + 5 + (T - 6) * 6, "entries read: %d", n_read);
    // clearing: n_sets == 0, a null table, a null index
    expect(bs.set(true, T, W, 0, tabs.data(), set_of.data(), B, MAXB), MGADMM_OK, "");
    CHECK(bs.B == 0 && bs.w.empty() && bs.set_of.empty(), "n_sets == 0 clears");
    expect(bs.set(true, T, W, S, tabs.data(), set_of.data(), B, MAXB), MGADMM_OK, "");
    expect(bs.set(false, T, W, S, nullptr, set_of.data(), B, MAXB), MGADMM_OK, "");      // (clears on any graph)
    CHECK(bs.B == 0, "a null table clears");
    expect(bs.set(true, T, W, S, tabs.data(), set_of.data(), B, MAXB), MGADMM_OK, "");
    expect(bs.set(true, T, W, S, tabs.data(), nullptr, B, MAXB), MGADMM_OK, "");
    CHECK(bs.B == 0, "a null index clears");

    // ---- the gate of a solve, decided after solvegate::solve_gate
    const solvegate::Facts fixed{true, MGADMM_PATH_AUTO, MGADMM_CG_PER_SAMPLE, MGADMM_ADMM_WHOLE_BATCH, 0, true, true, 30, T};
    solvegate::Facts f = fixed;
    expect(bandsets::solve_gate(bs, f, 5), MGADMM_OK, "");      // no table: nothing to refuse
    expect(bs.set(true, T, W, S, tabs.data(), set_of.data(), B, MAXB), MGADMM_OK, "");
    expect(bandsets::solve_gate(bs, f, B), MGADMM_OK, "");
    expect(bandsets::solve_gate(bs, f, B + 1), MGADMM_ERR_INVALID, "solve: the sample_bands table holds 70 samples, the solve has B = 71");
    f.check_stop = 1;
    expect(bandsets::solve_gate(bs, f, B), MGADMM_ERR_UNSUPPORTED,
           "solve: sample_bands with check_stop need admm_convergence per_sample (the whole_batch stop test would sum the residuals of "
           "different problems); or run a fixed count with check_stop = 0");
    CHECK(bandsets::solve_gate(bs, f, B).msg == solvegate::own_stop_only(bandsets::SAMPLE_BANDS, f).msg, "the wording of own_stop_only");
    expect(bandsets::solve_gate(bs, f, B - 1), MGADMM_ERR_INVALID, "solve: the sample_bands table holds 70 samples, the solve has B = 69");      // B first
    f.admm_convergence = MGADMM_ADMM_PER_SAMPLE;
    expect(bandsets::solve_gate(bs, f, B), MGADMM_OK, "");
    // both paths, both scalar types, either CG rule: nothing else is refused
    for (int f32 = 0; f32 < 2; ++f32)
        for (int path : {MGADMM_PATH_AUTO, MGADMM_PATH_STREAM, MGADMM_PATH_LDS})
            for (int cgc : {MGADMM_CG_PER_SAMPLE, MGADMM_CG_BATCH_MAX}) {
                solvegate::Facts q = fixed;
                q.f32 = f32 != 0; q.path = path; q.cg_convergence = cgc; q.lds_ok = f32 != 0;
                expect(bandsets::solve_gate(bs, q, B), MGADMM_OK, "");
            }

    // ---- the records of the LDS launches: a band table alone reads records of the scalars, everything else is table_of's
    {
        const solvegate::SetState none{0, 0, 0, 0, false}, sp{B, 0, 0, 0, false}, sch{0, 0, 5, B, false}, ad{0, 0, 0, 0, true};
        const BandSets off;
        auto same = [](const solvegate::TableChoice& a, const solvegate::TableChoice& b) {
            return a.table == b.table && a.sp_rows == b.sp_rows && a.sp_row0 == b.sp_row0 && a.stride_B == b.stride_B && a.scalar_records == b.scalar_records;
        };
        for (const auto& s : {none, sp, sch, ad}) {
            const auto base = solvegate::table_of(s, 2, 9);
            CHECK(same(bandsets::table_of(base, off), base), "without a band table the choice is table_of's");
            if (base.table != solvegate::TABLE_NONE) CHECK(same(bandsets::table_of(base, bs), base), "a table that is set stays");
        }
        const auto alone = bandsets::table_of(solvegate::table_of(none, 0, 9), bs);
        CHECK(alone.table == solvegate::TABLE_SAMPLE && alone.scalar_records && !alone.stride_B && alone.sp_rows == 0 && alone.sp_row0 == 0, "a band table alone");
    }

    // ---- the expansion: [T*skip][Bp], column b the table of set_of[b], the padded columns zero
    for (int Bp : {128, 70, 256}) {
        std::vector<float> exp;
        bs.expand(Bp, exp);
        CHECK(exp.size() == (size_t)T * W * Bp, "size of the expansion for Bp %d", Bp);
        size_t wrong = 0, pad_nonzero = 0;
        for (int e = 0; e < T * W; ++e)
            for (int b = 0; b < Bp; ++b) {
                const float v = exp[(size_t)e * Bp + b];
                if (b < B) wrong += memcmp(&v, &tabs[(size_t)set_of[(size_t)b] * T * W + e], sizeof(float)) != 0;
                else pad_nonzero += v != 0.0f || std::signbit(v);
            }
        CHECK(wrong == 0 && pad_nonzero == 0, "expansion for Bp %d: %zu wrong entries, %zu padding entries that are not +0", Bp, wrong, pad_nonzero);
    }
    {
        const std::vector<int32_t> padded = bs.padded_set_of(128);
        bool ok = padded.size() == 128;
        for (int b = 0; ok && b < 128; ++b) ok = padded[(size_t)b] == (b < B ? set_of[(size_t)b] : 0);
        CHECK(ok, "padded_set_of");
    }

    // ---- a narrow table in the solver's width: equal on the entries that are read, and the stencils agree bit for bit
    std::vector<float> x((size_t)T);
    for (int t = 0; t < T; ++t) x[(size_t)t] = (t % 5 - 2) * 37.25f + 1e-3f * (float)t - (t % 3 == 0 ? 411.f : 0.f);
    for (int s : {1, 2, 3, 5, 6}) {
        const std::vector<float> native = uniform_table(T, s, s), padded = bandsets::pad_width(native.data(), T, s, W);
        CHECK(padded == uniform_table(T, s, W), "pad_width against the table built in the wide layout, skip %d", s);
        for (int t = 0; t < T; ++t)
            for (int h = 0; h < W; ++h) {
                if (!bandsets::is_read(t, h, W)) continue;
                const float want = h < s && bandsets::is_read(t, h, s) ? native[(size_t)t * s + h] : 0.0f;
                CHECK(memcmp(&want, &padded[(size_t)t * W + h], sizeof(float)) == 0, "skip %d entry [%d][%d]", s, t, h);
            }
        const std::vector<float> a = stencils(native, T, s, x), b = stencils(padded, T, W, x);
        CHECK(memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0, "stencils of the padded table differ from the native ones, skip %d", s);
    }

    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("{\"sets\": %d, \"B\": %d, \"T\": %d, \"skip\": %d, \"entries_read\": %d, \"feature\": \"%s\"}\n", S, B, T, W, n_read, bandsets::SAMPLE_BANDS.name);
    return 0;
}
