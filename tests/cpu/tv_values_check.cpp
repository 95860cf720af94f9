// CPU check of csrc/tv_values.h (per-slice value tables of the time-varying weights).  Built with AddressSanitizer + UBSan and
// run as a program of its own by tests/test_tv_values_cpu.py.  On ragged random graphs, T = 2 (W_d: one slice) included:
//   - the table of W^T holds, slice by slice, the dense transpose of the slice, on one shared pattern;
//   - the tables in a permuted node order, read back through the permutation, are the caller's values (round trip);
//   - for every (operator, t in [0, T), row, GW in {4, 6}) the slice index lies in [0, S) and the highest entry offset the row
//     kernel forms (tv::max_offset: the fixed window, or the tail of a long row) lies inside the allocation; every such entry is
//     READ from a vector of exactly the table's size, so a wrong bound is a sanitizer report as well;
//   - check_values names the table and [slice][entry].
// Prints one JSON object.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "tv_values.h"

static int checks = 0, failed = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        ++checks;                                                           \
        if (!(c)) { ++failed; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } \
    } while (0)

// n rows of 0 .. maxlen entries, some longer than 6 (the tail loop), distinct columns per row
static HostCsr random_pattern(int n, int maxlen, std::mt19937& rng) {
    HostCsr A;
    A.n = n;
    A.rowptr.assign(1, 0);
    for (int i = 0; i < n; ++i) {
        const int len = std::min(n, (int)(rng() % (maxlen + 1)));
        std::vector<int> cols(n);
        std::iota(cols.begin(), cols.end(), 0);
        for (int e = 0; e < len; ++e) {
            std::swap(cols[e], cols[e + rng() % (n - e)]);
            A.col.push_back(cols[e]);
        }
        A.rowptr.push_back((int)A.col.size());
    }
    A.val.assign(A.col.size(), 0.0f);
    return A;
}

static std::vector<double> dense(const HostCsr& P, const float* vals) {
    std::vector<double> D((size_t)P.n * P.n, 0.0);
    for (int i = 0; i < P.n; ++i)
        for (int e = P.rowptr[i]; e < P.rowptr[i + 1]; ++e) D[(size_t)i * P.n + P.col[e]] += vals[e];
    return D;
}

static long offsets_checked = 0;

// every offset the kernel forms for operator (shift, S) on pattern P lies inside a table of tv::table_size(S, nnz) floats
static void check_offsets(const HostCsr& P, const std::vector<float>& table, int T, int shift, int S) {
    const int nnz = P.nnz();
    CHECK(table.size() == tv::table_size(S, nnz));
    volatile float sink = 0.0f;
    for (int GW : {4, 6})
        for (int t = 0; t < T; ++t) {
            const int s = tv::slice_of(t, shift, S);
            CHECK(s >= 0 && s < S);
            const int ts = t + shift;
            if (ts >= 0 && ts < T) CHECK(s == (shift < 0 ? t - 1 : t));      // the slice the reference reads (ADMM.py:147, 171, 200, 214)
            for (int i = 0; i < P.n; ++i) {
                const size_t hi = tv::max_offset(P.rowptr, nnz, i, t, shift, S, GW);
                CHECK(hi < table.size());
                // the loads themselves: the window of GW entries, then the tail
                const float* val = table.data() + (size_t)s * nnz;
                for (int u = 0; u < GW; ++u) sink = sink + val[P.rowptr[i] + u];
                for (int e = P.rowptr[i] + GW; e < P.rowptr[i + 1]; ++e) sink = sink + val[e];
                ++offsets_checked;
            }
        }
    (void)sink;
}

int main() {
    std::mt19937 rng(12345);
    for (int T : {2, 3, 4, 7})
        for (int n : {1, 5, 30, 67}) {
            const HostCsr A = random_pattern(n, n >= 30 ? 9 : 4, rng);
            const int nnz = A.nnz();
            for (int S : {T, T - 1}) {
                std::vector<float> vals((size_t)S * nnz);
                for (auto& v : vals) v = (float)(rng() % 1000) / 16.0f + 1.0f;
                std::vector<int> perm(n), iperm(n);
                std::iota(perm.begin(), perm.end(), 0);
                std::shuffle(perm.begin(), perm.end(), rng);
                for (int i = 0; i < n; ++i) iperm[perm[i]] = i;
                HostCsr pat, patT, patP, patTP;
                std::vector<float> tab, tabT, tabP, tabTP;
                CHECK(tv::build_table(A, vals.data(), S, false, nullptr, nullptr, pat, tab));
                CHECK(tv::build_table(A, vals.data(), S, true, nullptr, nullptr, patT, tabT));
                CHECK(tv::build_table(A, vals.data(), S, false, &perm, &iperm, patP, tabP));
                CHECK(tv::build_table(A, vals.data(), S, true, &perm, &iperm, patTP, tabTP));
                CHECK(pat.rowptr == A.rowptr && pat.col == A.col);
                for (int s = 0; s < S; ++s) {
                    const std::vector<double> D = dense(A, vals.data() + (size_t)s * nnz);
                    const std::vector<double> Dt = dense(patT, tabT.data() + (size_t)s * nnz);
                    const std::vector<double> Dp = dense(patP, tabP.data() + (size_t)s * nnz);
                    const std::vector<double> Dtp = dense(patTP, tabTP.data() + (size_t)s * nnz);
                    bool tr = true, rt = true, rtt = true, same = true;
                    for (int i = 0; i < n; ++i)
                        for (int j = 0; j < n; ++j) {
                            tr = tr && Dt[(size_t)j * n + i] == D[(size_t)i * n + j];
                            // internal row r is API node perm[r]: permuting back gives the caller's matrix
                            rt = rt && Dp[(size_t)iperm[i] * n + iperm[j]] == D[(size_t)i * n + j];
                            rtt = rtt && Dtp[(size_t)iperm[j] * n + iperm[i]] == D[(size_t)i * n + j];
                        }
                    for (int e = 0; e < nnz; ++e) same = same && tab[(size_t)s * nnz + e] == vals[(size_t)s * nnz + e];
                    CHECK(tr);
                    CHECK(rt);
                    CHECK(rtt);
                    CHECK(same);
                }
                for (int e = 0; e < tv::TV_PAD; ++e) CHECK(tabT[(size_t)S * nnz + e] == 0.0f);
                // Lu reads T slices with shift 0; Ldr / Ldr^T read T - 1 slices with shift -1 / +1
                if (S == T) {
                    check_offsets(patP, tabP, T, 0, S);
                } else {
                    check_offsets(patP, tabP, T, -1, S);
                    check_offsets(patTP, tabTP, T, +1, S);
                    check_offsets(patP, tabP, T, +1, S);      // transpose_by_gather: Ldr^T on W_d's own table
                }
            }
        }
    // the slice rule at its edges
    CHECK(tv::slice_of(0, -1, 1) == 0 && tv::slice_of(1, -1, 1) == 0);      // T = 2, Ldr
    CHECK(tv::slice_of(0, +1, 1) == 0 && tv::slice_of(1, +1, 1) == 0);      // T = 2, Ldr^T: t = T-1 clamped
    CHECK(tv::slice_of(5, 0, 6) == 5 && tv::slice_of(5, +1, 5) == 4 && tv::slice_of(5, -1, 5) == 4 && tv::slice_of(0, -1, 5) == 0);
    // refusals
    std::string err;
    std::vector<float> v(3 * 4, 1.0f);
    CHECK(tv::check_values("u_val_t", v.data(), 3, 3, 4, err));
    CHECK(!tv::check_values("u_val_t", v.data(), 2, 3, 4, err) && err.find("u_val_t") != std::string::npos && err.find("2 slices") != std::string::npos);
    v[2 * 4 + 1] = std::nanf("");
    CHECK(!tv::check_values("d_val_t", v.data(), 3, 3, 4, err) && err.find("d_val_t[2][1]") != std::string::npos);
    v[2 * 4 + 1] = INFINITY;
    CHECK(!tv::check_values("d_val_t", v.data(), 3, 3, 4, err) && err.find("d_val_t[2][1]") != std::string::npos);
    printf("{\"checks\": %d, \"failed\": %d, \"offsets\": %ld}\n", checks, failed, offsets_checked);
    return failed ? 1 : 0;
}
