// CPU check of the row plan of k_admm_lds (mixed-graph-admm_amd/csrc/lds_rows.h).
//   lds_rows_check <graph file> <nlead> <search steps> <order: 0 node | 1 in-degree | 2 tail class>
// graph file: the format of lds_banks_check.cpp ("N G TPG TS nlead", then per matrix "stream weight nnz", N+1 row pointers,
// nnz columns); the LAST matrix is W_d^T (with its diagonal, which is stripped here).  <nlead>: LDS_NLEAD of the kernel.
// Checks: node_of_row is a permutation in descending order of its key (in-degree, or tail pairs needed; stable) and
// row_of_node its inverse; npos / lim equal
// an independent count; in the table built on the relabelled graph every row keeps its entries, all of them below lim[r] and
// below npos of every wave that owns the row, the other positions are {own row, 0}; a replay of "wave w gathers npos[w]
// positions" equals the full-width product bit for bit; the identity plan has full counts and its table is, entry for
// entry, the one the planner built before the row plan existed (one full-width FIXED-stream search).  Prints "npos: ..." (wave order)
// and the conflict cycles the bank model (lds_banks.h) leaves per application of W_u, W_d and W_d^T under the order.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include "lds_plan.h"       // lds_rows.h; tail_pairs / table_width as the planner computes them

struct Csr {
    std::vector<int> rowptr, col;
    std::vector<float> val;
};

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    ldsbank::Geometry q;
    if (fscanf(f, "%d %d %d %d %d", &q.N, &q.G, &q.TPG, &q.TS, &q.nlead) != 5) return 2;
    q.nlead = atoi(argv[2]);
    const long steps = atol(argv[3]);
    const int order = atoi(argv[4]);
    if (order != ldsrows::NODE && order != ldsrows::IN_DEGREE && order != ldsrows::TAIL_CLASS) return 2;
    Csr full;
    std::vector<Csr> all;
    for (;;) {
        int stream, nnz;
        double w;
        if (fscanf(f, "%d %lf %d", &stream, &w, &nnz) != 3) break;
        full.rowptr.assign(q.N + 1, 0);
        full.col.assign(nnz, 0);
        for (auto& v : full.rowptr) if (fscanf(f, "%d", &v) != 1) return 2;
        for (auto& v : full.col) if (fscanf(f, "%d", &v) != 1) return 2;
        full.val.assign(nnz, 1.f);
        all.push_back(full);
    }
    fclose(f);
    const int N = q.N, G = q.G;
    // off-diagonal W_d^T with weights that are all different
    Csr wt;
    wt.rowptr.push_back(0);
    for (int i = 0; i < N; ++i) {
        for (int e = full.rowptr[i]; e < full.rowptr[i + 1]; ++e)
            if (full.col[e] != i) { wt.col.push_back(full.col[e]); wt.val.push_back(0.25f + 0.001f * (float)wt.col.size()); }
        wt.rowptr.push_back((int)wt.col.size());
    }
    std::vector<int> deg(N);
    int maxdeg = 0;
    for (int i = 0; i < N; ++i) { deg[i] = wt.rowptr[i + 1] - wt.rowptr[i]; maxdeg = std::max(maxdeg, deg[i]); }
    const int tp = ldsplan::tail_pairs(maxdeg, q.nlead);
    const int WT = ldsplan::table_width(tp, q.nlead);
    const int nw = (N * G + 63) / 64;

    const ldsrows::Plan p = ldsrows::make_plan(deg, G, WT, order, q.nlead);
    CHECK((int)p.node_of_row.size() == N && (int)p.row_of_node.size() == N && (int)p.npos.size() == nw && (int)p.lim.size() == N);
    std::vector<int> seen(N, 0);
    auto key = [&](int i) { return order == ldsrows::TAIL_CLASS ? (std::max(0, deg[i] - q.nlead) + 1) / 2 : deg[i]; };
    for (int r = 0; r < N; ++r) {
        const int i = p.node_of_row[r];
        CHECK(i >= 0 && i < N && !seen[i]++);
        CHECK(p.row_of_node[i] == r);
        if (r > 0) {
            const int j = p.node_of_row[r - 1];
            CHECK(order == ldsrows::NODE ? j < i : (key(j) > key(i) || (key(j) == key(i) && j < i)));
        }
    }
    // npos / lim counted per thread
    std::vector<int> npos(nw, 0), lim(N, 1 << 30);
    for (int w = 0; w < nw; ++w)
        for (int l = 0; l < 64; ++l) {
            const int tid = w * 64 + l;
            if (tid < N * G) npos[w] = std::max(npos[w], order == ldsrows::NODE ? WT : deg[p.node_of_row[tid % N]]);
        }
    for (int r = 0; r < N; ++r)
        for (int g = 0; g < G; ++g) lim[r] = std::min(lim[r], npos[(g * N + r) / 64]);
    CHECK(npos == p.npos && lim == p.lim);
    int moved = 0;
    for (int r = 0; r < N; ++r) moved += p.node_of_row[r] != r;
    printf("rows moved %d of %d\n", moved, N);
    printf("npos:");
    for (int w = 0; w < nw; ++w) printf(" %d", p.npos[w]);
    printf("\nwidth %d tail_pairs %d positions %d of %d\n", WT, tp, (int)std::accumulate(npos.begin(), npos.end(), 0), nw * WT);
    uint64_t word = 0;
    if (nw <= 16 && WT <= 15) {          // the launch word holds 16 waves of up to 15 positions (the instances with a compile-time tail: 11)
        CHECK(ldsrows::pack_npos(p, &word));
        for (int w = 0; w < nw; ++w) CHECK((int)((word >> (4 * w)) & 15) == p.npos[w]);
    } else if (maxdeg > 15) {
        CHECK(!ldsrows::pack_npos(p, &word));
    }

    // the table on the relabelled graph
    const Csr rl = ldsrows::relabel(wt, p);
    CHECK((int)rl.rowptr.size() == N + 1 && rl.col.size() == wt.col.size());
    for (int r = 0; r < N; ++r) {
        const int i = p.node_of_row[r];
        CHECK(rl.rowptr[r + 1] - rl.rowptr[r] == deg[i]);
        for (int e = 0; e < deg[i]; ++e) {
            CHECK(rl.col[rl.rowptr[r] + e] == p.row_of_node[wt.col[wt.rowptr[i] + e]]);
            CHECK(rl.val[rl.rowptr[r] + e] == wt.val[wt.rowptr[i] + e]);
        }
    }
    ldsbank::Result sr;
    const ldsrows::Table t = ldsrows::build_table(q, rl.rowptr, rl.col, rl.val, p, WT, true, steps, &sr);
    CHECK((int)t.col.size() == N * WT && t.val.size() == t.col.size() && t.from.size() == t.col.size());
    CHECK(sr.after <= sr.before);
    printf("bank search W_d^T: %.0f -> %.0f conflict cycles\n", sr.before, sr.after);
    // the fixed-width gathers of W_u and W_d (uniform graphs) see the same relabelling
    for (size_t k = 0; k + 1 < all.size(); ++k) {
        Csr off;
        off.rowptr.push_back(0);
        for (int i = 0; i < N; ++i) {
            for (int e = all[k].rowptr[i]; e < all[k].rowptr[i + 1]; ++e)
                if (all[k].col[e] != i) { off.col.push_back(all[k].col[e]); off.val.push_back(1.f); }
            off.rowptr.push_back((int)off.col.size());
        }
        const Csr r2 = ldsrows::relabel(off, p);
        ldsbank::Mat m;
        m.rowptr = r2.rowptr; m.col = r2.col; m.stream = ldsbank::FIXED;
        m.src.resize(m.col.size());
        for (size_t e = 0; e < m.src.size(); ++e) m.src[e] = (int)e;
        ldsbank::greedy_order(q, m);
        std::vector<int> pos(N);
        std::iota(pos.begin(), pos.end(), 0);
        const ldsbank::Result r = ldsbank::improve_targeted(q, m, pos, steps);
        printf("bank search matrix %zu: %.0f -> %.0f conflict cycles\n", k, r.before, r.after);
    }
    for (int r = 0; r < N; ++r) {
        std::map<std::pair<int, float>, int> want, have;
        for (int e = rl.rowptr[r]; e < rl.rowptr[r + 1]; ++e) ++want[{rl.col[e], rl.val[e]}];
        for (int e = 0; e < WT; ++e) {
            const int at = r * WT + e;
            if (t.from[at] >= 0) {
                CHECK(t.from[at] >= rl.rowptr[r] && t.from[at] < rl.rowptr[r + 1]);
                CHECK(t.col[at] == rl.col[t.from[at]] && t.val[at] == rl.val[t.from[at]]);
                ++have[{t.col[at], t.val[at]}];
                CHECK(e < p.lim[r]);
                for (int g = 0; g < G; ++g) CHECK(e < p.npos[(g * N + r) / 64]);
            } else {
                CHECK(t.col[at] == r && t.val[at] == 0.f);
            }
        }
        CHECK(want == have);
    }
    // replay: thread (g, r) of wave w gathers the first npos[w] positions; the full-width sum is what the kernel formed before
    std::vector<float> v(N);
    unsigned rng = 2463534242u;
    for (auto& x : v) { rng = rng * 1664525u + 1013904223u; x = (float)(int)(rng >> 8) / 8388608.f - 1.f; }
    for (int tid = 0; tid < N * G; ++tid) {
        const int r = tid % N, w = tid / 64;
        float a = 0.5f * v[r], b = a;
        for (int e = 0; e < WT; ++e) a = std::fmaf(t.val[r * WT + e], v[t.col[r * WT + e]], a);
        for (int e = 0; e < p.npos[w]; ++e) b = std::fmaf(t.val[r * WT + e], v[t.col[r * WT + e]], b);
        CHECK(std::memcmp(&a, &b, 4) == 0);
    }

    // node order: identity, every wave gathers every position, and the table search sees full-width rows
    const ldsrows::Plan id = ldsrows::make_plan(deg, G, WT, ldsrows::NODE);
    for (int r = 0; r < N; ++r) CHECK(id.node_of_row[r] == r && id.row_of_node[r] == r && id.lim[r] == WT);
    for (int w = 0; w < nw; ++w) CHECK(id.npos[w] == WT);
    const ldsrows::Table ti = ldsrows::build_table(q, wt.rowptr, wt.col, wt.val, id, WT, true, steps);
    {   // ... and is the table every instance had before the row plan existed: the full-width rows {entries, then own row}
        // handed to greedy_order + improve_targeted as one FIXED-stream matrix, positions taken from `src`
        ldsbank::Mat m;
        m.stream = ldsbank::FIXED;
        m.rowptr.push_back(0);
        std::vector<int> hcol;
        std::vector<float> hval;
        for (int i = 0; i < N; ++i) {
            const int e0 = wt.rowptr[i], len = wt.rowptr[i + 1] - e0;
            for (int e = 0; e < WT; ++e) {
                hcol.push_back(e < len ? wt.col[e0 + e] : i);
                hval.push_back(e < len ? wt.val[e0 + e] : 0.f);
            }
            m.rowptr.push_back((int)hcol.size());
        }
        m.col = hcol;
        m.src.resize(hcol.size());
        for (size_t e = 0; e < m.src.size(); ++e) m.src[e] = (int)e;
        ldsbank::greedy_order(q, m);
        std::vector<int> pos(N);
        std::iota(pos.begin(), pos.end(), 0);
        if (steps > 0) ldsbank::improve_targeted(q, m, pos, steps);
        for (int e = 0; e < N * WT; ++e) CHECK(ti.col[e] == hcol[m.src[e]] && ti.val[e] == hval[m.src[e]]);
    }
    for (int r = 0; r < N; ++r) {
        int real = 0;
        for (int e = 0; e < WT; ++e) real += ti.from[r * WT + e] >= 0;
        CHECK(real == deg[r]);
    }
    printf("OK\n");
    return 0;
}
