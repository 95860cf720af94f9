// Row plan of the uniform-row instances of k_admm_lds (lds_kernels.h) with a compile-time tail: which node a thread owns, and
// how many positions of the padded W_d^T table each wave gathers.  Plain C++, no HIP: compiled into libmgadmm.so
// (ldsplan::make, lds_plan.h) and into the CPU check tests/cpu/lds_rows_check.cpp.
//
// The W_d^T table has one width for every row (LDS_NLEAD register entries + 2 * tail_pairs tail entries); a row with fewer
// off-diagonal entries is padded with {own row, weight 0}.  A wave can skip a position only when it is a pad for ALL of its
// lanes.  In node order every wave holds a long row; with the long rows owned by the first threads of a time group most waves
// hold short rows only, and the largest in-degree among a wave's rows -- npos[w] -- is the number of positions that wave has
// to gather.  The LDS path then works on the RELABELLED graph (row r = node node_of_row[r], columns mapped by row_of_node):
// ghost rows, diagonals, the tables and the bank model see row numbers only; node numbers are left in the HBM-facing indices
// (x, y, mask).
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "lds_banks.h"

namespace ldsrows {

struct Plan {
    std::vector<int> node_of_row, row_of_node;   // [N] permutation and its inverse
    std::vector<int> npos;                       // [waves] table positions wave w gathers (ghost rows count 0)
    std::vector<int> lim;                        // [N] smallest npos over the G waves that hold a thread of row r
};
// (lim may lie below the number of leading entries -- a wave of rows of in-degree <= 4 -- although k_admm_lds gathers every
// leading position today: the table keeps "every real entry below npos of every owning wave" as its invariant, so that cutting
// the leading gathers per wave needs no other table.  The bank search of such rows is narrower than it has to be; at cfg2
// under the default order no wave is below the five leading entries.)

// Row orders: NODE = identity, every wave gathers every position; IN_DEGREE = stable sort by descending in-degree (the fewest
// positions per wave); TAIL_CLASS = stable sort by descending number of tail pairs a row needs (rows that fit the `nlead`
// leading entries keep node order among themselves: the neighbours of consecutive lanes stay consecutive rows, which is what
// keeps the gathers of W_u and W_d free of bank conflicts on road-like graphs).
enum Order { NODE = 0, IN_DEGREE = 1, TAIL_CLASS = 2 };

// deg[i]: off-diagonal in-degree of node i in W_d (= length of its W_d^T row); G time groups (thread g * N + r owns row r);
// width: positions of the table.
inline Plan make_plan(const std::vector<int>& deg, int G, int width, int order, int nlead = 0) {
    const int N = (int)deg.size();
    const int nw = (N * G + 63) / 64;
    const bool reorder = order != NODE;
    Plan p;
    p.node_of_row.resize(N);
    std::iota(p.node_of_row.begin(), p.node_of_row.end(), 0);
    auto key = [&](int i) { return order == TAIL_CLASS ? (std::max(0, deg[i] - nlead) + 1) / 2 : deg[i]; };
    if (reorder) std::stable_sort(p.node_of_row.begin(), p.node_of_row.end(), [&](int a, int b) { return key(a) > key(b); });
    p.row_of_node.resize(N);
    for (int r = 0; r < N; ++r) p.row_of_node[p.node_of_row[r]] = r;
    p.npos.assign(nw, reorder ? 0 : width);
    if (reorder)
        for (int tid = 0; tid < N * G; ++tid) p.npos[tid / 64] = std::max(p.npos[tid / 64], deg[p.node_of_row[tid % N]]);
    p.lim.assign(N, width);
    for (int tid = 0; tid < N * G; ++tid) p.lim[tid % N] = std::min(p.lim[tid % N], p.npos[tid / 64]);
    return p;
}

// npos as 4-bit fields of one word: field w = wave w (at most 16 waves of at most 15 positions)
inline bool pack_npos(const Plan& p, uint64_t* word) {
    if (p.npos.size() > 16) return false;
    uint64_t v = 0;
    for (size_t w = 0; w < p.npos.size(); ++w) {
        if (p.npos[w] < 0 || p.npos[w] > 15) return false;
        v |= (uint64_t)p.npos[w] << (4 * w);
    }
    *word = v;
    return true;
}

// a CSR structure on the relabelled graph: row r = row node_of_row[r] of the input, columns through row_of_node, the entries
// of a row in the order they had
template <typename Csr>
inline Csr relabel(const Csr& h, const Plan& p) {
    const int N = (int)p.node_of_row.size();
    Csr o = h;
    o.rowptr.assign(1, 0);
    o.col.clear();
    o.val.clear();
    for (int r = 0; r < N; ++r) {
        const int i = p.node_of_row[r];
        for (int e = h.rowptr[i]; e < h.rowptr[i + 1]; ++e) {
            o.col.push_back(p.row_of_node[h.col[e]]);
            o.val.push_back(h.val[e]);
        }
        o.rowptr.push_back((int)o.col.size());
    }
    return o;
}

// The W_d^T table of the kernel: `width` positions per row, [N][width].  Row r holds its off-diagonal entries (rowptr / col /
// val: rows and columns are row numbers) in the positions below lim[r], in the order the bank search picks
// (ldsbank::greedy_order + improve_targeted on the read stream "every lane reads the positions below lim of its row"), and
// {own row, 0} in the others.  from[r * width + e] = index of that entry in col / val, -1 for a pad.
struct Table {
    std::vector<int> col, from;
    std::vector<float> val;
};
inline Table build_table(const ldsbank::Geometry& q, const std::vector<int>& rowptr, const std::vector<int>& col, const std::vector<float>& val,
                         const Plan& p, int width, bool bank_order, long search_steps, ldsbank::Result* stats = nullptr) {
    const int N = q.N;
    ldsbank::Mat m;
    m.stream = ldsbank::FIXED;
    m.rowptr.push_back(0);
    for (int r = 0; r < N; ++r) {
        const int e0 = rowptr[r], len = rowptr[r + 1] - e0;
        const int w = std::max(len, std::min(p.lim[r], width));
        for (int e = 0; e < w; ++e) {
            m.col.push_back(e < len ? col[e0 + e] : r);
            m.src.push_back(e < len ? e0 + e : -1);
        }
        m.rowptr.push_back((int)m.col.size());
    }
    if (bank_order && !m.col.empty()) {
        // (the search carries `src` as indices into its own table)
        std::vector<int> src0 = m.src;
        for (size_t e = 0; e < m.src.size(); ++e) m.src[e] = (int)e;
        ldsbank::greedy_order(q, m);
        if (search_steps > 0) {
            std::vector<int> pos(N);
            std::iota(pos.begin(), pos.end(), 0);
            const ldsbank::Result r = ldsbank::improve_targeted(q, m, pos, search_steps);
            if (stats) *stats = r;
        }
        for (size_t e = 0; e < m.src.size(); ++e) m.src[e] = src0[m.src[e]];
    }
    Table t;
    t.col.resize((size_t)N * width);
    t.from.assign((size_t)N * width, -1);
    t.val.assign((size_t)N * width, 0.f);
    for (int r = 0; r < N; ++r) {
        const int e0 = m.rowptr[r], w = m.rowptr[r + 1] - e0;
        for (int e = 0; e < width; ++e) {
            const int s = e < w ? m.src[e0 + e] : -1;
            t.col[(size_t)r * width + e] = s >= 0 ? col[s] : r;
            t.val[(size_t)r * width + e] = s >= 0 ? val[s] : 0.f;
            t.from[(size_t)r * width + e] = s;
        }
    }
    return t;
}

}  // namespace ldsrows
