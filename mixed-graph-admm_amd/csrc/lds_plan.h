// Planner of the LDS-resident fused path: which k_admm_lds instance (lds_dispatch.h) a graph gets, the geometry of its
// workgroup, and the image of tables the kernel reads (layout: lds_args.h, LdsArgsCore::csr).  Plain C++, no HIP: compiled
// into libmgadmm.so (Engine::plan_lds uploads the image) and into the CPU check tests/cpu/lds_plan_check.cpp, which
// tests/test_lds_plan_cpu.py runs on the instance census and against images recorded from the planner's earlier form.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "host_csr.h"
#include "lds_banks.h"
#include "lds_consts.h"
#include "lds_rows.h"

namespace ldsplan {

constexpr size_t LDS_LIMIT = 160 * 1024;    // bytes of LDS a workgroup may take

// The planner's environment switches (tests / experiments; read when a solver is created)
struct Switches {
    bool tpg_set = false;         // MGADMM_LDS_TPG is set: only the width it names is considered
    int tpg = 0;
    bool sb_set = false;          // MGADMM_LDS_SB is set at all: no preference for the uniform-row width
    int sb = 0;                   // MGADMM_LDS_SB: 1 = one LDS vector for p and q (experiments)
    bool ragged = false;          // MGADMM_LDS_RAGGED: the generic instance also for a uniform-row graph
    bool noslots = false;         // MGADMM_LDS_NOSLOTS: no LDS vectors for per-thread operands
    int row_order = ldsrows::TAIL_CLASS;   // MGADMM_LDS_ROW_ORDER, 0 .. 2 (ldsrows::Order; see make())
    bool table_order = false;     // MGADMM_LDS_TABLE_ORDER: keep the table's entry order (no bank-aware order)
    long bank_search = 4000;      // MGADMM_LDS_BANK_SEARCH: steps of the bank-conflict search (0: greedy only)
    bool bank_stats = false;      // MGADMM_LDS_BANK_STATS: print what the search gained

    static Switches from_env() {
        Switches s;
        if (const char* e = getenv("MGADMM_LDS_TPG")) { s.tpg_set = true; s.tpg = atoi(e); }
        if (const char* e = getenv("MGADMM_LDS_SB")) { s.sb_set = true; s.sb = atoi(e); }
        s.ragged = getenv("MGADMM_LDS_RAGGED") != nullptr;
        s.noslots = getenv("MGADMM_LDS_NOSLOTS") != nullptr;
        if (const char* e = getenv("MGADMM_LDS_ROW_ORDER")) s.row_order = std::max(0, std::min(atoi(e), 2));
        s.table_order = getenv("MGADMM_LDS_TABLE_ORDER") != nullptr;
        if (const char* e = getenv("MGADMM_LDS_BANK_SEARCH")) s.bank_search = atol(e);
        s.bank_stats = getenv("MGADMM_LDS_BANK_STATS") != nullptr;
        return s;
    }
};

// The graph in API node order.  Band mode: W_d and W_d^T are not read.  transpose_by_gather: W_d^T is W_d itself.
struct Input {
    int T, N;
    bool band, transpose_by_gather;
    const HostCsr &Wu, &Wd, &WdT;
};

struct LdsPlan {
    bool ok = false;
    int G = 0, TPG = 0, TS = 0, nthreads = 0, block = 0, NR = 0, csr_ints = 0, maxt = 1024, sb = 0, uniform45 = 0, slots = 0;
    int tail_pairs = 0, lds_img0 = 0, lds_img_ints = 0;
    int off_rp_u = 0, off_rp_d = 0, off_en_u = 0, off_en_d = 0, off_lead_t = 0, off_tail_t = 0, off_diag = 0;
    int row_order = 0;            // ldsrows::Order of the thread -> row map (lds_rows.h); 0: node order
    int off_node = 0, off_rown = 0;   // node_of_row [NR] / row_of_node [N] in the global image
    uint64_t npos_word = 0;       // table positions per wave, 4-bit fields (LdsArgs::npos)
    size_t lds_bytes = 0;
    int cg_barriers = 0;          // workgroup barriers per CG iteration of a cLdr solve (MGADMM_Q_LDS_CG_BARRIERS)
    int64_t instance = -1;        // lds_instance_key of the k_admm_lds instance the plan is for
};

enum Status { PLANNED, NO_PLAN, ROWS_DO_NOT_FIT };   // NO_PLAN: the graph takes the streaming path; the last one is an error

// kNN tables with k = 4 and no pads (the reference's setting): every W_u row has 4, every W_d row 5 entries, one of them the
// diagonal.  Not with transpose_by_gather: the uniform-row instances take p . A p from |Ldr p|^2 (lds_kernels.h, lds_fold_v),
// which needs the exact transpose of W_d.
inline bool uniform_rows(const Input& in) {
    if (in.band || in.transpose_by_gather) return false;
    for (int i = 0; i < in.N; ++i) {
        int ndiag = 0;
        for (int e = in.Wd.rowptr[i]; e < in.Wd.rowptr[i + 1]; ++e) ndiag += in.Wd.col[e] == i;
        if (in.Wu.rowptr[i + 1] - in.Wu.rowptr[i] != 4 || in.Wd.rowptr[i + 1] - in.Wd.rowptr[i] != 5 || ndiag != 1) return false;
    }
    return true;
}

// Time steps per thread (0: none fits): the smallest width = the most threads, unless the uniform-row instance of width 8
// applies, which is the fastest form also for graphs small enough for narrower groups.
// (Twelve time steps per thread in a 640-thread workgroup -- 10 waves, 168 registers per thread, MGADMM_LDS_TPG=12 -- were
// 5 % ahead of eight in a 960-thread one while the eight-step instance still spilled around its solves, and are 4 %
// behind since it does not: cfg2 2.08 M against 2.17 M sample-iterations/s.  The smallest width stays the default.)
inline int choose_width(const Input& in, const Switches& sw, bool uniform) {
    const bool prefer8 = uniform && !sw.tpg_set && !sw.sb_set && !sw.ragged;
    int best = 0;
    for (int tpg : {1, 2, 3, 4, 6, 8, 12}) {
        if (in.T % tpg || (long)in.N * (in.T / tpg) > 1024) continue;
        if (sw.tpg_set && sw.tpg != tpg) continue;
        if (!best || (prefer8 && tpg == 8)) best = tpg;
    }
    return best;
}

// W_d^T: LDS_NLEAD leading entries per row + a tail table of 2 * tail_pairs entries per row (rows padded with {own row,
// weight 0}): one table width for every lane of the workgroup.  max_indeg: the longest off-diagonal row.
inline int tail_pairs(int max_indeg, int nlead = LDS_NLEAD) { return (std::max(0, max_indeg - nlead) + 1) / 2; }
inline int table_width(int pairs, int nlead = LDS_NLEAD) { return nlead + 2 * pairs; }

// h without its diagonal entries, which are added to dg: inside a CG solve their operand is the thread's own vector
// (registers), no LDS read
inline HostCsr strip_diag(const HostCsr& h, int N, std::vector<float>& dg) {
    HostCsr o;
    o.rowptr.push_back(0);
    for (int i = 0; i < N; ++i) {
        for (int e = h.rowptr[i]; e < h.rowptr[i + 1]; ++e) {
            if (h.col[e] == i) dg[i] += h.val[e];
            else { o.col.push_back(h.col[e]); o.val.push_back(h.val[e]); }
        }
        o.rowptr.push_back((int)o.col.size());
    }
    return o;
}

// h with the ghosts' rows N .. NR-1 appended: `fixed_len` entries {own row, weight 0} each
inline HostCsr with_ghosts(const HostCsr& h, int N, int NR, int fixed_len) {
    HostCsr o;
    o.rowptr.assign(h.rowptr.begin(), h.rowptr.begin() + N + 1);
    o.col = h.col; o.val = h.val;
    for (int r = N; r < NR; ++r) {
        for (int e = 0; e < fixed_len; ++e) { o.col.push_back(r); o.val.push_back(0.f); }
        o.rowptr.push_back((int)o.col.size());
    }
    return o;
}

// offsets of the image's parts (ints) for tables of nu + nd entries; returns the image's length
inline int lay_out(LdsPlan& p, int N, int nu, int nd) {
    auto al4 = [](int v) { return (v + 3) & ~3; };
    const int NR = p.NR;
    int off = 0;
    p.off_rp_u = off; off += NR + 1;
    p.off_rp_d = off; off += NR + 1;
    off = al4(off);
    p.off_en_u = off; off += 2 * nu;
    p.off_en_d = off; off += 2 * nd;
    p.off_lead_t = off; off += 2 * NR * LDS_NLEAD;
    off = al4(off);
    p.off_tail_t = off; off += 2 * NR * 2 * p.tail_pairs + 4;     // + one pair: gather_tail requests the next pair ahead
    const int tail_ints = off - p.off_tail_t;
    p.off_diag = off; off += 2 * NR;
    off += 8;                                        // the paired loops of the ragged gathers read three entries ahead
    p.off_node = off; off += NR;                     // node_of_row (ghost rows: 0), read by k_admm_lds once per trip
    p.off_rown = off; off += N;                      // row_of_node, read by k_init_lds / k_state_layout
    p.csr_ints = off;
    // the part every workgroup copies to LDS: all tables, or -- the uniform-row instances read their fixed-length rows from
    // the global image once per solve -- the tail table alone
    p.lds_img0 = p.uniform45 ? p.off_tail_t : 0;
    p.lds_img_ints = p.uniform45 ? tail_ints : p.off_diag;
    return off;
}

// dynamic LDS of a workgroup: the vectors at row stride `stride`, the reduction scratch, the slot vectors and the image part
inline size_t lds_bytes(const LdsPlan& p, int stride, int slots) {
    const size_t LN = (size_t)p.NR * stride;
    return sizeof(float) * ((p.sb ? 1 : 2) * LN + ((4 - (LN & 3)) & 3) + 32 + 16 * 12 + (size_t)slots * 2 * p.block * p.TPG)
           + sizeof(int) * (size_t)p.lds_img_ints;
}

// The tables of a plan written into its image.
// Bank-aware entry order (lds_banks.h).  A gather instruction reads entry e of 64 consecutive threads' rows (64 consecutive
// nodes, mostly); ds_read_b128 serves it in four groups of 16 lanes, and two lanes of a group collide when their neighbour
// rows start in the same 16-byte slot of the 256-byte bank line.  WHICH neighbour sits in entry e of a row is free.  Round 1
// kept the table order (36 % of the LDS cycles of k_admm_lds were bank conflicts); round 2 a greedy order, rows in node
// order, as the start of a min-conflicts search against an exact replay of the kernel's read stream
// (ldsbank::improve_targeted): cfg2 goes from 7 800 to 1 200 weighted conflict cycles in 0.15 s of host time per solver.
// The sum of a row runs in the chosen order (fixed per graph: repeatable).
struct ImageWriter {
    const LdsPlan& p;
    const Switches& sw;
    ldsbank::Geometry q;
    bool bank_order;
    std::vector<int>& img;

    void put_entry(int at, int col, float w) {
        img[at] = col * p.TS;                            // LDS float offset of the neighbour's time row
        memcpy(&img[at + 1], &w, 4);
    }
    // order[e] = index into h.col / h.val of the entry the kernel reads at position e (real rows only; ghosts' rows follow as they are)
    std::vector<int> entry_order(const HostCsr& h, ldsbank::Stream stream) {
        std::vector<int> order(h.nnz());
        for (int e = 0; e < h.nnz(); ++e) order[e] = e;
        if (!bank_order || h.nnz() == 0) return order;
        const int N = q.N;
        ldsbank::Mat m;
        m.rowptr.assign(h.rowptr.begin(), h.rowptr.begin() + N + 1);
        m.col.assign(h.col.begin(), h.col.begin() + h.rowptr[N]);
        m.src.assign(order.begin(), order.begin() + h.rowptr[N]);
        m.stream = stream;
        ldsbank::greedy_order(q, m);
        if (sw.bank_search > 0) {
            std::vector<int> pos(N);
            for (int i = 0; i < N; ++i) pos[i] = i;
            const ldsbank::Result r = ldsbank::improve_targeted(q, m, pos, sw.bank_search);
            if (sw.bank_stats)
                fprintf(stderr, "[mgadmm] lds bank search: stream %d, %d entries: %.0f -> %.0f conflict cycles per application (%ld steps)\n",
                        (int)stream, h.rowptr[N], r.before, r.after, r.moves);
        }
        for (int e = 0; e < h.rowptr[N]; ++e) order[e] = m.src[e];
        return order;
    }
    void put_csr(const HostCsr& h, int off_rp, int off_en, ldsbank::Stream stream) {
        const std::vector<int> order = entry_order(h, stream);
        for (int i = 0; i <= p.NR; ++i) img[off_rp + i] = h.rowptr[i];
        for (int e = 0; e < h.nnz(); ++e) put_entry(off_en + 2 * e, h.col[order[e]], h.val[order[e]]);
    }
    // W_d^T as a table of `WT` entries per row: the row's entries, then {own row, 0}; every lane reads every position (FIXED
    // stream of the bank model), the first LDS_NLEAD positions from registers, the others from the tail table.  With a row
    // plan the entries of row r sit in the positions below lim[r] (what every wave that owns the row gathers).
    void put_table(const HostCsr& off_diag_t, const ldsrows::Plan& rows, int WT) {
        const int N = q.N, NR = p.NR, tp = p.tail_pairs;
        ldsbank::Result sr;
        const ldsrows::Table ht = ldsrows::build_table(q, off_diag_t.rowptr, off_diag_t.col, off_diag_t.val, rows, WT, bank_order, sw.bank_search, &sr);
        if (bank_order && sw.bank_search > 0 && sw.bank_stats)
            fprintf(stderr, "[mgadmm] lds bank search: W_d^T table, %d entries: %.0f -> %.0f conflict cycles per application (%ld steps)\n",
                    off_diag_t.rowptr[N], sr.before, sr.after, sr.moves);
        for (int r = 0; r < NR; ++r)
            for (int e = 0; e < WT; ++e) {
                const int at = e < LDS_NLEAD ? p.off_lead_t + 2 * (r * LDS_NLEAD + e)
                                             : p.off_tail_t + 2 * (r * 2 * tp + (e - LDS_NLEAD));
                if (r < N) put_entry(at, ht.col[(size_t)r * WT + e], ht.val[(size_t)r * WT + e]);
                else put_entry(at, r, 0.f);
            }
        put_entry(p.off_tail_t + 2 * NR * 2 * tp, 0, 0.f);
        put_entry(p.off_tail_t + 2 * NR * 2 * tp + 2, 0, 0.f);
    }
};

// The plan and the image for a graph.  NO_PLAN leaves a default plan (ok == false) and an empty image.
inline Status make(const Input& in, const Switches& sw, LdsPlan& p, std::vector<int>& img) {
    const int T = in.T, N = in.N;
    const bool band = in.band;
    p = LdsPlan();
    img.clear();
    const bool uniform = uniform_rows(in);
    const int best = choose_width(in, sw, uniform);
    if (!best) return NO_PLAN;
    p.TPG = best;
    p.G = T / best;
    p.nthreads = N * p.G;
    p.block = (p.nthreads + 63) / 64 * 64;
    // register budget: the kernel is compiled for the smallest workgroup-size class that holds the block
    p.maxt = (best == 12 && p.block <= 640) ? 640 : 1024;
    p.sb = (sw.sb && ((best == 12 && p.maxt == 640) || best == 8)) ? 1 : 0;
    // the threads of the last wave that own no element are GHOSTS (lds_kernels.h): each gets an LDS row of zeros and table
    // rows of zero weights
    const int NR = p.NR = N + (p.block - p.nthreads);
    // the uniform-row instances (widths 8 and 12): unrolled gathers, rows read from the global image into registers,
    // p . A p of a cLdr solve folded into the q exchange -- one barrier less per CG iteration than the generic instances,
    // which with a single LDS vector need one more
    p.uniform45 = (uniform && (best == 8 || best == 12) && !p.sb && !sw.ragged) ? 1 : 0;
    p.cg_barriers = p.uniform45 ? 3 : 4 + p.sb;
    std::vector<int> deg_t(N, 0);                         // off-diagonal in-degree of W_d = length of a W_d^T row
    if (!band)
        for (int i = 0; i < N; ++i)
            for (int e = in.WdT.rowptr[i]; e < in.WdT.rowptr[i + 1]; ++e) deg_t[i] += in.WdT.col[e] != i;
    const int tp = p.tail_pairs = band ? 0 : tail_pairs(N > 0 ? *std::max_element(deg_t.begin(), deg_t.end()) : 0);
    const int WT = table_width(tp);
    const bool ct_tail = p.uniform45 && tp <= 3;          // the pair count is a compile-time constant of the instance
    // ROW PLAN (lds_rows.h) of the uniform-row instances with a compile-time tail: the rows that need tail pairs are owned
    // by the first threads of every time group, so that most waves hold rows that fit the leading entries and gather no tail
    // pair at all (a wave gathers as many table positions as its longest row holds).  From here on the planner works on the
    // relabelled graph (row numbers); node numbers stay in the HBM-facing indices (node_of_row for k_admm_lds, row_of_node
    // for k_init_lds / k_state_layout).
    // MGADMM_LDS_ROW_ORDER: 2 (default) = by tail pairs needed, node order inside a class; 1 = by in-degree (fewest positions,
    // but the neighbours of consecutive lanes are scattered: the bank conflicts of all three gathers cost more than the
    // positions save); 0 = node order and full counts (the A/B leg).  The other instances: always node order.
    p.row_order = ct_tail ? sw.row_order : 0;
    const ldsrows::Plan rows = ldsrows::make_plan(deg_t, p.G, WT, p.row_order, LDS_NLEAD);
    if (ct_tail && !ldsrows::pack_npos(rows, &p.npos_word)) return ROWS_DO_NOT_FIT;

    // host tables: relabelled, diagonals kept out (W_d^T of every instance, W_d of the uniform-row ones), ghosts' rows appended
    const HostCsr Wu = p.row_order ? ldsrows::relabel(in.Wu, rows) : in.Wu;
    const HostCsr Wd = band ? HostCsr() : (p.row_order ? ldsrows::relabel(in.Wd, rows) : in.Wd);
    const HostCsr WdT = band ? HostCsr() : (p.row_order ? ldsrows::relabel(in.WdT, rows) : in.WdT);
    std::vector<float> diag_d(NR, 0.f), diag_t(NR, 0.f);
    const HostCsr off_diag_t = band ? HostCsr() : strip_diag(WdT, N, diag_t);
    const HostCsr hu = with_ghosts(Wu, N, NR, p.uniform45 ? 4 : 0);
    const HostCsr hd = band ? HostCsr() : with_ghosts(p.uniform45 ? strip_diag(Wd, N, diag_d) : Wd, N, NR, p.uniform45 ? 4 : 0);
    const int ints = lay_out(p, N, hu.nnz(), hd.nnz());
    // LDS row stride: T padded to an odd number of 16-byte slots (rows then start on every bank group); the unpadded
    // stride when the padded vectors do not fit
    int ts = (T + 3) / 4 * 4;
    if (((ts / 4) & 1) == 0) ts += 4;
    if (lds_bytes(p, ts, 0) > LDS_LIMIT) ts = T;
    if (lds_bytes(p, ts, 0) > LDS_LIMIT) { p = LdsPlan(); return NO_PLAN; }
    p.TS = ts;
    // two more LDS vectors for per-thread operands (uniform-row instances): when they fit beside the padded images
    p.slots = (p.uniform45 && !sw.noslots && lds_bytes(p, ts, 1) <= LDS_LIMIT) ? 1 : 0;
    p.lds_bytes = lds_bytes(p, ts, p.slots);
    p.instance = p.uniform45 ? lds_instance_key(best, false, p.maxt, false, 4, 5, p.slots, ct_tail ? tp : -1)
                             : lds_instance_key(best, band, p.maxt, p.sb, 0, 0, false, -1);

    img.assign(ints, 0);
    ldsbank::Geometry q;
    q.N = N; q.G = p.G; q.TPG = best; q.TS = ts; q.nlead = LDS_NLEAD;
    ImageWriter w{p, sw, q, !band && best % 4 == 0 && ((ts / 4) & 1) && !sw.table_order, img};
    const ldsbank::Stream fixed_or_pairs = p.uniform45 ? ldsbank::FIXED : ldsbank::PAIRS;     // gather_regs / gather
    w.put_csr(hu, p.off_rp_u, p.off_en_u, fixed_or_pairs);
    if (!band) {
        w.put_csr(hd, p.off_rp_d, p.off_en_d, fixed_or_pairs);
        w.put_table(off_diag_t, rows, WT);
        memcpy(&img[p.off_diag], diag_d.data(), sizeof(float) * NR);
        memcpy(&img[p.off_diag + NR], diag_t.data(), sizeof(float) * NR);
    }
    for (int r = 0; r < N; ++r) { img[p.off_node + r] = rows.node_of_row[r]; img[p.off_rown + r] = rows.row_of_node[r]; }
    p.ok = true;
    return PLANNED;
}

}  // namespace ldsplan
