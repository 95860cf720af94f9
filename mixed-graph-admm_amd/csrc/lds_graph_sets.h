// Per-sample graph weights on the LDS-resident path (mgadmm_solver_set_sample_graphs): S weight sets of ONE topology, planned
// into images that differ from the solver's own image in the weight words and the diagonal floats only, laid out back to back
// at a fixed stride.  Workgroup b of k_admm_lds_pp reads the image of set gset[b] (lds_kernels.h, MG_LDS_IMG); the plan --
// instance, geometry, every offset, the row plan -- is the solver's.  Plain C++ like lds_plan.h, no HIP and no environment
// reads: compiled into libmgadmm.so (Engine::set_sample_graphs) and into the CPU check tests/cpu/lds_graph_sets_check.cpp.
//
// The planner's structure depends on the neighbour lists alone (the bank search of lds_banks.h replays column offsets with
// fixed seeds, the row plan of lds_rows.h counts in-degrees), so a set with the solver's pattern gets the solver's structure.
// That is CHECKED, not assumed: every set is planned by ldsplan::make with the solver's switches and compared field by field
// and int by int; the first difference is named.  Typical causes: a sigma so small that a weight underflows to 0 and the table
// builder of the caller drops the entry, another k, another transpose rule.
#pragma once
#include <atomic>
#include <string>
#include <thread>

#include "lds_plan.h"

namespace ldssets {

using ldsplan::LdsPlan;

// ints between two images of a table: the image length rounded up to 16 bytes (every image starts as aligned as the first)
inline int img_stride(const LdsPlan& p) { return (p.csr_ints + 3) & ~3; }

// is word `at` of an image a weight (the second int of an entry {LDS offset, weight}) or a diagonal float?  Everything
// else is structure: row pointers, LDS offsets of the entries, pads, node_of_row, row_of_node
inline bool is_weight_word(const LdsPlan& p, int at) {
    if (at >= p.off_en_u && at < p.off_diag) return (at & 1) != 0;      // (off_en_u and off_tail_t are multiples of 4)
    return at >= p.off_diag && at < p.off_diag + 2 * p.NR;
}

// part of the image that holds word `at`
inline const char* part_of(const LdsPlan& p, int at) {
    if (at < p.off_rp_d) return "rp_u";
    if (at < p.off_en_u) return "rp_d";
    if (at < p.off_en_d) return "en_u";
    if (at < p.off_lead_t) return "en_d";
    if (at < p.off_tail_t) return "lead_t";
    if (at < p.off_diag) return "tail_t";
    if (at < p.off_node) return "diag";
    if (at < p.off_rown) return "node_of_row";
    return "row_of_node";
}

// first plan field of `p` that differs from the solver's plan `ref` (nullptr: none)
inline const char* plan_diff(const LdsPlan& ref, const LdsPlan& p) {
#define MG_SETS_FIELD(f) if (ref.f != p.f) return #f;
    MG_SETS_FIELD(ok) MG_SETS_FIELD(instance) MG_SETS_FIELD(nthreads) MG_SETS_FIELD(block) MG_SETS_FIELD(NR) MG_SETS_FIELD(TS)
    MG_SETS_FIELD(tail_pairs) MG_SETS_FIELD(G) MG_SETS_FIELD(TPG) MG_SETS_FIELD(maxt) MG_SETS_FIELD(sb) MG_SETS_FIELD(uniform45)
    MG_SETS_FIELD(slots) MG_SETS_FIELD(row_order) MG_SETS_FIELD(off_rp_u) MG_SETS_FIELD(off_rp_d) MG_SETS_FIELD(off_en_u)
    MG_SETS_FIELD(off_en_d) MG_SETS_FIELD(off_lead_t) MG_SETS_FIELD(off_tail_t) MG_SETS_FIELD(off_diag) MG_SETS_FIELD(off_node)
    MG_SETS_FIELD(off_rown) MG_SETS_FIELD(lds_img0) MG_SETS_FIELD(lds_img_ints) MG_SETS_FIELD(csr_ints) MG_SETS_FIELD(lds_bytes)
    MG_SETS_FIELD(cg_barriers)
#undef MG_SETS_FIELD
    if (ref.npos_word != p.npos_word) return "npos";
    return nullptr;
}

// One more weight set for a solver whose graph was planned as (ref, ref_img) with the switches `sw`: the set's image in
// `img`, or false and in `why` the first thing that differs from the solver's plan ("<field>: ..." -- a plan field by its
// name in LdsPlan, or a part of the image: rp_u, rp_d, en_u, en_d, lead_t, tail_t, node_of_row, row_of_node).
inline bool plan_set(const LdsPlan& ref, const std::vector<int>& ref_img, const ldsplan::Input& in, const ldsplan::Switches& sw,
                     std::vector<int>& img, std::string& why) {
    LdsPlan p;
    ldsplan::Switches quiet = sw;
    quiet.bank_stats = false;
    const ldsplan::Status st = ldsplan::make(in, quiet, p, img);
    if (st != ldsplan::PLANNED) {
        why = st == ldsplan::NO_PLAN ? "ok: the LDS-resident path cannot hold this set" : "npos: the set's row plan does not fit its launch word";
        return false;
    }
    if (const char* f = plan_diff(ref, p)) {
        why = std::string(f) + ": the set's plan differs from the solver's";
        return false;
    }
    if (img.size() != ref_img.size()) { why = "csr_ints: image length"; return false; }
    for (int at = 0; at < (int)img.size(); ++at) {
        if (img[at] == ref_img[at] || is_weight_word(ref, at)) continue;
        char buf[160];
        snprintf(buf, sizeof(buf), "%s: word %d of the image is %d, the solver's is %d", part_of(ref, at), at, img[at], ref_img[at]);
        why = buf;
        return false;
    }
    return true;
}

// The table of S sets: image s at table[s * stride].  false: *bad_set and `why` name the first set that does not share the
// solver's structure (as plan_set).  The sets are planned by up to `threads` host threads side by side (a set costs the
// solver's own bank search; ldsplan::make shares no state between calls).
inline bool build_table(const LdsPlan& ref, const std::vector<int>& ref_img, const std::vector<ldsplan::Input>& sets,
                        const ldsplan::Switches& sw, std::vector<int>& table, int* bad_set, std::string& why, int threads = 1) {
    const int stride = img_stride(ref), S = (int)sets.size();
    table.assign((size_t)stride * S, 0);
    std::vector<std::string> whys((size_t)S);
    std::vector<char> bad((size_t)S, 0);
    std::atomic<int> next{0};
    auto work = [&]() {
        std::vector<int> img;
        for (int s = next++; s < S; s = next++) {
            if (!plan_set(ref, ref_img, sets[(size_t)s], sw, img, whys[(size_t)s])) { bad[(size_t)s] = 1; continue; }
            memcpy(&table[(size_t)s * stride], img.data(), sizeof(int) * img.size());
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < std::min(threads, S); ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    for (int s = 0; s < S; ++s)
        if (bad[(size_t)s]) { *bad_set = s; why = whys[(size_t)s]; table.clear(); return false; }
    return true;
}

}  // namespace ldssets
