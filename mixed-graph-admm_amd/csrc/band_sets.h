// Per-sample temporal band weights (mgadmm_solver_set_sample_bands): S tables of one width for a band (line-graph) solver,
// sample b of a solve reads table set_of_sample[b] (a skip-connection sweep as one batch: a narrower interval is the solver's
// width with zero hops).  The host side: the argument checks and their messages, the caller's arrays, the decisions of a solve
// that come after solvegate::solve_gate, which records the LDS launches read, and the expansion the streaming kernels read.
// Plain C++ like lds_graph_sets.h, no HIP and no environment reads: compiled into libmgadmm.so (Engine) and into the CPU check
// tests/cpu/band_sets_check.cpp.
//
// Which entries count: row t of a table holds the weights of x[t-1-s], s = 0 .. skip-1 (ADMM.py:43-49).  Ldr at step t reads
// [t][s] for t-1-s >= 0, Ldr^T at step t reads [t+1+s][s]: only entries with s < min(t, skip) are ever read, as with the graph's
// own table; the others are neither checked nor compared.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

// (Result, refuse, Facts, Feature, own_stop_only and TableChoice are solve_gate.h's, which whoever includes this header includes
// before it: the engine, which stays the only unit of the library that includes solve_gate.h, and the CPU check)

namespace bandsets {

using solvegate::Facts;
using solvegate::refuse;
using solvegate::Result;

// the wording of the feature in the shared refusals of solve_gate.h
constexpr solvegate::Feature SAMPLE_BANDS = {"sample_bands", " (per-sample temporal band weights)", "are", "need", "", "", "sample_bands", "", false};

// is entry [t][s] of a table of width `skip` read by an operator?
inline bool is_read(int t, int s, int skip) { return s < (t < skip ? t : skip); }

struct BandSets {
    int B = 0;                          // samples of the table; 0 = none set
    int n_sets = 0, T = 0, skip = 0;
    std::vector<float> w;               // [n_sets][T][skip], as the caller gave them
    std::vector<int32_t> set_of;        // [B]

    void clear() { B = n_sets = T = skip = 0; w.clear(); set_of.clear(); }

    // The setter as the ABI has it: n_sets == 0 or a null pointer clears.  band / T_ / skip_: the solver's graph.  A call that
    // refuses leaves the state as it was
    Result set(bool band, int T_, int skip_, int n, const float* band_w, const int32_t* set_of_sample, int B_, int max_batch) {
        if (n == 0 || band_w == nullptr || set_of_sample == nullptr) { clear(); return {}; }
        if (!band)
            return refuse(MGADMM_ERR_UNSUPPORTED, "set_sample_bands: the solver's graph is not MGADMM_TEMPORAL_BAND: a spatial temporal graph has "
                          "no band table to vary (sample_graphs varies its W_d)");
        if (B_ < 1 || B_ > max_batch) return refuse(MGADMM_ERR_INVALID, "set_sample_bands: batch %d outside [1, max_batch=%d]", B_, max_batch);
        if (n < 1 || n > max_batch) return refuse(MGADMM_ERR_INVALID, "set_sample_bands: n_sets %d outside [1, max_batch=%d]", n, max_batch);
        for (int b = 0; b < B_; ++b)
            if (set_of_sample[b] < 0 || set_of_sample[b] >= n)
                return refuse(MGADMM_ERR_INVALID, "set_sample_bands: set_of_sample[%d] = %d outside [0, n_sets=%d)", b, set_of_sample[b], n);
        for (int j = 0; j < n; ++j)
            for (int t = 0; t < T_; ++t)
                for (int s = 0; s < skip_; ++s)
                    if (is_read(t, s, skip_) && !std::isfinite(band_w[((size_t)j * T_ + t) * skip_ + s]))
                        return refuse(MGADMM_ERR_INVALID, "set_sample_bands: band_w[%d][%d][%d] is not finite", j, t, s);
        B = B_; n_sets = n; T = T_; skip = skip_;
        w.assign(band_w, band_w + (size_t)n * T_ * skip_);
        set_of.assign(set_of_sample, set_of_sample + B_);
        return {};
    }

    // The table the streaming kernels read: [T*skip][Bp] floats, column b the table of set_of[b], the padded columns B .. Bp-1
    // zero (Bp >= B: the padded batch of the solve's geometry)
    void expand(int Bp, std::vector<float>& out) const {
        out.assign((size_t)T * skip * Bp, 0.0f);
        for (int e = 0; e < T * skip; ++e)
            for (int b = 0; b < B; ++b) out[(size_t)e * Bp + b] = w[(size_t)set_of[b] * T * skip + e];
    }
    // set_of padded to n entries (the pads read set 0; no workgroup runs for them)
    std::vector<int32_t> padded_set_of(int n) const {
        std::vector<int32_t> o((size_t)n, 0);
        for (int b = 0; b < B && b < n; ++b) o[(size_t)b] = set_of[(size_t)b];
        return o;
    }
};

// A narrow table in the solver's width: [T][skip_from] -> [T][skip_to], skip_from <= skip_to, the new hops zero.  On the entries
// that are read it equals the native table, and `acc += 0 * v` leaves an accumulator that started at +0 bit for bit
inline std::vector<float> pad_width(const float* tab, int T, int skip_from, int skip_to) {
    std::vector<float> o((size_t)T * skip_to, 0.0f);
    for (int t = 0; t < T; ++t)
        for (int s = 0; s < skip_from && s < skip_to; ++s) o[(size_t)t * skip_to + s] = tab[(size_t)t * skip_from + s];
    return o;
}

// A solve of B samples with the table `bs` set: decided after every refusal of solvegate::solve_gate, before anything is
// enqueued.  The samples solve different problems: the rule and wording of solvegate::own_stop_only
inline Result solve_gate(const BandSets& bs, const Facts& f, int B) {
    if (bs.B == 0) return {};
    if (B != bs.B) return refuse(MGADMM_ERR_INVALID, "solve: the %s table holds %d samples, the solve has B = %d", SAMPLE_BANDS.table, bs.B, B);
    return solvegate::own_stop_only(SAMPLE_BANDS, f);
}

// Which records the launches of a solve on the LDS path read: a band table takes the kernels k_admm_lds_pp, which read records,
// so a state for which solvegate::table_of names no table reads records of the scalars (as with a graph table alone)
inline solvegate::TableChoice table_of(const solvegate::TableChoice& base, const BandSets& bs) {
    if (bs.B == 0 || base.table != solvegate::TABLE_NONE) return base;
    return {solvegate::TABLE_SAMPLE, 0, 0, false, true};
}

}  // namespace bandsets
