// Time-varying edge weights of the streaming path: the per-slice value tables k_rows_tv (stream_tv_kernels.h) reads, and the
// rule that says which slice a row at output time t takes.  Plain C++, no HIP: compiled into libmgadmm.so
// (mgadmm_graph_set_time_weights in graph.hip builds and uploads the tables, Engine::rows_v launches on them) and into the CPU
// check tests/cpu/tv_values_check.cpp.
//
// A table holds S slices of the values of ONE CSR pattern (row pointers and column indices are shared: the pattern comes from
// connect_list alone), slice after slice with no gap, and TV_PAD zero entries after the last one:
//     val_t[s * nnz + e]      s in [0, S), e in [0, nnz)          size S * nnz + TV_PAD floats
// The row kernel loads a fixed window of GW entries per row whatever the row's length; what it reads past a row's end lies in
// the next row, the next slice or the pad, and is discarded.
#pragma once
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

#include "host_csr.h"
#include "mg_hd.h"

namespace tv {

constexpr int TV_PAD = 8;      // entries after the last slice (CSR_PAD of stream_kernels.h)

// Slice of an S-slice table that the rows of output time t read, for an operator that gathers from time t + shift:
//   Lu     shift  0, S = T      slice t
//   Ldr    shift -1, S = T - 1  slice t - 1   (t = 0: no gather; the clamp keeps the loads of that row inside the table)
//   Ldr^T  shift +1, S = T - 1  slice t       (t = T - 1: no gather, clamped likewise)
MG_HD inline int slice_of(int t, int shift, int S) {
    const int s = t + (shift < 0 ? shift : 0);
    return s < 0 ? 0 : (s >= S ? S - 1 : s);
}

// floats of a table of S slices
inline size_t table_size(int S, int nnz) { return (size_t)S * nnz + TV_PAD; }

// Highest entry offset a row kernel with gather window GW forms in a table for row i at time t: the fixed window behind the
// row's first entry, or the row's last entry where the tail loop runs (rows longer than GW)
inline size_t max_offset(const std::vector<int>& rowptr, int nnz, int i, int t, int shift, int S, int GW) {
    const int e0 = rowptr[i], e1 = rowptr[i + 1];
    const int last = e1 - e0 > GW ? e1 - 1 : e0 + GW - 1;
    return (size_t)slice_of(t, shift, S) * nnz + last;
}

// The caller's arrays vals[n_slices][nnz]: the slice count and every value.  false: `err` names the table and [slice][entry]
inline bool check_values(const char* name, const float* vals, int n_slices, int want_slices, int nnz, std::string& err) {
    if (n_slices != want_slices) {
        err = std::string(name) + ": " + std::to_string(n_slices) + " slices, the graph needs " + std::to_string(want_slices);
        return false;
    }
    for (int s = 0; s < n_slices; ++s)
        for (int e = 0; e < nnz; ++e)
            if (!std::isfinite(vals[(size_t)s * nnz + e])) {
                err = std::string(name) + "[" + std::to_string(s) + "][" + std::to_string(e) + "] is not finite";
                return false;
            }
    return true;
}

// The table of one matrix in the internal node order.  A: the caller's pattern (API node order; its values are not read);
// vals[S][A.nnz()]: the slices on that pattern; transpose: the table of A^T (the exact transpose of every slice); perm / iperm:
// the internal node order, or null for the caller's.  Every slice goes through transpose_csr / permute_csr on its own; `pat`
// receives the structure of slice 0, and a slice whose structure differs from it is refused (it cannot: the structure follows
// from the pattern alone).
inline bool build_table(const HostCsr& A, const float* vals, int S, bool transpose, const std::vector<int>* perm,
                        const std::vector<int>* iperm, HostCsr& pat, std::vector<float>& table) {
    const int nnz = A.nnz();
    table.assign(table_size(S, nnz), 0.0f);
    HostCsr cur = A, tmp;
    for (int s = 0; s < S; ++s) {
        cur.rowptr = A.rowptr;
        cur.col = A.col;
        cur.val.assign(vals + (size_t)s * nnz, vals + (size_t)(s + 1) * nnz);
        if (transpose) { transpose_csr(cur, tmp); std::swap(cur, tmp); }
        if (perm) { permute_csr(cur, *perm, *iperm, tmp); std::swap(cur, tmp); }
        if (s == 0) pat = cur;
        else if (cur.rowptr != pat.rowptr || cur.col != pat.col) return false;
        for (int e = 0; e < nnz; ++e) table[(size_t)s * nnz + e] = cur.val[e];
    }
    return true;
}

}  // namespace tv
