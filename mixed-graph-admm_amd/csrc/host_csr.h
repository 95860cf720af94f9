// Host-side CSR container (plain C++: also used by the CPU-only checks of the tile builders).
#pragma once
#include <vector>

struct HostCsr {
    int n = 0;
    std::vector<int> rowptr, col;
    std::vector<float> val;
    int nnz() const { return (int)col.size(); }
};

// At = A^T.  Rows are visited in increasing order, so the entries of every transposed row are sorted by source row: a fixed
// summation order, results are bitwise repeatable (no atomics anywhere).
inline void transpose_csr(const HostCsr& A, HostCsr& At) {
    const int n = A.n, nnz = A.nnz();
    At.n = n;
    At.rowptr.assign(n + 1, 0);
    At.col.resize(nnz);
    At.val.resize(nnz);
    for (int e = 0; e < nnz; ++e) At.rowptr[A.col[e] + 1]++;
    for (int i = 0; i < n; ++i) At.rowptr[i + 1] += At.rowptr[i];
    std::vector<int> fill(At.rowptr.begin(), At.rowptr.end() - 1);
    for (int i = 0; i < n; ++i)
        for (int e = A.rowptr[i]; e < A.rowptr[i + 1]; ++e) {
            const int d = fill[A.col[e]]++;
            At.col[d] = i;
            At.val[d] = A.val[e];
        }
}

// Row i of `out` is row perm[i] of A with its columns renamed by iperm (iperm[perm[i]] = i): A in the internal node order
// `perm`.  The entries of a row keep their order.
inline void permute_csr(const HostCsr& A, const std::vector<int>& perm, const std::vector<int>& iperm, HostCsr& out) {
    const int n = A.n;
    out.n = n;
    out.rowptr.assign(n + 1, 0);
    out.col.clear();
    out.val.clear();
    out.col.reserve(A.nnz());
    out.val.reserve(A.nnz());
    for (int i = 0; i < n; ++i) {
        const int src = perm[i];
        for (int e = A.rowptr[src]; e < A.rowptr[src + 1]; ++e) {
            out.col.push_back(iperm[A.col[e]]);
            out.val.push_back(A.val[e]);
        }
        out.rowptr[i + 1] = (int)out.col.size();
    }
}
