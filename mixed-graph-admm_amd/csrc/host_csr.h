// Host-side CSR container (plain C++: also used by the CPU-only checks of the tile builders).
#pragma once
#include <vector>

struct HostCsr {
    int n = 0;
    std::vector<int> rowptr, col;
    std::vector<float> val;
    int nnz() const { return (int)col.size(); }
};

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
