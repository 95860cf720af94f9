// CPU check of the LDS-tiled row kernel's tables (mixed-graph-admm_amd/csrc/tile_meta.h): replays the dataflow of the HIP
// kernel k_tile on the host -- per tile an LDS image of the own rows, then of the halo rows the kernel loads (slots wave and
// wave + 4 of every wave always; wave + 8, + 12, + 16 only when slot wave + 8 is in use: everything else is poisoned with
// NaN here), the first TILE_GW local slots of a row read from the image, the overflow CSR read from the global vector --
// and compares selfc x - sum w x with the CSR product.  It also asserts the invariants k_tile relies on (see the FAIL
// messages).  Test infrastructure (g++ only).
//   usage: tile_meta_check <n> <k> <R> <GW> <kind> <perm> <hub_indeg> <transpose>
//     kind 0: k nearest neighbours (and the node itself) on a jittered grid walked in strips; 1: k + 1 random columns per row
//     perm 1: the tables are built for the graph in another node order (shuffled clusters of 16 nodes, every second one
//             reversed), permuted by the library's permute_csr as the engine does for a cluster-ordered graph
//     hub_indeg > 0: that many rows list node 0; transpose 1: the tables are built for the transposed matrix (ragged rows)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <numeric>
#include <random>

#include "tile_meta.h"

static HostCsr transpose(const HostCsr& A) {
    HostCsr At;
    At.n = A.n;
    At.rowptr.assign(A.n + 1, 0);
    At.col.resize(A.nnz());
    At.val.resize(A.nnz());
    for (int e = 0; e < A.nnz(); ++e) At.rowptr[A.col[e] + 1]++;
    for (int i = 0; i < A.n; ++i) At.rowptr[i + 1] += At.rowptr[i];
    std::vector<int> fill(At.rowptr.begin(), At.rowptr.end() - 1);
    for (int i = 0; i < A.n; ++i)
        for (int e = A.rowptr[i]; e < A.rowptr[i + 1]; ++e) {
            int d = fill[A.col[e]]++;
            At.col[d] = i;
            At.val[d] = A.val[e];
        }
    return At;
}

#define FAIL(...) do { printf("FAIL " __VA_ARGS__); printf("\n"); return 1; } while (0)

int main(int argc, char** argv) {
    if (argc < 9) return 2;
    const int n = atoi(argv[1]), k = atoi(argv[2]), R = atoi(argv[3]), GW = atoi(argv[4]), kind = atoi(argv[5]), perm_on = atoi(argv[6]),
              hub = atoi(argv[7]), tr = atoi(argv[8]);
    std::mt19937 rng(11);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const int side = std::max(1, (int)std::ceil(std::sqrt((double)n)));
    std::vector<double> px(n), py(n);
    for (int i = 0; i < n; ++i) {
        const int strip = (i / side) / 8, in = i - strip * 8 * side, cx = in / 8, cy = in % 8;
        px[i] = cx + 0.8 * U(rng);
        py[i] = strip * 8 + ((cx & 1) ? 7 - cy : cy) + 0.8 * U(rng);
    }
    HostCsr W;
    W.n = n;
    W.rowptr.push_back(0);
    for (int i = 0; i < n; ++i) {
        std::vector<int> cols;
        if (kind == 0) {
            std::vector<std::pair<double, int>> d;
            for (int j = 0; j < n; ++j) {
                const double dx = px[i] - px[j], dy = py[i] - py[j];
                d.push_back({dx * dx + dy * dy, j});
            }
            std::sort(d.begin(), d.end());
            int take = std::min<int>(k + 1, (int)d.size());
            if (i % 13 == 5) take = std::min(take, 2);          // ragged rows
            for (int u = 0; u < take; ++u) cols.push_back(d[u].second);
        } else {
            while ((int)cols.size() < std::min(k + 1, n)) {
                const int c = (int)(U(rng) * n) % n;
                if (std::find(cols.begin(), cols.end(), c) == cols.end()) cols.push_back(c);
            }
        }
        if (hub > 0 && i >= 1 && i <= hub && std::find(cols.begin(), cols.end(), 0) == cols.end()) cols.back() = 0;
        for (int c : cols) {
            W.col.push_back(c);
            W.val.push_back((float)(0.05 + 0.9 * U(rng)));
        }
        W.rowptr.push_back((int)W.col.size());
    }
    HostCsr A = tr ? transpose(W) : W;
    bool differs = false;
    if (perm_on) {
        // a cluster order that is not the order the graph was built in: clusters of 16 consecutive nodes taken in a shuffled
        // sequence, the nodes of every second cluster reversed.  The builder gets the matrix in that internal order from
        // permute_csr, the function the library applies (host_csr.h, through mg_permute_csr)
        const int csize = 16, nc = (n + csize - 1) / csize;
        std::vector<int> order(nc), perm, iperm(n);
        std::iota(order.begin(), order.end(), 0);
        std::shuffle(order.begin(), order.end(), rng);
        for (int c : order) {
            const int lo = c * csize, hi = std::min(n, lo + csize);
            for (int j = lo; j < hi; ++j) perm.push_back((c & 1) ? hi - 1 - (j - lo) : j);
        }
        for (int i = 0; i < n; ++i) iperm[perm[i]] = i;
        HostCsr P;
        permute_csr(A, perm, iperm, P);
        // P[i][iperm[c]] = A[perm[i]][c], entry by entry
        if (P.n != n || P.nnz() != A.nnz()) FAIL("permuted matrix: size");
        for (int i = 0; i < n; ++i) {
            const int src = perm[i], len = A.rowptr[src + 1] - A.rowptr[src];
            if (P.rowptr[i + 1] - P.rowptr[i] != len) FAIL("permuted matrix: length of row %d", i);
            for (int e = 0; e < len; ++e)
                if (P.col[P.rowptr[i] + e] != iperm[A.col[A.rowptr[src] + e]] || P.val[P.rowptr[i] + e] != A.val[A.rowptr[src] + e])
                    FAIL("permuted matrix: row %d entry %d", i, e);
        }
        differs = P.rowptr != A.rowptr || P.col != A.col;
        A = P;
    }
    int maxrow = 0;
    for (int i = 0; i < n; ++i) maxrow = std::max(maxrow, A.rowptr[i + 1] - A.rowptr[i]);

    TileMetaHost tm;
    build_tile_meta(A, n, R, GW, tm);
    const int ntile = (n + R - 1) / R;
    if (tm.ntile != ntile || (int)tm.halo.size() != ntile * TILE_HMAX || (int)tm.tl_col.size() != n * GW || (int)tm.tl_w.size() != n * GW ||
        (int)tm.h_rowptr.size() != n + 1)
        FAIL("table sizes");
    // h_rowptr is monotone from 0 and the padding is present
    if (tm.h_rowptr[0] != 0) FAIL("h_rowptr[0]");
    for (int i = 0; i < n; ++i)
        if (tm.h_rowptr[i + 1] < tm.h_rowptr[i]) FAIL("h_rowptr not monotone at row %d", i);
    const int novf = tm.h_rowptr[n];
    if ((int)tm.h_col.size() != novf + TILE_META_PAD || (int)tm.h_val.size() != novf + TILE_META_PAD) FAIL("overflow padding missing");
    for (int e = novf; e < novf + TILE_META_PAD; ++e)
        if (tm.h_col[e] != 0 || tm.h_val[e] != 0.f) FAIL("overflow padding not zero");

    std::vector<double> x(n);
    for (auto& v : x) v = U(rng) - 0.5;
    const double selfc = 1.0, nan = std::numeric_limits<double>::quiet_NaN();
    double err = 0;
    int halo_max = 0, halo_full = 0, ovf_len = 0, ovf_halo = 0, second_batch_skipped = 0;
    for (int tl = 0; tl < ntile; ++tl) {
        const int lo = tl * R, hi = std::min(n, lo + R);
        const int* hl = &tm.halo[(size_t)tl * TILE_HMAX];
        // the halo list is a prefix of distinct out-of-tile rows
        int nh = 0;
        while (nh < TILE_HMAX && hl[nh] >= 0) ++nh;
        for (int s = nh; s < TILE_HMAX; ++s)
            if (hl[s] != -1) FAIL("tile %d: halo slot %d in use behind an unused one", tl, s);
        for (int s = 0; s < nh; ++s) {
            if (hl[s] >= n || (hl[s] >= lo && hl[s] < hi)) FAIL("tile %d: halo row %d out of range or inside the tile", tl, hl[s]);
            for (int s2 = 0; s2 < s; ++s2)
                if (hl[s2] == hl[s]) FAIL("tile %d: halo row %d listed twice", tl, hl[s]);
        }
        halo_max = std::max(halo_max, nh);
        halo_full += nh == TILE_HMAX;
        // LDS image as k_tile fills it: own rows (rows past a short tile's end are clamped to its last row), halo slots
        std::vector<double> img(R + TILE_HMAX, nan);
        for (int l = 0; l < R; ++l) img[l] = x[std::min(lo + l, hi - 1)];
        for (int wave = 0; wave < 4; ++wave) {
            for (int s = wave; s < wave + 8; s += 4) img[R + s] = x[hl[s] >= 0 ? hl[s] : lo];
            if (hl[wave + 8] >= 0)
                for (int s = wave + 8; s < TILE_HMAX; s += 4) img[R + s] = x[hl[s] >= 0 ? hl[s] : lo];
            else
                ++second_batch_skipped;
        }
        for (int i = lo; i < hi; ++i) {
            const int* tc = &tm.tl_col[(size_t)i * GW];
            const float* tw = &tm.tl_w[(size_t)i * GW];
            // local entries + overflow entries = the CSR row, each entry once, in CSR order
            int u = 0, o = tm.h_rowptr[i];
            for (int e = A.rowptr[i]; e < A.rowptr[i + 1]; ++e) {
                const int c = A.col[e];
                int g = -1;
                if (u < GW) {
                    const int lc = tc[u];
                    if (lc < 0 || lc >= R + nh || (lc < R && lc >= hi - lo)) FAIL("row %d slot %d: local index %d (tile rows %d, halo rows %d)", i, u, lc, hi - lo, nh);
                    g = lc < R ? lo + lc : hl[lc - R];
                }
                if (u < GW && g == c && tw[u] == A.val[e]) ++u;
                else if (o < tm.h_rowptr[i + 1] && tm.h_col[o] == c && tm.h_val[o] == A.val[e]) {
                    ++o;
                    if (u < GW) ++ovf_halo; else ++ovf_len;
                } else
                    FAIL("row %d: entry %d (column %d) is neither the next local slot nor the next overflow entry", i, e - A.rowptr[i], c);
            }
            if (o != tm.h_rowptr[i + 1]) FAIL("row %d: %d overflow entries left over", i, tm.h_rowptr[i + 1] - o);
            for (; u < GW; ++u)
                if (tc[u] != i - lo || tw[u] != 0.f) FAIL("row %d: pad slot %d is (%d, %g), not the row itself with weight 0", i, u, tc[u], (double)tw[u]);
            // the kernel's sum
            double s = 0;
            for (int v = 0; v < GW; ++v) s += (double)tw[v] * img[tc[v]];
            for (int e = tm.h_rowptr[i]; e < tm.h_rowptr[i + 1]; ++e) s += (double)tm.h_val[e] * x[tm.h_col[e]];
            double r = 0;
            for (int e = A.rowptr[i]; e < A.rowptr[i + 1]; ++e) r += (double)A.val[e] * x[A.col[e]];
            const double d = std::fabs((selfc * x[i] - s) - (selfc * x[i] - r));
            if (!(d <= 1e-12)) FAIL("row %d: |tile - CSR| = %g", i, d);
            err = std::max(err, d);
        }
    }
    printf("permuted %d tiles %d last_tile_rows %d max_row %d halo_max %d halo_full %d overflow %d by_length %d by_halo %d skipped_batches %d max_err %.3e\n",
           (int)differs, ntile, n - (ntile - 1) * R, maxrow, halo_max, halo_full, novf, ovf_len, ovf_halo, second_batch_skipped, err);
    printf("OK\n");
    return 0;
}
