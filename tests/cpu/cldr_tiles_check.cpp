// CPU check of the fused cLdr tile metadata (mixed-graph-admm_amd/csrc/cldr_tiles.h): replays the dataflow of the HIP
// kernel k_cldr on the host -- per tile an image P of x_t on the 2-hop set C2 and an image Q of q_{t+1} = (Ldr x)_{t+1}
// on the 1-hop set C1, swept over the time steps -- and compares the result with Ldr^T(Ldr x) evaluated directly from
// the CSR matrices with the operator definitions of reference ADMM.py:150-228.  Test infrastructure (g++ only).
//   usage: cldr_tiles_check <n> <T> <Rcap> <C1cap> <C2cap> <GD> <GT> <cluster> [k] [hubs] [hub_indeg] [stride] [row_limit]
//          cldr_tiles_check <n> <T> g<geometry> <GD> <GT> <cluster> [k] [hubs] [hub_indeg] [stride] [row_limit]
//     g1 ... g4: the caps of the engine's tile geometry of that number (CLDR_GEOMS in cldr_tiles.h)
//     k (4): neighbours per W_d row beside the node itself;  hubs x hub_indeg: that many nodes are listed by hub_indeg rows
//     each (rows hub + stride, hub + 2 stride, ...; stride 0: rows hub + 1, hub + 2, ... whose other entries are rows of that
//     set as well -- a star, the hub's 2-hop set stays small): W_d^T rows of about hub_indeg entries;  row_limit: as MGADMM_CLDR_ROWS
//          cldr_tiles_check @<file> ...: W_d is read from the file (n, then per row its length and (column, weight) pairs) and
//     <n>, [k] and the hub arguments are ignored: the census graphs of tests/stream_census.py
//   The first output line states the longest W_d and W_d^T row; INELIGIBLE when the builder refuses the graph.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>

#include "cldr_tiles.h"

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

int main(int argc, char** argv) {
    if (argc < 7) return 2;
    HostCsr Wd;
    if (argv[1][0] == '@') {
        FILE* f = fopen(argv[1] + 1, "r");
        if (!f || fscanf(f, "%d", &Wd.n) != 1) return 2;
        Wd.rowptr.push_back(0);
        for (int i = 0; i < Wd.n; ++i) {
            int len = 0;
            if (fscanf(f, "%d", &len) != 1) return 2;
            for (int e = 0; e < len; ++e) {
                int c; float w;
                if (fscanf(f, "%d %f", &c, &w) != 2 || c < 0 || c >= Wd.n) return 2;
                Wd.col.push_back(c);
                Wd.val.push_back(w);
            }
            Wd.rowptr.push_back((int)Wd.col.size());
        }
        fclose(f);
    }
    const bool from_file = Wd.n > 0;
    const int n = from_file ? Wd.n : atoi(argv[1]), T = atoi(argv[2]);
    CldrCaps caps{};
    int a = 3;
    if (argv[3][0] == 'g') {
        const int geom = atoi(argv[3] + 1);
        if (geom < 1 || geom > 4) return 2;
        caps = cldr_caps_of(geom, atoi(argv[4]), atoi(argv[5]));
        a = 6;
    } else {
        if (argc < 9) return 2;
        caps = CldrCaps{atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7])};
        a = 8;
    }
    auto opt = [&](int i, int dflt) { return a + i < argc ? atoi(argv[a + i]) : dflt; };
    const int cluster = atoi(argv[a]);
    const int k = opt(1, 4), hubs = opt(2, 0), hub_indeg = opt(3, 0), stride = opt(4, 1), row_limit = opt(5, 0);
    std::mt19937 rng(7);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    if (!from_file) {
        // points on a jittered grid walked in boustrophedon strips: consecutive rows are spatial neighbours
        const int side = (int)std::ceil(std::sqrt((double)n));
        std::vector<double> px(n), py(n);
        for (int i = 0; i < n; ++i) {
            const int strip = (i / side) / 8, in = i - strip * 8 * side, cx = in / 8, cy = in % 8;
            px[i] = cx + 0.8 * U(rng);
            py[i] = strip * 8 + ((cx & 1) ? 7 - cy : cy) + 0.8 * U(rng);
        }
        Wd.n = n;
        Wd.rowptr.push_back(0);
        for (int i = 0; i < n; ++i) {
            std::vector<std::pair<double, int>> d;
            for (int j = 0; j < n; ++j) {
                const double dx = px[i] - px[j], dy = py[i] - py[j];
                if (dx * dx + dy * dy < 36.0) d.push_back({dx * dx + dy * dy, j});
            }
            std::sort(d.begin(), d.end());
            int take = std::min<int>(k + 1, (int)d.size());
            if (i % 97 == 0) take = std::min(take, 2);          // ragged rows
            // a row that lists a hub: its last entry is replaced by the hub (if the hub is not among its entries already)
            for (int h = 0; h < hubs; ++h) {
                const int hub = (int)((long)h * n / hubs), off = i - hub;
                if (stride == 0 && off > 0 && off <= hub_indeg) {
                    // star: the row lists itself, the hub and the leaves nearest to it by index (the 2-hop set of the hub stays small)
                    std::vector<std::pair<double, int>> star{d[0], {1.0, hub}};
                    for (int s = 1; (int)star.size() < take && s <= hub_indeg; ++s)
                        for (int j : {i - s, i + s})
                            if (j > hub && j <= hub + hub_indeg && (int)star.size() < take) star.push_back({1.0 + s, j});
                    take = (int)star.size();
                    d = star;
                } else if (stride > 0 && off > 0 && off % stride == 0 && off / stride <= hub_indeg && take >= 2) {
                    bool there = false;
                    for (int u = 0; u < take; ++u) there |= d[u].second == hub;
                    if (!there) d[take - 1].second = hub;
                }
            }
            double s = 0;
            for (int u = 0; u < take; ++u) s += std::exp(-std::sqrt(d[u].first) / 3.0);
            for (int u = 0; u < take; ++u) {
                Wd.col.push_back(d[u].second);
                Wd.val.push_back((float)(std::exp(-std::sqrt(d[u].first) / 3.0) / s));
            }
            Wd.rowptr.push_back((int)Wd.col.size());
        }
    }
    HostCsr WdT = transpose(Wd);
    std::vector<int> cuts;
    for (int c = 0; c < n; c += cluster) cuts.push_back(c);
    int max_d = 0, max_t = 0, rows_d_max = 0;
    for (int i = 0; i < n; ++i) {
        max_d = std::max(max_d, Wd.rowptr[i + 1] - Wd.rowptr[i]);
        max_t = std::max(max_t, WdT.rowptr[i + 1] - WdT.rowptr[i]);
    }
    for (int i = 0; i < n; ++i) rows_d_max += Wd.rowptr[i + 1] - Wd.rowptr[i] == max_d;
    printf("rows max_d %d rows_of_max_d %d max_t %d caps %d %d %d\n", max_d, rows_d_max, max_t, caps.Rcap, caps.C1cap, caps.C2cap);
    CldrTiles tl;
    if (!build_cldr_tiles(Wd, WdT, cuts, caps, tl, row_limit)) {
        printf("INELIGIBLE\n");
        return 0;
    }
    int max_tile_rows = 0;
    for (int t = 0; t < tl.NT; ++t) max_tile_rows = std::max(max_tile_rows, tl.n0[t + 1] - tl.n0[t]);
    if (max_tile_rows > (row_limit > 0 ? std::min(row_limit, caps.Rcap) : caps.Rcap)) { printf("FAIL tile rows %d\n", max_tile_rows); return 1; }
    // tiles partition the rows
    if (tl.n0.front() != 0 || tl.n0.back() != n) { printf("FAIL partition\n"); return 1; }
    std::vector<double> x((size_t)T * n), ref((size_t)T * n), got((size_t)T * n, 1e300);
    for (auto& v : x) v = U(rng) - 0.5;
    // direct: q = Ldr x ; y = Ldr^T q   (kNN branch, quirk Q1 irrelevant because q_0 = 0)
    std::vector<double> q((size_t)T * n, 0.0);
    for (int t = 1; t < T; ++t)
        for (int i = 0; i < n; ++i) {
            double s = 0;
            for (int e = Wd.rowptr[i]; e < Wd.rowptr[i + 1]; ++e) s += (double)Wd.val[e] * x[(size_t)(t - 1) * n + Wd.col[e]];
            q[(size_t)t * n + i] = x[(size_t)t * n + i] - s;
        }
    for (int t = 0; t < T; ++t)
        for (int i = 0; i < n; ++i) {
            double s = 0;
            if (t + 1 < T)
                for (int e = WdT.rowptr[i]; e < WdT.rowptr[i + 1]; ++e) s += (double)WdT.val[e] * q[(size_t)(t + 1) * n + WdT.col[e]];
            ref[(size_t)t * n + i] = q[(size_t)t * n + i] - s;
        }
    // kernel dataflow.  cldr_gather reads the first GFIX slots of a row without a test and the others in pairs (u0, u0 + 1)
    // only while the row's entry count is above u0 (GFIX = 6 of the W_d slots; of the W_d^T slots 6, or 4 when GT > 12)
    const CldrCaps& c = tl.caps;
    const int GDF = std::min(c.GD, 6), GTF = c.GT < 6 ? c.GT : (c.GT > 12 ? 4 : 6);
    auto slot_read = [](int u, int gfix, int cnt) { return u < gfix || cnt > gfix + ((u - gfix) & ~1); };
    for (int tile = 0; tile < tl.NT; ++tile) {
        const int n0 = tl.n0[tile], R = tl.n0[tile + 1] - n0, c1 = tl.nC1[tile], c2 = tl.nC2[tile];
        const int* rows = &tl.rows[(size_t)tile * c.C2cap];
        for (int l = 0; l < R; ++l)
            if (rows[l] != n0 + l) { printf("FAIL own rows\n"); return 1; }
        std::vector<double> P(c.C2cap, 0.0), Q(c.C1cap, 0.0), pnext(c.C2cap), pcur(c.Rcap), qprev(c.Rcap, 0.0), qnew(c.C1cap);
        for (int l = 0; l < c2; ++l) P[l] = x[rows[l]];
        for (int l = 0; l < R; ++l) pcur[l] = P[l];
        for (int t = 0; t < T; ++t) {
            const bool nxt = t + 1 < T;
            if (nxt) {
                for (int l = 0; l < c2; ++l) pnext[l] = x[(size_t)(t + 1) * n + rows[l]];
                for (int j = 0; j < c1; ++j) {                               // phase A: q_{t+1} on C1
                    double s = 0;
                    for (int u = 0; u < c.GD; ++u) {
                        const size_t o = ((size_t)tile * c.C1cap + j) * c.GD + u;
                        if (tl.dcol[o] < 0 || tl.dcol[o] >= c2) { printf("FAIL dcol range\n"); return 1; }
                        if (!slot_read(u, GDF, tl.dcnt[(size_t)tile * c.C1cap + j])) continue;
                        s += (double)tl.dw[o] * P[tl.dcol[o]];
                    }
                    qnew[j] = pnext[j] - s;
                    Q[j] = qnew[j];
                }
            }
            for (int i = 0; i < R; ++i) {                                   // phase C: y_t on the own rows
                double s = 0;
                if (nxt)
                    for (int u = 0; u < c.GT; ++u) {
                        const size_t o = ((size_t)tile * c.Rcap + i) * c.GT + u;
                        if (tl.tcol[o] < 0 || tl.tcol[o] >= c1) { printf("FAIL tcol range\n"); return 1; }
                        if (!slot_read(u, GTF, tl.tcnt[(size_t)tile * c.Rcap + i])) continue;
                        s += (double)tl.tw[o] * Q[tl.tcol[o]];
                    }
                got[(size_t)t * n + n0 + i] = qprev[i] - s;
            }
            if (nxt) {
                for (int l = 0; l < c2; ++l) P[l] = pnext[l];
                for (int i = 0; i < R; ++i) { qprev[i] = qnew[i]; pcur[i] = pnext[i]; }
            }
        }
    }
    double err = 0, nrm = 0;
    for (size_t i = 0; i < ref.size(); ++i) { err = std::max(err, std::fabs(ref[i] - got[i])); nrm = std::max(nrm, std::fabs(ref[i])); }
    printf("tiles %d maxR %d meanR %.1f C1 %.1f C2 %.1f  max err %.3e (max |ref| %.3f)\n", tl.NT, max_tile_rows, (double)n / tl.NT, (double)tl.sumC1 / tl.NT,
           (double)tl.sumC2 / tl.NT, err, nrm);
    if (!(err < 1e-12)) { printf("FAIL\n"); return 1; }
    printf("OK\n");
    return 0;
}
