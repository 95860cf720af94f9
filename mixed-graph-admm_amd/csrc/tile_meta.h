// Host-side table builder of the LDS-tiled row kernel (k_tile in stream_kernels.h).  Plain C++, no HIP: the same code is
// compiled into libmgadmm.so (Engine::tile_meta uploads the tables) and into the CPU check tests/cpu/tile_meta_check.cpp,
// which replays the kernel's dataflow on the host from these tables and compares it with the CSR product.
//
// Per (matrix, tile size R, slot count GW):
//   tl_col/tl_w [N][GW]      : the row's first GW "local" neighbours and weights.  Local index 0..R-1 = row of the own tile,
//                              R..R+H-1 = position in the tile's halo list; unused slots point at the row itself with weight 0
//   halo [NTILE][TILE_HMAX]  : global row indices of the tile's halo rows in order of first use, -1 = unused.  The list is a
//                              PREFIX (no -1 before a used slot): k_tile loads the slots wave, wave + 4 of a wave always and
//                              wave + 8, + 12, + 16 only when slot wave + 8 is in use
//   h_rowptr/h_col/h_val     : CSR of everything that did not fit (more than GW neighbours, more than TILE_HMAX halo rows):
//                              gathered from global memory, normally empty.  h_col / h_val carry TILE_META_PAD entries of
//                              padding (column 0, weight 0) past h_rowptr[N]
#pragma once
#include <algorithm>
#include <vector>

#include "host_csr.h"

constexpr int TILE_HMAX = 20;      // halo rows (out-of-tile neighbours) staged in LDS per tile and step
constexpr int TILE_META_PAD = 8;   // entries of padding behind the overflow CSR

struct TileMetaHost {
    int N = 0, R = 0, GW = 0, ntile = 0;
    std::vector<int> tl_col, halo, h_rowptr, h_col;
    std::vector<float> tl_w, h_val;
    int overflow() const { return h_rowptr.empty() ? 0 : h_rowptr.back(); }      // entries of the overflow CSR (without the padding)
};

// A: the matrix in the internal node order.
inline void build_tile_meta(const HostCsr& A, int N, int R, int TILE_GW, TileMetaHost& out) {
    const int ntile = (N + R - 1) / R;
    out = TileMetaHost();
    out.N = N; out.R = R; out.GW = TILE_GW; out.ntile = ntile;
    std::vector<int>&tc = out.tl_col, &hr = out.h_rowptr, &hcol = out.h_col, &halo = out.halo;
    std::vector<float>&tw = out.tl_w, &hval = out.h_val;
    tc.assign((size_t)N * TILE_GW, 0);
    hr.assign(N + 1, 0);
    halo.assign((size_t)ntile * TILE_HMAX, -1);
    tw.assign((size_t)N * TILE_GW, 0.f);
    for (int tl = 0; tl < ntile; ++tl) {
        const int lo = tl * R, hi = std::min(N, lo + R);
        // halo list of the tile: out-of-tile columns in order of first use, at most TILE_HMAX
        std::vector<int> hl;
        auto halo_pos = [&](int c) -> int {
            for (size_t k = 0; k < hl.size(); ++k)
                if (hl[k] == c) return (int)k;
            if ((int)hl.size() < TILE_HMAX) { hl.push_back(c); return (int)hl.size() - 1; }
            return -1;
        };
        for (int i = lo; i < hi; ++i) {
            int used = 0;
            for (int e = A.rowptr[i]; e < A.rowptr[i + 1]; ++e) {
                const int c = A.col[e];
                int local = -1;
                if (used < TILE_GW) {
                    if (c >= lo && c < hi) local = c - lo;
                    else {
                        const int hp = halo_pos(c);
                        if (hp >= 0) local = R + hp;
                    }
                }
                if (local >= 0) {
                    tc[(size_t)i * TILE_GW + used] = local;
                    tw[(size_t)i * TILE_GW + used] = A.val[e];
                    ++used;
                } else {
                    hcol.push_back(c);
                    hval.push_back(A.val[e]);
                }
            }
            for (; used < TILE_GW; ++used) tc[(size_t)i * TILE_GW + used] = i - lo;
            hr[i + 1] = (int)hcol.size();
        }
        for (size_t k = 0; k < hl.size(); ++k) halo[(size_t)tl * TILE_HMAX + k] = hl[k];
    }
    const size_t nh = hcol.size() + TILE_META_PAD;
    hcol.resize(nh, 0);
    hval.resize(nh, 0.f);
}
