// Launch plan of the streaming path (k_rows, k_tile, k_cldr in stream_kernels.h): the launch geometry of a batch, which kernel
// instance an operator application gets, whether Ldr^T Ldr runs fused, and which CG solves fold their vector update into the
// SpMM launch.  Plain C++, no HIP: compiled into libmgadmm.so (Engine<S> in engine.h asks and launches: its template ladders
// switch on the fields of a Choice) and into the CPU check tests/cpu/stream_plan_check.cpp, which tests/test_stream_plan_cpu.py
// runs against the dispatch model of tests/stream_census.py and against records of the rules' earlier form inside the engine.
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <cstdint>
#include <utility>

#include "cldr_tiles.h"
#include "host_csr.h"
#include "stream_geom.h"
#include "stream_keys.h"
#include "tile_meta.h"

namespace streamplan {

// The environment switches of the streaming path (tests / experiments), all read once, when a solver is created
struct Switches {
    int want_blocks = 2048;       // MGADMM_WANT_BLOCKS: workgroups of a k_rows launch, at least 64
    int tile = 1;                 // MGADMM_TILE=0: no LDS-tiled spatial kernel on cluster-ordered graphs (reorder = 2)
    int fused = 1;                // MGADMM_FUSED=0 keeps the two-pass cLdr (tests compare the two)
    int fold = 1;                 // MGADMM_FOLD=0: p = r + beta p and x += alpha p stay in their own kernel (EpiPUpdate)
    int fold_lu = 1;              // MGADMM_FOLD_LU=0: the same for the Lu kernel of the zu solve only
    int sweep_rev = 1;            // MGADMM_SWEEP_REV=0: r -= alpha Ap sweeps the time slices upwards like every other kernel
    int cldr_tile_major = 1;      // MGADMM_CLDR_ORDER=0: chunks of a tile adjacent in dispatch order
    int tile_r = 8;               // MGADMM_TILE_R: node rows per tile of k_tile, 8 or 20 (make_tile_geom)
    int cldr_geom = 0;            // MGADMM_CLDR_GEOM: geometry of k_cldr, 1 .. 4 (3 and 4: float only); 0: the scalar type's default
    int cldr_rows = 0;            // MGADMM_CLDR_ROWS: rows-per-tile limit of the k_cldr tile builder (0: the geometry's cap)
    bool tile_stats = false;      // MGADMM_TILE_STATS is set: print how the tile tables fit the graph

    // get(name): the switch's text or nullptr; elem: bytes of the scalar type
    template <class Get>
    static Switches from_strings(Get get, int elem) {
        Switches s;
        if (const char* e = get("MGADMM_WANT_BLOCKS")) s.want_blocks = std::max(64, atoi(e));
        if (const char* e = get("MGADMM_TILE")) s.tile = atoi(e);
        if (const char* e = get("MGADMM_FUSED")) s.fused = atoi(e);
        if (const char* e = get("MGADMM_FOLD")) s.fold = atoi(e);
        if (const char* e = get("MGADMM_FOLD_LU")) s.fold_lu = atoi(e);
        if (const char* e = get("MGADMM_SWEEP_REV")) s.sweep_rev = atoi(e);
        if (const char* e = get("MGADMM_CLDR_ORDER")) s.cldr_tile_major = atoi(e);
        if (const char* e = get("MGADMM_TILE_R")) { const int rr = atoi(e); if (rr == 8 || rr == 20) s.tile_r = rr; }
        if (const char* e = get("MGADMM_CLDR_GEOM")) { const int v = atoi(e); if (v >= 1 && v <= 4 && (v <= 2 || elem == 4)) s.cldr_geom = v; }
        if (const char* e = get("MGADMM_CLDR_ROWS")) s.cldr_rows = atoi(e);
        s.tile_stats = get("MGADMM_TILE_STATS") != nullptr;
        return s;
    }
    static Switches from_env(int elem) {
        return from_strings([](const char* name) -> const char* { return getenv(name); }, elem);
    }
};

// What the rules read of the graph and the scalar type
struct Facts {
    int elem = 4;                 // bytes of the scalar type: 4 or 8
    int T = 0, N = 0;
    bool spatial = true;          // MGADMM_TEMPORAL_SPATIAL (kNN / physical); false: the band (line-graph) mode
    int reorder = 0;              // 2: cluster order
    int q1 = 0;
    int max_u = 0, max_d = 0, max_dt = 0;   // the longest row of W_u, W_d, W_d^T
    int avg_dt = 0;               // ceil(mean row length) of W_d^T
    bool time_varying = false;    // per-slice weights (mgadmm_graph_set_time_weights): the plain row kernels only, see tiled()
};

// The matrix of an operator application.  W_U .. W_DT in the order of the engine's tile tables
enum Mat { M_NONE, M_BAND, M_WU, M_WD, M_WDT };

// One kernel instance up to its epilogue and source: STREAM_K_ROWS (GW), STREAM_K_TILE (GW = TILE_GW, MR) or STREAM_K_CLDR (VEC =
// VECT; geom, GD, GT)
struct Choice {
    int kernel = STREAM_K_ROWS;
    int mat = M_NONE;
    int VEC = 1;
    int GW = 4;                   // k_rows: gather window, 4 or 6; k_tile: neighbour slots per row kept in VGPR lanes, 4 / 6 / 8
    int MR = 0;                   // k_tile: rows per wave, 2 (8-row tiles) or 5 (20-row tiles)
    int geom = 0, GD = 0, GT = 0; // k_cldr: index into CLDR_GEOMS, W_d / W_d^T slots per row
};

// MINW of a k_cldr geometry (waves per SIMD the kernel is compiled for).  Geometry 2 in float64 (104 KiB of LDS: one workgroup
// per CU) takes 2; float: 4 = 128 VGPRs (6 waves per SIMD = 80 VGPRs spilled 87-100 of them in the folded form)
constexpr int cldr_minw(int geom, int elem) { return geom == 2 && elem == 8 ? 2 : 4; }

// LDS a workgroup of k_cldr may take: the kernels' dynamic limit is raised to it, and a geometry above it gives way to geometry 2
constexpr int CLDR_LDS_LIMIT = 150 * 1024;

// Slots per row of the k_cldr tables for W_d (A) and W_d^T (At), both in the internal node order -> (gd, gt).
// W_d^T: 12, or 16 / 24 when a row is longer (round 3: the PEMS-like graphs of 600 ... 2000 nodes have rows of 13 and 14 entries
// and fell back to the two-pass path; the 16-slot instance is 5 % slower on graphs that do not need it).  W_d: 6 (no test at
// all) when no row is longer, else 8.  A longer row than 8 / 24: build_cldr_tiles refuses the graph
inline std::pair<int, int> cldr_slots(const HostCsr& A, const HostCsr& At) {
    int gd = 6, gt = 12;
    for (int i = 0; i < A.n; ++i) {
        if (A.rowptr[i + 1] - A.rowptr[i] > 6) gd = 8;
        const int tl = At.rowptr[i + 1] - At.rowptr[i];
        if (tl > 12) gt = std::max(gt, tl > 16 ? 24 : 16);
    }
    return {gd, gt};
}

struct Planner {
    Facts f;
    Switches sw;
    int geom = 2;                 // k_cldr geometry in force (index into CLDR_GEOMS)

    Planner() {}
    // The geometry of k_cldr: geometry 1 for float (measured on cfg3, N = 10 000, B = 512, SpMM + LHS launch / with the folded
    // vector update: geometry 1 380 us / 644 us, geometry 2 700 us / -; a 16 / 32 / 48-row geometry 0 of 80 KiB ran 365 us /
    // 711 us and spilled 52 VGPRs in the folded form: removed in round 3), the narrow geometry 2 for float64 (104 KiB); then
    // the switch; then geometry 2 when the images of the chosen one do not fit
    Planner(const Facts& facts, const Switches& switches) : f(facts), sw(switches) {
        geom = f.elem == 4 ? 1 : 2;
        if (sw.cldr_geom) geom = sw.cldr_geom;
        if (cldr_lds_bytes(dims().VECT) > (size_t)CLDR_LDS_LIMIT) geom = 2;
    }
    const CldrGeomDims& dims() const { return CLDR_GEOMS[geom]; }
    size_t cldr_lds_bytes(int vect) const { return (size_t)dims().NW * (dims().MQ + dims().MP) * 64 * vect * f.elem; }

    // ---------------------------------------------------------------- geometry
    Geom make_geom(int B) const {
        Geom q;
        q.T = f.T; q.N = f.N; q.B = B;
        int vecw;
        if (f.elem == 4) vecw = B >= 192 ? 4 : (B >= 96 ? 2 : 1);
        else vecw = B >= 96 ? 2 : 1;
        const int cw = 64 * vecw;
        q.VEC = vecw;
        q.Bp = (B + cw - 1) / cw * cw;
        q.CH = q.Bp / cw;
        // persistent-sized grid: ~want_blocks workgroups in total, a multiple of 8 per column chunk
        int g8 = sw.want_blocks / (8 * q.CH);
        if (g8 < 1) g8 = 1;
        q.G8 = g8;
        q.P = 8 * g8;
        // rows per work item: 16 (4 per wave) unless the problem is too small to give every workgroup two items
        long rows = (long)f.T * f.N;
        int ri = 16;
        while (ri > 4 && rows / ri < 2L * q.P) ri -= 4;
        q.RI = ri;
        const int per_xcd = (f.N + 7) / 8;
        q.NBL = (per_xcd + ri - 1) / ri;
        q.NX = q.NBL * ri;
        q.n_items = f.T * q.NBL;
        q.grid = q.P * q.CH;
        q.rev = 0;
        return q;
    }

    // the LDS-tiled spatial kernel: cluster-ordered kNN / physical graphs.  Not with time-varying weights: the tile tables of
    // k_tile and k_cldr hold one slice, so such a graph gets the plan MGADMM_TILE=0 gives it (row kernels, two-pass Ldr^T Ldr,
    // separate EpiPUpdate: cldr_wanted, fold1 and fold2 all follow from this)
    bool tiled() const { return sw.tile && f.reorder >= 2 && f.spatial && !f.time_varying; }
    int tile_rows() const { return tiled() ? sw.tile_r : 0; }      // (MGADMM_Q_TILE_ROWS)
    // geometry of the LDS-tiled spatial kernel for the same column layout as `q`
    bool make_tile_geom(const Geom& q, TileGeom& tg) const {
        if (!tiled()) return false;
        tg.T = f.T; tg.N = f.N; tg.B = q.B; tg.Bp = q.Bp; tg.VEC = q.VEC; tg.CH = q.CH;
        // tile size: 8 rows (2 per wave).  With the rows per wave a template constant the register footprint
        // follows the tile size (EpiLhs: 100 VGPRs at 2 rows, 148 at 5), and the kernel is latency-bound, so
        // more resident workgroups win: SpMM inside CG on the 10k-node graph 4.30 TB/s at 20 rows, 4.60 at 12,
        // 4.72 at 8, 4.71 at 4 (more halo reads); the 100k-node graph is flat (4.86 -> 4.91).  MGADMM_TILE_R=20
        // selects the large tile for experiments.
        const int best = sw.tile_r;
        tg.R = best;
        tg.NTILE = (f.N + best - 1) / best;
        tg.TPX = (tg.NTILE + 7) / 8;
        tg.P = 8 * tg.TPX;
        tg.grid = tg.P * q.CH;
        const size_t row_bytes = (size_t)64 * q.VEC * f.elem;
        tg.lds_bytes = (int)std::max(row_bytes * (best + TILE_HMAX), (size_t)3 * q.VEC * 64 * f.elem);
        return true;
    }

    // geometry of k_cldr over tile tables of NT tiles
    CldrGeom make_cldr_geom(const Geom& q, int NT) const {
        int vect = dims().VECT;
        CldrGeom cg;
        cg.T = f.T; cg.N = f.N; cg.B = q.B; cg.Bp = q.Bp;
        while (q.Bp % (64 * vect)) vect /= 2;              // never happens: Bp is padded to the solver's own vector width
        cg.CH = q.Bp / (64 * vect);
        cg.NT = NT;
        cg.TPX = (cg.NT + 7) / 8;
        cg.P = 8 * cg.TPX;
        cg.grid = cg.P * cg.CH;
        cg.tile_major = sw.cldr_tile_major;
        cg.q1 = f.q1;
        cg.lds_bytes = (int)cldr_lds_bytes(vect);
        return cg;
    }
    // the fused kernel needs Bp to be a multiple of its own chunk width (float64: chunks of at most 128 columns)
    bool cldr_width_fits(const Geom& q) const { return q.Bp % (64 * dims().VECT) == 0 && (f.elem == 4 || dims().VECT <= 2); }

    // ---------------------------------------------------------------- Ldr^T Ldr: one k_cldr launch or two passes
    bool cldr_wanted() const { return sw.fused && tiled(); }      // the engine builds the tile tables at the first application
    // NT: tiles of the tables; 0: none (not built, or the graph does not fit the slot counts: hub rows)
    bool fused(const Geom& q, int NT) const { return cldr_wanted() && NT > 0 && cldr_width_fits(q); }
    Choice cldr_choice(int gd, int gt) const {
        Choice c;
        c.kernel = STREAM_K_CLDR; c.mat = M_WD; c.VEC = dims().VECT; c.GW = 0; c.geom = geom; c.GD = gd; c.GT = gt;
        return c;
    }

    // ---------------------------------------------------------------- one operator application
    // k_tile where the tile geometry exists, for a spatial operator without a per-row self factor (Ln keeps k_rows); else k_rows
    Choice choose(Mat m, bool self_w, const Geom& q) const {
        Choice c;
        c.mat = m; c.VEC = q.VEC;
        const bool spatial_op = m == M_WU || m == M_WD || m == M_WDT;
        if (spatial_op && !self_w && tiled()) {
            // neighbour slots kept in VGPR lanes: 4 for W_u (k = 4), 6 for W_d, 8 for the ragged W_d^T rows
            const int max_row = m == M_WU ? f.max_u : (m == M_WD ? f.max_d : f.max_dt);
            c.kernel = STREAM_K_TILE;
            c.GW = max_row <= 4 ? 4 : (m == M_WDT || max_row > 6 ? 8 : 6);
            c.MR = sw.tile_r == 20 ? 5 : 2;
            return c;
        }
        // gather window of the row kernel: 4 in-flight neighbour rows for the k=4 spatial Laplacian, 6 otherwise
        const int mr = !spatial_op ? 0 : (m == M_WU ? f.max_u : (m == M_WD ? f.max_d : f.avg_dt));
        c.GW = mr <= 4 ? 4 : 6;
        return c;
    }

    // ---------------------------------------------------------------- CG: the vector update folded into the SpMM launch
    // Lu with the CG vector update folded into its loads (k_tile with TileSrcFold): zu solve.  Built for the production shape
    // only (k = 4 table: 4 slots per row; 8-row tiles; the solver's widest vector): other shapes keep the separate EpiPUpdate launch
    int lu_fold_vec() const { return f.elem == 4 ? 4 : 2; }
    bool lu_fold_fits(const Geom& q) const {
        return sw.fold && sw.fold_lu && tiled() && q.VEC == lu_fold_vec() && f.max_u <= 4 && sw.tile_r != 20;
    }
    Choice lu_fold_choice() const {
        Choice c;
        c.kernel = STREAM_K_TILE; c.mat = M_WU; c.VEC = lu_fold_vec(); c.GW = 4; c.MR = 2;
        return c;
    }
    // kind: the left-hand side (LhsDef::kind: 0 diagonal, 1 with Ldr^T Ldr, 2 with Lu).  kind 1 on the fused kernel: the vector
    // update of iteration k (p = r + beta p, x += alpha p) is folded into the SpMM launch of iteration k+1 (k_cldr with
    // CldrSrcFold); kind 2 (zu solve): the same fold in the LDS-tiled Lu kernel
    bool fold1(int kind, const Geom& q, int NT) const { return kind == 1 && sw.fold && fused(q, NT); }
    bool fold2(int kind, const Geom& q) const { return kind == 2 && lu_fold_fits(q); }

    // ---------------------------------------------------------------- instance key (stream_keys.h)
    // epi: the ID of the epilogue functor; fold: TileSrcFold / CldrSrcFold (k_rows has no source argument)
    int64_t key(const Choice& c, int epi, bool fold) const {
        const bool f64 = f.elem == 8;
        if (c.kernel == STREAM_K_ROWS) return stream_key(STREAM_K_ROWS, f64, c.VEC, epi, false, c.GW);
        if (c.kernel == STREAM_K_TILE) return stream_key(STREAM_K_TILE, f64, c.VEC, epi, fold, c.GW, c.MR);
        const CldrGeomDims& d = CLDR_GEOMS[c.geom];
        return stream_key(STREAM_K_CLDR, f64, d.VECT, epi, fold, d.NW, d.MA, d.MQ, d.MP, c.GD, c.GT, cldr_minw(c.geom, f.elem));
    }
};

}  // namespace streamplan
