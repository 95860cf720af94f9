// Solver engine: host-side orchestration of the ADMM loop of reference ADMM.py:511-648 over the streaming HIP kernels
// (stream_kernels.h) for either scalar type, with what a solver of either type answers about the LDS-resident float32 path
// (the plan record, the host state of the per-sample features, the refusals of solve_gate.h).  That path's driver is LdsEngine
// (lds_engine.h), derived from Engine<float>: solver_f32.hip creates it, solver_f64.hip the plain Engine<double> (separate
// translation units: the library builds in parallel).
#pragma once
#include <math.h>
#include <cmath>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <tuple>
#include <type_traits>

#include "common.h"
#include "cldr_tiles.h"
#include "tile_meta.h"
#include "stream_keys.h"
#include "stream_kernels.h"
#include "stream_tv_kernels.h"
#include "stream_plan.h"
#include "lds_adapt.h"      // ldsadapt::Params, validate: set_adaptive_rho checks its arguments for either scalar type
#include "lds_plan.h"
#include "lds_param_table.h"
#include "solve_gate.h"
#include "band_sets.h"

namespace {

enum VecId {
    V_XA, V_XB, V_ZUA, V_ZUB, V_ZDA, V_ZDB, V_PHIA, V_PHIB, V_GAM, V_GU, V_GD, V_Y, V_MASK,
    V_R, V_P, V_Q, V_AP, V_RHS, V_TMP, V_IO0, V_IO1, V_COUNT
};

constexpr int LAG = 2;          // CG iterations enqueued ahead of the host's convergence check
constexpr int NRED_MAX = 6;
constexpr int PROF_POOL = 32768;
constexpr int NACT_LOG = 1 << 16;   // pinned log of the per-iteration active-sample counts (one int per CG iteration enqueued)

template <typename S>
struct Engine : EngineBase {
    mgadmm_solver* sv;
    mgadmm_graph* g;
    mgadmm_params p;
    int T, N, Bmax, Bp_max;
    hipStream_t st = nullptr;

    // Every block below belongs to its member (DevBuf / PinnedBuf, dev_buf.h), which knows its capacity: no size is kept beside it
    S* vec[V_COUNT] = {nullptr};      // views into vec_pool
    DevBuf<S> vec_pool;
    size_t vec_elems = 0;
    DevBuf<S> partials;
    // CG scalars
    DevBuf<S> d_rr, d_alpha, d_beta, d_alpha_hist, d_beta_hist;
    DevBuf<int> d_active, d_iters_tmp, d_nact, d_nonfinite;
    // history (sized by the iteration limits: alloc_iter_dependent)
    DevBuf<double> d_ps, d_hist, d_dxps, d_dxpart, d_hist_ps;
    DevBuf<int> d_cg_iters;
    // pinned host
    PinnedBuf<int> h_nact;
    PinnedBuf<double> h_row;
    PinnedBuf<int> h_flag;
    Event ev_ring[LAG + 1];
    // R == 0: the tables are not valid (tile_meta sets R and GW after the last upload succeeded)
    struct TileMetaDev { int R = 0; int GW = 0; DevBuf<int> tl_col; DevBuf<float> tl_w; DevBuf<int> halo, h_rowptr, h_col; DevBuf<float> h_val; };
    TileMetaDev tmeta[3];         // W_u, W_d, W_d^T metadata for the tile size in use
    // fused cLdr kernel (k_cldr): tile tables for the geometry in use; state 0 = not built yet, 1 = usable, -1 = the graph
    // does not fit its slot counts (hub rows): the two-pass form stays
    struct CldrDev {
        int state = 0, NT = 0;
        int gd = 8, gt = 12;      // W_d / W_d^T slots per row of the tables (streamplan::cldr_slots)
        DevBuf<int> n0, nC, rows, dcol, dcnt, tcol, tcnt;
        DevBuf<float> dw, tw;
    } cldr_dev;
    streamplan::Planner plan;     // geometry and kernel choice of the streaming path (stream_plan.h); its switches are read in init_workspace
    int cur_P = 0;                // partial rows written by the last row-kernel launch (k_rows or k_tile)
    int64_t ws_bytes = 0;
    // LDS-resident fused path (float32, small graphs): the plan record (none for float64), what the queries report of its last
    // launch, and the host state of the per-sample features solve_gate.h decides on.  The device side: LdsEngine (lds_engine.h)
    ldsplan::LdsPlan lds;
    int lds_chunk = LDS_MAXJ;   // MGADMM_LDS_CHUNK: ADMM iterations per k_admm_lds launch when the iteration count is fixed (1 .. LDS_MAXJ)
    int64_t lds_instance = -1;       // MGADMM_Q_LDS_INSTANCE: template arguments of the k_admm_lds instance of the last launch
    int lds_unit = -1;               // MGADMM_Q_LDS_UNIT: which compilation of the instances it came from (0 / 1 / 2 = k_admm_lds / _ps / _pp)
    solvegate::WeightTables wt;      // the caller's arrays of set_sample_params and set_param_schedule
    bool ad_on = false;              // adaptive penalties (mgadmm_solver_set_adaptive_rho, lds_adapt.h): the parameters
    ldsadapt::Params ad;
    int ad_start = 0;
    int ad_last_periods = 0;         // of the last solve (mgadmm_solver_get_adaptive_history); 0 periods: it did not adapt
    int sg_B = 0;                    // samples of the graph table (mgadmm_solver_set_sample_graphs); 0: none set
    // per-sample temporal band weights (mgadmm_solver_set_sample_bands, band_sets.h): the caller's tables, and for the streaming
    // kernels their expansion to a weight per batch column, [T*skip][bs_Bp] floats for the geometry of a solve of bs.B samples.
    // band_wb: non-null only while a solve with the table runs -- the fine-grained entry points and two_loops read the graph's own table
    bandsets::BandSets bs;
    DevBuf<float> d_bs_exp;
    int bs_Bp = 0;
    const float* band_wb = nullptr;
    StreamKeyLog stream_keys;        // MGADMM_Q_STREAM_KEYS / _KEY0 + i: distinct k_rows / k_tile / k_cldr instances launched (stream_keys.h)
    // profiling
    bool prof_on = false;
    std::vector<Event> prof_ev;
    std::vector<int> prof_tag;
    std::vector<double> prof_lb;   // algorithmic bytes of each timed launch
    std::vector<int> prof_ref;     // h_nact index that tells whether the launch did work (-1: unconditional launch)
    int prof_cur_ref = -1;         // set by cg_internal around the launches of one CG iteration
    int nact_cur = 0;              // next free slot of the h_nact log
    bool nact_locked = false;      // profiling session has used the whole log: later solves use the scratch tail
    int64_t prof_noop = 0;         // timed launches that returned at the converged-CG guard
    size_t prof_used = 0;
    int64_t prof_count[MGADMM_NPROF] = {0};
    double prof_bytes[MGADMM_NPROF] = {0};

    explicit Engine(mgadmm_solver* s) : sv(s), g(s->g), p(s->p), T(s->g->T), N(s->g->N), Bmax(s->Bmax) {}

    ~Engine() override { (void)hipSetDevice(g->device); }      // (in the body: it runs before the members release their blocks)

    // ---------------------------------------------------------------- geometry (the rules: stream_plan.h)
    streamplan::Facts plan_facts() const {
        streamplan::Facts f;
        f.elem = (int)sizeof(S); f.T = T; f.N = N; f.spatial = g->mode == MGADMM_TEMPORAL_SPATIAL; f.reorder = g->reorder; f.q1 = g->q1;
        f.max_u = g->Wu.max_row; f.max_d = g->Wd.max_row; f.max_dt = g->WdT.max_row; f.avg_dt = g->WdT.avg_row_ceil;
        f.time_varying = g->time_varying;
        return f;
    }
    // which matrix a spatial operator applies (the graph hands out its three device tables; transpose_by_gather: Ldr^T reads W_d's)
    streamplan::Mat mat_of(const OpDesc& op) const {
        if (op.kind != OPK_SPATIAL) return op.kind == OPK_BAND ? streamplan::M_BAND : streamplan::M_NONE;
        return op.rowptr == g->Wu.rowptr.get() ? streamplan::M_WU : (op.rowptr == g->Wd.rowptr.get() ? streamplan::M_WD : streamplan::M_WDT);
    }

    // host-side preprocessing of one CSR matrix for tile size R (see TileMeta in stream_kernels.h)
    int tile_meta(int which, int R, int TILE_GW, TileMeta& out) {
        TileMetaDev& d = tmeta[which];
        if (d.R != R || d.GW != TILE_GW) {
            const HostCsr& src = which == 0 ? g->hWu : (which == 1 ? g->hWd : g->hWdT);
            HostCsr A;
            if (g->has_perm) mg_permute_csr(src, g->perm, g->iperm, A);
            else A = src;
            TileMetaHost tm;
            build_tile_meta(A, N, R, TILE_GW, tm);      // (tile_meta.h: plain C++, replayed on the CPU by tests/cpu/tile_meta_check.cpp)
            const int ntile = tm.ntile;
            const std::vector<int>&tc = tm.tl_col, &hr = tm.h_rowptr, &hcol = tm.h_col, &halo = tm.halo;
            const std::vector<float>&tw = tm.tl_w, &hval = tm.h_val;
            if (plan.sw.tile_stats) {           // diagnostics: how well the tile geometry fits the graph
                long hsum = 0; int hfull = 0;
                for (int tl = 0; tl < ntile; ++tl) {
                    int c = 0;
                    for (int k = 0; k < TILE_HMAX; ++k) c += halo[(size_t)tl * TILE_HMAX + k] >= 0;
                    hsum += c; hfull += c == TILE_HMAX;
                }
                fprintf(stderr, "[mgadmm] tile_meta matrix %d: R=%d GW=%d tiles=%d  halo rows/tile mean %.2f (capacity %d, full tiles %d)  "
                                "entries %d, overflow entries %zu (%.2f %%)\n", which, R, TILE_GW, ntile, (double)hsum / ntile, TILE_HMAX,
                        hfull, A.nnz(), (size_t)tm.overflow(), 100.0 * tm.overflow() / std::max(1, A.nnz()));
            }
            MG_HIP(hipStreamSynchronize(st));      // no launch reads the old tables any more
            d.R = d.GW = 0;
            MG_BUF(d.tl_col.upload(tc));
            MG_BUF(d.tl_w.upload(tw));
            MG_BUF(d.halo.upload(halo));
            MG_BUF(d.h_rowptr.upload(hr));
            MG_BUF(d.h_col.upload(hcol));       // (with the padding)
            MG_BUF(d.h_val.upload(hval));
            d.R = R;
            d.GW = TILE_GW;
        }
        out.tl_col = d.tl_col.get(); out.tl_w = d.tl_w.get(); out.halo = d.halo.get(); out.h_rowptr = d.h_rowptr.get(); out.h_col = d.h_col.get(); out.h_val = d.h_val.get();
        return MGADMM_OK;
    }

    // ---------------------------------------------------------------- fused cLdr kernel (k_cldr)
    // Tile geometries (VECT columns per lane, NW waves, rows per wave of the tile / of C1 / of C2).  LDS per workgroup =
    // NW * (MQ + MP) * 64 * VECT * sizeof(S).  Which one is in force: streamplan::Planner (plan.geom), with the measurements.
    template <int VECT_, int NW_, int MA_, int MQ_, int MP_, int MINW_>
    struct ClG { static constexpr int VECT = VECT_, NW = NW_, MA = MA_, MQ = MQ_, MP = MP_, MINW = MINW_; };
    // (the numbers live in cldr_tiles.h, CLDR_GEOMS: the CPU replay of the tile builder reads the same table)
    template <int I, int MINW_>
    using ClGOf = ClG<CLDR_GEOMS[I].VECT, CLDR_GEOMS[I].NW, CLDR_GEOMS[I].MA, CLDR_GEOMS[I].MQ, CLDR_GEOMS[I].MP, MINW_>;
    typedef ClGOf<1, streamplan::cldr_minw(1, sizeof(S))> ClG1;     // 16 / 32 / 40 rows of 256 columns: 72 KiB (float), two workgroups per CU   (default)
    typedef ClGOf<2, streamplan::cldr_minw(2, sizeof(S))> ClG2;    // 64 / 88 / 120 rows of 64 columns: 52 KiB (float) / 104 KiB (double)
    typedef ClGOf<3, streamplan::cldr_minw(3, sizeof(S))> ClG3;    // 32 / 64 / 80 rows of 128 columns: 72 KiB (float): twice the rows per tile, a smaller halo share
    typedef ClGOf<4, streamplan::cldr_minw(4, sizeof(S))> ClG4;    // 32 / 48 / 64 rows of 256 columns, 16 waves: 112 KiB (float), one workgroup per CU
    // tiles of the tables, built and uploaded at the first operator application; 0: no fused kernel for this solver
    int cldr_tiles() {
        if (!plan.cldr_wanted()) return 0;
        if (cldr_dev.state == 0) cldr_prepare();
        return cldr_dev.state == 1 ? cldr_dev.NT : 0;
    }
    void cldr_prepare() {
        cldr_dev.state = -1;
        HostCsr A, At;
        if (g->has_perm) { mg_permute_csr(g->hWd, g->perm, g->iperm, A); mg_permute_csr(g->hWdT, g->perm, g->iperm, At); }
        else { A = g->hWd; At = g->hWdT; }
        std::tie(cldr_dev.gd, cldr_dev.gt) = streamplan::cldr_slots(A, At);
        const CldrCaps caps = cldr_caps_of(plan.geom, cldr_dev.gd, cldr_dev.gt);
        CldrTiles tl;
        if (!build_cldr_tiles(A, At, g->cluster_starts, caps, tl, plan.sw.cldr_rows)) return;
        if (plan.sw.tile_stats)
            fprintf(stderr, "[mgadmm] cldr tiles (geometry %d): %d tiles, rows/tile %.1f, |C1| %.1f, |C2| %.1f (caps %d/%d/%d): reads %.2fx, q recomputed %.2fx\n",
                    plan.geom, tl.NT, (double)N / tl.NT, (double)tl.sumC1 / tl.NT, (double)tl.sumC2 / tl.NT, caps.Rcap, caps.C1cap, caps.C2cap,
                    (double)tl.sumC2 / N, (double)tl.sumC1 / N);
        std::vector<int> nC((size_t)2 * tl.NT);
        for (int t = 0; t < tl.NT; ++t) { nC[2 * t] = tl.nC1[t]; nC[2 * t + 1] = tl.nC2[t]; }
        CldrDev& c = cldr_dev;
        if (c.n0.upload(tl.n0) || c.nC.upload(nC) || c.rows.upload(tl.rows) || c.dcol.upload(tl.dcol) || c.dw.upload(tl.dw) ||
            c.dcnt.upload(tl.dcnt) || c.tcol.upload(tl.tcol) || c.tw.upload(tl.tw) || c.tcnt.upload(tl.tcnt)) {
            (void)hipGetLastError();
            return;
        }
        cldr_dev.NT = tl.NT;
        cldr_dev.state = 1;
    }
    bool cldr_fits(const Geom& q) { return plan.fused(q, cldr_tiles()); }
    template <class G, template <typename, int> class E, template <typename, int> class SRC, class... A>
    int rows_cldr_g(const Geom& q, const SRC<S, G::VECT>& src, const int* live, A... a) {
        const int cl_gd = cldr_dev.gd, cl_gt = cldr_dev.gt;      // (streamplan::cldr_slots)
        if (cl_gt == 12) return cl_gd == 6 ? rows_cldr_gd<G, 6, 12, E, SRC>(q, src, live, a...) : rows_cldr_gd<G, 8, 12, E, SRC>(q, src, live, a...);
        if (cl_gt == 16) return cl_gd == 6 ? rows_cldr_gd<G, 6, 16, E, SRC>(q, src, live, a...) : rows_cldr_gd<G, 8, 16, E, SRC>(q, src, live, a...);
        return cl_gd == 6 ? rows_cldr_gd<G, 6, 24, E, SRC>(q, src, live, a...) : rows_cldr_gd<G, 8, 24, E, SRC>(q, src, live, a...);
    }
    template <class G, int GD, int GT, template <typename, int> class E, template <typename, int> class SRC, class... A>
    int rows_cldr_gd(const Geom& q, const SRC<S, G::VECT>& src, const int* live, A... a) {
        const CldrGeom cg = plan.make_cldr_geom(q, cldr_dev.NT);
        const CldrDev& c = cldr_dev;
        CldrMeta mm{c.n0.get(), c.nC.get(), c.rows.get(), c.dcol.get(), c.dw.get(), c.dcnt.get(), c.tcol.get(), c.tw.get(), c.tcnt.get()};
        typedef E<S, G::VECT> Epi;
        auto fn = k_cldr<S, G::VECT, Epi, SRC<S, G::VECT>, G::NW, G::MA, G::MQ, G::MP, GD, GT, G::MINW>;
        MG_TRY(allow_dynamic_lds((const void*)fn, streamplan::CLDR_LDS_LIMIT));
        stream_keys.note(plan.key(plan.cldr_choice(GD, GT), Epi::ID, SRC<S, G::VECT>::FOLD));
        hipLaunchKernelGGL(fn, dim3(cg.grid), dim3(G::NW * 64), cg.lds_bytes, st, cg, mm, src, Epi{a...}, partials.get(), live);
        cur_P = cg.P;
        return MGADMM_OK;
    }
    template <template <typename, int> class E, template <typename, int> class SRC, class MK, class... A>
    int rows_cldr_any(const Geom& q, MK mk_src, const int* live, int tag, double bytes, A... a) {
        const bool timed = prof_open(tag, bytes);
        int rc;
        if constexpr (sizeof(S) == 4) {
            switch (plan.geom) {
                case 1: rc = rows_cldr_g<ClG1, E, SRC>(q, mk_src(ClG1()), live, a...); break;
                case 3: rc = rows_cldr_g<ClG3, E, SRC>(q, mk_src(ClG3()), live, a...); break;
                case 4: rc = rows_cldr_g<ClG4, E, SRC>(q, mk_src(ClG4()), live, a...); break;
                default: rc = rows_cldr_g<ClG2, E, SRC>(q, mk_src(ClG2()), live, a...); break;
            }
        } else {
            rc = rows_cldr_g<ClG2, E, SRC>(q, mk_src(ClG2()), live, a...);
        }
        if (timed) prof_close();
        MG_TRY(rc);
        MG_HIP(hipGetLastError());
        return MGADMM_OK;
    }
    // in -> epilogue(l = Ldr^T Ldr in); `passes`: algorithmic vector passes of the launch for the roofline accounting
    template <template <typename, int> class E, class... A>
    int rows_cldr(const Geom& q, const S* in, const int* live, int tag, int passes, A... a) {
        const double bytes = pass_bytes(q, passes) + csr_bytes(g->op_ldr()) + csr_bytes(g->op_ldrt());
        return rows_cldr_any<E, CldrSrcPlain>(q, [&](auto gg) { return CldrSrcPlain<S, decltype(gg)::VECT>{in}; }, live, tag, bytes, a...);
    }
    // the same with the CG direction formed on load: in = p_new = r + beta p_old; owners store p_new and x += alpha p_old
    template <template <typename, int> class E, class... A>
    int rows_cldr_fold(const Geom& q, const S* r, const S* p_old, S* p_new, S* x, const int* live, int tag, int passes, A... a) {
        const double bytes = pass_bytes(q, passes) + csr_bytes(g->op_ldr()) + csr_bytes(g->op_ldrt());
        return rows_cldr_any<E, CldrSrcFold>(q, [&](auto gg) { return CldrSrcFold<S, decltype(gg)::VECT>{r, p_old, p_new, x, d_alpha.get(), d_beta.get()}; },
                                             live, tag, bytes, a...);
    }

    int ensure_partials(const Geom& q) {
        TileGeom tg;
        int pmax = plan.make_tile_geom(q, tg) ? std::max(q.P, tg.P) : q.P;
        if (cldr_fits(q)) pmax = std::max(pmax, plan.make_cldr_geom(q, cldr_dev.NT).P);
        size_t need = (size_t)NRED_MAX * pmax * q.Bp;
        const size_t had = partials.capacity();
        if (need <= had) return MGADMM_OK;
        MG_HIP(hipStreamSynchronize(st));      // no launch reads the old block any more
        MG_BUF(partials.reserve(need));
        ws_bytes += (int64_t)(need - had) * sizeof(S);
        return MGADMM_OK;
    }

    // the workspace and the buffers of the streaming path, which the LDS path borrows (LdsEngine::init plans after it)
    int init_workspace() {
        MG_HIP(hipSetDevice(g->device));
        plan = streamplan::Planner(plan_facts(), streamplan::Switches::from_env((int)sizeof(S)));
        if (const char* e = getenv("MGADMM_LDS_CHUNK")) lds_chunk = std::max(1, std::min(atoi(e), LDS_MAXJ));
        Geom q = plan.make_geom(Bmax);
        Bp_max = q.Bp;
        // Bp for smaller batches never exceeds Bp_max rounded to 256
        Bp_max = std::max(Bp_max, ((Bmax + 63) / 64) * 64);
        vec_elems = (size_t)T * N * Bp_max;
        MG_BUF(vec_pool.reserve(vec_elems * V_COUNT));
        ws_bytes += (int64_t)vec_elems * V_COUNT * sizeof(S);
        for (int i = 0; i < V_COUNT; ++i) vec[i] = vec_pool.get() + vec_elems * i;
        MG_BUF(d_rr.reserve(Bp_max));
        MG_BUF(d_alpha.reserve(Bp_max));
        MG_BUF(d_beta.reserve(Bp_max));
        MG_BUF(d_active.reserve(Bp_max));
        MG_BUF(d_iters_tmp.reserve(Bp_max));
        MG_BUF(d_nonfinite.upload({0}));
        MG_BUF(d_ps.reserve((size_t)MGADMM_NMETRIC * Bp_max));
        const int nbk = (N + 63) / 64;
        MG_BUF(d_dxpart.reserve((size_t)T * nbk));
        MG_BUF(h_row.reserve(MGADMM_NMETRIC + 1));
        MG_BUF(h_flag.reserve(4));
        for (auto& e : ev_ring) MG_HIP(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
        MG_BUF(alloc_iter_dependent((size_t)p.max_admm_iter));
        return MGADMM_OK;
    }
    int init() override {
        MG_TRY(init_workspace());
        return refused(solvegate::admm_convergence_gate(facts(p), "solver_create"));
    }

    // What this solver refuses is decided in solve_gate.h from these facts (with the parameters `q` in force or about to be
    // set) and from what is set; the engine reports the answer
    solvegate::Facts facts(const mgadmm_params& q) const {
        return {std::is_same<S, float>::value, q.path, q.cg_convergence, q.admm_convergence, q.check_stop, lds.ok, g->mode == MGADMM_TEMPORAL_BAND, N, T};
    }
    solvegate::SetState set_state() const { return {wt.sp_B, sg_B, wt.sch_rows, wt.sch_B, ad_on}; }
    // time-varying weights (mgadmm_graph_set_time_weights) reach the row kernels only: the row sums of apply_op_Ln, the schedule
    // of two_loops and the images of the per-sample graphs hold one slice
    static int refuse_time_varying(const char* who) {
        mg_set_error("%s: not on a graph with time-varying weights (mgadmm_graph_set_time_weights)", who);
        return MGADMM_ERR_UNSUPPORTED;
    }
    static int refused(const solvegate::Result& r) { if (r.rc != MGADMM_OK) mg_set_error("%s", r.msg.c_str()); return r.rc; }

    // The buffers sized by the iteration limits: max_cg_iter of `p`, and `rows` ADMM iterations of history (max_admm_iter; two_loops:
    // outer x inner).  Called by set_params and at the head of every entry point that reads them, where it compares seven
    // capacities once they suffice: whatever an earlier call left, no launch sees a buffer smaller than `p` demands.  A buffer
    // grows on its own (Buf::reserve: a failure leaves it as it was); the error code of the first failure is returned
    int alloc_iter_dependent(size_t rows) {
        const size_t K = (size_t)p.max_cg_iter;
        if (int e = d_nact.reserve(K)) return e;
        if (int e = d_alpha_hist.reserve(3 * K * Bp_max)) return e;
        if (int e = d_beta_hist.reserve(3 * K * Bp_max)) return e;
        if (h_nact.capacity() < NACT_LOG + K) {
            if (int e = h_nact.reserve(NACT_LOG + K)) return e;
            nact_cur = 0;
        }
        if (int e = d_hist.reserve(rows * MGADMM_NMETRIC)) return e;
        if (int e = d_dxps.reserve(rows * T)) return e;
        return d_cg_iters.reserve(rows * 3 * Bp_max);
    }

    int set_params(const mgadmm_params& np) override {
        MG_REQUIRE(np.dtype == p.dtype, "set_params: dtype cannot change after solver_create");
        MG_REQUIRE(np.t_in >= 1 && np.t_in <= T, "set_params: t_in out of range");
        MG_REQUIRE(np.max_cg_iter >= 1 && np.max_admm_iter >= 1, "set_params: iteration limits must be >= 1");
        MG_REQUIRE(np.ablation >= 0 && np.ablation <= 3, "set_params: bad ablation");
        MG_REQUIRE(np.cg_convergence == MGADMM_CG_PER_SAMPLE || np.cg_convergence == MGADMM_CG_BATCH_MAX,
                   "set_params: cg_convergence should be per_sample (0) or batch_max (1), got %d", np.cg_convergence);
        MG_REQUIRE(np.max_inner_iter >= 0, "set_params: max_inner_iter must be >= 0 (got %d)", np.max_inner_iter);
        MG_TRY(refused(solvegate::set_params_gate(facts(np))));
        MG_TRY(refused(solvegate::admm_convergence_gate(facts(np), "set_params")));
        p = np;
        sv->p = np;
        MG_HIP(hipSetDevice(g->device));
        MG_BUF(alloc_iter_dependent((size_t)p.max_admm_iter));
        return MGADMM_OK;
    }

    // ---------------------------------------------------------------- per-sample and per-iteration ADMM weights
    // The host half: the caller's arrays are checked and kept (solve_gate.h); LdsEngine forms the device tables from them
    int set_sample_params(const mgadmm_sample_params* sp, int B) override {
        return refused(wt.set_sample(sp, B, Bmax));      // (sp == nullptr or B == 0 clears)
    }
    // Iteration k of the following solves reads row min(first_row + k, n_rows - 1) of the six arrays ([n_rows][B] row-major, or
    // [n_rows] with B == 0: every sample reads the same row); a null array follows the per-sample table or the scalar
    int set_param_schedule(const mgadmm_param_schedule* sch, int n_rows, int B, int first_row) override {
        MG_HIP(hipSetDevice(g->device));
        return refused(wt.set_schedule(sch, n_rows, B, first_row, Bmax));
    }

    // ---------------------------------------------------------------- adaptive penalties
    // Residual balancing of rho, rho_u, rho_d per sample (lds_adapt.h) in the solves that follow; `start`: iterations the
    // problem has run already (a resumed solve continues the periods).  nullptr clears
    int set_adaptive_rho(const mgadmm_adaptive_rho* ar, int start) override {
        if (ar == nullptr) { ad_on = false; return MGADMM_OK; }
        ldsadapt::Params q;
        q.every = ar->every; q.until = ar->until; q.mu = ar->mu; q.tau = ar->tau;
        q.tau_inv = 1.0 / ar->tau;
        for (int f = 0; f < 3; ++f) { q.rho_min[f] = ar->rho_min[f]; q.rho_max[f] = ar->rho_max[f]; }
        std::string why;
        if (!ldsadapt::validate(q, start, why)) {
            mg_set_error("set_adaptive_rho: %s", why.c_str());
            return MGADMM_ERR_INVALID;
        }
        ad = q; ad_start = start; ad_on = true;
        return MGADMM_OK;
    }

    // periods of the last solve's history (LdsEngine copies the history itself; a streaming solve never adapts)
    int get_adaptive_history(int, double*, int, int* n_periods) override {
        MG_REQUIRE(n_periods, "get_adaptive_history: n_periods is null");
        *n_periods = ad_last_periods;
        return MGADMM_OK;
    }

    // ---------------------------------------------------------------- per-sample graph weights
    // Sample b reads the weights of set set_of_sample[b].  The host half: n_sets == 0 clears, the argument checks, the gate;
    // LdsEngine plans and uploads the sets.  mgadmm_two_loops and the fine-grained entry points keep using the solver's own graph.
    int set_sample_graphs(int n_sets, mgadmm_graph* const* graphs, const int32_t* set_of_sample, int B) override {
        MG_HIP(hipSetDevice(g->device));
        if (n_sets == 0) { sg_B = 0; return MGADMM_OK; }
        if (g->time_varying) return refuse_time_varying("set_sample_graphs");
        MG_REQUIRE(n_sets >= 1 && graphs && set_of_sample, "set_sample_graphs: n_sets %d needs graphs and set_of_sample", n_sets);
        MG_REQUIRE(B >= 1 && B <= Bmax, "set_sample_graphs: batch %d outside [1, max_batch=%d]", B, Bmax);
        for (int b = 0; b < B; ++b)
            MG_REQUIRE(set_of_sample[b] >= 0 && set_of_sample[b] < n_sets, "set_sample_graphs: set_of_sample[%d] = %d outside [0, n_sets=%d)",
                       b, set_of_sample[b], n_sets);
        for (int s = 0; s < n_sets; ++s) {
            const mgadmm_graph* q = graphs[s];
            MG_REQUIRE(q, "set_sample_graphs: graphs[%d] is null", s);
            if (q->time_varying) return refuse_time_varying("set_sample_graphs");
            MG_REQUIRE(q->N == N && q->T == T, "set_sample_graphs: graphs[%d] has N = %d, T = %d, the solver's graph N = %d, T = %d", s, q->N, q->T, N, T);
            MG_REQUIRE(q->device == g->device, "set_sample_graphs: graphs[%d] lives on device %d, the solver on %d", s, q->device, g->device);
            MG_REQUIRE(q->mode == g->mode && q->transpose_by_gather == g->transpose_by_gather && q->q1 == g->q1 && q->skip == g->skip,
                       "set_sample_graphs: graphs[%d] differs from the solver's graph in temporal_mode, transpose_by_gather, q1_identity_t0 or skip", s);
            MG_REQUIRE(q->reorder == g->reorder && q->has_perm == g->has_perm && q->perm == g->perm,
                       "set_sample_graphs: graphs[%d] has another internal node order than the solver's graph", s);
        }
        return refused(solvegate::set_sample_graphs_gate(facts(p)));
    }

    // ---------------------------------------------------------------- per-sample temporal band weights
    // Sample b reads the band table of set set_of_sample[b] (band_sets.h: the checks, the caller's arrays).  Here also the table
    // of the streaming kernels, a weight per batch column of the geometry a solve of B samples gets; LdsEngine adds the tables
    // of the LDS path.  Synchronous: an old table is freed after the device has finished whatever read it
    int set_sample_bands(int n_sets, const float* band_w, const int32_t* set_of_sample, int B) override {
        MG_HIP(hipSetDevice(g->device));
        MG_TRY(refused(bs.set(g->mode == MGADMM_TEMPORAL_BAND, T, g->skip, n_sets, band_w, set_of_sample, B, Bmax)));
        MG_HIP(hipDeviceSynchronize());
        d_bs_exp.reset();
        bs_Bp = 0;
        if (bs.B == 0) return MGADMM_OK;
        std::vector<float> exp;
        const int Bp = plan.make_geom(bs.B).Bp;
        bs.expand(Bp, exp);
        if (d_bs_exp.upload(exp) != 0) {
            (void)hipGetLastError();
            bs.clear();
            mg_set_error("set_sample_bands: upload of the expanded table failed");
            return MGADMM_ERR_HIP;
        }
        bs_Bp = Bp;
        return MGADMM_OK;
    }

    int64_t workspace_bytes() const override { return ws_bytes; }
    int path_for(int) const override { return use_lds() ? MGADMM_PATH_LDS : MGADMM_PATH_STREAM; }
    // the fused LDS kernel runs one sample per workgroup with its CG loops inside: a batch-global stop cannot be expressed there
    bool use_lds() const { return lds.ok && p.path != MGADMM_PATH_STREAM && p.cg_convergence == MGADMM_CG_PER_SAMPLE; }
    int query(int what, int64_t* out) const override {
        switch (what) {
            case MGADMM_Q_LDS_OK: *out = lds.ok ? 1 : 0; break;
            case MGADMM_Q_LDS_TPG: *out = lds.TPG; break;
            case MGADMM_Q_LDS_THREADS: *out = lds.nthreads; break;
            case MGADMM_Q_LDS_BYTES: *out = (int64_t)lds.lds_bytes; break;
            case MGADMM_Q_LDS_ROW_STRIDE: *out = lds.TS; break;
            case MGADMM_Q_LDS_UNIFORM: *out = lds.uniform45; break;
            case MGADMM_Q_LDS_TAIL_PAIRS: *out = lds.tail_pairs; break;
            case MGADMM_Q_LDS_LEAD: *out = LDS_NLEAD; break;
            case MGADMM_Q_LDS_SLOTS: *out = lds.slots; break;
            case MGADMM_Q_LDS_CHUNK: *out = std::max(1, std::min(lds_chunk, LDS_MAXJ)); break;
            case MGADMM_Q_LDS_ROWS: *out = lds.NR; break;
            // (tables prepared by the first operator application; 0 as well when they exist but the batch the solver was created
            // for is no multiple of the kernel's chunk width: the two-pass form runs)
            case MGADMM_Q_CLDR_SLOTS: *out = cldr_dev.state == 1 && plan.cldr_width_fits(plan.make_geom(Bmax)) ? cldr_dev.gt : 0; break;
            case MGADMM_Q_LDS_INSTANCE: *out = lds_instance; break;
            case MGADMM_Q_LDS_UNIT: *out = lds_unit; break;
            case MGADMM_Q_LDS_CG_BARRIERS: *out = lds.ok ? lds.cg_barriers : 0; break;
            case MGADMM_Q_NNZ_U: *out = g->hWu.nnz(); break;
            case MGADMM_Q_NNZ_D: *out = g->hWd.nnz(); break;
            case MGADMM_Q_NNZ_DT: *out = g->hWdT.nnz(); break;
            case MGADMM_Q_TILE_ROWS: *out = plan.tile_rows(); break;
            case MGADMM_Q_STREAM_KEYS: *out = (int64_t)stream_keys.keys.size(); break;
            default:
                if (what >= MGADMM_Q_STREAM_KEY0 && (size_t)(what - MGADMM_Q_STREAM_KEY0) < stream_keys.keys.size()) {
                    *out = stream_keys.keys[what - MGADMM_Q_STREAM_KEY0];
                    break;
                }
                if (what >= MGADMM_Q_STREAM_KEY0) {
                    mg_set_error("solver_query: stream key %d of %zu", what - MGADMM_Q_STREAM_KEY0, stream_keys.keys.size());
                    return MGADMM_ERR_INVALID;
                }
                mg_set_error("solver_query: unknown item %d", what);
                return MGADMM_ERR_INVALID;
        }
        return MGADMM_OK;
    }

    // ---------------------------------------------------------------- profiling
    int prof_begin() override {
        MG_HIP(hipSetDevice(g->device));
        if (prof_ev.empty()) {
            prof_ev.resize(2 * PROF_POOL);
            for (auto& e : prof_ev) MG_HIP(hipEventCreateWithFlags(e.put(), hipEventDisableSystemFence));   // timing only: no system-scope cache flush per record
            prof_tag.resize(PROF_POOL);
            prof_lb.resize(PROF_POOL);
            prof_ref.resize(PROF_POOL);
        }
        prof_used = 0;
        nact_cur = 0;
        nact_locked = false;
        for (int i = 0; i < MGADMM_NPROF; ++i) { prof_count[i] = 0; prof_bytes[i] = 0; }
        prof_on = true;
        return MGADMM_OK;
    }
    int prof_end(int64_t* counts, double* total_ms, double* bytes) override {
        prof_on = false;
        MG_HIP(hipDeviceSynchronize());
        double ms[MGADMM_NPROF] = {0}, by[MGADMM_NPROF] = {0};
        int64_t timed[MGADMM_NPROF] = {0};
        prof_noop = 0;
        for (size_t i = 0; i < prof_used; ++i) {
            float f = 0;
            MG_HIP(hipEventElapsedTime(&f, prof_ev[2 * i], prof_ev[2 * i + 1]));
            // A speculative CG launch of iteration k+1 that found every sample converged after iteration k returns
            // at its `live` guard without touching its operands.  Whether that happened is read from the log of
            // active-sample counts the host copies back for its own convergence check (h_nact), not guessed from
            // the duration: such a launch is left out of BOTH the bytes and the time, so the reported rates are
            // those of launches that did the work.
            if (prof_ref[i] >= 0 && h_nact.get()[prof_ref[i]] == 0) {
                prof_noop++;
                continue;
            }
            ms[prof_tag[i]] += f;
            by[prof_tag[i]] += prof_lb[i];
            timed[prof_tag[i]]++;
        }
        for (int i = 0; i < MGADMM_NPROF; ++i) {
            counts[i] = timed[i];
            total_ms[i] = ms[i];
            bytes[i] = by[i];
        }
        return MGADMM_OK;
    }
    inline bool prof_open(int tag, double bytes) {
        if (!prof_on) return false;
        prof_count[tag]++;
        prof_bytes[tag] += bytes;
        if (tag == 3 || prof_used >= (size_t)PROF_POOL) return false;
        prof_tag[prof_used] = tag;
        prof_lb[prof_used] = bytes;
        prof_ref[prof_used] = prof_cur_ref;
        (void)hipEventRecord(prof_ev[2 * prof_used], st);
        return true;
    }
    inline void prof_close() {
        (void)hipEventRecord(prof_ev[2 * prof_used + 1], st);
        prof_used++;
    }

    double pass_bytes(const Geom& q, int passes) const { return (double)passes * q.B * (double)T * N * sizeof(S); }
    double csr_bytes(const OpDesc& op) const {
        if (op.kind != OPK_SPATIAL) return 0.0;
        const streamplan::Mat m = mat_of(op);
        const int nnz = m == streamplan::M_WU ? g->Wu.nnz : (m == streamplan::M_WD ? g->Wd.nnz : g->WdT.nnz);
        // (a per-slice table: the pattern once, the values of every slice the sweep reads)
        const double vals = op.val_t ? (double)op.n_slices * op.slice_stride * 4 : (double)nnz * 4;
        return (double)nnz * 4 + vals + (double)(N + 1) * 4;
    }

    // ---------------------------------------------------------------- launch helpers
    // hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: remember which (kernel, device)
    // pairs have been raised -- one solver per GPU may live in the same process.
    std::vector<const void*> lds_attr_done;
    int allow_dynamic_lds(const void* fn, int bytes) {
        for (const void* f : lds_attr_done)
            if (f == fn) return MGADMM_OK;
        MG_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        lds_attr_done.push_back(fn);
        return MGADMM_OK;
    }
    template <class E, class = void>
    struct is_elementwise : std::false_type {};
    template <class E>
    struct is_elementwise<E, std::void_t<decltype(E::ELEMENTWISE)>> : std::true_type {};

    // The ladders below turn a streamplan::Choice into a kernel instance; which one: the rules of stream_plan.h
    template <int VEC, class Epi, int TGW>
    int launch_tile(const streamplan::Choice& c, const TileGeom& tg, const OpDesc& op, const TileMeta& tmv, const S* in, const Epi& epi, const int* live) {
        return c.MR == 5 ? launch_tile2<VEC, Epi, TGW, 5>(c, tg, op, tmv, in, epi, live)
                         : launch_tile2<VEC, Epi, TGW, 2>(c, tg, op, tmv, in, epi, live);
    }
    template <int VEC, class Epi, int TGW, int MR>
    int launch_tile2(const streamplan::Choice& c, const TileGeom& tg, const OpDesc& op, const TileMeta& tmv, const S* in, const Epi& epi, const int* live) {
        auto fn = k_tile<S, VEC, Epi, TGW, MR>;
        MG_TRY(allow_dynamic_lds((const void*)fn, 80 * 1024));
        stream_keys.note(plan.key(c, Epi::ID, false));
        hipLaunchKernelGGL(fn, dim3(tg.grid), dim3(256), tg.lds_bytes, st, tg, op, tmv.tl_col, tmv.tl_w, tmv.halo, tmv.h_rowptr,
                           tmv.h_col, tmv.h_val, in, epi, partials.get(), live, TileSrcPlain<S, VEC>());
        return MGADMM_OK;
    }

    // ---- Lu with the CG vector update folded into its loads (k_tile with TileSrcFold): zu solve, where plan.fold2 says so
    static constexpr int LU_FOLD_VEC = sizeof(S) == 4 ? 4 : 2;
    template <template <typename, int> class E, class... A>
    int rows_lu_fold(const Geom& q, const S* r, const S* p_old, S* p_new, S* x, const int* live, int tag, int passes, A... a) {
        constexpr int VEC = LU_FOLD_VEC;
        typedef E<S, VEC> Epi;
        typedef TileSrcFold<S, VEC> Src;
        const OpDesc op = g->op_lu();
        const bool timed = prof_open(tag, pass_bytes(q, passes) + csr_bytes(op));
        const streamplan::Choice c = plan.lu_fold_choice();
        TileGeom tg;
        if (!plan.make_tile_geom(q, tg)) { mg_set_error("rows_lu_fold: no tile geometry"); return MGADMM_ERR_INVALID; }
        TileMeta tmv;
        MG_TRY(tile_meta(0, tg.R, 4, tmv));
        auto fn = k_tile<S, VEC, Epi, 4, 2, Src>;
        MG_TRY(allow_dynamic_lds((const void*)fn, 80 * 1024));
        stream_keys.note(plan.key(c, Epi::ID, true));
        hipLaunchKernelGGL(fn, dim3(tg.grid), dim3(256), tg.lds_bytes, st, tg, op, tmv.tl_col, tmv.tl_w, tmv.halo, tmv.h_rowptr,
                           tmv.h_col, tmv.h_val, r, Epi{a...}, partials.get(), live, Src{p_old, p_new, x, d_alpha.get(), d_beta.get()});
        cur_P = tg.P;
        if (timed) prof_close();
        MG_HIP(hipGetLastError());
        return MGADMM_OK;
    }

    template <int VEC, int GW, class Epi>
    int rows_v(const Geom& q, const streamplan::Choice& c, const OpDesc& op, const S* in, const Epi& epi, const int* live, int tag, double bytes) {
        const bool timed = prof_open(tag, bytes);
        if (c.kernel == STREAM_K_TILE) {
            if constexpr (is_elementwise<Epi>::value) {
                mg_set_error("rows: element-wise epilogue launched with a spatial operator");
                return MGADMM_ERR_INVALID;
            } else {
                TileGeom tg;
                plan.make_tile_geom(q, tg);
                TileMeta tmv;
                MG_TRY(tile_meta(c.mat - streamplan::M_WU, tg.R, c.GW, tmv));
                switch (c.GW) {
                    case 4: MG_TRY((launch_tile<VEC, Epi, 4>(c, tg, op, tmv, in, epi, live))); break;
                    case 6: MG_TRY((launch_tile<VEC, Epi, 6>(c, tg, op, tmv, in, epi, live))); break;
                    default: MG_TRY((launch_tile<VEC, Epi, 8>(c, tg, op, tmv, in, epi, live))); break;
                }
                cur_P = tg.P;
            }
        } else if (op.kind == OPK_SPATIAL && op.val_t != nullptr) {
            // time-varying weights: the twin of k_rows that takes a row's weights from the slice of its time step (no instance
            // key: stream_keys.h names the three time-invariant kernels)
            if constexpr (is_elementwise<Epi>::value) {
                mg_set_error("rows: element-wise epilogue launched with a spatial operator");
                return MGADMM_ERR_INVALID;
            } else {
                if (op.self_w != nullptr) {
                    mg_set_error("rows: no per-row self factor on time-varying weights");
                    return MGADMM_ERR_UNSUPPORTED;
                }
                hipLaunchKernelGGL((k_rows_tv<S, VEC, Epi, GW>), dim3(q.grid), dim3(256), 0, st, q, op, op.rowptr, op.col, op.val_t,
                                   in, epi, partials.get(), live);
                cur_P = q.P;
            }
        } else {
            stream_keys.note(plan.key(c, Epi::ID, false));
            hipLaunchKernelGGL((k_rows<S, VEC, Epi, GW>), dim3(q.grid), dim3(256), 0, st, q, op, op.rowptr, op.col, op.val,
                               op.band_w, in, epi, partials.get(), live);
            cur_P = q.P;
        }
        if (timed) prof_close();
        MG_HIP(hipGetLastError());
        return MGADMM_OK;
    }

    template <template <typename, int> class E, class... A>
    int rows(const Geom& q, const OpDesc& op, const S* in, const int* live, int tag, int passes, A... a) {
        const double bytes = pass_bytes(q, passes) + csr_bytes(op);
        const streamplan::Choice c = plan.choose(mat_of(op), op.self_w != nullptr, q);
        const bool wide = c.kernel == STREAM_K_ROWS && c.GW > 4;      // (k_tile: GW is its slot count, switched on in rows_v)
        switch (c.VEC) {
            case 1:
                return wide ? rows_v<1, 6>(q, c, op, in, E<S, 1>{a...}, live, tag, bytes)
                            : rows_v<1, 4>(q, c, op, in, E<S, 1>{a...}, live, tag, bytes);
            case 2:
                return wide ? rows_v<2, 6>(q, c, op, in, E<S, 2>{a...}, live, tag, bytes)
                            : rows_v<2, 4>(q, c, op, in, E<S, 2>{a...}, live, tag, bytes);
            case 4:
                if constexpr (sizeof(S) == 4)
                    return wide ? rows_v<4, 6>(q, c, op, in, E<S, 4>{a...}, live, tag, bytes)
                                : rows_v<4, 4>(q, c, op, in, E<S, 4>{a...}, live, tag, bytes);
        }
        mg_set_error("rows: unsupported VEC %d", c.VEC);
        return MGADMM_ERR_UNSUPPORTED;
    }

    template <int NRED, class Fin>
    int reduce(const Geom& q, const Fin& fin, const int* live) {
        prof_open(3, 0);
        hipLaunchKernelGGL((k_reduce<S, NRED, Fin>), dim3(q.Bp / 64), dim3(1024), 0, st, partials.get(), cur_P, q.Bp, fin, live);
        MG_HIP(hipGetLastError());
        return MGADMM_OK;
    }

    // Ldr / Ldr^T as a solve reads them: the graph's, with the per-column band weights while a solve with a band table runs
    OpDesc op_ldr() const { OpDesc o = g->op_ldr(); o.band_wb = band_wb; return o; }
    OpDesc op_ldrt() const { OpDesc o = g->op_ldrt(); o.band_wb = band_wb; return o; }
    static OpDesc op_none() {
        OpDesc o{};
        o.kind = OPK_NONE;
        return o;
    }

    int pack(const Geom& q, const void* src, int Ts, S* dst) {
        dim3 grid((N + 63) / 64, T, q.Bp / 64);
        prof_open(3, 0);
        hipLaunchKernelGGL((k_pack<S>), grid, dim3(256), 0, st, T, Ts, N, q.B, q.Bp, g->d_perm.get(), (const S*)src, dst);
        MG_HIP(hipGetLastError());
        return MGADMM_OK;
    }
    int unpack(const Geom& q, const S* src, void* dst) {
        dim3 grid((N + 63) / 64, T, q.Bp / 64);
        prof_open(3, 0);
        hipLaunchKernelGGL((k_unpack<S>), grid, dim3(256), 0, st, T, N, q.B, q.Bp, g->d_perm.get(), src, (S*)dst);
        MG_HIP(hipGetLastError());
        return MGADMM_OK;
    }
    int fill(S* dst, size_t n, S v) {
        hipLaunchKernelGGL((k_fill<S>), dim3(1024), dim3(256), 0, st, dst, n, v);
        MG_HIP(hipGetLastError());
        return MGADMM_OK;
    }
    size_t velems(const Geom& q) const { return (size_t)T * N * q.Bp; }

    int check_B(int B, const char* who) {
        MG_REQUIRE(B >= 1 && B <= Bmax, "%s: batch %d outside [1, max_batch=%d]", who, B, Bmax);
        MG_HIP(hipSetDevice(g->device));
        return MGADMM_OK;
    }

    LhsDef lhs_def(int which) const { return lhs_def_of(which, p.ablation, p.rho, p.rho_u, p.rho_d, p.mu_u, p.mu_d2); }      // (lds_param_table.h)

    // ---------------------------------------------------------------- operators (internal layout)
    int op_store(const Geom& q, const OpDesc& op, const S* in, S* out, int tag = 2) {
        return rows<EpiStore>(q, op, in, nullptr, tag, 2, out);
    }
    int cldr(const Geom& q, const S* in, S* out) {
        if (cldr_fits(q)) return rows_cldr<EpiStore>(q, in, nullptr, 2, 4, out);
        MG_TRY(op_store(q, g->op_ldr(), in, vec[V_Q]));
        return op_store(q, g->op_ldrt(), vec[V_Q], out);
    }

    // apply_op_Ln (ADMM.py:248-288): y[t] = [t>=1](s x[t] - W_d x[t-1]) + [t<=T-2](s x[t] - M x[t+1]), s_i = sum_j d_ew[i,j],
    // M = W_d^T (kNN: scatter_add) or W_d (physical: gather); line graph: x[t] - x[t+-1]/sqrt(2)
    int op_ln(const Geom& q, const S* in, S* out) {
        if (g->mode == MGADMM_TEMPORAL_BAND)
            return rows<EpiLnLine>(q, op_none(), in, nullptr, 2, 2, in, out, T, (size_t)N * q.Bp);
        if (!g->ln_rowsum) {
            std::vector<double> rs(N);
            for (int r = 0; r < N; ++r) {
                const int i = g->has_perm ? g->perm[r] : r;
                double a = 0.0;
                for (int e = g->hWd.rowptr[i]; e < g->hWd.rowptr[i + 1]; ++e) a += (double)g->hWd.val[e];
                rs[r] = a;
            }
            MG_BUF(g->ln_rowsum.upload(rs));      // (a failed copy leaves it empty: the next call builds it again)
        }
        OpDesc child = g->op_ldr();
        child.self_w = g->ln_rowsum.get();
        OpDesc father = g->op_ldrt();
        father.self_mode = SELF_LN_FATHER;
        father.q1 = 0;
        father.self_w = g->ln_rowsum.get();
        MG_TRY(rows<EpiStore>(q, child, in, nullptr, 2, 2, vec[V_Q]));
        return rows<EpiAddTo>(q, father, in, nullptr, 2, 3, (const S*)vec[V_Q], out);
    }

    // Ap = A p for an LhsDef; dot partial lands in partials[0]
    int lhs_apply(const Geom& q, const LhsDef& d, const S* pin, const S* mask, S* Ap, const int* live) {
        if (d.kind == 1) {
            // one launch = two SpMM applications (Ldr, Ldr^T): 2 x 8 B/element algorithmic
            if (cldr_fits(q))
                return rows_cldr<EpiLhs>(q, pin, live, 0, 4, (const S*)nullptr, mask, Ap, d.hth, p.t_in, (S)d.c1, (S)d.c2);
            MG_TRY(rows<EpiStore>(q, op_ldr(), pin, live, 0, 2, vec[V_Q]));
            return rows<EpiLhs>(q, op_ldrt(), vec[V_Q], live, 0, 3, pin, mask, Ap, d.hth, p.t_in, (S)d.c1, (S)d.c2);
        }
        if (d.kind == 2)
            return rows<EpiLhs>(q, g->op_lu(), pin, live, 0, 2, (const S*)nullptr, mask, Ap, d.hth, p.t_in, (S)d.c1, (S)d.c2);
        return rows<EpiLhs>(q, op_none(), pin, live, 1, 2, (const S*)nullptr, mask, Ap, d.hth, p.t_in, (S)d.c1, (S)0);
    }

    // ---------------------------------------------------------------- CG (ADMM.py:329-368)
    // rhs, x0, xout: internal layout.  iters_dev: int[Bp] destination for the per-sample counts.
    int cg_internal(const Geom& q, const LhsDef& d, const S* rhs, const S* x0, const S* mask, S* xout, int* iters_dev,
                    bool record, int* n_iter_launched = nullptr) {
        CgScalars<S> c;
        c.rr = d_rr.get(); c.alpha = d_alpha.get(); c.beta = d_beta.get(); c.active = d_active.get(); c.iters = iters_dev; c.n_active = d_nact.get();
        c.alpha_hist = record ? d_alpha_hist.get() : nullptr;
        c.beta_hist = record ? d_beta_hist.get() : nullptr;
        c.nonfinite = d_nonfinite.get();
        const int K = p.max_cg_iter;
        const int batch_max = p.cg_convergence == MGADMM_CG_BATCH_MAX ? 1 : 0;
        MG_HIP(hipMemsetAsync(d_nact.get(), 0, sizeof(int) * K, st));
        if (record) {
            MG_TRY(fill(d_alpha_hist.get(), (size_t)K * q.Bp, (S)NAN));
            MG_TRY(fill(d_beta_hist.get(), (size_t)K * q.Bp, (S)NAN));
        }
        S *r = vec[V_R], *pp = vec[V_P], *Ap = vec[V_AP];
        // r = rhs - A x0 ; p = r ; x = x0
        if (d.kind == 1 && cldr_fits(q)) {
            MG_TRY(rows_cldr<EpiCgInit>(q, x0, nullptr, 2, 7, (const S*)nullptr, rhs, mask, r, pp, xout, d.hth, p.t_in, (S)d.c1, (S)d.c2));
        } else if (d.kind == 1) {
            MG_TRY(rows<EpiStore>(q, op_ldr(), x0, nullptr, 2, 2, vec[V_Q]));
            MG_TRY(rows<EpiCgInit>(q, op_ldrt(), vec[V_Q], nullptr, 2, 6, x0, rhs, mask, r, pp, xout, d.hth, p.t_in,
                                   (S)d.c1, (S)d.c2));
        } else if (d.kind == 2) {
            MG_TRY(rows<EpiCgInit>(q, g->op_lu(), x0, nullptr, 2, 5, (const S*)nullptr, rhs, mask, r, pp, xout, d.hth,
                                   p.t_in, (S)d.c1, (S)d.c2));
        } else {
            MG_TRY(rows<EpiCgInit>(q, op_none(), x0, nullptr, 1, 5, (const S*)nullptr, rhs, mask, r, pp, xout, d.hth,
                                   p.t_in, (S)d.c1, (S)0));
        }
        MG_TRY((reduce<1>(q, FinCgInit<S>{c, q.B}, nullptr)));
        // slice of the pinned h_nact log used by this solve (a profiling session keeps every slice until prof_end)
        if (nact_cur + K > NACT_LOG) {
            if (prof_on) nact_locked = true;
            else nact_cur = 0;
        }
        const int base = nact_locked ? NACT_LOG : nact_cur;
        // the vector update of iteration k folded into the SpMM launch of iteration k+1 (k_cldr / k_tile, stream_plan.h): p
        // alternates between two buffers because other tiles still gather the old direction for their halos.  The x update
        // of the last iteration is applied after the loop.
        const bool fold1 = plan.fold1(d.kind, q, d.kind == 1 ? cldr_tiles() : 0);
        const bool fold2 = plan.fold2(d.kind, q);
        const bool fold = fold1 || fold2;
        S* pbuf[2] = {pp, vec[V_Q]};          // V_Q is free: the fused kernel keeps q = Ldr p on chip
        int k = 0;
        for (; k < K; ++k) {
            const int* live = k == 0 ? nullptr : d_nact.get() + (k - 1);
            prof_cur_ref = (k == 0 || nact_locked) ? -1 : base + k - 1;
            if (fold2) {
                // 1 SpMM application (8 B/element) + the absorbed vector update (20 B/element) per launch
                MG_TRY(rows_lu_fold<EpiLhs>(q, r, pbuf[k & 1], pbuf[(k + 1) & 1], xout, live, 0, 7, (const S*)nullptr, (const S*)nullptr, Ap,
                                            d.hth, p.t_in, (S)d.c1, (S)d.c2));
            } else if (fold1) {
                // 2 SpMM applications (16 B/element) + the absorbed vector update (20 B/element) per launch
                MG_TRY(rows_cldr_fold<EpiLhs>(q, r, pbuf[k & 1], pbuf[(k + 1) & 1], xout, live, 0, 9, (const S*)nullptr, (const S*)nullptr, Ap,
                                              d.hth, p.t_in, (S)d.c1, (S)d.c2));
            } else {
                MG_TRY(lhs_apply(q, d, pp, nullptr, Ap, live));                  // Ap = A p (no mask: quirk Q2)
            }
            MG_TRY((reduce<1>(q, FinCgAlpha<S>{c, k, q.Bp}, live)));
            {
                // r -= alpha Ap, r.r -- swept from the LAST time slice down: the SpMM kernel before it finished with the
                // last slices of Ap (still in the Infinity Cache), and the kernel after it starts with the first slices of r
                Geom qr = q;
                qr.rev = plan.sw.sweep_rev;
                MG_TRY(rows<EpiCgUpdate>(qr, op_none(), Ap, live, 1, 3, (const S*)d_alpha.get(), r));
            }
            MG_TRY((reduce<1>(q, FinCgBeta<S>{c, k, q.Bp, p.cg_tol, batch_max}, live)));
            if (!fold)
                MG_TRY(rows<EpiPUpdate>(q, op_none(), r, live, 1, 5, (const S*)d_alpha.get(), (const S*)d_beta.get(), xout, pp));   // x += alpha p, p = r + beta p
            prof_cur_ref = -1;
            MG_HIP(hipMemcpyAsync(h_nact.get() + base + k, d_nact.get() + k, sizeof(int), hipMemcpyDeviceToHost, st));
            MG_HIP(hipEventRecord(ev_ring[k % (LAG + 1)], st));
            if (k >= LAG) {
                MG_HIP(hipEventSynchronize(ev_ring[(k - LAG) % (LAG + 1)]));
                if (h_nact.get()[base + k - LAG] == 0) { ++k; break; }
            }
        }
        if (fold) {
            // the last iteration that did work: the first whose active count is 0 (later launches returned at the guard),
            // else the last one launched; its direction sits in pbuf[(kl + 1) & 1]
            MG_HIP(hipStreamSynchronize(st));
            const int launched = std::min(k, K);
            int kl = launched - 1;
            for (int j = 0; j < launched; ++j)
                if (h_nact.get()[base + j] == 0) { kl = j; break; }
            MG_TRY(rows<EpiXFinal>(q, op_none(), pbuf[(kl + 1) & 1], nullptr, 1, 3, (const S*)d_alpha.get(), xout));
        }
        if (!nact_locked) nact_cur += std::min(k, K);
        if (batch_max) {          // one iteration count for the whole batch: the first iteration after which no sample was above the tolerance
            hipLaunchKernelGGL(k_cg_batchmax_iters, dim3((q.B + 255) / 256), dim3(256), 0, st, (const int*)d_nact.get(), std::min(k, K), iters_dev, q.B);
            MG_HIP(hipGetLastError());
        }
        if (n_iter_launched) *n_iter_launched = k;
        return MGADMM_OK;
    }

    // ---------------------------------------------------------------- fine-grained ABI entry points
    int apply(int op, const void* x, void* y, int B, hipStream_t s) override {
        MG_TRY(check_B(B, "apply"));
        MG_REQUIRE(x && y, "apply: null pointer");
        if (op == MGADMM_OP_LN && g->time_varying) return refuse_time_varying("apply(MGADMM_OP_LN)");
        st = s;
        Geom q = plan.make_geom(B);
        MG_TRY(ensure_partials(q));
        MG_TRY(pack(q, x, T, vec[V_IO0]));
        switch (op) {
            case MGADMM_OP_LU: MG_TRY(op_store(q, g->op_lu(), vec[V_IO0], vec[V_IO1])); break;
            case MGADMM_OP_LDR: MG_TRY(op_store(q, g->op_ldr(), vec[V_IO0], vec[V_IO1])); break;
            case MGADMM_OP_LDRT: MG_TRY(op_store(q, g->op_ldrt(), vec[V_IO0], vec[V_IO1])); break;
            case MGADMM_OP_CLDR: MG_TRY(cldr(q, vec[V_IO0], vec[V_IO1])); break;
            case MGADMM_OP_LN: MG_TRY(op_ln(q, vec[V_IO0], vec[V_IO1])); break;
            default: mg_set_error("apply: bad op %d", op); return MGADMM_ERR_INVALID;
        }
        return unpack(q, vec[V_IO1], y);
    }

    int lhs(int which, const void* x, const void* mask, void* y, int B, hipStream_t s) override {
        MG_TRY(check_B(B, "lhs"));
        MG_REQUIRE(x && y, "lhs: null pointer");
        MG_REQUIRE(which >= 0 && which <= 2, "lhs: bad operator id %d", which);
        MG_REQUIRE(!(which == MGADMM_LHS_ZD && p.ablation == MGADMM_ABL_DGLR), "lhs: LHS_zd is undefined for ablation 'DGLR' (ADMM.py:392-399)");
        st = s;
        Geom q = plan.make_geom(B);
        MG_TRY(ensure_partials(q));
        MG_TRY(pack(q, x, T, vec[V_IO0]));
        const S* m = nullptr;
        if (mask && which == MGADMM_LHS_X) {
            MG_TRY(pack(q, mask, T, vec[V_MASK]));
            m = vec[V_MASK];
        }
        MG_TRY(lhs_apply(q, lhs_def(which), vec[V_IO0], m, vec[V_IO1], nullptr));
        return unpack(q, vec[V_IO1], y);
    }

    int phi_direct(const void* x, const void* gamma, void* phi, int B, hipStream_t s) override {
        MG_TRY(check_B(B, "phi_direct"));
        MG_REQUIRE(x && gamma && phi, "phi_direct: null pointer");
        st = s;
        Geom q = plan.make_geom(B);
        MG_TRY(ensure_partials(q));
        MG_TRY(pack(q, x, T, vec[V_IO0]));
        MG_TRY(pack(q, gamma, T, vec[V_TMP]));
        MG_TRY(rows<EpiPhiDirect>(q, g->op_ldr(), vec[V_IO0], nullptr, 2, 4, (const S*)vec[V_TMP], vec[V_IO1], (S)p.rho,
                                  (S)(p.mu_d1 / p.rho)));
        return unpack(q, vec[V_IO1], phi);
    }

    // float32 time moments of ADMM.py:772-775 over the t_in input steps: the mean of t, and den = the mean of t^2 - tm^2
    void time_moments(float& tm, float& den) const {
        float t2m = tm = 0;
        for (int t = 0; t < p.t_in; ++t) { tm += (float)t; t2m += (float)t * (float)t; }
        tm /= (float)p.t_in;
        t2m /= (float)p.t_in;
        den = t2m - tm * tm;
    }
    int guess_internal(const Geom& q, const S* ypad, S* x) {
        float tm, den;
        time_moments(tm, den);
        dim3 grid((N + 3) / 4, q.Bp / 64);
        hipLaunchKernelGGL((k_initial_guess<S>), grid, dim3(256), 0, st, T, p.t_in, N, q.Bp, (S)tm, (S)den, ypad, x);
        MG_HIP(hipGetLastError());
        return MGADMM_OK;
    }
    int interp_internal(const Geom& q, const S* y, const S* mask, int mask_f32, S* x) {
        dim3 grid((N + 3) / 4, q.Bp / 64);
        if (mask_f32 && sizeof(S) == 8)
            hipLaunchKernelGGL((k_initial_interp<S, true>), grid, dim3(256), 0, st, T, N, q.Bp, q.B, y, mask, x, d_nonfinite.get());
        else
            hipLaunchKernelGGL((k_initial_interp<S, false>), grid, dim3(256), 0, st, T, N, q.Bp, q.B, y, mask, x, d_nonfinite.get());
        MG_HIP(hipGetLastError());
        return MGADMM_OK;
    }

    int initial_guess(const void* y, void* x, int B, hipStream_t s) override {
        MG_TRY(check_B(B, "initial_guess"));
        MG_REQUIRE(x && y, "initial_guess: null pointer");
        st = s;
        Geom q = plan.make_geom(B);
        MG_TRY(pack(q, y, p.t_in, vec[V_Y]));
        MG_TRY(guess_internal(q, vec[V_Y], vec[V_IO1]));
        return unpack(q, vec[V_IO1], x);
    }

    int initial_interpolation(const void* y, const void* mask, int mask_f32, void* x, int B, hipStream_t s) override {
        MG_TRY(check_B(B, "initial_interpolation"));
        MG_REQUIRE(x && y && mask, "initial_interpolation: null pointer");
        st = s;
        Geom q = plan.make_geom(B);
        MG_TRY(pack(q, y, T, vec[V_Y]));
        MG_TRY(pack(q, mask, T, vec[V_MASK]));
        MG_TRY(interp_internal(q, vec[V_Y], vec[V_MASK], mask_f32, vec[V_IO1]));
        return unpack(q, vec[V_IO1], x);
    }

    int fetch_hist(const S* dev, size_t n, double* out, size_t B, size_t Bp, size_t K) {
        // dev: [K][Bp] -> out: [K][B] doubles
        std::vector<S> tmp(n);
        MG_HIP(hipMemcpyAsync(tmp.data(), dev, n * sizeof(S), hipMemcpyDeviceToHost, st));
        MG_HIP(hipStreamSynchronize(st));
        for (size_t k = 0; k < K; ++k)
            for (size_t b = 0; b < B; ++b) out[k * B + b] = (double)tmp[k * Bp + b];
        return MGADMM_OK;
    }

    int cg(int which, const void* rhs, const void* x0, const void* mask, void* x, int32_t* iters, double* alpha,
           double* beta, int B, hipStream_t s) override {
        MG_TRY(check_B(B, "cg"));
        MG_BUF(alloc_iter_dependent((size_t)p.max_admm_iter));      // (nothing to do unless an earlier set_params failed to allocate)
        MG_REQUIRE(rhs && x && iters, "cg: null pointer");
        MG_REQUIRE(which >= 0 && which <= 2, "cg: bad operator id %d", which);
        MG_REQUIRE(!(which == MGADMM_LHS_ZD && p.ablation == MGADMM_ABL_DGLR), "cg: LHS_zd is undefined for ablation 'DGLR'");
        st = s;
        Geom q = plan.make_geom(B);
        MG_TRY(ensure_partials(q));
        MG_HIP(hipMemsetAsync(d_nonfinite.get(), 0, sizeof(int), st));
        MG_TRY(pack(q, rhs, T, vec[V_RHS]));
        if (x0) MG_TRY(pack(q, x0, T, vec[V_IO0]));
        else MG_HIP(hipMemsetAsync(vec[V_IO0], 0, velems(q) * sizeof(S), st));
        const S* m = nullptr;
        if (mask && which == MGADMM_LHS_X) {
            MG_TRY(pack(q, mask, T, vec[V_MASK]));
            m = vec[V_MASK];
        }
        MG_TRY(cg_internal(q, lhs_def(which), vec[V_RHS], vec[V_IO0], m, vec[V_IO1], d_iters_tmp.get(), true));
        MG_TRY(unpack(q, vec[V_IO1], x));
        MG_HIP(hipMemcpyAsync(iters, d_iters_tmp.get(), sizeof(int) * B, hipMemcpyDeviceToHost, st));
        MG_HIP(hipMemcpyAsync(h_flag.get(), d_nonfinite.get(), sizeof(int), hipMemcpyDeviceToHost, st));
        MG_HIP(hipStreamSynchronize(st));
        const size_t K = p.max_cg_iter;
        if (alpha) MG_TRY(fetch_hist(d_alpha_hist.get(), K * q.Bp, alpha, B, q.Bp, K));
        if (beta) MG_TRY(fetch_hist(d_beta_hist.get(), K * q.Bp, beta, B, q.Bp, K));
        if (h_flag.get()[0]) {
            mg_set_error("cg: non-finite residual met");
            return MGADMM_ERR_NONFINITE;
        }
        return MGADMM_OK;
    }

    // ---------------------------------------------------------------- combined_loop (ADMM.py:511-648)
    // every state tensor the ablation uses must be present in a warm-start state
    bool has_phi() const { return p.ablation == MGADMM_ABL_NONE || p.ablation == MGADMM_ABL_DGLR; }      // the ablation iterates on (phi, gamma)
    bool has_zd() const { return p.ablation != MGADMM_ABL_DGLR; }                                        // ... on (zd, gamma_d)
    int check_state_in(const void* x0, const mgadmm_state* si) const {
        MG_REQUIRE(x0 && si && si->zu && si->gamma_u, "solve_from: x0, state_in.zu and state_in.gamma_u are required");
        MG_REQUIRE(!has_phi() || (si->phi && si->gamma), "solve_from: state_in.phi and state_in.gamma are required for this ablation");
        MG_REQUIRE(!has_zd() || (si->zd && si->gamma_d), "solve_from: state_in.zd and state_in.gamma_d are required for this ablation");
        return MGADMM_OK;
    }

    // per-sample metric history of a solve, when the caller asks for it
    int ensure_hist_ps(const mgadmm_history* hist, int B) {
        if (!hist || !hist->metrics_per_sample) return MGADMM_OK;
        MG_BUF(d_hist_ps.reserve((size_t)p.max_admm_iter * MGADMM_NMETRIC * B));
        return MGADMM_OK;
    }
    // The host's stop test after iteration `it` (ADMM.py:645-646): copies the metric row and the non-finite flag, waits for
    // the stream, and sets *stop when the loop ends here: both residual maxima are below admm_tol, or a NaN / Inf was met
    // (*rc_final = MGADMM_ERR_NONFINITE)
    int host_stop_test(int it, bool has_phi, bool has_zd, bool* stop, int* rc_final) {
        MG_HIP(hipMemcpyAsync(h_row.get(), d_hist.get() + (size_t)it * MGADMM_NMETRIC, sizeof(double) * MGADMM_NMETRIC, hipMemcpyDeviceToHost, st));
        MG_HIP(hipMemcpyAsync(h_flag.get(), d_nonfinite.get(), sizeof(int), hipMemcpyDeviceToHost, st));
        MG_HIP(hipStreamSynchronize(st));
        bool finite = h_flag.get()[0] == 0;
        for (int k = 0; k < MGADMM_NMETRIC; ++k) finite = finite && std::isfinite(h_row.get()[k]);
        if (!finite) { *rc_final = MGADMM_ERR_NONFINITE; *stop = true; return MGADMM_OK; }
        double pri = h_row.get()[MGADMM_M_PRI_ZU], dual = h_row.get()[MGADMM_M_DUAL_ZU];
        if (has_phi) { pri = std::max(pri, h_row.get()[MGADMM_M_PRI_PHI]); dual = std::max(dual, h_row.get()[MGADMM_M_DUAL_PHI]); }
        if (has_zd) { pri = std::max(pri, h_row.get()[MGADMM_M_PRI_ZD]); dual = std::max(dual, h_row.get()[MGADMM_M_DUAL_ZD]); }
        *stop = pri < p.admm_tol && dual < p.admm_tol;
        return MGADMM_OK;
    }

    // ---- what solve and two_loops share.  Bufs: the workspace vectors that hold the current / next x, zu, zd, phi
    struct Bufs {
        int xc = V_XA, xn = V_XB, zuc = V_ZUA, zun = V_ZUB, zdc = V_ZDA, zdn = V_ZDB, phc = V_PHIA, phn = V_PHIB;
        void swap_inner(bool has_zd) { std::swap(xc, xn); std::swap(zuc, zun); if (has_zd) std::swap(zdc, zdn); }
    };
    // packs y (mask mode: T steps, and the mask, returned in *m; prediction mode: t_in steps); `guess`: the first iterate to x
    int load_input(const Geom& q, const void* y, const void* mask, int mask_f32, bool guess, S* x, const S** m) {
        MG_TRY(pack(q, y, mask ? T : p.t_in, vec[V_Y]));
        if (mask) MG_TRY(pack(q, mask, T, vec[V_MASK]));
        *m = mask ? vec[V_MASK] : nullptr;
        if (!guess) return MGADMM_OK;
        return mask ? interp_internal(q, vec[V_Y], *m, mask_f32, x) : guess_internal(q, vec[V_Y], x);
    }
    // One inner ADMM step with the weights w = rho, rho_u, rho_d, mu_u, mu_d1, mu_d2: RHS_x, the x, zu and zd CG solves (counts
    // to it_base[3][Bp]) and the dual updates.  The caller reduces EpiDual's partial norms or not, and swaps the buffers
    int admm_step(const Geom& q, const double w[6], const Bufs& b, int* it_base, const S* m, bool record, mgadmm_history* hist, int it) {
        const bool has_phi = this->has_phi(), has_zd = this->has_zd();
        const S rho = (S)w[0], rho_u = (S)w[1], rho_d = (S)w[2];
        auto lhs_of = [&](int which) { return lhs_def_of(which, p.ablation, w[0], w[1], w[2], w[3], w[5]); };
        // ---- RHS_x (ADMM.py:556-564)
        if (has_phi) {
            MG_TRY(rows<EpiLin2>(q, op_none(), vec[V_GAM], nullptr, 3, 3, (const S*)vec[b.phc], vec[V_TMP], (S)1, rho));
            MG_TRY(rows<EpiRhsX>(q, op_ldrt(), vec[V_TMP], nullptr, 2, has_zd ? 7 : 5, (const S*)vec[b.zuc],
                                 (const S*)vec[b.zdc], (const S*)vec[V_GU], (const S*)vec[V_GD], (const S*)vec[V_Y],
                                 vec[V_RHS], rho_u, rho_d, 1, has_zd ? 1 : 0));
        } else {
            MG_TRY(rows<EpiRhsX>(q, op_none(), vec[b.zuc], nullptr, 3, 6, (const S*)vec[b.zuc], (const S*)vec[b.zdc],
                                 (const S*)vec[V_GU], (const S*)vec[V_GD], (const S*)vec[V_Y], vec[V_RHS], rho_u,
                                 rho_d, 0, 1));
        }
        // ---- x, zu, zd CG solves (ADMM.py:571-592)
        MG_TRY(cg_internal(q, lhs_of(MGADMM_LHS_X), vec[V_RHS], vec[b.xc], m, vec[b.xn], it_base, record));
        if (record) MG_TRY(save_coeffs(q.Bp, hist, it, 0, q.B));
        MG_TRY(rows<EpiLin2>(q, op_none(), vec[V_GU], nullptr, 3, 3, (const S*)vec[b.xn], vec[V_RHS], (S)0.5, (S)(w[1] / 2)));
        MG_TRY(cg_internal(q, lhs_of(MGADMM_LHS_ZU), vec[V_RHS], vec[b.zuc], nullptr, vec[b.zun], it_base + q.Bp, record));
        if (record) MG_TRY(save_coeffs(q.Bp, hist, it, 1, q.B));
        if (has_zd) {
            MG_TRY(rows<EpiLin2>(q, op_none(), vec[V_GD], nullptr, 3, 3, (const S*)vec[b.xn], vec[V_RHS], (S)0.5, (S)(w[2] / 2)));
            MG_TRY(cg_internal(q, lhs_of(MGADMM_LHS_ZD), vec[V_RHS], vec[b.zdc], nullptr, vec[b.zdn], it_base + 2 * q.Bp, record));
            if (record) MG_TRY(save_coeffs(q.Bp, hist, it, 2, q.B));
        }
        const S* zd_now = has_zd ? vec[b.zdn] : vec[b.zdc];
        // ---- dual updates + Laplacian-free residuals (ADMM.py:595-597, 612-636)
        return rows<EpiDual>(q, op_none(), vec[b.xn], nullptr, 3, has_zd ? 11 : 6, (const S*)vec[b.xc], (const S*)vec[b.zun],
                             (const S*)vec[b.zuc], zd_now, (const S*)vec[b.zdc], (const S*)vec[V_Y], m, vec[V_GU],
                             vec[V_GD], rho_u, rho_d, has_zd ? 1 : 0, p.t_in);
    }
    // x and the state the caller asked for, in the reference's layout
    int unpack_results(const Geom& q, const Bufs& b, void* x_out, const mgadmm_state* so) {
        MG_TRY(unpack(q, vec[b.xc], x_out));
        if (!so) return MGADMM_OK;
        void* const phi = has_phi() ? so->phi : nullptr, * const gamma = has_phi() ? so->gamma : nullptr;
        const std::pair<void*, int> out[] = {{so->zu, b.zuc}, {so->zd, b.zdc}, {phi, b.phc}, {gamma, V_GAM}, {so->gamma_u, V_GU}, {so->gamma_d, V_GD}};
        for (const auto& o : out) if (o.first) MG_TRY(unpack(q, vec[o.second], o.first));
        return MGADMM_OK;
    }

    // one solve on the LDS-resident path: LdsEngine's (lds_engine.h); use_lds() is false for every other engine
    virtual int solve_lds(const void*, const void*, int, const void*, const mgadmm_state*, void*, const mgadmm_state*, mgadmm_history*) {
        return MGADMM_ERR_UNSUPPORTED;
    }

    int solve(const void* y, const void* mask, int mask_f32, int B, const void* x0, const mgadmm_state* state_in, void* x_out,
              const mgadmm_state* state_out, mgadmm_history* hist, hipStream_t s) override {
        MG_TRY(check_B(B, "solve"));
        MG_BUF(alloc_iter_dependent((size_t)p.max_admm_iter));      // (as in cg)
        MG_REQUIRE(y && x_out, "solve: null pointer");
        if (state_in) MG_TRY(check_state_in(x0, state_in));
        st = s;
        ad_last_periods = 0;
        MG_TRY(refused(solvegate::solve_gate(facts(p), set_state(), B)));      // (before anything is enqueued; its order of refusals: solve_gate.h)
        MG_TRY(refused(bandsets::solve_gate(bs, facts(p), B)));                // (a band table: after every refusal of solve_gate)
        if (use_lds()) return solve_lds(y, mask, B, x0, state_in, x_out, state_out, hist);
        MG_TRY(refused(solvegate::admm_convergence_gate(facts(p), "solve")));       // (refused at solver_create / set_params already)
        const Geom q = plan.make_geom(B);
        // a band table: the Ldr / Ldr^T of this solve read a weight per batch column (op_ldr, op_ldrt) until it returns
        struct BandScope { const float*& wb; ~BandScope() { wb = nullptr; } } band_scope{band_wb};
        if (bs.B > 0) {
            MG_REQUIRE(d_bs_exp.get() && bs_Bp == q.Bp, "solve: the sample_bands table was expanded for %d columns, the solve has %d", bs_Bp, q.Bp);
            band_wb = d_bs_exp.get();
        }
        MG_TRY(ensure_partials(q));
        const size_t ne = velems(q);
        const bool has_phi = this->has_phi(), has_zd = this->has_zd();
        const int max_it = p.max_admm_iter;
        const bool record = p.record_cg_coeffs && hist && hist->cg_alpha && hist->cg_beta;
        MG_TRY(ensure_hist_ps(hist, B));
        MG_HIP(hipMemsetAsync(d_nonfinite.get(), 0, sizeof(int), st));
        MG_HIP(hipMemsetAsync(d_ps.get(), 0, sizeof(double) * MGADMM_NMETRIC * q.Bp, st));
        MG_HIP(hipMemsetAsync(d_cg_iters.get(), 0, sizeof(int) * (size_t)max_it * 3 * q.Bp, st));

        Bufs b;
        const S* m = nullptr;
        MG_TRY(load_input(q, y, mask, mask_f32, !state_in, vec[b.xc], &m));      // (a warm start brings its own x)
        if (state_in) {                       // warm start: the saved state replaces ADMM.py:529-544
            MG_TRY(pack(q, x0, T, vec[b.xc]));
            MG_TRY(pack(q, state_in->zu, T, vec[b.zuc]));
            MG_TRY(pack(q, state_in->gamma_u, T, vec[V_GU]));
            if (has_zd) {
                MG_TRY(pack(q, state_in->zd, T, vec[b.zdc]));
                MG_TRY(pack(q, state_in->gamma_d, T, vec[V_GD]));
            }
            if (has_phi) {
                MG_TRY(pack(q, state_in->phi, T, vec[b.phc]));
                MG_TRY(pack(q, state_in->gamma, T, vec[V_GAM]));
            }
        } else {
            MG_TRY(fill(vec[V_GU], ne, (S)0.1));
            MG_TRY(fill(vec[V_GD], ne, (S)0.1));
            if (has_phi) {
                MG_TRY(fill(vec[V_GAM], ne, (S)0.1));
                MG_TRY(op_store(q, op_ldr(), vec[b.xc], vec[b.phc]));
            }
            MG_HIP(hipMemcpyAsync(vec[b.zuc], vec[b.xc], ne * sizeof(S), hipMemcpyDeviceToDevice, st));
            MG_HIP(hipMemcpyAsync(vec[b.zdc], vec[b.xc], ne * sizeof(S), hipMemcpyDeviceToDevice, st));
        }

        // the six weights of an iteration: the row of the schedule (the shared form: solve_gate let no other through) or the scalars of `p`
        const ldsparam::Source wsrc = wt.source(true, p);
        int n_done = 0;
        int rc_final = MGADMM_OK;
        for (int it = 0; it < max_it; ++it) {
            double w[6];
            ldsparam::row_weights(wsrc, it, wt.sch_row0, w);
            const S rho = (S)w[0];
            MG_TRY(admm_step(q, w, b, d_cg_iters.get() + (size_t)it * 3 * q.Bp, m, record, hist, it));
            MG_TRY((reduce<6>(q, FinMetrics<6>{d_ps.get(), q.Bp, {MGADMM_M_XSHIFT, MGADMM_M_PRI_ZU, MGADMM_M_DUAL_ZU, has_zd ? MGADMM_M_PRI_ZD : -1,
                                                       has_zd ? MGADMM_M_DUAL_ZD : -1, MGADMM_M_RECOVER}}, nullptr)));
            // ---- phi prox, gamma update, Ldr-based residuals and regularisers (ADMM.py:600-606, 627-637)
            MG_TRY(rows<EpiPhi>(q, op_ldr(), vec[b.xn], nullptr, 2, has_phi ? 5 : 1, (const S*)vec[b.phc], vec[b.phn], vec[V_GAM],
                                rho, (S)(w[4] / w[0]), has_phi ? 1 : 0));
            MG_TRY((reduce<4>(q, FinMetrics<4>{d_ps.get(), q.Bp, {has_phi ? MGADMM_M_PRI_PHI : -1, has_phi ? MGADMM_M_DUAL_PHI : -1,
                                                       has_phi ? MGADMM_M_DGTV : -1, has_zd ? MGADMM_M_DGLR : -1}}, nullptr)));
            MG_TRY(rows<EpiDot>(q, g->op_lu(), vec[b.xn], nullptr, 2, 1));
            MG_TRY((reduce<1>(q, FinMetrics<1>{d_ps.get(), q.Bp, {MGADMM_M_GLR}}, nullptr)));
            const int nbk = (N + 63) / 64;
            hipLaunchKernelGGL((k_dxps<S>), dim3(T * nbk), dim3(256), 0, st, T, N, q.Bp, B, nbk, (const S*)vec[b.xn],
                               (const S*)vec[b.xc], d_dxpart.get());
            hipLaunchKernelGGL(k_dxps_final, dim3((T + 63) / 64), dim3(64), 0, st, T, nbk, (const double*)d_dxpart.get(),
                               d_dxps.get() + (size_t)it * T);
            hipLaunchKernelGGL(k_batch_metrics, dim3(MGADMM_NMETRIC), dim3(256), 0, st, (const double*)d_ps.get(), q.Bp, B,
                               d_hist.get() + (size_t)it * MGADMM_NMETRIC,
                               (hist && hist->metrics_per_sample) ? d_hist_ps.get() + (size_t)it * MGADMM_NMETRIC * B : nullptr);
            MG_HIP(hipGetLastError());
            b.swap_inner(has_zd);
            if (has_phi) std::swap(b.phc, b.phn);
            n_done = it + 1;
            if (p.check_stop) {
                bool stop = false;
                MG_TRY(host_stop_test(it, has_phi, has_zd, &stop, &rc_final));
                if (stop) break;
            }
        }
        MG_TRY(unpack_results(q, b, x_out, state_out));
        return finish_history(hist, n_done, B, q.Bp, rc_final);
    }

    // ---------------------------------------------------------------- two_loops (ADMM.py:410-508)
    // Same kernels as `solve`, other schedule: the phi / gamma update moves to an outer loop and every outer iteration
    // restarts the inner ADMM on (x, zu, zd, gamma_u, gamma_d) from zu = zd = x, gamma_u = gamma_d = 0.1.  No residual
    // history (the reference records none there: "TODO: residual", ADMM.py:494, 506); CG counts per inner iteration.
    int two_loops(const void* y, const void* mask, int mask_f32, int B, void* x_out, const mgadmm_state* state_out,
                  mgadmm_history* hist, hipStream_t s) override {
        MG_TRY(check_B(B, "two_loops"));
        MG_REQUIRE(y && x_out, "two_loops: null pointer");
        MG_REQUIRE(p.max_inner_iter >= 1, "two_loops: max_inner_iter must be >= 1 (got %d)", p.max_inner_iter);
        if (g->time_varying) return refuse_time_varying("two_loops");
        st = s;
        const Geom q = plan.make_geom(B);
        MG_TRY(ensure_partials(q));
        const size_t ne = velems(q);
        const bool has_phi = this->has_phi(), has_zd = this->has_zd();
        const int n_outer = p.max_admm_iter, n_inner = p.max_inner_iter;
        const size_t rows_needed = (size_t)n_outer * n_inner;
        if (const int e = alloc_iter_dependent(rows_needed)) {          // d_cg_iters holds one row of 3 x Bp counts per inner iteration
            (void)hipGetLastError();
            mg_set_error("two_loops: cannot allocate the CG-count history of %zu inner iterations x %d samples (%s)", rows_needed,
                         Bp_max, mg_buf_error(e));
            return MGADMM_ERR_NOMEM;
        }
        MG_HIP(hipMemsetAsync(d_nonfinite.get(), 0, sizeof(int), st));
        MG_HIP(hipMemsetAsync(d_ps.get(), 0, sizeof(double) * MGADMM_NMETRIC * q.Bp, st));
        MG_HIP(hipMemsetAsync(d_cg_iters.get(), 0, sizeof(int) * rows_needed * 3 * q.Bp, st));
        Bufs b;
        const S* m = nullptr;
        MG_TRY(load_input(q, y, mask, mask_f32, true, vec[b.xc], &m));
        if (has_phi) {
            MG_TRY(fill(vec[V_GAM], ne, (S)0.1));
            MG_TRY(op_store(q, g->op_ldr(), vec[b.xc], vec[b.phc]));
        }
        const double w[6] = {p.rho, p.rho_u, p.rho_d, p.mu_u, p.mu_d1, p.mu_d2};      // the scalars: a schedule is not read here
        int n_done = 0;
        for (int o = 0; o < n_outer; ++o) {
            MG_TRY(fill(vec[V_GU], ne, (S)0.1));
            MG_TRY(fill(vec[V_GD], ne, (S)0.1));
            MG_HIP(hipMemcpyAsync(vec[b.zuc], vec[b.xc], ne * sizeof(S), hipMemcpyDeviceToDevice, st));
            MG_HIP(hipMemcpyAsync(vec[b.zdc], vec[b.xc], ne * sizeof(S), hipMemcpyDeviceToDevice, st));
            for (int in = 0; in < n_inner; ++in) {
                // (no CG coefficients are recorded and EpiDual's fused norms are not kept: ADMM.py:488-490)
                MG_TRY(admm_step(q, w, b, d_cg_iters.get() + ((size_t)o * n_inner + in) * 3 * q.Bp, m, false, nullptr, 0));
                b.swap_inner(has_zd);
            }
            if (has_phi) {          // phi = phi_direct(x, gamma); gamma += rho (phi - Ldr x)   (ADMM.py:497-504)
                MG_TRY(rows<EpiPhi>(q, g->op_ldr(), vec[b.xc], nullptr, 2, 5, (const S*)vec[b.phc], vec[b.phn], vec[V_GAM], (S)p.rho,
                                    (S)(p.mu_d1 / p.rho), 1));
                std::swap(b.phc, b.phn);
            }
            n_done = o + 1;
        }
        MG_TRY(unpack_results(q, b, x_out, state_out));
        if (hist) {
            hist->n_iters = n_done;
            if (hist->cg_iters) MG_TRY(fetch_cg_iters(hist->cg_iters, rows_needed, B, q.Bp));
        }
        MG_HIP(hipMemcpyAsync(h_flag.get(), d_nonfinite.get(), sizeof(int), hipMemcpyDeviceToHost, st));
        MG_HIP(hipStreamSynchronize(st));
        if (h_flag.get()[0]) {
            mg_set_error("two_loops: NaN/Inf met in the iterates (cf. the asserts of ADMM.py:432-504)");
            return MGADMM_ERR_NONFINITE;
        }
        return MGADMM_OK;
    }

    // the CG counts of `rows` iterations: [rows][3][Bp] on the device -> out[rows][3][B]
    int fetch_cg_iters(int32_t* out, size_t rows, int B, int Bp) {
        std::vector<int> tmp(rows * 3 * Bp);
        MG_HIP(hipMemcpyAsync(tmp.data(), d_cg_iters.get(), sizeof(int) * tmp.size(), hipMemcpyDeviceToHost, st));
        MG_HIP(hipStreamSynchronize(st));
        for (size_t r = 0; r < rows * 3; ++r) memcpy(out + r * B, tmp.data() + r * Bp, sizeof(int) * B);
        return MGADMM_OK;
    }
    // copies the device-side history of a finished solve into the caller's host buffers
    // nps: iterations of every sample of a solve that stopped per sample (its delta_x_per_step is not formed), else nullptr
    int finish_history(mgadmm_history* hist, int n_done, int B, int Bp, int rc_final, const int* nps = nullptr) {
        if (hist) {
            hist->n_iters = n_done;
            if (hist->n_iters_per_sample)
                for (int b = 0; b < B; ++b) hist->n_iters_per_sample[b] = nps ? nps[b] : n_done;
            if (hist->metrics)
                MG_HIP(hipMemcpyAsync(hist->metrics, d_hist.get(), sizeof(double) * (size_t)n_done * MGADMM_NMETRIC, hipMemcpyDeviceToHost, st));
            if (hist->delta_x_per_step && !nps)
                MG_HIP(hipMemcpyAsync(hist->delta_x_per_step, d_dxps.get(), sizeof(double) * (size_t)n_done * T, hipMemcpyDeviceToHost, st));
            if (hist->metrics_per_sample)
                MG_HIP(hipMemcpyAsync(hist->metrics_per_sample, d_hist_ps.get(), sizeof(double) * (size_t)n_done * MGADMM_NMETRIC * B,
                                      hipMemcpyDeviceToHost, st));
            if (hist->cg_iters) MG_TRY(fetch_cg_iters(hist->cg_iters, n_done, B, Bp));
        }
        MG_HIP(hipMemcpyAsync(h_flag.get(), d_nonfinite.get(), sizeof(int), hipMemcpyDeviceToHost, st));
        MG_HIP(hipStreamSynchronize(st));
        if (rc_final == MGADMM_OK && h_flag.get()[0]) rc_final = MGADMM_ERR_NONFINITE;
        if (rc_final == MGADMM_OK && hist && hist->metrics) {
            for (size_t k = 0; k < (size_t)n_done * MGADMM_NMETRIC; ++k)
                if (!std::isfinite(hist->metrics[k])) rc_final = MGADMM_ERR_NONFINITE;
        }
        if (rc_final == MGADMM_ERR_NONFINITE) mg_set_error("solve: NaN/Inf met in the iterates (cf. the asserts of ADMM.py:534-606)");
        return rc_final;
    }

    // the CG coefficients of solve `which` of iteration `it`, which stand at [from][K][Bp] of the device buffers
    int save_coeffs(int Bp, mgadmm_history* hist, int it, int which, int B, int from = 0) {
        const size_t K = p.max_cg_iter;
        double* a = hist->cg_alpha + ((size_t)it * 3 + which) * K * B;
        double* b = hist->cg_beta + ((size_t)it * 3 + which) * K * B;
        MG_TRY(fetch_hist(d_alpha_hist.get() + (size_t)from * K * Bp, K * Bp, a, B, Bp, K));
        return fetch_hist(d_beta_hist.get() + (size_t)from * K * Bp, K * Bp, b, B, Bp, K);
    }
};

}  // namespace
