// Driver of the LDS-resident fused path (kernels of lds_kernels.h behind the launch interface of lds_args.h): the float32
// engine, Engine<float> (engine.h) with the plan's device image, the device tables of the per-sample features and one solve
// on that path (solve_lds, the one virtual Engine::solve calls).  What decides -- the plan, the schedule, the refusals -- is
// in lds_plan.h, lds_schedule.h and solve_gate.h; this drives the HIP calls.  Included by solver_f32.hip only.
#pragma once
#include <stdio.h>

#include <thread>

#include "engine.h"
#include "lds_args.h"
#include "lds_graph_sets.h"
#include "lds_schedule.h"

namespace {

struct LdsEngine final : Engine<float> {
    int dev_cus = 0;               // compute units of the device (staggered start of k_admm_lds)
    DevBuf<int> d_lds_csr;
    DevBuf<double> d_slice_sums;      // [ceil(Bmax/64)][T*N]: delta_x_per_step, the sums of x - x_old over every 64-sample slice
    // the whole-batch metric kernels (lds_args.h, mg_lds_metrics) beside a k_admm_lds launch and on an idle GPU
    LdsMetricShape metric_busy{64, 0}, metric_idle{256, 0};
    // ADMM outer loop of the LDS path without host round trips (solve_lds): device stop word, second metric buffer, helper
    // stream for the whole-batch metric kernels and the events that order the two streams
    int lds_async = 1;            // MGADMM_LDS_ASYNC=0: one stream, the host tests the stop criterion after every iteration
    DevBuf<int> d_stop;
    DevBuf<double> d_ps_ring;     // [LDS_SETS][J][NMETRIC][Bp]: per-sample metric sums of the chunked schedule
    // per-sample stop of the outer loop (MGADMM_ADMM_PER_SAMPLE)
    DevBuf<int> d_pstop;          // [Bp_max] stop words, [1] number of stopped samples, [Bp_max] iterations of every sample
    DevBuf<double> d_ps_full;     // [max_admm_iter][NMETRIC][Bp]: per-sample metric sums of every iteration (allocated on first use)
    // per-sample ADMM weights (mgadmm_solver_set_sample_params) and per-iteration weights (mgadmm_solver_set_param_schedule):
    // the device tables of the records k_admm_lds_pp reads (the caller's arrays: Engine::wt).  d_sp: wt.sp_B records, rebuilt
    // whenever the arrays or the scalars change; d_sch: wt.sch_rows x B records, formed when a solve starts and kept until
    // something it was formed from changes
    DevBuf<LdsSampleParams> d_sp;      // [Bmax]
    DevBuf<LdsSampleParams> d_sch;
    int sch_up_B = 0;             // batch the device table was formed for; 0 = it has to be formed
    // adaptive penalties (Engine::ad, lds_adapt.h): per solve the table of max_admm_iter x B records k_lds_adapt writes between
    // the launches, the six weights of every sample as doubles and the history of the three penalties by period
    DevBuf<LdsSampleParams> d_ad_tab;
    DevBuf<double> d_ad_w, d_ad_hist;
    int ad_last_B = 0;            // of the last solve that adapted (mgadmm_solver_get_adaptive_history)
    // per-sample graph weights (mgadmm_solver_set_sample_graphs, lds_graph_sets.h): the images of the sets back to back and the
    // set of every sample; the solver's own image and the planner's switches are kept for the comparison with every set
    DevBuf<int> d_sg_img;         // [sets][img_stride]
    DevBuf<int> d_sg_set;         // [Bp_max]
    std::vector<int> lds_img_host;
    // per-sample temporal band weights (mgadmm_solver_set_sample_bands, band_sets.h; the caller's arrays: Engine::bs): the
    // tables of the sets back to back and the set of every sample
    DevBuf<float> d_bs_w;         // [sets][T*skip]
    DevBuf<int> d_bs_set;         // [Bp_max]
    ldsplan::Switches lds_sw;
    // iterate buffers of solve_lds by slot number (lds_schedule.h): the 15 workspace vectors this path does not use otherwise
    // hold the LDS_SETS (J - 1) + LDS_NBOUND = 13 slots of J = 4; chunks longer than 4 iterations (up to LDS_MAXJ) get the
    // rest in lds_ring_extra on the first solve that asks for them, kept for the solver's lifetime
    static constexpr int ring_ids[] = {V_XA, V_XB, V_ZUB, V_ZDB, V_PHIB, V_Y, V_MASK, V_R, V_P, V_Q, V_AP, V_RHS, V_TMP, V_IO0, V_IO1};
    static constexpr int NRING = (int)(sizeof(ring_ids) / sizeof(ring_ids[0]));
    std::vector<DevBuf<float>> lds_ring_extra;
    Stream st_side;
    Event ev_main[LDS_NBOUND], ev_side[LDS_NBOUND];

    using Engine<float>::Engine;
    ~LdsEngine() override { (void)hipSetDevice(g->device); }      // (before the members release, as in ~Engine)

    int init() override {
        MG_TRY(init_workspace());
        if (const char* e = getenv("MGADMM_LDS_ASYNC")) lds_async = atoi(e);
        MG_TRY(plan_lds());
        return refused(solvegate::admm_convergence_gate(facts(p), "solver_create"));
    }

    // ---------------------------------------------------------------- the setters: Engine's host half, then the device tables
    int set_params(const mgadmm_params& np) override {
        const mgadmm_params old = p;
        const int rc = Engine<float>::set_params(np);      // (p is replaced once nothing refuses np)
        if (p.rho != old.rho || p.rho_u != old.rho_u || p.rho_d != old.rho_d || p.mu_u != old.mu_u || p.mu_d1 != old.mu_d1 ||
            p.mu_d2 != old.mu_d2 || p.ablation != old.ablation)
            sch_up_B = 0;      // (the schedule's records follow the scalars where it names no weight)
        MG_TRY(rc);
        return wt.sp_B > 0 ? upload_sample_params(wt.sp_B) : (int)MGADMM_OK;      // (fields that were not given follow the new scalars)
    }

    int set_sample_params(const mgadmm_sample_params* sp, int B) override {
        MG_TRY(Engine<float>::set_sample_params(sp, B));
        sch_up_B = 0;
        if (wt.sp_B == 0) return MGADMM_OK;
        MG_HIP(hipSetDevice(g->device));
        return upload_sample_params(wt.sp_B);
    }
    // record b of the device table from sample b's six doubles: the expressions and casts solve_lds uses for the scalars
    // (n records; without a weights table -- a solve with a graph table alone -- every record holds the scalars)
    int upload_sample_params(int n) {
        std::vector<LdsSampleParams> rec;
        ldsparam::fill_records(wt.source(false, p), p.ablation, n, rec);      // (lds_param_table.h: one row, no schedule)
        MG_BUF(d_sp.reserve((size_t)Bmax));
        MG_BUF(d_sp.upload(rec));
        return MGADMM_OK;
    }

    // Synchronous like set_sample_graphs: the old device table is freed after the device has finished whatever read it
    int set_param_schedule(const mgadmm_param_schedule* sch, int n_rows, int B, int first_row) override {
        MG_HIP(hipSetDevice(g->device));
        if ((sch == nullptr || n_rows == 0) && d_sch) {      // clears
            MG_HIP(hipDeviceSynchronize());
            d_sch.reset();
        }
        MG_TRY(Engine<float>::set_param_schedule(sch, n_rows, B, first_row));
        sch_up_B = 0;
        return MGADMM_OK;
    }
    // the device table of a solve of B samples on the LDS path: sch_rows x B records
    int upload_param_schedule(int B) {
        if (sch_up_B == B && d_sch) return MGADMM_OK;
        std::vector<LdsSampleParams> rec;
        ldsparam::fill_records(wt.source(true, p), p.ablation, B, rec);
        MG_BUF(d_sch.upload(rec));
        sch_up_B = B;
        return MGADMM_OK;
    }

    // the history of the last solve: rho_hist[p][3][B] = rho, rho_u, rho_d of period p (NaN past a sample's own stop)
    int get_adaptive_history(int B, double* rho_hist, int max_periods, int* n_periods) override {
        MG_TRY(Engine<float>::get_adaptive_history(B, rho_hist, max_periods, n_periods));
        if (ad_last_periods == 0 || rho_hist == nullptr || max_periods <= 0) return MGADMM_OK;
        MG_REQUIRE(B == ad_last_B, "get_adaptive_history: the last adaptive_rho solve had B = %d, not %d", ad_last_B, B);
        MG_HIP(hipSetDevice(g->device));
        MG_HIP(hipMemcpy(rho_hist, d_ad_hist.get(), sizeof(double) * 3 * (size_t)B * std::min(max_periods, ad_last_periods), hipMemcpyDeviceToHost));
        return MGADMM_OK;
    }

    // Every set is planned with the solver's switches and shares its topology (lds_graph_sets.h names the first difference).
    int set_sample_graphs(int n_sets, mgadmm_graph* const* graphs, const int32_t* set_of_sample, int B) override {
        MG_HIP(hipSetDevice(g->device));
        if (n_sets == 0 && d_sg_img) {
            MG_HIP(hipDeviceSynchronize());
            d_sg_img.reset();
        }
        MG_TRY(Engine<float>::set_sample_graphs(n_sets, graphs, set_of_sample, B));      // (n_sets == 0 clears; the checks, the gate)
        if (n_sets == 0) return MGADMM_OK;
        // plan every set (the bank search of a set takes as long as the solver's own: sets are planned side by side)
        std::vector<ldsplan::Input> sets;
        for (int s = 0; s < n_sets; ++s)
            sets.push_back(ldsplan::Input{T, N, false, graphs[s]->transpose_by_gather != 0, graphs[s]->hWu, graphs[s]->hWd, graphs[s]->hWdT});
        std::vector<int> table;
        std::string differs;
        int bad = -1;
        if (!ldssets::build_table(lds, lds_img_host, sets, lds_sw, table, &bad, differs, std::min(8, (int)std::thread::hardware_concurrency()))) {
            mg_set_error("set_sample_graphs: sample_graphs set %d does not share the solver's topology -- %s (a weight that underflowed to 0 and "
                         "was dropped, another k or other neighbour lists?)", bad, differs.c_str());
            return MGADMM_ERR_UNSUPPORTED;
        }
        std::vector<int> set_of((size_t)Bp_max, 0);
        std::copy(set_of_sample, set_of_sample + B, set_of.begin());
        DevBuf<int> fresh;      // (a local owner: whatever fails below, the new images are released)
        MG_BUF(fresh.reserve(table.size()));
        if (fresh.upload(table) != 0) {
            mg_set_error("set_sample_graphs: upload of the images failed");
            return MGADMM_ERR_HIP;
        }
        MG_BUF(d_sg_set.reserve((size_t)Bp_max));
        MG_HIP(hipDeviceSynchronize());          // no launch reads the old table any more
        MG_BUF(d_sg_set.upload(set_of));
        d_sg_img = std::move(fresh);
        sg_B = B;
        return MGADMM_OK;
    }

    // The tables lie back to back as the caller gave them: workgroup b of k_admm_lds_pp reads the one of set d_bs_set[b]
    int set_sample_bands(int n_sets, const float* band_w, const int32_t* set_of_sample, int B) override {
        MG_TRY(Engine<float>::set_sample_bands(n_sets, band_w, set_of_sample, B));      // (the checks; synchronises; clears)
        d_bs_w.reset();
        if (bs.B == 0) return MGADMM_OK;
        const std::vector<int32_t> set_of = bs.padded_set_of(Bp_max);
        MG_BUF(d_bs_set.reserve((size_t)Bp_max));
        MG_BUF(d_bs_w.upload(bs.w));
        MG_BUF(d_bs_set.upload(set_of));
        return MGADMM_OK;
    }

    // ---------------------------------------------------------------- LDS-resident fused path
    int plan_lds() {
        if (hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, g->device) != hipSuccess) { (void)hipGetLastError(); dev_cus = 0; }
        // which k_admm_lds instance, its geometry and the image of its tables: plain host code, lds_plan.h
        if (g->time_varying) return MGADMM_OK;      // the images hold one slice of weights: no plan, MGADMM_Q_LDS_OK = 0, solve_gate.h refuses the rest
        std::vector<int> img;
        const ldsplan::Input in{T, N, g->mode == MGADMM_TEMPORAL_BAND, g->transpose_by_gather != 0, g->hWu, g->hWd, g->hWdT};
        lds_sw = ldsplan::Switches::from_env();
        const ldsplan::Status planned = ldsplan::make(in, lds_sw, lds, img);
        if (planned == ldsplan::ROWS_DO_NOT_FIT) {
            mg_set_error("lds: row plan does not fit its launch word (%d waves)", lds.block / 64);
            return MGADMM_ERR_INVALID;
        }
        if (planned == ldsplan::NO_PLAN) return MGADMM_OK;
        MG_BUF(d_lds_csr.upload(img));
        lds_img_host = img;
        MG_BUF(d_slice_sums.reserve((size_t)T * N * ((size_t)(Bmax + 63) / 64)));
        // MGADMM_LDS_METRIC_SHAPE=<threads>x<workgroups> (workgroups 0: one task per thread): the busy shape, for experiments
        if (const char* e = getenv("MGADMM_LDS_METRIC_SHAPE")) {
            int nt = 0, wgs = 0;
            if (sscanf(e, "%dx%d", &nt, &wgs) == 2 && (nt == 64 || nt == 256 || nt == 512) && wgs >= 0) metric_busy = LdsMetricShape{nt, wgs};
        }
        MG_BUF(d_stop.upload({0}));
        MG_BUF(d_ps_ring.reserve((size_t)LDS_SETS * LDS_MAXJ * MGADMM_NMETRIC * Bp_max));
        MG_BUF(d_pstop.reserve(2 * (size_t)Bp_max + 1));
        {
            // helper stream of the overlapped outer loop: non-blocking (the caller's stream may be the legacy default stream,
            // which would serialise a blocking stream with itself), lowest priority (the k_admm_lds workgroups of the next
            // iteration take the CUs first; the one-wave workgroups of the metric kernels fill the room they leave)
            int lo = 0, hi = 0;
            MG_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
            if (const char* e = getenv("MGADMM_LDS_SIDE_PRIO")) lo = atoi(e) > 0 ? hi : lo;
            MG_HIP(hipStreamCreateWithPriority(st_side.put(), hipStreamNonBlocking, lo));
            for (auto& e : ev_main) MG_HIP(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
            for (auto& e : ev_side) MG_HIP(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
        }
        return MGADMM_OK;
    }

    // row_of_node on the device for the kernels that convert between node order and the thread-major state (nullptr: identity)
    const int* lds_row_of_node() const { return lds.row_order ? d_lds_csr.get() + lds.off_rown : nullptr; }

    int launch_lds(const LdsArgs& a, int B) {
        const bool timed = prof_open(0, 0.0);
        LdsLaunch L{lds.instance, lds.block, lds.lds_bytes, &lds_instance, &lds_unit};
        const int rc = mg_lds_iteration(L, a, B, st);
        if (timed) prof_close();
        return rc;
    }

    // ---------------------------------------------------------------- solve_lds: one solve on the LDS path
    struct LdsRun {                       // what the members below share
        ldssched::Schedule s;
        LdsArgs a;
        int B, Bp;
        bool has_phi, has_zd, record, cold;   // cold: no warm-start state
        float* xo;                        // the caller's x_out
        mgadmm_history* hist;
        int n_done = 0, rc = MGADMM_OK;
        std::vector<int> ad_bounds;       // adaptive penalties: iterations done at every step enqueued so far
    };

    // buffer of an iterate slot; slots beyond the workspace vectors are allocated here
    int lds_ring_reserve(int slots) {
        while (NRING + (int)lds_ring_extra.size() < slots) {
            DevBuf<float> b;
            MG_BUF(b.reserve(vec_elems));
            lds_ring_extra.push_back(std::move(b));
            ws_bytes += (int64_t)(vec_elems * sizeof(float));
        }
        return MGADMM_OK;
    }
    float* lds_ring(int slot) const { return slot < NRING ? vec[ring_ids[slot]] : lds_ring_extra[slot - NRING].get(); }
    // iterate k (k = 0: the initial guess)
    float* lds_xbuf(const LdsRun& r, int k) const {
        const int slot = r.s.slot_of_iterate(k);
        return slot == ldssched::X_OUT ? r.xo : lds_ring(slot);
    }

    // the part of the launch arguments that no schedule changes.  zu, zd, phi and the dual variables: workspace vectors in the
    // kernel's thread-major layout (lds_kernels.h, lds_state_index)
    void lds_fill_args(LdsRun& r, const void* y, const void* mask) const {
        LdsArgs& a = r.a;
        a = LdsArgs{};
        a.T = T; a.N = N; a.TN = T * N; a.TS = lds.TS; a.t_in = p.t_in; a.G = lds.G; a.B = r.B; a.Bp = r.Bp;
        a.nthreads = lds.nthreads; a.NR = lds.NR; a.tail_pairs = lds.tail_pairs;
        a.has_phi = r.has_phi; a.has_zd = r.has_zd;
        const LhsDef dx = lhs_def(MGADMM_LHS_X);
        a.lhsx_kind = dx.kind == 1 ? 1 : 0;
        a.cx1 = (float)dx.c1; a.cx2 = (float)dx.c2;
        a.band = g->mode == MGADMM_TEMPORAL_BAND; a.skip = g->skip;
        a.q1 = a.band ? 0 : g->q1;
        a.max_cg = p.max_cg_iter; a.record = r.record ? 1 : 0;
        a.rho = (float)p.rho; a.rho_u = (float)p.rho_u; a.rho_d = (float)p.rho_d;
        a.mu_u = (float)p.mu_u; a.mu_d1 = (float)p.mu_d1; a.mu_d2 = (float)p.mu_d2;
        a.cg_tol2 = p.cg_tol * p.cg_tol;
        a.csr = d_lds_csr.get(); a.lds_img0 = lds.lds_img0; a.lds_img_ints = lds.lds_img_ints;
        a.off_rp_u = lds.off_rp_u; a.off_rp_d = lds.off_rp_d;
        a.off_en_u = lds.off_en_u; a.off_en_d = lds.off_en_d; a.off_lead_t = lds.off_lead_t; a.off_tail_t = lds.off_tail_t; a.off_diag = lds.off_diag;
        a.npos = lds.npos_word; a.off_node = lds.off_node;
        a.band_w = g->band_w.get();
        a.zu = vec[V_ZUA]; a.zd = vec[V_ZDA]; a.phi = vec[V_PHIA];
        a.gam = vec[V_GAM]; a.gu = vec[V_GU]; a.gd = vec[V_GD];
        // staggered start (k_admm_lds): only when the launch runs several rounds of workgroups per CU
        const int ncu = dev_cus > 0 ? dev_cus : 256;
        int us = 48;
        if (const char* e = getenv("MGADMM_LDS_STAGGER_US")) us = atoi(e);
        a.stagger_wgs = ncu;
        a.stagger_ticks = (r.B >= 2 * ncu && us > 0) ? us * 100 : 0;
        a.y = (const float*)y; a.mask = (const float*)mask;
        a.alpha_hist = r.record ? d_alpha_hist.get() : nullptr; a.beta_hist = r.record ? d_beta_hist.get() : nullptr;
        a.nonfinite = d_nonfinite.get();
    }

    // iterate 0 and the state: a warm start is converted into the thread-major layout, a cold start forms ADMM.py:528-544
    int lds_state_in(const LdsRun& r, const void* x0, const mgadmm_state* si) {
        const LdsArgs& a = r.a;
        float* const x = lds_xbuf(r, 0);
        if (!si) {
            float tm, den;
            time_moments(tm, den);
            return mg_lds_init(a.mask != nullptr, T, p.t_in, N, lds.TPG, r.B, tm, den, a.y, a.mask, x, a.zu, a.zd, a.gam, a.gu, a.gd,
                               d_nonfinite.get(), lds_row_of_node(), st);
        }
        if (x0 != nullptr && x != x0) MG_HIP(hipMemcpyAsync(x, x0, (size_t)r.B * T * N * sizeof(float), hipMemcpyDeviceToDevice, st));
        auto in = [&](float* dst, const void* src) {
            return src == nullptr ? (int)MGADMM_OK : mg_lds_state_layout(true, T, N, lds.TPG, r.B, (const float*)src, dst, lds_row_of_node(), st);
        };
        MG_TRY(in(a.zu, si->zu));
        MG_TRY(in(a.gu, si->gamma_u));
        MG_TRY(in(a.zd, si->zd));            // the vectors an ablation does not iterate on are carried through
        MG_TRY(in(a.gd, si->gamma_d));
        MG_TRY(in(a.phi, si->phi));
        return in(a.gam, si->gamma);
    }
    // the state the caller asked for, in the reference's layout
    int lds_state_out(const LdsRun& r, const mgadmm_state* so) {
        const LdsArgs& a = r.a;
        auto out = [&](void* dst, const float* src) {
            return dst == nullptr ? (int)MGADMM_OK : mg_lds_state_layout(false, T, N, lds.TPG, r.B, src, (float*)dst, lds_row_of_node(), st);
        };
        MG_TRY(out(so->zu, a.zu));
        MG_TRY(out(so->zd, a.zd));
        if (r.has_phi) {
            MG_TRY(out(so->phi, a.phi));
            MG_TRY(out(so->gamma, a.gam));
        }
        MG_TRY(out(so->gamma_u, a.gu));
        return out(so->gamma_d, a.gd);
    }

    // the whole-batch metrics of iteration `it` (delta_x_per_step, norms / means over the samples) on stream `s`: two launches;
    // busy: a k_admm_lds launch runs beside them (the helper stream of CHUNKS while the caller's stream has launches left)
    int lds_batch_metrics(const LdsRun& r, int it, const double* ps, hipStream_t s, bool busy) {
        const bool per_sample = r.hist && r.hist->metrics_per_sample;
        LdsMetricArgs m;
        m.T = T; m.N = N; m.B = r.B; m.Bp = r.Bp;
        m.x = lds_xbuf(r, it + 1); m.xo = lds_xbuf(r, it);
        m.scratch = d_slice_sums.get(); m.dxps = d_dxps.get() + (size_t)it * T; m.stop = r.a.stop;
        m.ps = ps; m.out = d_hist.get() + (size_t)it * MGADMM_NMETRIC;
        m.out_ps = per_sample ? d_hist_ps.get() + (size_t)it * MGADMM_NMETRIC * r.B : nullptr;
        return mg_lds_metrics(m, busy ? metric_busy : metric_idle, s);
    }

    // The host's late look at a device word (the stop word, the number of stopped samples): after step `c` the word is copied
    // to the pinned ring, and *word is what it was after step c - LAG (0 while there is no such step): ldssched::lag_step
    int lagged_word(int c, const int* d_word, int* word) {
        const ldssched::LagStep l = ldssched::lag_step(c, LAG);
        MG_HIP(hipMemcpyAsync(h_flag.get() + 1 + l.put, d_word, sizeof(int), hipMemcpyDeviceToHost, st));
        MG_HIP(hipEventRecord(ev_ring[l.put], st));
        *word = 0;
        if (l.get >= 0) {
            MG_HIP(hipEventSynchronize(ev_ring[l.get]));
            *word = h_flag.get()[1 + l.get];
        }
        return MGADMM_OK;
    }

    // Adaptive penalties, start of a solve: every row of the table holds the records of the start weights (the per-sample
    // table where one is set, otherwise the scalars), period 0 of the history the start penalties, the later periods NaN
    int adapt_begin(LdsRun& r) {
        const int B = r.B, max_it = r.s.max_it;
        const ldsparam::Source src = wt.source(false, p);
        std::vector<LdsSampleParams> row, rec;
        ldsparam::fill_records(src, p.ablation, B, row);      // (one row: no schedule)
        rec.reserve((size_t)max_it * B);
        for (int k = 0; k < max_it; ++k) rec.insert(rec.end(), row.begin(), row.end());
        std::vector<double> w((size_t)ldsparam::NW * B);
        for (int f = 0; f < ldsparam::NW; ++f)
            for (int b = 0; b < B; ++b) w[(size_t)f * B + b] = ldsparam::weight_of(src, f, 0, b);
        const size_t hist_rows = (size_t)max_it / ad.every + 2;
        MG_BUF(d_ad_tab.upload(rec));
        MG_BUF(d_ad_w.upload(w));
        MG_BUF(d_ad_hist.reserve(hist_rows * 3 * B));
        MG_HIP(hipMemcpy(d_ad_hist.get(), w.data(), sizeof(double) * 3 * B, hipMemcpyHostToDevice));
        MG_HIP(hipMemsetAsync(d_ad_hist.get() + (size_t)3 * B, 0xFF, sizeof(double) * (hist_rows - 1) * 3 * B, st));      // (all bits set: a NaN)
        ad_last_B = B;
        return MGADMM_OK;
    }
    // after the launch whose last iteration is `it`: the step, if one follows that iteration (ldsadapt::step_after), on the
    // caller's stream; ps = the per-sample sums [NMETRIC][Bp] of iteration `it`
    int adapt_step(LdsRun& r, int it, const double* ps) {
        if (!ad_on || !ldsadapt::step_after(it, ad_start, ad.every, ad.until)) return MGADMM_OK;
        const ldsadapt::Rows rows = ldsadapt::rows_after(it, ad_start, ad.every, ad.until, r.s.max_it);
        r.ad_bounds.push_back(it + 1);
        LdsAdaptArgs k;
        k.ps = ps; k.pstop = r.a.pstop; k.w = d_ad_w.get(); k.table = d_ad_tab.get();
        k.hist = d_ad_hist.get() + r.ad_bounds.size() * 3 * (size_t)r.B;
        k.B = r.B; k.Bp = r.Bp; k.row_first = rows.first; k.row_last = rows.last;
        k.ablation = p.ablation; k.has_phi = r.has_phi; k.has_zd = r.has_zd;
        k.q = ad;
        return mg_lds_adapt(k, st);
    }

    // CHUNKS: one launch per chunk on the caller's stream; the whole-batch metrics of the chunk on the helper stream, ordered by
    // the events of lds_schedule.h (per-sample stop: one stream, no metrics, the host ends when every sample has stopped)
    int lds_run_chunks(LdsRun& r) {
        LdsArgs& a = r.a;
        const size_t row = (size_t)MGADMM_NMETRIC * r.Bp;
        int c = 0;
        for (; c < r.s.chunks(); ++c) {
            const ldssched::Chunk ch = r.s.chunk(c);
            a.first = ch.it0 == 0 && r.cold;      // phi = Ldr x0 is formed by the first iteration of a cold start
            a.J = ch.Jc;
            for (int k = 0; k <= ch.Jc; ++k) a.xs[k] = lds_xbuf(r, ch.it0 + k);
            a.cg_iters = d_cg_iters.get() + (size_t)ch.it0 * 3 * r.Bp;
            a.it0 = ch.it0;                       // (read with the per-sample stop and with a schedule of weights)
            if (r.s.per_sample) {
                a.ps = d_ps_full.get() + (size_t)ch.it0 * row;
                MG_TRY(launch_lds(a, r.B));
                MG_TRY(adapt_step(r, ch.it0 + ch.Jc - 1, a.ps + (size_t)(ch.Jc - 1) * row));      // (the sums of every iteration are kept)
                r.n_done = ch.it0 + ch.Jc;
                int stopped = 0;
                MG_TRY(lagged_word(c, a.pstop_count, &stopped));
                if (stopped == r.B) break;        // the launches enqueued since returned at their guards
                continue;
            }
            a.ps = d_ps_ring.get() + (size_t)ch.set * r.s.J * row;
            if (ch.wait >= 0) MG_HIP(hipStreamWaitEvent(st, ev_side[ch.wait], 0));
            MG_TRY(launch_lds(a, r.B));
            MG_HIP(hipEventRecord(ev_main[ch.ev], st));
            MG_HIP(hipStreamWaitEvent(st_side, ev_main[ch.ev], 0));
            // adaptive penalties: the step reads the last row of the chunk's metric set on `st`, in stream order before launch
            // c + 1; the first launch that writes the set again is launch c + 3 on the same stream, so the hazard rule of
            // lds_schedule.h holds as it stands (the metric kernels beside it only read the set)
            MG_TRY(adapt_step(r, ch.it0 + ch.Jc - 1, a.ps + (size_t)(ch.Jc - 1) * row));
            // (after the last chunk the caller's stream has nothing left: its metrics take the whole GPU)
            const bool busy = c + 1 < r.s.chunks();
            for (int k = 0; k < ch.Jc; ++k) MG_TRY(lds_batch_metrics(r, ch.it0 + k, a.ps + (size_t)k * row, st_side, busy));
            MG_HIP(hipEventRecord(ev_side[ch.ev], st_side));
            r.n_done = ch.it0 + ch.Jc;
        }
        if (!r.s.per_sample && r.s.join(c) >= 0) MG_HIP(hipStreamWaitEvent(st, ev_side[r.s.join(c)], 0));
        return MGADMM_OK;
    }

    // SYNC and DEVSTOP: one iteration per launch, everything on the caller's stream
    int lds_run_steps(LdsRun& r) {
        LdsArgs& a = r.a;
        const size_t K = p.max_cg_iter;
        for (int it = 0; it < r.s.max_it; ++it) {
            a.first = it == 0 && r.cold;          // phi = Ldr x0 is formed by the first launch of a cold start
            a.J = 1;
            a.xs[0] = lds_xbuf(r, it); a.xs[1] = lds_xbuf(r, it + 1);
            a.cg_iters = d_cg_iters.get() + (size_t)it * 3 * r.Bp;
            a.ps = d_ps.get();
            a.it0 = it;                           // (read with the per-sample stop and with a schedule of weights)
            if (r.s.per_sample) a.ps = d_ps_full.get() + (size_t)it * MGADMM_NMETRIC * r.Bp;
            if (r.record) {
                MG_TRY(fill(d_alpha_hist.get(), 3 * K * r.Bp, (float)NAN));
                MG_TRY(fill(d_beta_hist.get(), 3 * K * r.Bp, (float)NAN));
            }
            MG_TRY(launch_lds(a, r.B));
            MG_TRY(adapt_step(r, it, a.ps));
            if (!r.s.per_sample) MG_TRY(lds_batch_metrics(r, it, a.ps, st, false));
            if (r.record) {
                for (int w = 0; w < 3; ++w)
                    if (w < 2 || r.has_zd) MG_TRY(save_coeffs(r.Bp, r.hist, it, w, r.B, w));
            }
            r.n_done = it + 1;
            if (r.s.per_sample) {         // (the host is in step with the device here: the count of this very launch)
                MG_HIP(hipMemcpyAsync(h_flag.get() + 1, a.pstop_count, sizeof(int), hipMemcpyDeviceToHost, st));
                MG_HIP(hipStreamSynchronize(st));
                if (h_flag.get()[1] == r.B) break;
            } else if (r.s.kind == ldssched::DEVSTOP) {
                int sw = 0;
                MG_TRY(mg_lds_stop_test(d_hist.get() + (size_t)it * MGADMM_NMETRIC, d_nonfinite.get(), r.has_phi, r.has_zd, p.admm_tol, it, d_stop.get(), st));
                MG_TRY(lagged_word(it, d_stop.get(), &sw));
                if (sw != 0) break;       // the launches enqueued since returned at their guards
            } else if (p.check_stop) {
                bool stop = false;
                MG_TRY(host_stop_test(it, r.has_phi, r.has_zd, &stop, &r.rc));
                if (stop) break;
            }
        }
        if (r.s.kind == ldssched::DEVSTOP) {
            // the stop word after everything enqueued has run: 0 = no stop (all enqueued iterations ran), k > 0 = the stop
            // test passed at the end of iteration k - 1, k < 0 = iteration -k - 1 met a NaN / Inf
            MG_HIP(hipMemcpyAsync(h_flag.get() + 1, d_stop.get(), sizeof(int), hipMemcpyDeviceToHost, st));
            MG_HIP(hipStreamSynchronize(st));
            const int sw = h_flag.get()[1];
            if (sw > 0) r.n_done = sw;
            else if (sw < 0) { r.n_done = -sw; r.rc = MGADMM_ERR_NONFINITE; }
        }
        return MGADMM_OK;
    }

    // per-sample stop: r.n_done iterations were enqueued; the history from the stop words and the per-sample sums, the
    // iterations of every sample to `nps`, the largest of them to r.n_done
    int lds_finish_per_sample(LdsRun& r, std::vector<int>& nps) {
        int* const d_nps = d_pstop.get() + Bp_max + 1;
        MG_TRY(mg_lds_ps_history(d_ps_full.get(), d_pstop.get(), r.n_done, r.s.max_it, r.B, r.Bp, d_nps, d_hist.get(),
                                 (r.hist && r.hist->metrics_per_sample) ? d_hist_ps.get() : nullptr, st));
        nps.resize(r.B);
        MG_HIP(hipMemcpyAsync(nps.data(), d_nps, sizeof(int) * r.B, hipMemcpyDeviceToHost, st));
        MG_HIP(hipStreamSynchronize(st));
        r.n_done = *std::max_element(nps.begin(), nps.end());
        return MGADMM_OK;
    }

    int solve_lds(const void* y, const void* mask, int B, const void* x0, const mgadmm_state* state_in, void* x_out,
                  const mgadmm_state* state_out, mgadmm_history* hist) override {
        LdsRun r;
        r.B = B; r.Bp = (B + 63) / 64 * 64;
        r.has_phi = has_phi(); r.has_zd = has_zd();
        r.record = p.record_cg_coeffs && hist && hist->cg_alpha && hist->cg_beta;
        r.cold = !state_in;
        r.hist = hist;
        // The caller's output buffers ARE the working state of this path (same (B, T*N) layout): no copy-out at the end
        // (round 2 until here: seven 120 MB device copies per solve at cfg2 = 0.7 ms of a 59 ms solve).  The iterates are
        // assigned to buffers so that the one of the LAST iteration lands in x_out (an early stop on another buffer
        // costs one copy).  Outputs must not alias y / mask (mgadmm.h).
        r.xo = static_cast<float*>(x_out);
        r.s = ldssched::Schedule::pick(lds_async != 0, r.record, p.check_stop != 0, p.admm_convergence == MGADMM_ADMM_PER_SAMPLE,
                                       ad_on ? ldsadapt::adapt_J(ad.every, std::max(1, std::min(lds_chunk, LDS_MAXJ))) : lds_chunk,
                                       p.max_admm_iter);
        const ldssched::Schedule& s = r.s;
        const bool chunked = s.kind == ldssched::CHUNKS;
        MG_TRY(ensure_hist_ps(hist, B));
        MG_HIP(hipMemsetAsync(d_nonfinite.get(), 0, sizeof(int), st));
        MG_HIP(hipMemsetAsync(d_ps.get(), 0, sizeof(double) * MGADMM_NMETRIC * r.Bp, st));
        MG_HIP(hipMemsetAsync(d_cg_iters.get(), 0, sizeof(int) * (size_t)s.max_it * 3 * r.Bp, st));
        if (s.per_sample) {
            MG_BUF(d_ps_full.reserve((size_t)s.max_it * MGADMM_NMETRIC * r.Bp));
            MG_HIP(hipMemsetAsync(d_pstop.get(), 0, sizeof(int) * ((size_t)Bp_max + 1), st));
        }
        MG_TRY(lds_ring_reserve(s.slots()));
        lds_fill_args(r, y, mask);
        MG_TRY(lds_state_in(r, x0, state_in));
        if (s.kind == ldssched::DEVSTOP) {
            r.a.stop = d_stop.get();
            MG_HIP(hipMemsetAsync(d_stop.get(), 0, sizeof(int), st));
        }
        if (chunked && !s.per_sample) MG_HIP(hipMemsetAsync(d_ps_ring.get(), 0, sizeof(double) * LDS_SETS * s.J * MGADMM_NMETRIC * r.Bp, st));
        if (s.per_sample) {
            r.a.pstop = d_pstop.get(); r.a.pstop_count = d_pstop.get() + Bp_max; r.a.x_final = r.xo; r.a.admm_tol = p.admm_tol;
        }
        if (sg_B > 0) {                   // (B == sg_B: solve_gate) workgroup b reads the image of set d_sg_set[b]
            r.a.csr = d_sg_img.get(); r.a.img_stride = ldssets::img_stride(lds); r.a.gset = d_sg_set.get();
        }
        // the table of records the launches read (with one they take the kernels k_admm_lds_pp); trip k of a launch reads
        // row sched_row(it0 + k, sp_row0, sp_rows) of it
        if (bs.B > 0) {                   // (B == bs.B: bandsets::solve_gate) workgroup b reads the band table of set d_bs_set[b]
            r.a.band_w = d_bs_w.get(); r.a.bset = d_bs_set.get();
        }
        const solvegate::TableChoice tc = bandsets::table_of(solvegate::table_of(set_state(), wt.sch_row0, s.max_it), bs);
        if (tc.scalar_records) MG_TRY(upload_sample_params(B));      // (a graph or band table without a weights table)
        switch (tc.table) {
            case solvegate::TABLE_NONE: break;
            case solvegate::TABLE_SAMPLE: r.a.sp = d_sp.get(); break;      // (B == sp_B: solve_gate)
            case solvegate::TABLE_SCHEDULE: MG_TRY(upload_param_schedule(B)); r.a.sp = d_sch.get(); break;
            case solvegate::TABLE_ADAPTIVE: MG_TRY(adapt_begin(r)); r.a.sp = d_ad_tab.get(); break;      // the steps between the launches write it
        }
        r.a.sp_rows = tc.sp_rows; r.a.sp_row0 = tc.sp_row0; r.a.sp_stride = tc.stride_B ? B : 0;
        MG_TRY(chunked ? lds_run_chunks(r) : lds_run_steps(r));
        std::vector<int> nps;         // per-sample stop: iterations of every sample
        if (s.per_sample) MG_TRY(lds_finish_per_sample(r, nps));
        if (ad_on)      // periods of the history: the start values and the steps that followed an iteration some sample ran
            ad_last_periods = 1 + (int)std::count_if(r.ad_bounds.begin(), r.ad_bounds.end(), [&](int n) { return n <= r.n_done; });
        // (per-sample stop: a stopped sample stored x_out[b] itself, the others ran max_it iterations and their last iterate is x_out)
        float* const xc = s.per_sample ? r.xo : lds_xbuf(r, r.n_done);
        if (xc != r.xo)       // early stop on another buffer
            MG_HIP(hipMemcpyAsync(x_out, xc, (size_t)B * T * N * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (state_out) MG_TRY(lds_state_out(r, state_out));
        return finish_history(hist, r.n_done, B, r.Bp, r.rc, s.per_sample ? nps.data() : nullptr);
    }
};

}  // namespace
