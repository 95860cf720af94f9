// Choice of the k_admm_lds instance for a launch.  Included by lds_launch.hip (the kernels k_admm_lds) and by lds_launch_ps.hip
// (the same instances with the per-sample stop test, k_admm_lds_ps: lds_kernels.h, MGADMM_LDS_PER_SAMPLE_STOP): two
// translation units that compile side by side.
#pragma once
#include <mutex>
#include <utility>
#include <vector>

#include <cstdint>
#include "lds_kernels.h"

#ifndef MG_LDS_UNIT
#error "MG_LDS_UNIT: the translation unit that includes lds_dispatch.h says which kernels it compiles (MGADMM_Q_LDS_UNIT)"
#endif

namespace {

std::mutex g_attr_mu;
std::vector<std::pair<const void*, int>> g_attr_done;     // (kernel, device) pairs whose dynamic-LDS limit has been raised

int allow_lds(const void* fn, int bytes) {
    int dev = 0;
    MG_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_attr_mu);
    for (auto& e : g_attr_done)
        if (e.first == fn && e.second == dev) return MGADMM_OK;
    MG_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));   // a per-DEVICE property
    g_attr_done.push_back({fn, dev});
    return MGADMM_OK;
}

// The instances the library ships, as the template arguments <TPG, BAND, MAXT, SB, NU, ND, SLOTS, TP> of k_admm_lds
// (lds_kernels.h; tests/lds_census.py holds a problem for each).  Generic instances (ragged rows or band mode): every width
// in the 1024-thread class, width 12 also in the 640-thread class; a single LDS vector (SB) for 12 / 640 and 8 / 1024.
// Uniform-row instances (4 entries per W_u row, 5 per W_d row): widths 8 and 12, the pair count TP of the W_d^T tail table
// a compile-time constant up to 3 pairs (-1: longer tails, pair count at run time), with and without slot vectors --
// without only in the 1024-thread class of width 12 (342 .. 512 nodes in two time groups), which has no room for them.
#define MG_LDS_GENERIC(X, TPG, MAXT, SB) X(TPG, false, MAXT, SB, 0, 0, false, -1) X(TPG, true, MAXT, SB, 0, 0, false, -1)
#define MG_LDS_UNIFORM(X, TPG, MAXT, SLOTS) \
    X(TPG, false, MAXT, false, 4, 5, SLOTS, 0) X(TPG, false, MAXT, false, 4, 5, SLOTS, 1) X(TPG, false, MAXT, false, 4, 5, SLOTS, 2) \
    X(TPG, false, MAXT, false, 4, 5, SLOTS, 3) X(TPG, false, MAXT, false, 4, 5, SLOTS, -1)
#define MG_LDS_INSTANCES(X) \
    MG_LDS_GENERIC(X, 1, 1024, false) MG_LDS_GENERIC(X, 2, 1024, false) MG_LDS_GENERIC(X, 3, 1024, false) MG_LDS_GENERIC(X, 4, 1024, false) \
    MG_LDS_GENERIC(X, 6, 1024, false) MG_LDS_GENERIC(X, 8, 1024, false) MG_LDS_GENERIC(X, 12, 1024, false) MG_LDS_GENERIC(X, 12, 640, false) \
    MG_LDS_GENERIC(X, 12, 640, true) MG_LDS_GENERIC(X, 8, 1024, true) \
    MG_LDS_UNIFORM(X, 8, 1024, false) MG_LDS_UNIFORM(X, 8, 1024, true) MG_LDS_UNIFORM(X, 12, 640, false) MG_LDS_UNIFORM(X, 12, 640, true) \
    MG_LDS_UNIFORM(X, 12, 1024, false)

template <int TPG, bool BAND, int MAXT, bool SB, int NU, int ND, bool SLOTS, int TP>
int launch(const LdsLaunch& L, const LdsArgs& a, int B, hipStream_t st) {
    auto fn = MG_LDS_KERNEL<TPG, BAND, MAXT, SB, NU, ND, SLOTS, TP>;
    MG_TRY(allow_lds((const void*)fn, 160 * 1024));
    hipLaunchKernelGGL(fn, dim3(B), dim3(L.block), L.lds_bytes, st, a);
    MG_HIP(hipGetLastError());
    if (L.instance) *L.instance = lds_instance_key(TPG, BAND, MAXT, SB, NU, ND, SLOTS, TP);   // which instance ran (tests: the instance census)
    if (L.unit) *L.unit = MG_LDS_UNIT;      // ... of which translation unit (defined beside MG_LDS_KERNEL by the file that includes this one)
    return MGADMM_OK;
}

// the instance of this translation unit's kernel for a plan
int lds_dispatch(const LdsLaunch& L, const LdsArgs& a, int B, hipStream_t st) {
    if (a.J < 1 || a.J > LDS_MAXJ || a.NR * 1 < a.N || L.block - a.nthreads != a.NR - a.N) {
        mg_set_error("lds: launch geometry (J %d, rows %d for %d nodes, %d of %d threads own elements)", a.J, a.NR, a.N, a.nthreads, L.block);
        return MGADMM_ERR_INVALID;
    }
    switch (L.key) {
#define MG_LDS_CASE(...) case lds_instance_key(__VA_ARGS__): return launch<__VA_ARGS__>(L, a, B, st);
        MG_LDS_INSTANCES(MG_LDS_CASE)
#undef MG_LDS_CASE
    }
    const int64_t k = L.key;        // the planner asked for a combination that is not shipped
    mg_set_error("lds: no k_admm_lds instance for <TPG %d, band %d, MAXT %d, SB %d, NU %d, ND %d, slots %d, TP %d>", (int)(k & 0xFF),
                 (int)(k >> 8 & 1), (int)(k >> 21 & 0x7FF), (int)(k >> 9 & 1), (int)(k >> 11 & 0x1F), (int)(k >> 16 & 0x1F),
                 (int)(k >> 10 & 1), (int)(k >> 32 & 0xFF) - 1);
    return MGADMM_ERR_UNSUPPORTED;
}

}  // namespace
