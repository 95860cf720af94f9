// Constants of the LDS-resident path shared by the kernels' launch interface (lds_args.h) and the host-only planner
// (lds_plan.h).  Plain C++, no HIP.
#pragma once
#include <cstdint>

// entries of a W_d^T row that k_admm_lds keeps in registers during a CG solve (the rest of the row: the padded tail table)
constexpr int LDS_NLEAD = 5;
// most ADMM iterations one k_admm_lds launch runs (LdsArgs::J; the x pointer table has one entry more)
constexpr int LDS_MAXJ = 16;

// The template arguments of a k_admm_lds instance packed into one word: what the planner chooses, what lds_dispatch.h
// launches by and what MGADMM_Q_LDS_INSTANCE reports (mgadmm/_lib.py, decode_lds_instance)
constexpr int64_t lds_instance_key(int tpg, bool band, int maxt, bool sb, int nu, int nd, bool slots, int tp) {
    return tpg | (int64_t)band << 8 | (int64_t)sb << 9 | (int64_t)slots << 10 | (int64_t)nu << 11 | (int64_t)nd << 16 |
           (int64_t)maxt << 21 | (int64_t)(tp + 1) << 32;
}
