// Adaptive ADMM penalties on the LDS-resident path (mgadmm_solver_set_adaptive_rho): residual balancing (Boyd et al.,
// "Distributed optimization and statistical learning via ADMM", section 3.4.1) of rho, rho_u and rho_d per sample, applied
// at launch boundaries by k_lds_adapt (lds_launch.hip), which writes the rows of the weight table (lds_param_table.h) the
// next launches of k_admm_lds_pp read.  This header holds the rule and the planning: plain C++ like lds_param_table.h, no
// HIP header and no environment reads; compiled into libmgadmm.so (Engine, k_lds_adapt) and into the CPU check
// tests/cpu/lds_adapt_check.cpp.
//
// The pairs: (PRI_ZU, DUAL_ZU) -> rho_u, (PRI_PHI, DUAL_PHI) -> rho, (PRI_ZD, DUAL_ZD) -> rho_d; the sums are the SQUARES
// the kernels store (metrics_per_sample).  The reference's dual residuals are unscaled (||z - z_old||, ADMM.py:618, 630, 636),
// so the rule scales them by the current penalty itself.  For phi the surrogate rho ||phi - phi_old|| stands for the dual
// residual rho ||Ldr^T (phi - phi_old)||: the kernels do not form Ldr^T of the difference, and the rule compares orders
// of magnitude (mu), which a factor of the size of ||Ldr|| does not change in kind.
//
// Arithmetic: double multiplications, comparisons and selects only, in the written order -- no division, nothing a
// compiler could contract into a multiply-add -- so the host, the device and a numpy restatement agree bit for bit.
#pragma once
#include <cstdio>
#include <string>

#include "lds_consts.h"        // LDS_MAXJ
#include "lds_param_table.h"   // MG_HD, ldsparam::NW, record_of

namespace ldsadapt {

// order of the three penalties everywhere in this header: the first three weights of lds_param_table.h
enum { RHO = 0, RHO_U = 1, RHO_D = 2 };

struct Params {
    int every = 0;         // an adaptation step follows every `every`-th iteration (counted over resumed solves: `start`)
    int until = 0;         // no step after global iteration count `until`; 0: no limit
    double mu = 0, tau = 0;
    double tau_inv = 0;    // 1.0 / tau, formed once by the host
    double rho_min[3] = {0, 0, 0}, rho_max[3] = {0, 0, 0};
};

// one pair: penalty r, primal and (unscaled) dual residual sums, squared
MG_HD inline double balance(double r, double pri2, double dual2, double mu, double tau, double tau_inv, double lo, double hi) {
    const double s2 = r * r * dual2;
    const double m2 = mu * mu;
    if (pri2 > m2 * s2) {
        const double up = r * tau;
        return up < hi ? up : hi;
    }
    if (s2 > m2 * pri2) {
        const double down = r * tau_inv;
        return down > lo ? down : lo;
    }
    return r;              // balanced, or a NaN / 0 on both sides: neither comparison holds
}

// w[0 .. 2] = rho, rho_u, rho_d, updated in place; res = the six sums PRI_ZU, DUAL_ZU, PRI_PHI, DUAL_PHI, PRI_ZD, DUAL_ZD of one
// iteration.  A pair the ablation does not iterate on is left alone
MG_HD inline void step(double w[3], const double res[6], int has_phi, int has_zd, const Params& q) {
    w[RHO_U] = balance(w[RHO_U], res[0], res[1], q.mu, q.tau, q.tau_inv, q.rho_min[RHO_U], q.rho_max[RHO_U]);
    if (has_phi) w[RHO] = balance(w[RHO], res[2], res[3], q.mu, q.tau, q.tau_inv, q.rho_min[RHO], q.rho_max[RHO]);
    if (has_zd) w[RHO_D] = balance(w[RHO_D], res[4], res[5], q.mu, q.tau, q.tau_inv, q.rho_min[RHO_D], q.rho_max[RHO_D]);
}

// ---------------------------------------------------------------- planning
// iterations per launch: the largest J <= chunk_request that divides `every`, so that every step falls on a launch boundary
constexpr int adapt_J(int every, int chunk_request) {
    int j = chunk_request < every ? chunk_request : every;
    if (j < 1) j = 1;
    while (every % j != 0) --j;
    return j;
}

// is iteration `it` of a solve that starts at global iteration `start` followed by an adaptation step?
constexpr bool step_after(int it, int start, int every, int until) {
    return (start + it + 1) % every == 0 && (until <= 0 || start + it + 1 <= until);
}

// rows [first, last) of a table of max_it rows (row = iteration of the solve) the step after iteration `it` writes: the
// next period, clamped to the table; after the last step of the solve's range every row up to the end
struct Rows { int first, last; };
constexpr Rows rows_after(int it, int start, int every, int until, int max_it) {
    return {it + 1 < max_it ? it + 1 : max_it,
            (it + 1 + every < max_it && step_after(it + every, start, every, until)) ? it + 1 + every : max_it};
}

// false: `why` names the offending parameter
inline bool validate(const Params& q, int start, std::string& why) {
    char buf[200];
    buf[0] = 0;
    static const char* const names[3] = {"rho", "rho_u", "rho_d"};
    if (q.every < 1 || q.every > LDS_MAXJ) snprintf(buf, sizeof(buf), "adaptive_rho: every = %d outside [1, %d]", q.every, LDS_MAXJ);
    else if (q.until < 0) snprintf(buf, sizeof(buf), "adaptive_rho: until = %d is negative (0: no limit)", q.until);
    else if (!(q.mu > 1.0) || !(q.mu < 1e150)) snprintf(buf, sizeof(buf), "adaptive_rho: mu = %g, should be > 1 (and < 1e150)", q.mu);
    else if (!(q.tau > 1.0) || !(q.tau < 1e150)) snprintf(buf, sizeof(buf), "adaptive_rho: tau = %g, should be > 1 (and < 1e150)", q.tau);
    else if (start < 0) snprintf(buf, sizeof(buf), "adaptive_rho: start = %d is negative", start);
    else if (start % q.every != 0) snprintf(buf, sizeof(buf), "adaptive_rho: start = %d is no multiple of every = %d", start, q.every);
    else
        for (int f = 0; f < 3 && !buf[0]; ++f)
            if (!(q.rho_min[f] > 0.0) || !(q.rho_min[f] <= q.rho_max[f]) || !(q.rho_max[f] < 1e300))
                snprintf(buf, sizeof(buf), "adaptive_rho: rho_min[%s] = %g, rho_max[%s] = %g, should be 0 < rho_min <= rho_max (finite)",
                         names[f], q.rho_min[f], names[f], q.rho_max[f]);
    if (!buf[0]) return true;
    why = buf;
    return false;
}

}  // namespace ldsadapt
