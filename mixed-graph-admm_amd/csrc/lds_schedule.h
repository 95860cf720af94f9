// Schedule of the ADMM outer loop of the LDS-resident path (Engine::solve_lds): which schedule a solve takes, which buffer
// holds iterate k, which metric set and which events a chunk uses, and the ring behind the host's late look at a device
// word.  Plain C++, no HIP, no environment: tests/cpu/lds_schedule_check.cpp replays it on the CPU.
//
// The outer loop (ADMM.py:546-646) is one loop with the stop test at its end.  A solve takes one of
//   SYNC     (MGADMM_LDS_ASYNC=0, or the CG coefficients are recorded: the host copies them out per iteration)
//            one stream, the host reads the metrics of an iteration and tests the stop criterion before it enqueues the next;
//   DEVSTOP  (check_stop) one stream, the stop test runs on the device (k_lds_stop_test sets the stop word, every later
//            launch returns at its guard), the host enqueues iterations ahead and looks at the word LAG iterations late:
//            same iterates and history, no host round trip per iteration;
//   CHUNKS   (fixed iteration count) one k_admm_lds launch runs a CHUNK of J iterations on every sample (the workgroup keeps
//            its sample: see the kernel); every iterate x_k goes to a buffer of its own, and the whole-batch metric kernels
//            of a chunk (delta_x_per_step re-reads x_k and x_{k+1} of the batch, 241 MB per iteration at cfg2) run on a
//            helper stream beside the launch of the next chunks, which leaves HBM idle.  J = 1 is the overlapped
//            one-iteration-per-launch schedule of round 2.
// Per-sample stop (MGADMM_ADMM_PER_SAMPLE with check_stop): the test runs INSIDE k_admm_lds, after every iteration of a
// launch, on the sample the workgroup owns -- it needs nothing from outside the workgroup.  So the solve takes the CHUNKS
// schedule (SYNC when the CG coefficients are recorded): a sample that stops writes x_out[b] itself and sets its stop word,
// its workgroup returns at the guard of every later launch; the host reads the number of stopped samples LAG launches late
// and ends when it equals B.  The per-sample sums of every iteration go to a buffer of their own (no metric sets, no helper
// stream, no events); delta_x_per_step is not formed; the whole-batch history is made at the end (k_lds_ps_history).
//
// Buffers of CHUNKS: the iterates at chunk boundaries (k = c J) rotate through LDS_NBOUND = 4 buffers, the J - 1 iterates
// inside a chunk and the per-sample metric sums of a chunk through LDS_SETS = 3 sets; the iterate of the LAST iteration is
// the caller's x_out in every schedule.  Hazard rule: the metric kernels of chunk c read its J + 1 iterates and its metric
// set on the helper stream; the first launch that writes any of them again is launch c + 3 (interior set and metric set
// c % 3; its last boundary buffer (c + 4) % 4 is the start of chunk c), so LAUNCH c WAITS FOR THE METRICS OF CHUNK c - 3,
// and an event slot (c % 4) is recorded again only after every wait that names it has been issued.  Two sets / three boundary
// buffers (until the end of round 3) made launch c wait for the metrics of chunk c - 2, which run BESIDE launch c - 1 and
// get CU slots only when it drains: 0.45 ms between two 26 ms launches (profiles/r03/cfg2_iteration_timeline.txt).
#pragma once
#include "lds_consts.h"

constexpr int LDS_SETS = 3;     // interior iterate-buffer sets / per-sample metric sets of CHUNKS (chunks in flight)
constexpr int LDS_NBOUND = 4;   // iterate buffers at the chunk boundaries; event slots of either stream

namespace ldssched {

enum Kind { SYNC, DEVSTOP, CHUNKS };
constexpr int X_OUT = -1;       // slot_of_iterate: the caller's x_out

struct Chunk {
    int it0, Jc;      // first iteration and length: the launch reads iterate it0 and writes it0 + 1 .. it0 + Jc
    int set;          // metric set the launch writes and the chunk's metric kernels read
    int ev;           // event slot recorded after the launch (ev_main) and after its metrics (ev_side)
    int wait;         // ev_side slot the launch waits on first, -1: none
};

struct Schedule {
    Kind kind;
    bool per_sample;  // the stop test runs per sample inside the kernel
    int J, max_it;    // iterations per launch (1 unless CHUNKS), iterations of the solve

    static Schedule pick(bool async, bool record, bool check_stop, bool per_sample_conv, int chunk_request, int max_it) {
        Schedule s;
        s.per_sample = per_sample_conv && check_stop;
        s.kind = (!async || record) ? SYNC : ((check_stop && !s.per_sample) ? DEVSTOP : CHUNKS);
        int j = chunk_request < LDS_MAXJ ? chunk_request : LDS_MAXJ;
        if (j > max_it) j = max_it;
        s.J = s.kind == CHUNKS && j > 1 ? j : 1;
        s.max_it = max_it;
        return s;
    }
    // iterate buffers in use; the engine maps a slot number to a buffer
    int slots() const { return kind == CHUNKS ? LDS_SETS * (J - 1) + LDS_NBOUND : 2; }
    // iterate k (k = 0: the initial guess) lives in this slot
    int slot_of_iterate(int k) const {
        if (k == max_it) return X_OUT;
        if (kind != CHUNKS) return k & 1;
        if (k % J == 0) return (k / J) % LDS_NBOUND;                                  // chunk boundary
        return LDS_NBOUND + ((k / J) % LDS_SETS) * (J - 1) + (k % J - 1);             // inside chunk k / J
    }
    int chunks() const { return (max_it + J - 1) / J; }
    Chunk chunk(int c) const {
        const int it0 = c * J, left = max_it - it0;
        return {it0, J < left ? J : left, c % LDS_SETS, c % LDS_NBOUND, c >= LDS_SETS ? (c - LDS_SETS) % LDS_NBOUND : -1};
    }
    // ev_side slot the caller's stream waits on after `n` chunks (the helper stream runs in order: the last event covers all)
    static int join(int n) { return n > 0 ? (n - 1) % LDS_NBOUND : -1; }
};

// The host looks at a device word `lag` steps late: after step c the word is copied to pinned slot `put` and event `put` is
// recorded; the host then waits for event `get` (step c - lag) and reads pinned slot `get`; -1: nothing to read yet
struct LagStep { int put, get; };
constexpr LagStep lag_step(int c, int lag) { return {c % (lag + 1), c >= lag ? (c - lag) % (lag + 1) : -1}; }

}  // namespace ldssched
