// CPU check of the owning buffer of the engines (mixed-graph-admm_amd/csrc/dev_buf.h) over a counting memory policy backed
// by malloc / free that fails its n-th allocation or its n-th copy on request.  Built with AddressSanitizer + UBSan: a block
// released twice, used after its release or never released ends the program (LeakSanitizer at exit).
//   dev_buf_check            runs the checks, prints one JSON object, exit status 1 on the first failure
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "dev_buf.h"

static int n_checks = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        ++n_checks;                                                        \
        if (!(cond)) {                                                     \
            fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond);    \
            return 1;                                                      \
        }                                                                  \
    } while (0)

struct TestMem {
    static int live, allocs, copies, releases, refused;      // blocks alive; calls made so far; allocations refused on request
    static int fail_alloc, fail_copy;               // the n-th call from now fails (1 = the next); 0 = none
    static constexpr int ERR_ALLOC = 2, ERR_COPY = 719;
    static int calls() { return allocs + copies + releases; }
    static int alloc(void** p, size_t bytes) {
        ++allocs;
        if (fail_alloc > 0 && --fail_alloc == 0) { ++refused; return ERR_ALLOC; }
        *p = malloc(bytes);
        memset(*p, 0xAB, bytes);      // (a fresh block never looks like the old contents)
        ++live;
        return 0;
    }
    static int to_device(void* dst, const void* src, size_t bytes) {
        ++copies;
        if (fail_copy > 0 && --fail_copy == 0) return ERR_COPY;
        memcpy(dst, src, bytes);
        return 0;
    }
    static void release(void* p) {
        ++releases;
        --live;
        free(p);
    }
};
int TestMem::live = 0, TestMem::refused = 0, TestMem::allocs = 0, TestMem::copies = 0, TestMem::releases = 0, TestMem::fail_alloc = 0, TestMem::fail_copy = 0;

template <class T> using TBuf = Buf<T, TestMem>;
static_assert(!std::is_copy_constructible<TBuf<int>>::value && !std::is_copy_assignable<TBuf<int>>::value, "Buf is not copyable");
static_assert(std::is_nothrow_move_constructible<TBuf<int>>::value && std::is_nothrow_move_assignable<TBuf<int>>::value, "Buf is movable");

// The history buffers of an engine as Engine::alloc_iter_dependent reserves them: d_nact [K], d_alpha_hist [3 K Bp],
// d_cg_iters [I 3 Bp]; the error code of the first failure comes back, the buffers before it have grown
struct Histories {
    static constexpr size_t Bp = 64;
    TBuf<int> nact;
    TBuf<float> alpha;
    TBuf<int> cg_iters;
    int reserve(size_t K, size_t I) {
        if (int e = nact.reserve(K)) return e;
        if (int e = alpha.reserve(3 * K * Bp)) return e;
        return cg_iters.reserve(I * 3 * Bp);
    }
    // every buffer covers what its capacity claims: written end to end (AddressSanitizer watches the block's bounds)
    bool touch() {
        if (!nact || !alpha || !cg_iters) return false;
        memset(nact.get(), 0, nact.capacity() * sizeof(int));
        memset(alpha.get(), 0, alpha.capacity() * sizeof(float));
        memset(cg_iters.get(), 0, cg_iters.capacity() * sizeof(int));
        return true;
    }
    bool holds(size_t K, size_t I) const { return nact.capacity() >= K && alpha.capacity() >= 3 * K * Bp && cg_iters.capacity() >= I * 3 * Bp; }
};

// LdsEngine::set_sample_graphs: the new table is uploaded into a local buffer and moved into the member after the steps that
// can still fail (`later` is their status); an early return releases the local block
static int stage_table(TBuf<int>& member, const std::vector<int>& table, int later) {
    TBuf<int> fresh;
    if (int e = fresh.upload(table)) return e;
    if (later) return later;
    member = std::move(fresh);
    return 0;
}

int main() {
    typedef TestMem M;
    // --- scope: the destructor releases; an empty buffer makes no call
    {
        TBuf<int> e;
        CHECK(!e && e.get() == nullptr && e.capacity() == 0);
    }
    CHECK(M::calls() == 0);
    {
        TBuf<double> b;
        CHECK(b.reserve(10) == 0 && b && b.capacity() == 10 && M::live == 1);
        b.get()[9] = 1.0;
    }
    CHECK(M::live == 0 && M::allocs == 1 && M::releases == 1);

    // --- a move transfers the block and leaves the source empty
    {
        TBuf<int> a;
        CHECK(a.reserve(4) == 0);
        int* const blk = a.get();
        TBuf<int> b(std::move(a));
        CHECK(b.get() == blk && b.capacity() == 4 && !a && a.capacity() == 0 && M::live == 1);
        TBuf<int> c;
        CHECK(c.reserve(2) == 0 && M::live == 2);
        c = std::move(b);                 // the target's own block is released
        CHECK(c.get() == blk && c.capacity() == 4 && !b && b.capacity() == 0 && M::live == 1);
        std::vector<TBuf<int>> ring;      // (the extra iterate buffers of the LDS path live in a vector)
        ring.push_back(std::move(c));
        for (int i = 0; i < 5; ++i) { TBuf<int> x; CHECK(x.reserve(3) == 0); ring.push_back(std::move(x)); }
        CHECK(ring[0].get() == blk && !c && M::live == 6);
    }
    CHECK(M::live == 0);

    // --- reserve at or below the capacity: no call of Mem
    {
        TBuf<int> a;
        CHECK(a.reserve(8) == 0);
        const int before = M::calls();
        int* const blk = a.get();
        CHECK(a.reserve(8) == 0 && a.reserve(3) == 0 && a.reserve(0) == 0);
        CHECK(M::calls() == before && a.get() == blk && a.capacity() == 8);
    }
    CHECK(M::live == 0);

    // --- a failed growing reserve: pointer, capacity and contents as they were; the next one succeeds
    {
        TBuf<int> a;
        CHECK(a.upload({1, 2, 3, 4}) == 0);
        int* const blk = a.get();
        M::fail_alloc = 1;
        CHECK(a.reserve(100) == M::ERR_ALLOC);
        CHECK(a.get() == blk && a.capacity() == 4 && M::live == 1);
        CHECK(a.get()[0] == 1 && a.get()[3] == 4);
        CHECK(a.reserve(100) == 0 && a.capacity() == 100 && M::live == 1);      // (the old block went after the new one came)
        a.get()[99] = 7;
        TBuf<int> e;                      // ... and on an empty buffer: still empty
        M::fail_alloc = 1;
        CHECK(e.reserve(5) == M::ERR_ALLOC && !e && e.capacity() == 0);
    }
    CHECK(M::live == 0);

    // --- upload: a failed copy keeps the old block and leaks nothing
    {
        TBuf<int> a;
        CHECK(a.upload({5, 6}) == 0 && a.capacity() == 2);
        int* const blk = a.get();
        M::fail_copy = 1;
        CHECK(a.upload({1, 2, 3, 4, 5, 6}) == M::ERR_COPY);      // has to grow: the copy into the new block fails
        CHECK(a.get() == blk && a.capacity() == 2 && a.get()[0] == 5 && a.get()[1] == 6 && M::live == 1);
        M::fail_alloc = 1;
        CHECK(a.upload({1, 2, 3}) == M::ERR_ALLOC && a.get() == blk && a.capacity() == 2 && M::live == 1);
        M::fail_copy = 1;
        CHECK(a.upload({9}) == M::ERR_COPY);                     // fits: pointer and capacity stay
        CHECK(a.get() == blk && a.capacity() == 2 && M::live == 1);
        CHECK(a.upload({1, 2, 3}) == 0 && a.capacity() == 3 && a.get()[2] == 3 && M::live == 1);
        const int allocs = M::allocs;
        CHECK(a.upload({8, 9}) == 0 && M::allocs == allocs && a.capacity() == 3 && a.get()[0] == 8 && a.get()[1] == 9);      // in place
        TBuf<double> e;                   // Engine::op_ln: no table yet, the copy fails -> still none, and the next call builds it
        M::fail_copy = 1;
        CHECK(e.upload({0.5, 0.25}) == M::ERR_COPY && !e && e.capacity() == 0 && M::live == 1);
        CHECK(e.upload({0.5, 0.25}) == 0 && e && e.get()[1] == 0.25);
    }
    CHECK(M::live == 0);

    // --- a table staged in a local buffer: a failure after the upload leaks nothing and leaves the member's table in place
    {
        TBuf<int> member;
        CHECK(stage_table(member, {1, 2, 3}, 0) == 0 && member.capacity() == 3 && M::live == 1);
        int* const blk = member.get();
        CHECK(stage_table(member, {4, 5, 6, 7}, 77) == 77 && member.get() == blk && member.get()[2] == 3 && M::live == 1);
        M::fail_copy = 1;
        CHECK(stage_table(member, {4, 5, 6, 7}, 0) == M::ERR_COPY && member.get() == blk && M::live == 1);
        CHECK(stage_table(member, {4, 5, 6, 7}, 0) == 0 && member.capacity() == 4 && member.get()[3] == 7 && M::live == 1);
    }
    CHECK(M::live == 0);

    // --- a size whose byte count overflows size_t: refused, no call of Mem
    {
        TBuf<double> a;
        const int before = M::calls();
        CHECK(a.reserve(SIZE_MAX) == BUF_TOO_LARGE && a.reserve(SIZE_MAX / sizeof(double) + 1) == BUF_TOO_LARGE);
        CHECK(M::calls() == before && !a && a.capacity() == 0);
        CHECK(a.reserve(3) == 0);
        const int mid = M::calls();
        CHECK(a.reserve(SIZE_MAX / 2) == BUF_TOO_LARGE && M::calls() == mid && a.capacity() == 3);
        M::fail_alloc = 1;                // the largest count that does not overflow reaches Mem (which refuses it here)
        CHECK(a.reserve(SIZE_MAX / sizeof(double)) == M::ERR_ALLOC && M::calls() == mid + 1 && a.capacity() == 3);
    }
    CHECK(M::live == 0);

    // --- upload of an empty vector: a one-element block, no copy
    {
        TBuf<float> a;
        const int copies = M::copies;
        CHECK(a.upload({}) == 0 && a && a.capacity() == 1 && M::copies == copies);
        a.get()[0] = 1.f;
    }
    CHECK(M::live == 0);

    // --- reset, then reserve
    {
        TBuf<int> a;
        CHECK(a.reserve(6) == 0);
        a.reset();
        CHECK(!a && a.capacity() == 0 && M::live == 0);
        a.reset();                        // (twice: nothing to release)
        CHECK(M::live == 0);
        CHECK(a.reserve(2) == 0 && a.capacity() == 2 && M::live == 1);
        a.get()[1] = 3;
    }
    CHECK(M::live == 0);

    // --- the sequence of set_params calls that used to leave a recorded capacity without its buffers: (K1, I1), then
    // (K2, I2) with the second allocation failing, then (K2, I2) again
    const size_t K1 = 5, I1 = 2, K2 = 40, I2 = 6;
    int covered_after_failure = 0, holds_after_retry = 0;
    {
        Histories h;
        CHECK(h.reserve(K1, I1) == 0 && h.holds(K1, I1) && h.touch());
        M::fail_alloc = 2;
        CHECK(h.reserve(K2, I2) == M::ERR_ALLOC);
        CHECK(h.nact.capacity() == K2);                                   // the first buffer grew,
        CHECK(h.alpha.capacity() == 3 * K1 * Histories::Bp);              // the second is as it was,
        CHECK(h.cg_iters.capacity() == I1 * 3 * Histories::Bp);           // the third was not reached
        CHECK(!h.holds(K2, I2) && h.holds(K1, I1));                       // nothing claims (K2, I2)
        covered_after_failure = h.touch();
        CHECK(covered_after_failure);
        CHECK(h.reserve(K2, I2) == 0);
        holds_after_retry = h.holds(K2, I2) && h.touch();
        CHECK(holds_after_retry);
        const int before = M::calls();
        CHECK(h.reserve(K2, I2) == 0 && h.reserve(K1, I1) == 0 && M::calls() == before);      // the head of every later solve
    }
    CHECK(M::live == 0 && M::fail_alloc == 0 && M::fail_copy == 0);
    CHECK(M::releases == M::allocs - M::refused);      // every block that came was given back once

    printf("{\"checks\": %d, \"live\": %d, \"allocs\": %d, \"releases\": %d, \"refused\": %d, \"copies\": %d, \"covered_after_failure\": %d, "
           "\"holds_after_retry\": %d}\n", n_checks, M::live, M::allocs, M::releases, M::refused, M::copies, covered_after_failure, holds_after_retry);
    return 0;
}
