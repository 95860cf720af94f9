// CPU check of the data front end's launch geometry (mixed-graph-admm_amd/csrc/frontend_geom.h), built with
// AddressSanitizer + UBSan: a signed overflow in the start-index test would end the program here.
//   frontend_geom_check            runs the checks, prints one JSON object, exit status 1 on the first failure
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "frontend_geom.h"

static int n_checks = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        ++n_checks;                                                        \
        if (!(cond)) {                                                     \
            fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond);    \
            return 1;                                                      \
        }                                                                  \
    } while (0)

// every element of [0, total) is visited once by `for (i = block * 256 + thread; i < total; i += grid * 256)`
// (the loop is replayed for ranges of up to 4 Mi elements; beyond that a grid of at least one workgroup is all it takes)
static bool stride_covers(int64_t total, unsigned grid) {
    if (grid < 1) return false;
    if (total > (4 << 20)) return true;
    std::vector<unsigned char> seen((size_t)total, 0);
    for (unsigned blk = 0; blk < grid; ++blk)
        for (int th = 0; th < fegeom::BLOCK; ++th)
            for (int64_t i = (int64_t)blk * fegeom::BLOCK + th; i < total; i += (int64_t)grid * fegeom::BLOCK) ++seen[(size_t)i];
    for (unsigned char s : seen)
        if (s != 1) return false;
    return true;
}

int main() {
    using namespace fegeom;
    // --- window_in_range: no wrap for any start index
    const struct { long long n_steps; int win; } series[] = {{80, 24}, {4, 1}, {24, 24}, {1, 1}, {MAX_STEPS, 24}, {INT64_MAX, 24}};
    for (const auto& s : series) {
        const long long last = s.n_steps - s.win;
        CHECK(window_in_range(0, s.win, s.n_steps));
        CHECK(window_in_range(last, s.win, s.n_steps));
        if (last < INT64_MAX) CHECK(!window_in_range(last + 1, s.win, s.n_steps));
        if (s.n_steps < INT64_MAX) CHECK(!window_in_range(s.n_steps, s.win, s.n_steps));
        CHECK(!window_in_range(-1, s.win, s.n_steps));
        CHECK(window_in_range(INT64_MAX, s.win, s.n_steps) == (last == INT64_MAX));
        CHECK(window_in_range(INT64_MAX - s.win + 1, s.win, s.n_steps) == (INT64_MAX - s.win + 1 <= last));      // s0 + win wraps to INT64_MIN
        CHECK(!window_in_range(INT64_MIN, s.win, s.n_steps));
        CHECK(!window_in_range(1LL << 40, s.win, s.n_steps) || s.n_steps > (1LL << 40));
    }
    // agreement with the plain definition wherever that does not overflow
    for (long long n = 1; n <= 9; ++n)
        for (int w = 1; w <= n; ++w)
            for (long long s0 = -3; s0 <= 12; ++s0) CHECK(window_in_range(s0, w, n) == (s0 >= 0 && s0 + w <= n));

    // --- row chunks of series_stats
    CHECK(stats_chunks(1) == 1);
    CHECK(stats_chunks(255) == 1);
    CHECK(stats_chunks(256) == 1);
    CHECK(stats_chunks(257) == 2);
    CHECK(MAX_STEPS == 16776960);
    CHECK(stats_chunks(MAX_STEPS - 1) == MAX_GRID_Y);
    CHECK(stats_chunks(MAX_STEPS) == MAX_GRID_Y);
    CHECK(steps_supported(MAX_STEPS) && !steps_supported(MAX_STEPS + 1) && stats_chunks(MAX_STEPS + 1) == 0);
    CHECK(!steps_supported(0) && !steps_supported(-1) && !steps_supported(INT64_MAX) && stats_chunks(INT64_MAX) == 0);
    const int64_t steps[] = {1, 2, 5, 255, 256, 257, 513, 17856, MAX_STEPS - 256, MAX_STEPS - 255, MAX_STEPS - 1, MAX_STEPS};
    const int cols[] = {1, 63, 64, 65, 255, 256, 257, 307, 100000};
    for (int64_t n : steps) {
        const int nc = stats_chunks(n);
        CHECK((int64_t)nc * ST_ROWS >= n && (int64_t)(nc - 1) * ST_ROWS < n);      // covers the rows, no empty chunk
        for (int c : cols) {
            const Grid g1 = stats_partials_grid(nc, c), g2 = stats_finish_grid(c);
            CHECK(g1.y == (unsigned)nc && g1.y >= 1 && g1.y <= (unsigned)MAX_GRID_Y);
            CHECK((int64_t)g1.x * ST_COLS >= c && (int64_t)(g1.x - 1) * ST_COLS < c);
            CHECK(g2.y == 1 && (int64_t)g2.x * FIN_COLS >= c && (int64_t)(g2.x - 1) * FIN_COLS < c);
        }
    }

    // --- grids of series_affine and gather_windows: a stride loop of gridDim.x * 256 threads covers the range
    const int64_t totals[] = {1, 3, 255, 256, 257, 4550, (int64_t)AFFINE_MAX_BLOCKS * BLOCK - 1, (int64_t)AFFINE_MAX_BLOCKS * BLOCK,
                              (int64_t)AFFINE_MAX_BLOCKS * BLOCK + 1, 2107400, 17856LL * 307, MAX_STEPS * 307, INT64_MAX - 255};
    for (int64_t t : totals) {
        const Grid g = affine_grid(t);
        CHECK(g.y == 1 && g.x >= 1 && g.x <= (unsigned)AFFINE_MAX_BLOCKS);
        CHECK((int64_t)g.x * BLOCK >= t || g.x == (unsigned)AFFINE_MAX_BLOCKS);
        CHECK(g.x == 1 || (int64_t)(g.x - 1) * BLOCK < t);                           // no workgroup without work
        CHECK(stride_covers(t, g.x));
    }
    const int64_t pers[] = {1, 255, 256, 257, 16383, 16384, 16385, 24 * 700, 70 * 257, 24LL * 100000, (int64_t)INT32_MAX * 2048};
    const int Bs[] = {1, 2, 64, 65534, MAX_WINDOWS};
    for (int64_t p : pers)
        for (int B : Bs) {
            const Grid g = windows_grid(p, B);
            CHECK(g.y == (unsigned)B && g.y <= (unsigned)MAX_GRID_Y);
            CHECK(g.x >= 1 && g.x <= (unsigned)WINDOW_MAX_BLOCKS);
            CHECK((int64_t)g.x * BLOCK >= p || g.x == (unsigned)WINDOW_MAX_BLOCKS);
            CHECK(g.x == 1 || (int64_t)(g.x - 1) * BLOCK < p);
            CHECK(stride_covers(p, g.x));
        }
    CHECK(MAX_WINDOWS == 65535);
    printf("{\"checks\": %d, \"max_steps\": %" PRId64 ", \"max_windows\": %d, \"chunks_at_limit\": %d}\n", n_checks, MAX_STEPS, MAX_WINDOWS,
           stats_chunks(MAX_STEPS));
    return 0;
}
