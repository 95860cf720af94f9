// Instance keys of the streaming-path kernels (k_rows, k_tile, k_cldr in stream_kernels.h).  Plain C++, no HIP: the launch
// sites of engine.h note the key of the instance the plan chose (stream_plan.h, Planner::key: the template arguments packed
// into one int64) and keep the distinct keys of a solver in first-launch order (MGADMM_Q_STREAM_KEYS / MGADMM_Q_STREAM_KEY0
// + i); mgadmm/_lib.py (decode_stream_key) turns a key back into the name `nm -C` prints for the instance.  Tests only: the
// cost is a linear search over a few dozen keys per launch.
//
//   bits  0 ..  1   kernel: 0 k_rows, 1 k_tile, 2 k_cldr
//   bit   2         scalar type: 0 float, 1 double
//   bits  3 ..  5   VEC (k_rows, k_tile) / VECT (k_cldr): 1, 2 or 4
//   bits  6 .. 10   epilogue (the ID of the functor in stream_kernels.h, STREAM_EPI_NAMES below)
//   bit  11         source: 0 Plain, 1 Fold (TileSrcFold / CldrSrcFold; k_rows has no source argument)
//   bits 12 + 6 i   integer argument i, 6 bits each:  k_rows  GW
//                                                     k_tile  TILE_GW, MR
//                                                     k_cldr  NW, MA, MQ, MP, GD, GT, MINW
#pragma once
#include <cstdint>
#include <vector>

enum StreamKernel { STREAM_K_ROWS = 0, STREAM_K_TILE = 1, STREAM_K_CLDR = 2 };

// epilogue functors by ID (stream_kernels.h gives every one a `static constexpr int ID`)
constexpr const char* STREAM_EPI_NAMES[] = {"EpiStore", "EpiLhs", "EpiCgInit", "EpiCgUpdate", "EpiPUpdate", "EpiXFinal", "EpiLin2",
                                            "EpiRhsX", "EpiDual", "EpiPhi", "EpiPhiDirect", "EpiDot", "EpiLnLine", "EpiAddTo"};
constexpr int STREAM_EPI_COUNT = (int)(sizeof(STREAM_EPI_NAMES) / sizeof(STREAM_EPI_NAMES[0]));
constexpr int STREAM_KEY_ARG0 = 12, STREAM_KEY_ARG_BITS = 6, STREAM_KEY_NARGS = 7;

constexpr int64_t stream_key(int kernel, bool is_double, int vec, int epi, bool fold, int a0 = 0, int a1 = 0, int a2 = 0, int a3 = 0,
                             int a4 = 0, int a5 = 0, int a6 = 0) {
    return (int64_t)kernel | (int64_t)(is_double ? 1 : 0) << 2 | (int64_t)vec << 3 | (int64_t)epi << 6 | (int64_t)(fold ? 1 : 0) << 11 |
           (int64_t)a0 << STREAM_KEY_ARG0 | (int64_t)a1 << (STREAM_KEY_ARG0 + 6) | (int64_t)a2 << (STREAM_KEY_ARG0 + 12) |
           (int64_t)a3 << (STREAM_KEY_ARG0 + 18) | (int64_t)a4 << (STREAM_KEY_ARG0 + 24) | (int64_t)a5 << (STREAM_KEY_ARG0 + 30) |
           (int64_t)a6 << (STREAM_KEY_ARG0 + 36);
}
static_assert(stream_key(STREAM_K_CLDR, true, 4, STREAM_EPI_COUNT - 1, true, 16, 8, 11, 15, 8, 24, 4) > 0, "a key is a positive int64");
static_assert(STREAM_EPI_COUNT <= 32, "the epilogue ID has 5 bits");

// distinct keys of one solver in first-launch order
struct StreamKeyLog {
    std::vector<int64_t> keys;
    void note(int64_t k) {
        for (int64_t v : keys)
            if (v == k) return;
        keys.push_back(k);
    }
};
