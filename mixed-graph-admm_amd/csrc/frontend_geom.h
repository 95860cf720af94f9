// Launch geometry and range tests of the data front end (frontend.hip): the row chunks and grids of series_stats, the
// grids of series_affine and gather_windows, and the start-index test of k_windows.  Plain C++, no HIP:
// tests/cpu/frontend_geom_check.cpp compiles it with g++ under AddressSanitizer + UBSan.
#pragma once
#include <cstdint>

#include "mg_hd.h"

namespace fegeom {

constexpr int ST_ROWS = 256;                  // time steps per partial of k_col_partials (one workgroup row chunk)
constexpr int ST_COLS = 64;                   // columns per workgroup of k_col_partials
constexpr int FIN_COLS = 256;                 // columns per workgroup of k_col_finish
constexpr int BLOCK = 256;                    // threads per workgroup of k_affine / k_windows
constexpr int MAX_GRID_Y = 65535;             // gridDim.y the launches stay within: the smallest limit of any HIP platform
constexpr int64_t MAX_STEPS = (int64_t)MAX_GRID_Y * ST_ROWS;      // 16 776 960: one row chunk per gridDim.y
constexpr int MAX_WINDOWS = MAX_GRID_Y;       // one window per gridDim.y
constexpr int AFFINE_MAX_BLOCKS = 8192;       // k_affine strides over the rest
constexpr int WINDOW_MAX_BLOCKS = 64;         // k_windows strides over the rest of a window

struct Grid {
    unsigned x, y;
};

// Is [s0, s0 + win) inside [0, n_steps)?  Callers guarantee 1 <= win <= n_steps, so n_steps - win cannot wrap, whereas
// s0 + win does for a start index close to 2^63.
MG_HD inline bool window_in_range(long long s0, int win, long long n_steps) { return s0 >= 0 && s0 <= n_steps - win; }

inline bool steps_supported(int64_t n_steps) { return n_steps >= 1 && n_steps <= MAX_STEPS; }

// Row chunks of series_stats; 0 where the series is longer than one launch covers (steps_supported is false).
inline int stats_chunks(int64_t n_steps) {
    return steps_supported(n_steps) ? (int)((n_steps + ST_ROWS - 1) / ST_ROWS) : 0;
}

inline Grid stats_partials_grid(int nchunk, int n_cols) { return {(unsigned)((n_cols + ST_COLS - 1) / ST_COLS), (unsigned)nchunk}; }

inline Grid stats_finish_grid(int n_cols) { return {(unsigned)((n_cols + FIN_COLS - 1) / FIN_COLS), 1u}; }

inline Grid affine_grid(int64_t total) {
    const int64_t blocks = (total + BLOCK - 1) / BLOCK;
    return {(unsigned)(blocks < AFFINE_MAX_BLOCKS ? blocks : AFFINE_MAX_BLOCKS), 1u};
}

inline Grid windows_grid(int64_t per_window, int B) {
    const int64_t blocks = (per_window + BLOCK - 1) / BLOCK;
    return {(unsigned)(blocks < WINDOW_MAX_BLOCKS ? blocks : WINDOW_MAX_BLOCKS), (unsigned)B};
}

}  // namespace fegeom
