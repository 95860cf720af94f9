// Launch geometry of the streaming kernels (k_rows, k_tile, k_cldr in stream_kernels.h): the records the kernels take by value.
// Plain C++, no HIP: stream_plan.h fills them, and tests/cpu/stream_plan_check.cpp prints every field on the CPU.
#pragma once

struct Geom {
    int T, N, B, Bp;
    int VEC, CH;         // columns per lane; column chunks of 64*VEC
    int RI;              // rows per work item
    int NX, NBL;         // node rows owned by one XCD (multiple of RI); work items per time slice and XCD
    int n_items;         // T * NBL work items per (XCD, column chunk), enumerated t-major
    int G8;              // workgroups per (XCD, column chunk)
    int P;               // partial-sum rows per column = 8 * G8 (one per workgroup of a chunk)
    int grid;            // 8 * G8 * CH workgroups
    int rev;             // 1: sweep the time slices from T-1 down to 0 (see Engine::cg_internal: the slices a kernel touches
                         //    LAST are the ones still in the 256 MiB Infinity Cache when the next kernel starts)
};

// (k_tile)
struct TileGeom {
    int T, N, B, Bp;
    int VEC, CH;
    int R;        // node rows per tile (<= 4 * TILE_MAXR)
    int NTILE;    // tiles per column chunk
    int TPX;      // tile slots per XCD = ceil(NTILE / 8)
    int P;        // partial rows per column = 8 * TPX
    int grid;     // 8 * TPX * CH workgroups
    int lds_bytes;
};

// (k_cldr)
struct CldrGeom {
    int T, N, B, Bp;
    int CH;           // column chunks of 64*VECT
    int NT;           // tiles
    int TPX;          // tile slots per XCD = ceil(NT / 8)
    int P;            // partial rows per column = 8 * TPX
    int grid;         // 8 * TPX * CH workgroups
    int tile_major;   // 1: consecutive workgroups of an XCD take consecutive TILES of one chunk (shared halos stay hot in
                      //    its L2); 0: consecutive workgroups take the CHUNKS of one tile (whole rows are consumed together)
    int q1;           // quirk Q1 self coefficient at t = 0 (immaterial: q_0 = 0)
    int lds_bytes;
};
