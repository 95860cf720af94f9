// Row kernel of the streaming path for time-varying edge weights (gfx950, wave64): the twin of k_rows (stream_kernels.h) for
// the OPK_SPATIAL operators Lu, Ldr and Ldr^T whose weights differ from one time slice to the next.
//
// Geometry (Geom), XCD ownership, the t-major sweep, the scalar prefetch of the next rows' metadata, the epilogue functors and
// the products and their order are those of k_rows.  The one difference: the weights of a row at output time t come from slice
// tv::slice_of(t, op.shift, op.n_slices) of the per-slice value table val_t[S][nnz] (tv_values.h); row pointers and column
// indices are shared by all slices.  A work item lies in one time slice, so the slice base is one scalar address per item.
// Like k_rows the kernel loads a fixed window of GW (column, weight) pairs per row: a read past the row's end lands in the next
// row, the next slice or the TV_PAD entries after the last slice, and is discarded by the `ok` test of row_entries.  The rows
// without a gather (t = 0 of Ldr, t = T-1 of Ldr^T) still load; the clamp of slice_of keeps those loads inside the table.
#pragma once
#include "stream_kernels.h"
#include "tv_values.h"

static_assert(tv::TV_PAD == CSR_PAD, "the per-slice tables are padded like the CSR arrays");

template <typename S, int VEC, class Epi, int GW>
__global__ __launch_bounds__(256) void k_rows_tv(Geom g, OpDesc op, const int* __restrict__ rowptr,
                                                 const int* __restrict__ colidx, const float* __restrict__ val_t,
                                                 const S* __restrict__ in, Epi epi_in, S* __restrict__ partials,
                                                 const int* __restrict__ live) {
    if (live != nullptr && *live == 0) return;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int xcd = blockIdx.x & 7;
    const int q = blockIdx.x >> 3;
    const int chunk = q % g.CH;
    const int r = q / g.CH;
    const int col0 = (chunk * 64 + lane) * VEC;
    const int slot = xcd * g.G8 + r;       // this workgroup's position inside a round / partial row

    Epi epi = epi_in;
    epi.begin(col0);
    constexpr int NR = Epi::NRED > 0 ? Epi::NRED : 1;
    S acc[NR][VEC];
#pragma unroll
    for (int rr = 0; rr < NR; ++rr)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[rr][v] = S(0);

    const int xlo = xcd * g.NX, xhi = min(g.N, xlo + g.NX);   // node rows this XCD owns, for every time slice
    for (int item = r; item < g.n_items; item += g.G8) {
        const int tq = item / g.NBL;
        const int nb = item - tq * g.NBL;
        const int t = g.rev ? g.T - 1 - tq : tq;
        const int n0 = xlo + nb * g.RI;
        const int n1 = min(xhi, n0 + g.RI);
        int i = n0 + wave;
        if (i >= n1) continue;
        const int ts = t + op.shift;
        const bool tvalid = ts >= 0 && ts < g.T;
        // the weights of this item's time slice (wave-uniform: fetched through the scalar cache like the shared pattern)
        const float* __restrict__ val = val_t + (size_t)tv::slice_of(t, op.shift, op.n_slices) * op.slice_stride;
        S selfc = S(1);
        if (op.self_mode == SELF_LDR) selfc = (t >= 1) ? S(1) : S(0);
        else if (op.self_mode == SELF_LDRT) selfc = (t > 0 || op.q1) ? S(1) : S(0);
        else if (op.self_mode == SELF_LN_FATHER) selfc = (t + 1 < g.T) ? S(1) : S(0);
        const S* gbase = in + (size_t)(tvalid ? ts : t) * g.N * g.Bp + col0;   // slice the gathers read
        const S* obase = in + (size_t)t * g.N * g.Bp + col0;                  // slice of the rows we own
        RowMeta<GW> cur, nxt;
        int be0, be1, ne0, ne1;
        row_bounds(rowptr, i, be0, be1);
        if (!tvalid) be1 = be0;
        row_entries<GW>(colidx, val, be0, be1, i, cur);
        row_bounds(rowptr, min(i + 4, g.N - 1), ne0, ne1);
        if (!tvalid) ne1 = ne0;
        for (; i < n1; i += 4) {
            const size_t roff = (size_t)i * g.Bp;
            Vec<S, VEC> sum;
#pragma unroll
            for (int v = 0; v < VEC; ++v) sum.v[v] = S(0);
            if (cur.e1 - cur.e0 > GW) {          // entries past the fixed gather window (rare rows)
                for (int e = cur.e0 + GW; e < cur.e1; ++e) {
                    const Vec<S, VEC> x = ldv<S, VEC>(gbase + (size_t)colidx[e] * g.Bp);
                    const S w = (S)val[e];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) sum.v[v] += w * x.v[v];
                }
            }
            // own row + GW neighbour rows in flight together; pad slots re-read the own node (weight 0)
            const Vec<S, VEC> self = ldv<S, VEC>(obase + roff);
            Vec<S, VEC> nv[GW];
#pragma unroll
            for (int u = 0; u < GW; ++u) nv[u] = ldv<S, VEC>(gbase + (size_t)cur.c[u] * g.Bp);
            __builtin_amdgcn_sched_barrier(0);   // keep the loads issued up here
            // scalar prefetch for the rows this wave handles next (one and two steps ahead)
            row_entries<GW>(colidx, val, ne0, ne1, min(i + 4, g.N - 1), nxt);
            int fe0, fe1;
            row_bounds(rowptr, min(i + 8, g.N - 1), fe0, fe1);
            if (!tvalid) fe1 = fe0;
#pragma unroll
            for (int u = 0; u < GW; ++u)
#pragma unroll
                for (int v = 0; v < VEC; ++v) sum.v[v] += (S)cur.w[u] * nv[u].v[v];
            Vec<S, VEC> l;
#pragma unroll
            for (int v = 0; v < VEC; ++v) l.v[v] = selfc * self.v[v] - sum.v[v];
            epi.row(t, (size_t)t * g.N * g.Bp + roff + col0, self, l, acc);
            cur = nxt;
            ne0 = fe0;
            ne1 = fe1;
        }
    }

    if (Epi::NRED > 0) {
        __shared__ S sm[3][VEC][64];
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            if (wave > 0) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) sm[wave - 1][v][lane] = acc[rr][v];
            }
            __syncthreads();
            if (wave == 0) {
                Vec<S, VEC> o;
#pragma unroll
                for (int v = 0; v < VEC; ++v) o.v[v] = ((acc[rr][v] + sm[0][v][lane]) + sm[1][v][lane]) + sm[2][v][lane];
                stv<S, VEC>(partials + ((size_t)rr * g.P + slot) * g.Bp + col0, o);
            }
            __syncthreads();
        }
    }
}
