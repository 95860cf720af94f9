// CPU run of the launch plan of the streaming path (mixed-graph-admm_amd/csrc/stream_plan.h).
//   stream_plan_check <elem> <T> <N> <B> <mode> <reorder> <q1> <max_u> <max_d> <max_dt> <avg_dt> <NT> [MGADMM_<SWITCH>=<value> ...]
//   stream_plan_check @<file>          one such case per line
// elem: bytes of the scalar type (4 / 8); mode: 0 spatial, 1 band; max_u, max_d, max_dt: the longest row of W_u, W_d, W_d^T;
// avg_dt: ceil(mean row length) of W_d^T; NT: tiles of the k_cldr tables (0: none).  The switches are arguments, handed to
// Switches::from_strings: the program reads no environment.
// Prints one JSON object per case: the switches as parsed, every field of Geom, TileGeom (null: no tile geometry) and CldrGeom,
// the k_cldr geometry in force with the slot pair of a graph whose longest rows are max_d and max_dt, the stream key (epilogue
// EpiStore, plain source) of every operand class and of k_cldr, the fused flag, and the two fold flags of each left-hand side.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>
#include "stream_plan.h"

using namespace streamplan;

// a matrix of n rows with one entry each, but row n / 2 with `longest`: all the slot scan reads is the row lengths
static HostCsr rows_of(int n, int longest) {
    HostCsr h;
    h.n = n;
    h.rowptr.push_back(0);
    for (int i = 0; i < n; ++i) {
        const int len = i == n / 2 ? longest : std::min(1, longest);
        for (int e = 0; e < len; ++e) { h.col.push_back((i + e) % n); h.val.push_back(1.f); }
        h.rowptr.push_back((int)h.col.size());
    }
    return h;
}

static int run_case(const std::vector<std::string>& a) {
    if (a.size() < 12) return 2;
    int v[12];
    for (int i = 0; i < 12; ++i) v[i] = atoi(a[i].c_str());
    Facts f;
    f.elem = v[0]; f.T = v[1]; f.N = v[2];
    const int B = v[3];
    f.spatial = v[4] == 0; f.reorder = v[5]; f.q1 = v[6];
    f.max_u = v[7]; f.max_d = v[8]; f.max_dt = v[9]; f.avg_dt = v[10];
    const int NT = v[11];
    if ((f.elem != 4 && f.elem != 8) || f.T < 1 || f.N < 1 || B < 1 || NT < 0) return 2;
    for (size_t i = 12; i < a.size(); ++i)
        if (a[i].compare(0, 7, "MGADMM_") != 0 || a[i].find('=') == std::string::npos) return 2;
    const Switches sw = Switches::from_strings([&](const char* name) -> const char* {
        const size_t n = strlen(name);
        for (size_t i = 12; i < a.size(); ++i)
            if (a[i].compare(0, n, name) == 0 && a[i][n] == '=') return a[i].c_str() + n + 1;
        return nullptr;
    }, f.elem);
    const Planner p(f, sw);

    printf("{\"switches\": {\"want_blocks\": %d, \"tile\": %d, \"fused\": %d, \"fold\": %d, \"fold_lu\": %d, \"sweep_rev\": %d, \"cldr_tile_major\": %d, "
           "\"tile_r\": %d, \"cldr_geom\": %d, \"cldr_rows\": %d, \"tile_stats\": %d}",
           sw.want_blocks, sw.tile, sw.fused, sw.fold, sw.fold_lu, sw.sweep_rev, sw.cldr_tile_major, sw.tile_r, sw.cldr_geom, sw.cldr_rows, (int)sw.tile_stats);
    const Geom q = p.make_geom(B);
    printf(", \"geom\": {\"T\": %d, \"N\": %d, \"B\": %d, \"Bp\": %d, \"VEC\": %d, \"CH\": %d, \"RI\": %d, \"NX\": %d, \"NBL\": %d, \"n_items\": %d, \"G8\": %d, "
           "\"P\": %d, \"grid\": %d, \"rev\": %d}", q.T, q.N, q.B, q.Bp, q.VEC, q.CH, q.RI, q.NX, q.NBL, q.n_items, q.G8, q.P, q.grid, q.rev);
    TileGeom tg;
    if (p.make_tile_geom(q, tg))
        printf(", \"tile\": {\"T\": %d, \"N\": %d, \"B\": %d, \"Bp\": %d, \"VEC\": %d, \"CH\": %d, \"R\": %d, \"NTILE\": %d, \"TPX\": %d, \"P\": %d, \"grid\": %d, "
               "\"lds_bytes\": %d}", tg.T, tg.N, tg.B, tg.Bp, tg.VEC, tg.CH, tg.R, tg.NTILE, tg.TPX, tg.P, tg.grid, tg.lds_bytes);
    else
        printf(", \"tile\": null");
    printf(", \"tile_rows\": %d", p.tile_rows());
    const CldrGeom cg = p.make_cldr_geom(q, NT);
    printf(", \"cldr\": {\"T\": %d, \"N\": %d, \"B\": %d, \"Bp\": %d, \"CH\": %d, \"NT\": %d, \"TPX\": %d, \"P\": %d, \"grid\": %d, \"tile_major\": %d, \"q1\": %d, "
           "\"lds_bytes\": %d}", cg.T, cg.N, cg.B, cg.Bp, cg.CH, cg.NT, cg.TPX, cg.P, cg.grid, cg.tile_major, cg.q1, cg.lds_bytes);
    const std::pair<int, int> slots = cldr_slots(rows_of(f.N, f.max_d), rows_of(f.N, f.max_dt));
    printf(", \"cldr_width_fits\": %d, \"geom_index\": %d, \"gd\": %d, \"gt\": %d", (int)p.cldr_width_fits(q), p.geom, slots.first, slots.second);

    const int epi_store = 0;                                 // (STREAM_EPI_NAMES[0])
    if (strcmp(STREAM_EPI_NAMES[epi_store], "EpiStore") != 0) return 3;
    const struct { const char* name; Mat m; bool self_w; } ops[] = {{"none", M_NONE, false}, {"band", M_BAND, false}, {"lu", M_WU, false},
        {"ldr", M_WD, false}, {"ldrt", M_WDT, false}, {"ldr+self", M_WD, true}, {"ldrt+self", M_WDT, true}};
    printf(", \"keys\": {");
    for (const auto& o : ops) printf("\"%s\": %" PRId64 ", ", o.name, p.key(p.choose(o.m, o.self_w, q), epi_store, false));
    printf("\"cldr\": %" PRId64 "}", p.key(p.cldr_choice(slots.first, slots.second), epi_store, false));
    printf(", \"fused\": %d, \"fold\": [", (int)p.fused(q, NT));
    for (int kind = 0; kind < 3; ++kind) printf("%s[%d, %d]", kind ? ", " : "", (int)p.fold1(kind, q, NT), (int)p.fold2(kind, q));
    printf("]}\n");
    return 0;
}

static std::vector<std::string> words(const std::string& line) {
    std::istringstream in(line);
    std::vector<std::string> w;
    for (std::string s; in >> s;) w.push_back(s);
    return w;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (argv[1][0] != '@') return run_case(std::vector<std::string>(argv + 1, argv + argc));
    FILE* f = fopen(argv[1] + 1, "r");
    if (!f) return 2;
    char buf[1024];
    int rc = 0;
    while (rc == 0 && fgets(buf, sizeof buf, f)) {
        const std::vector<std::string> w = words(buf);
        if (!w.empty()) rc = run_case(w);
    }
    fclose(f);
    return rc;
}
