// CPU run of the weight-set planner of the LDS-resident path (mixed-graph-admm_amd/csrc/lds_graph_sets.h).
//   lds_graph_sets_check <graph file> [MGADMM_LDS_<SWITCH>=<value> ...]
// graph file and switches: as tests/cpu/lds_plan_check.cpp reads them.  The file's graph is the solver's graph.  NSETS weight
// sets of its pattern are formed (set 0: the file's weights; set j: every weight of edge (i, c) times a factor that depends on
// j, i and c, the same in W_d and W_d^T), planned into one table, and checked:
//   * the image of set j at j * img_stride equals, byte for byte, what ldsplan::make returns for set j planned alone;
//   * the plan of set j alone equals the solver's plan in every field, its node_of_row / row_of_node equal set 0's;
//   * the images of two sets differ (the check is not run on four copies of one set);
//   * three sets that must be refused, each with the name of what differs: one off-diagonal W_d entry dropped, another k (the
//     last neighbour of every row dropped), and the other transpose rule (transpose_by_gather flipped).
// Prints one JSON object with the stride, the image length and the three refusals.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "lds_graph_sets.h"

static bool read_csr(FILE* f, int N, HostCsr& h) {
    int nnz = 0;
    if (fscanf(f, "%d", &nnz) != 1 || nnz < 0) return false;
    h.n = N;
    h.rowptr.assign(N + 1, 0);
    h.col.assign(nnz, 0);
    h.val.assign(nnz, 0.f);
    for (auto& v : h.rowptr) if (fscanf(f, "%d", &v) != 1) return false;
    for (auto& v : h.col) if (fscanf(f, "%d", &v) != 1 || v < 0 || v >= N) return false;
    for (auto& v : h.val) {
        uint32_t bits;
        if (fscanf(f, "%" SCNx32, &bits) != 1) return false;
        memcpy(&v, &bits, 4);
    }
    return h.rowptr[0] == 0 && h.rowptr[N] == nnz;
}

// weight factor of edge (dst row i, src column c) in set j: 1 for set 0, else a scale of the set times a perturbation of the edge
static float factor(int j, int i, int c) {
    if (j == 0) return 1.f;
    const uint32_t h = (uint32_t)(i * 2654435761u) ^ (uint32_t)(c * 40503u + 977u * j);
    return (0.5f + 0.75f * j) * (0.9f + 0.2f * (float)(h % 1024u) / 1024.f);
}
static HostCsr scaled(const HostCsr& h, int j, bool transposed) {
    HostCsr o = h;
    for (int i = 0; i < h.n; ++i)
        for (int e = h.rowptr[i]; e < h.rowptr[i + 1]; ++e) o.val[e] = h.val[e] * (transposed ? factor(j, h.col[e], i) : factor(j, i, h.col[e]));
    return o;
}
// exact transpose, entries of a row by source row (csrc/graph.hip, mg_transpose_csr)
static HostCsr transpose(const HostCsr& h) {
    HostCsr t;
    t.n = h.n;
    t.rowptr.assign(h.n + 1, 0);
    for (int c : h.col) ++t.rowptr[c + 1];
    for (int i = 0; i < h.n; ++i) t.rowptr[i + 1] += t.rowptr[i];
    t.col.assign(h.col.size(), 0);
    t.val.assign(h.col.size(), 0.f);
    std::vector<int> at(t.rowptr.begin(), t.rowptr.end() - 1);
    for (int i = 0; i < h.n; ++i)
        for (int e = h.rowptr[i]; e < h.rowptr[i + 1]; ++e) { t.col[at[h.col[e]]] = i; t.val[at[h.col[e]]++] = h.val[e]; }
    return t;
}
// h without entry `drop` of its arrays
static HostCsr without(const HostCsr& h, const std::vector<char>& drop) {
    HostCsr o;
    o.n = h.n;
    o.rowptr.push_back(0);
    for (int i = 0; i < h.n; ++i) {
        for (int e = h.rowptr[i]; e < h.rowptr[i + 1]; ++e)
            if (!drop[e]) { o.col.push_back(h.col[e]); o.val.push_back(h.val[e]); }
        o.rowptr.push_back((int)o.col.size());
    }
    return o;
}

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(int argc, char** argv) {
    constexpr int NSETS = 4;
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int T, N, band, tbg;
    HostCsr Wu, Wd, WdT;
    if (fscanf(f, "%d %d %d %d", &T, &N, &band, &tbg) != 4 || N < 1 || !read_csr(f, N, Wu) || !read_csr(f, N, Wd) || !read_csr(f, N, WdT)) return 2;
    fclose(f);
    if (band) return 2;
    for (int i = 2; i < argc; ++i)
        if (strncmp(argv[i], "MGADMM_LDS_", 11) != 0 || !strchr(argv[i], '=') || putenv(argv[i]) != 0) return 2;
    const ldsplan::Switches sw = ldsplan::Switches::from_env();

    // the solver's plan
    const ldsplan::Input in0{T, N, false, tbg != 0, Wu, Wd, WdT};
    ldsplan::LdsPlan ref;
    std::vector<int> ref_img;
    CHECK(ldsplan::make(in0, sw, ref, ref_img) == ldsplan::PLANNED && ref.ok);

    // the sets and their table
    std::vector<HostCsr> su, sd, st;
    for (int j = 0; j < NSETS; ++j) { su.push_back(scaled(Wu, j, false)); sd.push_back(scaled(Wd, j, false)); st.push_back(scaled(WdT, j, tbg == 0)); }
    std::vector<ldsplan::Input> sets;
    for (int j = 0; j < NSETS; ++j) sets.push_back(ldsplan::Input{T, N, false, tbg != 0, su[j], sd[j], st[j]});
    std::vector<int> table;
    std::string why;
    int bad = -1;
    // (two host threads: the library plans the sets side by side)
    if (!ldssets::build_table(ref, ref_img, sets, sw, table, &bad, why, 2)) { printf("FAILED: set %d refused: %s\n", bad, why.c_str()); return 1; }
    const int stride = ldssets::img_stride(ref);
    CHECK(stride >= ref.csr_ints && stride % 4 == 0 && stride - ref.csr_ints < 4 && table.size() == (size_t)stride * NSETS);
    for (int j = 0; j < NSETS; ++j) {
        ldsplan::LdsPlan p;
        std::vector<int> img;
        CHECK(ldsplan::make(sets[j], sw, p, img) == ldsplan::PLANNED);
        CHECK(ldssets::plan_diff(ref, p) == nullptr);
        CHECK((int)img.size() == ref.csr_ints);
        CHECK(memcmp(&table[(size_t)j * stride], img.data(), sizeof(int) * img.size()) == 0);           // byte for byte
        for (int k = ref.csr_ints; k < stride; ++k) CHECK(table[(size_t)j * stride + k] == 0);
        CHECK(memcmp(&table[(size_t)j * stride + ref.off_node], &table[ref.off_node], sizeof(int) * (ref.NR + N)) == 0);   // node_of_row, row_of_node
        if (j == 0) CHECK(img == ref_img);
        else {
            CHECK(memcmp(&table[(size_t)j * stride], &table[(size_t)(j - 1) * stride], sizeof(int) * ref.csr_ints) != 0);
            int nw = 0;                  // weight words that differ from set 0's: most of them
            for (int at = 0; at < ref.csr_ints; ++at) {
                if (ldssets::is_weight_word(ref, at)) nw += img[at] != ref_img[at];
                else CHECK(img[at] == ref_img[at]);
            }
            CHECK(nw >= Wu.nnz());
        }
    }

    // refusals
    std::vector<int> img;
    std::string r_drop, r_k, r_tbg;
    {   // one off-diagonal entry of W_d dropped (a weight that underflowed to 0 in a table builder that skips zeros)
        int victim = -1;
        for (int i = 0; i < N && victim < 0; ++i)
            for (int e = Wd.rowptr[i]; e < Wd.rowptr[i + 1]; ++e) if (Wd.col[e] != i) victim = e;
        CHECK(victim >= 0);
        std::vector<char> drop(Wd.nnz(), 0);
        drop[victim] = 1;
        const HostCsr d = without(Wd, drop), t = tbg ? d : transpose(d);
        CHECK(!ldssets::plan_set(ref, ref_img, ldsplan::Input{T, N, false, tbg != 0, Wu, d, t}, sw, img, r_drop));
    }
    {   // another k: the last neighbour of every row that has more than two entries
        std::vector<char> du(Wu.nnz(), 0), dd(Wd.nnz(), 0);
        for (int i = 0; i < N; ++i) {
            if (Wu.rowptr[i + 1] - Wu.rowptr[i] > 2) du[Wu.rowptr[i + 1] - 1] = 1;
            if (Wd.rowptr[i + 1] - Wd.rowptr[i] > 2) dd[Wd.rowptr[i + 1] - 1] = 1;
        }
        const HostCsr u = without(Wu, du), d = without(Wd, dd), t = tbg ? d : transpose(d);
        CHECK(!ldssets::plan_set(ref, ref_img, ldsplan::Input{T, N, false, tbg != 0, u, d, t}, sw, img, r_k));
    }
    {   // the other transpose rule
        const HostCsr t = tbg ? transpose(Wd) : Wd;
        CHECK(!ldssets::plan_set(ref, ref_img, ldsplan::Input{T, N, false, tbg == 0, Wu, Wd, t}, sw, img, r_tbg));
    }
    auto field = [](const std::string& s) { return s.substr(0, s.find(':')); };
    printf("{\"sets\": %d, \"img_stride\": %d, \"csr_ints\": %d, \"instance\": %" PRId64 ", \"uniform45\": %d, \"dropped\": \"%s\", \"other_k\": \"%s\", "
           "\"other_transpose\": \"%s\"}\n", NSETS, stride, ref.csr_ints, ref.instance, ref.uniform45, field(r_drop).c_str(), field(r_k).c_str(),
           field(r_tbg).c_str());
    return 0;
}
