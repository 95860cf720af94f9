// CPU run of the planner of the LDS-resident path (mixed-graph-admm_amd/csrc/lds_plan.h).
//   lds_plan_check <graph file> [MGADMM_LDS_<SWITCH>=<value> ...]
// graph file (text): "T N band transpose_by_gather", then W_u, W_d and W_d^T, each as "nnz", N+1 row pointers, nnz columns
// and nnz values -- the bit patterns of the float32 weights in hex (band mode: W_d and W_d^T with nnz 0).  The switches are
// put into the environment and read back through Switches::from_env, as the library reads them.
// Prints one JSON object: the status, every plan field, the instance (packed and as `nm -C` names it), the barrier count
// and the 64-bit FNV-1a hash of the image.  Checks that the image has the planned length and that the offsets are in order.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "lds_plan.h"

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

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int T, N, band, tbg;
    HostCsr Wu, Wd, WdT;
    if (fscanf(f, "%d %d %d %d", &T, &N, &band, &tbg) != 4 || N < 1 || !read_csr(f, N, Wu) || !read_csr(f, N, Wd) || !read_csr(f, N, WdT)) return 2;
    fclose(f);
    for (int i = 2; i < argc; ++i)
        if (strncmp(argv[i], "MGADMM_LDS_", 11) != 0 || !strchr(argv[i], '=') || putenv(argv[i]) != 0) return 2;

    const ldsplan::Input in{T, N, band != 0, tbg != 0, Wu, Wd, WdT};
    ldsplan::LdsPlan p;
    std::vector<int> img;
    const ldsplan::Status st = ldsplan::make(in, ldsplan::Switches::from_env(), p, img);
    CHECK(p.ok == (st == ldsplan::PLANNED));
    if (p.ok) {
        CHECK((int)img.size() == p.csr_ints && p.NR >= N && p.block - p.nthreads == p.NR - N && p.block % 64 == 0 && p.block <= p.maxt);
        CHECK(p.off_rp_u == 0 && p.off_rp_u < p.off_rp_d && p.off_rp_d < p.off_en_u && p.off_en_u <= p.off_en_d && p.off_en_d <= p.off_lead_t);
        CHECK(p.off_lead_t < p.off_tail_t && p.off_tail_t < p.off_diag && p.off_diag < p.off_node && p.off_node + p.NR == p.off_rown);
        CHECK(p.off_rown + N == p.csr_ints && p.lds_img0 + p.lds_img_ints <= p.off_diag && p.lds_bytes <= ldsplan::LDS_LIMIT);
        CHECK(p.off_tail_t - p.off_lead_t >= 2 * p.NR * LDS_NLEAD && p.off_diag - p.off_tail_t == 4 * p.NR * p.tail_pairs + 4);
    } else {
        CHECK(img.empty() || st == ldsplan::ROWS_DO_NOT_FIT);
    }
    uint64_t h = 1469598103934665603ull;                 // FNV-1a over the image's bytes
    const unsigned char* b = reinterpret_cast<const unsigned char*>(img.data());
    for (size_t i = 0; i < img.size() * sizeof(int); ++i) h = (h ^ b[i]) * 1099511628211ull;
    const int64_t k = p.instance;
    char name[128] = "";
    if (k >= 0)
        snprintf(name, sizeof(name), "k_admm_lds<%d, %s, %d, %s, %d, %d, %s, %d>", (int)(k & 0xFF), (k >> 8 & 1) ? "true" : "false",
                 (int)(k >> 21 & 0x7FF), (k >> 9 & 1) ? "true" : "false", (int)(k >> 11 & 0x1F), (int)(k >> 16 & 0x1F),
                 (k >> 10 & 1) ? "true" : "false", (int)(k >> 32 & 0xFF) - 1);
    printf("{\"status\": %d, \"ok\": %d, \"G\": %d, \"TPG\": %d, \"TS\": %d, \"nthreads\": %d, \"block\": %d, \"NR\": %d, \"csr_ints\": %d, "
           "\"maxt\": %d, \"sb\": %d, \"uniform45\": %d, \"slots\": %d, \"tail_pairs\": %d, \"lds_img0\": %d, \"lds_img_ints\": %d, "
           "\"off_rp_u\": %d, \"off_rp_d\": %d, \"off_en_u\": %d, \"off_en_d\": %d, \"off_lead_t\": %d, \"off_tail_t\": %d, \"off_diag\": %d, "
           "\"row_order\": %d, \"off_node\": %d, \"off_rown\": %d, \"npos_word\": \"%016" PRIx64 "\", \"lds_bytes\": %zu, "
           "\"cg_barriers\": %d, \"instance\": %" PRId64 ", \"instance_name\": \"%s\", \"image_ints\": %zu, \"image_hash\": \"%016" PRIx64 "\"}\n",
           (int)st, (int)p.ok, p.G, p.TPG, p.TS, p.nthreads, p.block, p.NR, p.csr_ints, p.maxt, p.sb, p.uniform45, p.slots, p.tail_pairs,
           p.lds_img0, p.lds_img_ints, p.off_rp_u, p.off_rp_d, p.off_en_u, p.off_en_d, p.off_lead_t, p.off_tail_t, p.off_diag,
           p.row_order, p.off_node, p.off_rown, p.npos_word, p.lds_bytes, p.cg_barriers, k, name, img.size(), h);
    return 0;
}
