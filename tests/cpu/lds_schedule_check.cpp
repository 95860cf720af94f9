// CPU replay of the outer-loop schedule of the LDS-resident path (mixed-graph-admm_amd/csrc/lds_schedule.h).
//   lds_schedule_check
// For every max_it in 1 .. 70 and every chunk request in 1 .. 16 (CHUNKS), and every max_it for SYNC and DEVSTOP, it issues
// what Engine::solve_lds issues, in its order: launch c on the main stream (reads the slot of iterate it0, writes the slots
// of it0 + 1 .. it0 + Jc and metric set c), the metric kernels of chunk c on the helper stream (read the slots of
// it0 .. it0 + Jc and the set), and the event records and waits the header names.  Happens-before is stream order plus those
// events (a vector clock per stream).  Checked: (a) no write of a slot or a set before an earlier read of it (nor a read
// before the write it needs); (b) an event slot a wait names was last recorded by the chunk the wait is meant for; (c) the
// slot layout; (d) the lagged-read ring; (e) the same checker reports a hazard on the round-3 variant "two sets, three
// boundary buffers" with the wait three chunks back.  Prints one JSON object with J, the slot count and hashes of the slot
// and chunk tables (tests/golden/lds_schedule_parent.json); exit status 1 and a FAILED line when a check does not hold.
#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>
#include "lds_schedule.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return false; } } while (0)

struct Hash {                                            // 64-bit FNV-1a over a sequence of ints
    uint64_t h = 1469598103934665603ull;
    void add(int v) { for (int i = 0; i < 4; ++i) h = (h ^ (((uint32_t)v >> (8 * i)) & 0xFF)) * 1099511628211ull; }
};

struct Real : ldssched::Schedule {                       // the header's schedule; launch c waits for the metrics of chunk c - 3
    explicit Real(const ldssched::Schedule& s) : ldssched::Schedule(s) {}
    static int wait_back() { return LDS_SETS; }
};
struct Round3Wrong {                                     // two sets, three boundary buffers, but the wait of today: a hazard
    int J, max_it;
    static int wait_back() { return 3; }
    int slots() const { return 2 * (J - 1) + 3; }
    int slot_of_iterate(int k) const {
        if (k == max_it) return ldssched::X_OUT;
        return k % J == 0 ? (k / J) % 3 : 3 + ((k / J) % 2) * (J - 1) + (k % J - 1);
    }
    int chunks() const { return (max_it + J - 1) / J; }
    ldssched::Chunk chunk(int c) const { return {c * J, J < max_it - c * J ? J : max_it - c * J, c % 2, c % 3, c >= 3 ? (c - 3) % 3 : -1}; }
    static int join(int n) { return n > 0 ? (n - 1) % 3 : -1; }
};

struct Clock { int at[2] = {0, 0}; };                    // what a stream has seen of the main (0) and the helper (1) stream
struct Event { Clock seen; int chunk = -1; };
struct Access { int stream, pos; };
struct Resource { Access written{0, 0}; std::vector<Access> reads; };      // (iterate 0: written before the loop)

// true when the replay of CHUNKS over `s` meets no hazard and the layout holds; `why` names the first failure
template <class Sched>
bool replay_chunks(const Sched& s, std::string& why) {
    const int nslot = s.slots();
    std::vector<Resource> res(nslot + 1 + 8);            // slots, x_out, metric sets
    auto slot_res = [&](int k) -> Resource& { const int sl = s.slot_of_iterate(k); return res[sl == ldssched::X_OUT ? nslot : sl]; };
    Clock now[2];
    Event ev_main[8], ev_side[8];
    auto join = [](Clock& c, const Clock& o) { for (int i = 0; i < 2; ++i) if (o.at[i] > c.at[i]) c.at[i] = o.at[i]; };
    auto before = [&](const Access& a, int stream) { return now[stream].at[a.stream] >= a.pos; };
    auto read = [&](Resource& r, int stream, const char* what, int c) {
        if (!before(r.written, stream)) { why = std::string("read before write: ") + what + " chunk " + std::to_string(c); return false; }
        r.reads.push_back({stream, now[stream].at[stream]});
        return true;
    };
    auto write = [&](Resource& r, int stream, const char* what, int c) {
        for (const Access& a : r.reads)
            if (!before(a, stream)) { why = std::string("write before a pending read: ") + what + " launch " + std::to_string(c); return false; }
        r.reads.clear();
        r.written = {stream, now[stream].at[stream]};
        return true;
    };
    for (int k = 0; k <= s.max_it; ++k) {                // (c) layout
        const int sl = s.slot_of_iterate(k);
        if ((sl == ldssched::X_OUT) != (k == s.max_it) || sl >= nslot || sl < ldssched::X_OUT) { why = "slot out of range"; return false; }
    }
    const int n = s.chunks();
    for (int c = 0; c < n; ++c) {
        const ldssched::Chunk ch = s.chunk(c);
        if (ch.it0 != c * s.J || ch.Jc < 1 || ch.Jc > s.J || ch.it0 + ch.Jc > s.max_it || (c == n - 1) != (ch.it0 + ch.Jc == s.max_it)) { why = "chunk bounds"; return false; }
        for (int i = 0; i <= ch.Jc; ++i)
            for (int j = i + 1; j <= ch.Jc; ++j)
                if (s.slot_of_iterate(ch.it0 + i) == s.slot_of_iterate(ch.it0 + j)) { why = "two iterates of a chunk share a slot"; return false; }
        Resource& set = res[nslot + 1 + ch.set];
        // main stream: wait, launch, record
        if (ch.wait >= 0) {
            if (ev_side[ch.wait].chunk != c - s.wait_back()) { why = "launch " + std::to_string(c) + " waits on an event of chunk " + std::to_string(ev_side[ch.wait].chunk); return false; }
            join(now[0], ev_side[ch.wait].seen);
        }
        ++now[0].at[0];
        if (!read(slot_res(ch.it0), 0, "iterate", c)) return false;
        for (int k = 1; k <= ch.Jc; ++k) if (!write(slot_res(ch.it0 + k), 0, "iterate slot", c)) return false;
        if (!write(set, 0, "metric set", c)) return false;
        ev_main[ch.ev] = {now[0], c};
        // helper stream: wait for the launch, metrics, record
        if (ev_main[ch.ev].chunk != c) { why = "ev_main"; return false; }
        join(now[1], ev_main[ch.ev].seen);
        ++now[1].at[1];
        for (int k = 0; k <= ch.Jc; ++k) if (!read(slot_res(ch.it0 + k), 1, "iterate", c)) return false;
        if (!read(set, 1, "metric set", c)) return false;
        ev_side[ch.ev] = {now[1], c};
    }
    const int j = s.join(n);
    if (j < 0 || ev_side[j].chunk != n - 1) { why = "the join names chunk " + std::to_string(j < 0 ? -1 : ev_side[j].chunk); return false; }
    join(now[0], ev_side[j].seen);
    if (now[0].at[1] != now[1].at[1]) { why = "helper stream not joined"; return false; }
    return true;
}

// (d) the host reads, at step c, the word and the event written at step c - lag, and no word is rewritten unread
static bool lag_ring(int lag, int steps) {
    std::vector<int> word(lag + 1, -1), event(lag + 1, -1);
    std::vector<bool> unread(lag + 1, false);
    for (int c = 0; c < steps; ++c) {
        const ldssched::LagStep l = ldssched::lag_step(c, lag);
        CHECK(l.put >= 0 && l.put <= lag && !unread[l.put]);
        word[l.put] = event[l.put] = c;
        unread[l.put] = true;
        CHECK((l.get >= 0) == (c >= lag));
        if (l.get < 0) continue;
        CHECK(l.get <= lag && word[l.get] == c - lag && event[l.get] == c - lag && unread[l.get]);
        unread[l.get] = false;
    }
    return true;
}

static bool run() {
    using ldssched::Schedule;
    printf("{\"pick\": [");                              // kind and per_sample for async, record, check_stop, per_sample_conv = bits 3 .. 0
    for (int f = 0; f < 16; ++f) {
        const Schedule s = Schedule::pick(f & 8, f & 4, f & 2, f & 1, 5, 9);
        CHECK(s.max_it == 9 && s.J == (s.kind == ldssched::CHUNKS ? 5 : 1));
        printf("%s[%d, %d]", f ? ", " : "", (int)s.kind, (int)s.per_sample);
    }
    printf("],\n\"rows\": {");
    const char* const names[3] = {"SYNC", "DEVSTOP", "CHUNKS"};
    std::string why;
    int max_slots_j4 = 0;
    for (int kind = 0; kind < 3; ++kind) {
        for (int req = 1; req <= (kind == ldssched::CHUNKS ? LDS_MAXJ : 1); ++req) {
            Hash iterates, chunks;
            std::string js, slots;
            for (int max_it = 1; max_it <= 70; ++max_it) {
                const Schedule s = Schedule::pick(kind != ldssched::SYNC, false, kind == ldssched::DEVSTOP, false, req, max_it);
                CHECK((int)s.kind == kind && !s.per_sample && s.J >= 1 && s.J <= LDS_MAXJ && s.J <= (req < max_it ? req : max_it));
                js += (max_it > 1 ? ", " : "") + std::to_string(s.J);
                slots += (max_it > 1 ? ", " : "") + std::to_string(s.slots());
                iterates.add(max_it);
                for (int k = 0; k <= max_it; ++k) iterates.add(s.slot_of_iterate(k));
                if (kind != ldssched::CHUNKS) {           // one stream: an iteration reads one slot and writes the other
                    CHECK(s.slots() == 2 && s.chunks() == max_it);
                    for (int k = 0; k <= max_it; ++k) {
                        const int sl = s.slot_of_iterate(k);
                        CHECK(k == max_it ? sl == ldssched::X_OUT : (sl == 0 || sl == 1));
                        CHECK(k == 0 || sl != s.slot_of_iterate(k - 1));
                    }
                    continue;
                }
                if (s.J <= 4 && s.slots() > max_slots_j4) max_slots_j4 = s.slots();
                if (!replay_chunks(Real(s), why)) { printf("FAILED (max_it %d, J %d): %s\n", max_it, s.J, why.c_str()); return false; }
                // the per-sample stop takes the same slots (one stream, no events)
                const Schedule ps = Schedule::pick(true, false, true, true, req, max_it);
                CHECK(ps.kind == ldssched::CHUNKS && ps.per_sample && ps.J == s.J && ps.slots() == s.slots());
                for (int k = 0; k <= max_it; ++k) CHECK(ps.slot_of_iterate(k) == s.slot_of_iterate(k));
                chunks.add(max_it);
                chunks.add(s.chunks());
                for (int c = 0; c < s.chunks(); ++c) {
                    const ldssched::Chunk ch = s.chunk(c);
                    for (int v : {ch.it0, ch.Jc, ch.set, ch.wait, ch.ev}) chunks.add(v);
                }
                chunks.add(Schedule::join(s.chunks()));
            }
            printf("%s\n\"%s/%d\": {\"J\": [%s], \"slots\": [%s], \"iterates\": \"%016" PRIx64 "\", \"chunks\": \"%016" PRIx64 "\"}",
                   kind || req > 1 ? "," : "", names[kind], req, js.c_str(), slots.c_str(), iterates.h, chunks.h);
        }
    }
    CHECK(max_slots_j4 == 13 && max_slots_j4 <= 15);      // the workspace vectors hold every slot of J <= 4
    printf("},\n\"lag\": [");
    for (int c = 0; c < 12; ++c) printf("%s[%d, %d]", c ? ", " : "", ldssched::lag_step(c, 2).put, ldssched::lag_step(c, 2).get);
    printf("],\n");
    for (int lag = 1; lag <= 4; ++lag) CHECK(lag_ring(lag, 40));
    // (e) the checker can fail: the first (max_it, J) at which the wrong variant shows its hazard
    int hazards = 0, first_it = 0, first_j = 0;
    std::string first_why;
    for (int J = 1; J <= LDS_MAXJ; ++J)
        for (int max_it = 1; max_it <= 70; ++max_it) {
            const bool ok = replay_chunks(Round3Wrong{J, max_it}, why);
            CHECK(ok == (max_it <= 2 * J));              // it takes a third launch to overwrite what chunk 0's metrics read
            if (!ok && !hazards++) { first_it = max_it; first_j = J; first_why = why; }
        }
    CHECK(hazards > 0 && first_why.find("write before a pending read") == 0);
    printf("\"wrong_variant\": {\"hazards\": %d, \"first\": [%d, %d], \"why\": \"%s\"}}\n", hazards, first_it, first_j, first_why.c_str());
    return true;
}

int main() { return run() ? 0 : 1; }
