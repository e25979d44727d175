// Host check of K1Q's ring and barrier schedule (deoss_amd/csrc/quad_ring.hpp): a producer and a
// consumer state machine, built from the same constexpr functions the two waves of
// leaf_kernel_quad use and following the kernel's control flow, are stepped through every stage
// count 0 .. 8 and through waves of two leaf classes with every pair of block counts 0 .. 40.
// Asserted: both sides execute the same number of barriers; no read or prefetch touches a slot
// whose stage is not complete; no write touches a slot with a read still to come; the stream of
// every run fills once and drains at the run's last block, with every block's words in the
// register set it is read from; the per-block path reads its stage's slot; every leaf hashes
// exactly its blocks.  Depth 3 is the wide kernel (one stream per run of stages), depth 2 the
// schedule of the compact kernel (one stream per stage).  Stand-alone: prints "quad ring OK".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../deoss_amd/csrc/quad_ring.hpp"

namespace qr = dm::quad_ring;

#define CHECK(c)                                                                         \
    do {                                                                                 \
        if (!(c)) {                                                                      \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s  [%s]\n", __FILE__, __LINE__, #c, g_case); \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

static char g_case[128];
constexpr int kLeaves = 8;

struct Access {
    uint64_t stage;
    uint32_t slot;
    uint64_t interval;   // 0: before barrier 0; b + 1: between barrier b and barrier b + 1
};

struct Wave {
    bool active[kLeaves];
    uint64_t nb[kLeaves];
    uint64_t ni() const {
        uint64_t m = 0;
        for (int l = 0; l < kLeaves; l++) m = nb[l] > m ? nb[l] : m;
        return qr::stages(m);
    }
};

// ---- producer: leaf_kernel_quad's first wave ----
struct Producer {
    std::vector<Access> writes;
    uint64_t barriers = 0;
    void run(uint64_t NI, int depth) {
        uint32_t slot = 0;
        for (uint64_t s = 0; s < qr::stages_before_first_barrier(depth); s++) {
            if (s < NI) writes.push_back({s, slot, barriers});
            slot = qr::next_slot(slot, depth);
        }
        barriers++;
        for (uint64_t it = 0; it < NI; it++) {
            const uint64_t s = qr::stage_written_after_barrier(it, depth);
            if (s < NI) writes.push_back({s, slot, barriers});
            slot = qr::next_slot(slot, depth);
            barriers++;
        }
    }
};

// ---- consumer: leaf_kernel_quad's second wave ----
struct Consumer {
    struct Set {
        uint64_t stage = ~0ull;
        uint32_t block = ~0u;
        bool ready = false;   // waited for since it was issued
    };
    std::vector<Access> reads;
    uint64_t barriers = 0;
    bool stream_open = false;
    uint64_t fills = 0, drains = 0, runs = 0;
    uint64_t hashed[kLeaves] = {}, final_at[kLeaves] = {};
    Set sets[qr::kSets];

    void load(uint64_t stage, uint32_t slot, uint32_t block) {
        reads.push_back({stage, slot, barriers});
        sets[qr::set_of(block)] = Set{stage, block, false};
    }
    void wait() {
        for (Set& s : sets) s.ready = true;
    }
    // a run of n whole stages from stage `it` (slot `slot`), `stream`: one stream per run
    uint32_t run_stages(const Wave& w, const bool (&running)[kLeaves], uint64_t it, uint32_t slot, uint64_t n,
                        int depth) {
        runs++;
        for (uint32_t k = 0; k < (uint32_t)qr::kAhead; k++) load(it, slot, k);
        for (uint64_t s = 0; s < n; s++) {
            const bool last = s + 1 == n;
            const uint32_t nslot = qr::next_slot(slot, depth);
            for (uint32_t k = 0; k < (uint32_t)qr::kBlocks; k++) {
                wait();
                if (qr::block_prefetches(k, last)) {
                    const qr::BlockRef pf = qr::prefetch_of(k);
                    load(it + s + pf.dstage, pf.dstage ? nslot : slot, pf.block);
                }
                const Set& cur = sets[qr::set_of(k)];
                CHECK(cur.ready && cur.stage == it + s && cur.block == k);
                if (s == 0 && k == 0) {
                    CHECK(!stream_open);
                    stream_open = true;
                    fills++;
                } else {
                    CHECK(stream_open);
                }
                if (qr::block_links(k, last)) {
                    // the link reads the next block's first words
                    const Set& nx = sets[qr::set_of(k + 1)];
                    CHECK(nx.ready && nx.stage == it + s + (k + 1) / qr::kBlocks && nx.block == (k + 1) % qr::kBlocks);
                } else {
                    stream_open = false;
                    drains++;
                }
                for (int l = 0; l < kLeaves; l++)
                    if (running[l]) hashed[l]++;
            }
            barriers++;
            slot = nslot;
            CHECK(stream_open == !last);
        }
        (void)w;
        return slot;
    }
    void run(const Wave& w, int depth, bool xstage) {
        const uint64_t NS = w.ni();
        uint32_t slot = 0;
        barriers++;
        for (uint64_t it = 0; it < NS;) {
            bool running[kLeaves];
            uint64_t end = ~0ull;
            for (int l = 0; l < kLeaves; l++) {
                running[l] = qr::leaf_running(w.active[l], w.nb[l], it);
                const uint64_t e = qr::leaf_run_end(running[l], w.nb[l], NS);
                end = e < end ? e : end;
            }
            if (xstage) {
                if (it < end) {
                    slot = run_stages(w, running, it, slot, end - it, depth);
                    it = end;
                }
            } else {
                for (; it < end; it++) slot = run_stages(w, running, it, slot, 1, depth);
            }
            for (int l = 0; l < kLeaves; l++)
                if (running[l]) final_at[l] = hashed[l];
            if (it == NS) break;
            bool inside = false;
            for (int l = 0; l < kLeaves; l++) inside |= qr::leaf_ends_inside(w.active[l], w.nb[l], it);
            if (!inside) continue;
            // the per-block path: no stream, 16 reads of the stage's slot per block
            CHECK(!stream_open);
            for (uint32_t k = 0; k < (uint32_t)qr::kBlocks; k++) {
                reads.push_back({it, slot, barriers});
                for (int l = 0; l < kLeaves; l++)
                    if (it * qr::kBlocks + k < w.nb[l]) hashed[l]++;
            }
            for (int l = 0; l < kLeaves; l++)
                if (w.nb[l] > it * qr::kBlocks) final_at[l] = hashed[l];
            barriers++;
            it++;
            slot = qr::next_slot(slot, depth);
        }
        CHECK(!stream_open && fills == drains && fills == runs);
    }
};

static uint64_t g_waves = 0, g_reads = 0;

static void check_wave(const Wave& w, int depth, bool xstage) {
    const uint64_t NI = w.ni();
    Producer p;
    p.run(NI, depth);
    Consumer c;
    c.run(w, depth, xstage);
    CHECK(p.barriers == qr::barriers(NI) && c.barriers == p.barriers);
    // every stage is written once, into its slot, before the barrier that publishes it
    CHECK(p.writes.size() == NI);
    for (uint64_t s = 0; s < NI; s++) {
        CHECK(p.writes[s].stage == s && p.writes[s].slot == qr::slot_of(s, depth));
        CHECK(s < qr::complete_after_barrier(p.writes[s].interval, depth));
    }
    for (const Access& r : c.reads) {
        CHECK(r.stage < NI);                                  // never a stage the producer does not write
        CHECK(r.slot == qr::slot_of(r.stage, depth));
        CHECK(r.interval >= 1 && r.stage < qr::complete_after_barrier(r.interval - 1, depth));
        CHECK(p.writes[r.stage].interval < r.interval);       // complete: written in an earlier interval
        // the slot is not written again (by any later stage) until a later interval
        for (uint64_t s = r.stage + (uint64_t)depth; s < NI; s += (uint64_t)depth) CHECK(p.writes[s].interval > r.interval);
    }
    for (int l = 0; l < kLeaves; l++) {
        const uint64_t want = w.active[l] ? w.nb[l] : 0;
        if (w.active[l]) CHECK(c.final_at[l] == want);
    }
    g_waves++;
    g_reads += c.reads.size();
}

int main() {
    for (int depth = 2; depth <= qr::kWideDepth; depth++) {
        const bool xstage = depth == qr::kWideDepth;
        // every stage count 0 .. 8, all leaves alike, with and without a partial last stage
        for (uint64_t ns = 0; ns <= 8; ns++) {
            for (uint64_t extra = 0; extra < (uint64_t)qr::kBlocks; extra++) {
                Wave w;
                for (int l = 0; l < kLeaves; l++) {
                    w.active[l] = true;
                    w.nb[l] = ns * qr::kBlocks + extra;
                }
                std::snprintf(g_case, sizeof g_case, "depth %d stages %llu + %llu blocks", depth,
                              (unsigned long long)ns, (unsigned long long)extra);
                check_wave(w, depth, xstage);
            }
        }
        // two leaf classes in one wave, every pair of block counts; the second class active or not
        for (uint64_t a = 0; a <= 40; a++) {
            for (uint64_t b = 0; b <= 40; b++) {
                for (int inactive = 0; inactive < 2; inactive++) {
                    Wave w;
                    for (int l = 0; l < kLeaves; l++) {
                        const bool second = l >= 3;   // 3 + 5 leaves
                        w.active[l] = !(second && inactive);
                        w.nb[l] = second ? (inactive ? 0 : b) : a;
                    }
                    std::snprintf(g_case, sizeof g_case, "depth %d nb %llu / %llu%s", depth, (unsigned long long)a,
                                  (unsigned long long)b, inactive ? " (inactive)" : "");
                    check_wave(w, depth, xstage);
                }
            }
        }
    }
    // the slot walk of both waves is the stage's slot
    for (int depth = 2; depth <= 3; depth++) {
        uint32_t slot = 0;
        for (uint64_t s = 0; s < 100; s++) {
            CHECK(slot == qr::slot_of(s, depth));
            slot = qr::next_slot(slot, depth);
        }
    }
    std::printf("quad ring OK: %llu waves, %llu ring reads checked\n", (unsigned long long)g_waves,
                (unsigned long long)g_reads);
    return 0;
}
