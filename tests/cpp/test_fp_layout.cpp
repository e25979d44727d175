// Host test of the FullProcessing layout (deoss_amd/csrc/fp_layout.hpp): no GPU, built plain and
// with ASan/UBSan by tests/test_fp_host.py.
//
// For (k, m) in {(4, 8), (1, 1), (8, 4), (3, 2)} and ns in {1, 2, 5} segments:
//  1. frag_ptr and the leaf table equal an independent triple loop written here; a table over
//     several pieces is the segments of all pieces, then the fragments of all pieces (the rule of
//     the processing stream's batches); the fragments-only table is its second part;
//  2. the striped digest order is a bijection onto [0, ns * (1 + total)) and striped_to_one_pass
//     reproduces the one-pass order;
//  3. the pending-file tags round-trip (fragment id 0, segment 0 = ~0, ids up to 2^40);
//  4. slot geometry, including a slot smaller than one segment.
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "../../deoss_amd/csrc/fp_layout.hpp"

using namespace dm_fp;

static int failures = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures++ < 20) {                                         \
                std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);  \
                std::fprintf(stderr, __VA_ARGS__);                         \
                std::fprintf(stderr, "\n");                                \
            }                                                              \
        }                                                                  \
    } while (0)

static const int kShapes[4][2] = {{4, 8}, {1, 1}, {8, 4}, {3, 2}};
static const uint64_t kSegs[3] = {1, 2, 5};

// A piece of ns segments in one buffer: the segments, then their parity (as a stream chunk).
struct Buf {
    std::vector<uint8_t> mem;
    uint64_t ns;
    Buf(const FpLayout& L, uint64_t n) : mem(n * (L.seg + L.pbytes)), ns(n) {}
    const uint8_t* data() const { return mem.data(); }
    const uint8_t* parity(const FpLayout& L) const { return mem.data() + ns * L.seg; }
};

// The table stated independently of fp_layout.hpp (only k, m and seg are read): the segments of
// every piece, then for every piece, segment and fragment index the fragment's address.
static void expect_table(const FpLayout& L, const std::vector<Buf>& bufs, bool segments, std::vector<uint64_t>& addr,
                         std::vector<uint64_t>& lens) {
    addr.clear();
    lens.clear();
    if (segments)
        for (const Buf& b : bufs)
            for (uint64_t t = 0; t < b.ns; t++) {
                addr.push_back(reinterpret_cast<uint64_t>(b.data() + t * L.seg));
                lens.push_back(L.seg);
            }
    for (const Buf& b : bufs)
        for (uint64_t t = 0; t < b.ns; t++)
            for (int j = 0; j < L.k + L.m; j++) {
                const uint8_t* p = j < L.k ? b.data() + t * L.seg + (uint64_t)j * (L.seg / L.k)
                                           : b.parity(L) + t * (uint64_t)L.m * (L.seg / L.k) +
                                                 (uint64_t)(j - L.k) * (L.seg / L.k);
                addr.push_back(reinterpret_cast<uint64_t>(p));
                lens.push_back(L.seg / L.k);
            }
}

static void check_tables(const FpLayout& L, int k, int m) {
    CHECK(L.k == k && L.m == m && L.total == k + m && L.frag == L.seg / (uint64_t)k && L.pbytes == (uint64_t)m * L.frag,
          "layout fields k=%d m=%d", k, m);
    for (uint64_t ns : kSegs) {
        std::vector<Buf> one;
        one.emplace_back(L, ns);
        // frag_ptr against the loop
        for (uint64_t t = 0; t < ns; t++)
            for (int j = 0; j < L.total; j++) {
                const uint8_t* want = j < k ? one[0].data() + t * L.seg + (uint64_t)j * L.frag
                                            : one[0].parity(L) + (t * (uint64_t)m + (uint64_t)(j - k)) * L.frag;
                CHECK(L.frag_ptr(one[0].data(), one[0].parity(L), t, j) == want, "frag_ptr k=%d m=%d t=%llu j=%d", k, m,
                      (unsigned long long)t, j);
            }
        // one piece, with and without segments; then three pieces of ns, 1 and ns + 1 segments
        for (int shape = 0; shape < 2; shape++) {
            std::vector<Buf> bufs;
            bufs.emplace_back(L, ns);
            if (shape == 1) {
                bufs.emplace_back(L, 1);
                bufs.emplace_back(L, ns + 1);
            }
            std::vector<FpPiece> pieces;
            uint64_t all = 0;
            for (const Buf& b : bufs) {
                pieces.push_back({b.data(), b.parity(L), b.ns});
                all += b.ns;
            }
            for (int segments = 0; segments < 2; segments++) {
                std::vector<uint64_t> wa, wl;
                expect_table(L, bufs, segments != 0, wa, wl);
                const uint64_t T = segments ? L.leaves(all) : all * (uint64_t)L.total;
                CHECK(wa.size() == T, "table size k=%d m=%d ns=%llu", k, m, (unsigned long long)ns);
                std::vector<uint64_t> addr(T, 0), lens(T, 0);
                const uint64_t got = leaf_table(L, pieces.data(), pieces.size(), segments != 0, addr.data(), lens.data());
                CHECK(got == T, "leaf_table count %llu, want %llu", (unsigned long long)got, (unsigned long long)T);
                CHECK(addr == wa && lens == wl, "leaf_table k=%d m=%d ns=%llu pieces=%zu segments=%d", k, m,
                      (unsigned long long)ns, pieces.size(), segments);
            }
            // the one-pass digest slots name the rows of the (single-piece) table
            if (shape == 0) {
                std::vector<uint64_t> addr(L.leaves(ns)), lens(L.leaves(ns));
                leaf_table(L, pieces.data(), 1, true, addr.data(), lens.data());
                for (uint64_t t = 0; t < ns; t++) {
                    CHECK(addr[L.seg_slot(t)] == reinterpret_cast<uint64_t>(bufs[0].data() + t * L.seg), "seg_slot");
                    for (int j = 0; j < L.total; j++)
                        CHECK(addr[L.frag_slot(ns, t, j)] ==
                                  reinterpret_cast<uint64_t>(L.frag_ptr(bufs[0].data(), bufs[0].parity(L), t, j)),
                              "frag_slot t=%llu j=%d", (unsigned long long)t, j);
                }
            }
        }
    }
}

static void check_striped(const FpLayout& L) {
    for (uint64_t ns : kSegs) {
        const uint64_t T = L.leaves(ns);
        CHECK(T == ns * (1 + (uint64_t)L.total), "leaves");
        std::set<uint64_t> seen;
        for (uint64_t t = 0; t < ns; t++) seen.insert(L.seg_slot(t));
        for (uint64_t t = 0; t < ns; t++)
            for (int j = 0; j < L.total; j++) {
                const uint64_t s = L.striped_frag_slot(ns, t, j);
                CHECK(s >= ns && s < T, "striped slot %llu out of [ns, T)", (unsigned long long)s);
                seen.insert(s);
                // the formulas of the striped pass: a row of ns per data fragment index, then parity by segment
                const uint64_t want = j < L.k ? ns * (1 + (uint64_t)j) + t
                                              : ns * (1 + (uint64_t)L.k) + t * (uint64_t)L.m + (uint64_t)(j - L.k);
                CHECK(s == want, "striped slot k=%d m=%d t=%llu j=%d", L.k, L.m, (unsigned long long)t, j);
            }
        CHECK(seen.size() == T && *seen.begin() == 0 && *seen.rbegin() == T - 1, "striped map is no bijection (k=%d m=%d ns=%llu)",
              L.k, L.m, (unsigned long long)ns);
        // digest of a leaf = its one-pass slot, written at its striped slot
        std::vector<uint8_t> lv(32 * T), want(32 * T), got(32 * T, 0xee);
        auto put = [](uint8_t* d, uint64_t v) {
            for (int b = 0; b < 32; b++) d[b] = (uint8_t)(v * 131 + (uint64_t)b * 7 + (v >> 8));
        };
        for (uint64_t t = 0; t < ns; t++) {
            put(lv.data() + 32 * L.seg_slot(t), L.seg_slot(t));
            put(want.data() + 32 * L.seg_slot(t), L.seg_slot(t));
            for (int j = 0; j < L.total; j++) {
                put(lv.data() + 32 * L.striped_frag_slot(ns, t, j), L.frag_slot(ns, t, j));
                put(want.data() + 32 * L.frag_slot(ns, t, j), L.frag_slot(ns, t, j));
            }
        }
        L.striped_to_one_pass(ns, lv.data(), got.data(), got.data() + 32 * ns);
        CHECK(got == want, "striped_to_one_pass k=%d m=%d ns=%llu", L.k, L.m, (unsigned long long)ns);
    }
}

static void check_tags() {
    const FpLayout L(4, 8, 4096 * 4);
    CHECK(L.frag_id(0, 0) == 0 && L.frag_id(3, 5) == 3 * 12 + 5, "frag_id");
    CHECK(frag_tag(0) == 0 && !tag_is_seg(frag_tag(0)) && tag_offset(frag_tag(0)) == 0, "fragment id 0");
    CHECK(seg_tag(0) == ~0ull && tag_is_seg(seg_tag(0)) && tag_offset(seg_tag(0)) == 0, "segment 0");
    const uint64_t ids[] = {0, 1, 11, 12, 255, 1ull << 20, (1ull << 40) - 1, 1ull << 40};
    for (uint64_t id : ids) {
        CHECK(!tag_is_seg(frag_tag(id)) && tag_offset(frag_tag(id)) == 32 * id, "fragment tag %llu", (unsigned long long)id);
        CHECK(tag_is_seg(seg_tag(id)) && tag_offset(seg_tag(id)) == 32 * id, "segment tag %llu", (unsigned long long)id);
        CHECK(frag_tag(id) != seg_tag(id), "tags collide at %llu", (unsigned long long)id);
    }
    std::vector<uint8_t> segd(32 * 3), fragd(32 * 3 * 12);
    for (uint64_t gs = 0; gs < 3; gs++) {
        CHECK(tag_digest(segd.data(), fragd.data(), seg_tag(gs)) == segd.data() + 32 * gs, "tag_digest segment");
        for (int j = 0; j < 12; j++)
            CHECK(tag_digest(segd.data(), fragd.data(), frag_tag(L.frag_id(gs, j))) == fragd.data() + 32 * (gs * 12 + j),
                  "tag_digest fragment");
    }
}

static void check_slots() {
    const FpLayout L(4, 8, 4096 * 4);   // seg 16 KiB, parity 32 KiB per segment
    struct {
        uint64_t slot, spd, spp, cap;
    } cases[] = {
        {64ull << 20, 4096, 2048, 64ull << 20},
        {16384, 1, 1, 32768},     // one segment; less than one parity set
        {1000, 1, 1, 32768},      // smaller than one segment: still one of each
        {32768, 2, 1, 32768},
        {100000, 6, 3, 98304},    // whole segments / parity sets only
    };
    for (const auto& c : cases) {
        const FpSlots s = fp_slots(L, c.slot);
        CHECK(s.spd == c.spd && s.spp == c.spp && s.cap == c.cap, "slot %llu: spd %llu spp %llu cap %llu",
              (unsigned long long)c.slot, (unsigned long long)s.spd, (unsigned long long)s.spp, (unsigned long long)s.cap);
    }
    const FpLayout P(8, 4, 8 * 16);   // parity smaller than the segment
    const FpSlots s = fp_slots(P, 300);
    CHECK(s.spd == 2 && s.spp == 4 && s.cap == 256, "parity-light layout: %llu %llu %llu", (unsigned long long)s.spd,
          (unsigned long long)s.spp, (unsigned long long)s.cap);
}

int main() {
    for (const auto& sh : kShapes) {
        const FpLayout L(sh[0], sh[1], (uint64_t)sh[0] * 64);   // 64-byte fragments
        check_tables(L, sh[0], sh[1]);
        check_striped(L);
    }
    check_tags();
    check_slots();
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("fp layout OK\n");
    return 0;
}
