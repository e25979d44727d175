// Host test of the range plan (deoss_amd/csrc/range_plan.hpp): no GPU, built plain and with
// ASan/UBSan by tests/test_range_plan_host.py.
//
//  1. exhaustive at segment = 128, k = 4 (32-byte fragments, two AES blocks each): every valid size
//     of {1, 112, 113, 128, 129, 300, 384}, with and without a cipher, both settings of the padding
//     flag, every (off, len): seg0, ntouched, need and the windows against a model that walks the
//     range byte by byte;
//  2. other shapes: k = 1, k = 8, a fragment of one block, a segment of two blocks;
//  3. every error: an empty range, one that leaves the object (also by overflow), a size that does
//     not end in the last piece, a segment a cipher cannot use, a segment that is no multiple of
//     16 x k.
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "../../deoss_amd/csrc/range_plan.hpp"

using namespace dm_range;

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

struct Model {
    uint64_t seg0 = 0, ntouched = 0;
    std::map<uint64_t, std::set<uint64_t>> need;      // segment -> data fragments
    std::map<uint64_t, std::set<uint64_t>> blocks;    // segment -> blocks decrypted for the range (cipher) / bytes (none)
    std::set<uint64_t> pad;                           // segments whose padding is checked
};

// Byte by byte: where plaintext byte x lies, what decrypting it needs.
static Model model(uint64_t segment, int k, bool cipher, uint64_t off, uint64_t len, int flags) {
    Model m;
    const uint64_t piece = cipher ? segment - 16 : segment, frag = segment / k, n = segment / 16;
    m.seg0 = off / piece;
    for (uint64_t x = off; x < off + len; x++) {
        const uint64_t s = x / piece, o = x % piece;
        if (!cipher) {
            m.need[s].insert(o / frag);
            m.blocks[s].insert(o);
            continue;
        }
        const uint64_t b = o / 16;
        m.blocks[s].insert(b);
        m.need[s].insert(16 * b / frag);
        if (b > 0) m.need[s].insert(16 * (b - 1) / frag);   // the predecessor block; the IV before block 0
    }
    m.ntouched = m.need.size();
    if (cipher)
        for (auto& e : m.need) {
            const bool first = e.first == m.seg0 && !(flags & kNoPaddingCheck);
            if (!first && !e.second.count((uint64_t)k - 1)) continue;
            m.pad.insert(e.first);
            e.second.insert(16 * (n - 1) / frag);
            if (!m.blocks[e.first].count(n - 2)) e.second.insert(16 * (n - 2) / frag);   // the padding block's predecessor
        }
    return m;
}

static uint64_t compare(uint64_t size, uint64_t nseg, uint64_t segment, int k, bool cipher, uint64_t off, uint64_t len,
                        int flags) {
    Plan p;
    const std::string err = plan(size, nseg, segment, k, cipher, off, len, flags, p);
    CHECK(err.empty(), "plan(%llu, %llu, %llu): %s", (unsigned long long)size, (unsigned long long)off,
          (unsigned long long)len, err.c_str());
    if (!err.empty()) return 0;
    const Model m = model(segment, k, cipher, off, len, flags);
    const uint64_t n = segment / 16;
    bool ok = p.seg0 == m.seg0 && p.ntouched == m.ntouched && p.need.size() == m.ntouched * (uint64_t)k;
    for (uint64_t t = 0; ok && t < p.ntouched; t++)
        for (int j = 0; j < k; j++) ok &= (p.need[t * k + j] != 0) == (m.need.at(p.seg0 + t).count((uint64_t)j) != 0);
    // the windows: per segment one range window over exactly the model's blocks, then at most one
    // window of the last two blocks; the padding is checked exactly on the model's segments
    std::map<uint64_t, std::set<uint64_t>> got;
    std::set<uint64_t> pad;
    uint64_t prev_seg = ~0ull;
    for (const Window& w : p.win) {
        ok &= w.seg >= p.seg0 && w.seg < p.seg0 + p.ntouched && w.bytes > 0 && w.first + w.bytes <= segment;
        if (!cipher) {
            ok &= w.flags == 0 && w.seg != prev_seg;
            for (uint64_t o = w.first; o < w.first + w.bytes; o++) got[w.seg].insert(o);
            prev_seg = w.seg;
            continue;
        }
        ok &= w.first % 16 == 0 && w.bytes % 16 == 0;
        const uint64_t b0 = w.first / 16, nb = w.bytes / 16;
        ok &= ((w.flags & kWinPrevIv) != 0) == (b0 == 0);
        if (w.flags & kWinPadOnly) {
            ok &= w.seg == prev_seg && (w.flags & kWinCheckPad) && b0 == n - 2 && nb == 2 && !pad.count(w.seg);
            pad.insert(w.seg);
            continue;
        }
        ok &= w.seg != prev_seg;
        prev_seg = w.seg;
        uint64_t plain = nb;
        if (w.flags & kWinCheckPad) {
            ok &= b0 + nb == n && nb >= 2;
            pad.insert(w.seg);
            plain--;
        }
        for (uint64_t b = b0; b < b0 + plain; b++) got[w.seg].insert(b);
    }
    ok &= got == m.blocks && pad == m.pad;
    CHECK(ok, "size %llu segment %llu k %d cipher %d off %llu len %llu flags %d", (unsigned long long)size,
          (unsigned long long)segment, k, (int)cipher, (unsigned long long)off, (unsigned long long)len, flags);
    return 1;
}

static uint64_t exhaustive(uint64_t size, uint64_t segment, int k, bool cipher) {
    const uint64_t piece = cipher ? segment - 16 : segment, nseg = (size + piece - 1) / piece;
    uint64_t cases = 0;
    for (int flags : {0, (int)kNoPaddingCheck})
        for (uint64_t off = 0; off < size; off++)
            for (uint64_t len = 1; off + len <= size; len++) cases += compare(size, nseg, segment, k, cipher, off, len, flags);
    return cases;
}

static void expect_error(const char* what, uint64_t size, uint64_t nseg, uint64_t segment, int k, bool cipher, uint64_t off,
                         uint64_t len, const char* text) {
    Plan p;
    const std::string err = plan(size, nseg, segment, k, cipher, off, len, 0, p);
    CHECK(err.find(text) != std::string::npos, "%s: got \"%s\", want \"%s\"", what, err.c_str(), text);
}

int main() {
    uint64_t cases = 0;
    for (uint64_t size : {1ull, 112ull, 113ull, 128ull, 129ull, 300ull, 384ull})
        for (bool cipher : {false, true}) cases += exhaustive(size, 128, 4, cipher);
    std::printf("cases 128 4 %llu\n", (unsigned long long)cases);
    uint64_t other = 0;
    for (bool cipher : {false, true}) {
        other += exhaustive(100, 64, 1, cipher);    // one data fragment
        other += exhaustive(200, 128, 8, cipher);   // a fragment of one block: a block's predecessor is always another fragment
        other += exhaustive(70, 32, 2, cipher);     // with a cipher: one plaintext block and its padding block
        other += exhaustive(260, 256, 2, cipher);
    }
    std::printf("cases other %llu\n", (unsigned long long)other);

    expect_error("len 0", 300, 3, 128, 4, false, 5, 0, "is empty or does not lie");
    expect_error("past the end", 300, 3, 128, 4, false, 299, 2, "is empty or does not lie");
    expect_error("off past the end", 300, 3, 128, 4, false, 300, 1, "is empty or does not lie");
    expect_error("overflow", 300, 3, 128, 4, false, ~0ull - 1, 5, "is empty or does not lie");
    expect_error("size / nseg", 300, 2, 128, 4, false, 0, 1, "size 300 does not end in the last of 2 segments of 128 bytes");
    expect_error("size / nseg", 256, 3, 128, 4, false, 0, 1, "does not end in the last of 3 segments");
    expect_error("size / pieces", 300, 2, 128, 4, true, 0, 1, "size 300 does not end in the last of 2 pieces of 112 bytes");
    expect_error("size 0", 0, 1, 128, 4, false, 0, 1, "does not end in the last of");
    expect_error("nseg 0", 1, 0, 128, 4, false, 0, 1, "does not end in the last of");
    expect_error("cipher segment", 1, 1, 16, 1, true, 0, 1, "has no room for a block and its padding block");
    expect_error("segment shape", 1, 1, 100, 4, false, 0, 1, "must be a non-zero multiple of 16 x 4 data shards");
    expect_error("segment 0", 1, 1, 0, 4, false, 0, 1, "must be a non-zero multiple");
    expect_error("k", 1, 1, 128, 0, false, 0, 1, "must be a non-zero multiple");
    expect_error("k", 1, 1, 16 * 9, 9, false, 0, 1, "must be a non-zero multiple");
    // the largest object: nothing overflows on the way
    {
        Plan p;
        const uint64_t seg = 32ull << 20, nseg = (~0ull) / seg;
        const std::string err = plan(nseg * seg, nseg, seg, 4, false, nseg * seg - 2, 2, 0, p);
        CHECK(err.empty() && p.seg0 == nseg - 1 && p.ntouched == 1 && p.need[3] == 1 && p.need[0] == 0, "largest object: %s",
              err.c_str());
    }
    if (failures) {
        std::fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    std::printf("range plan OK\n");
    return 0;
}
