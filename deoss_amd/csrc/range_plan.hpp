// range_plan.hpp -- what a ranged restore decides before any GPU work (pure host code: no HIP, no
// context): which segments a byte range (off, len) of an object touches, which data fragments of
// each hold its bytes, and which window of every touched segment is read (and, with a cipher,
// decrypted) on the device.
//
// Shared by range_capi.inl (dm_range_plan, dm_restore_range_buffer, dm_retrieve_range) and the host
// tests (tests/cpp/test_range_plan.cpp, plain and ASan/UBSan; tests/test_range_plan.py through
// dm_range_plan against a brute-force model).  A gateway calls the plan first, to decide which
// fragments to fetch from miners.
//
// Without a cipher a piece is a segment: byte x of the object is byte x % segment of segment
// x / segment, in data fragment (x % segment) / (segment / k).
// With a cipher (cipher_scheme.hpp; RECALLED, NOT PINNED, as everything there) a piece is
// P = segment - 16 plaintext bytes and every segment its own CBC chain with a fixed IV: plaintext
// byte o of a piece lies in ciphertext block o / 16, and decrypting blocks b0 .. b1 needs ciphertext
// blocks max(b0 - 1, 0) .. b1 (the IV stands in for block -1).  A range that begins in the first
// block of data fragment j > 0 therefore needs fragment j - 1 as well.
// A wrong cipher shows in the padding block (the segment's last), as in the full restore.  It is
// checked on the first touched segment (unless kNoPaddingCheck) and on every segment whose range
// reaches fragment k - 1 anyway: a window that ends in the last plaintext block is extended by the
// padding block, any other segment gets one more window of the last two blocks, whose plaintext
// block is not part of the range (kWinPadOnly).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "cipher_scheme.hpp"

namespace dm_range {

constexpr int kNoPaddingCheck = 8;   // DM_RANGE_NO_PADDING_CHECK
constexpr int kMaxData = 8;          // dm::kRsMaxIn

enum : uint32_t {
    kWinPrevIv = 1,    // the window starts at block 0: the IV is its predecessor block
    kWinCheckPad = 2,  // the window's last block is the padding block: checked, not plaintext
    kWinPadOnly = 4,   // the extra window of blocks n - 2, n - 1: no block of it belongs to the range
};

struct Window {
    uint64_t seg;     // segment of the object
    uint64_t first;   // first byte read, within the segment (with a cipher: of the first block decrypted)
    uint64_t bytes;   // byte count (with a cipher: a multiple of 16)
    uint32_t flags;   // kWin*; 0 without a cipher
    uint32_t pad_ = 0;
};

struct Plan {
    uint64_t seg0 = 0, ntouched = 0;
    std::vector<uint8_t> need;   // [ntouched][k]: 1 = the data fragment's bytes are needed
    std::vector<Window> win;     // by segment; a segment's kWinPadOnly window follows its range window
};

// The plan of bytes [off, off + len) of an object of `size` plaintext bytes in nseg segments.
// Returns "" or the error's text (DM_ERR_INVALID).
inline std::string plan(uint64_t size, uint64_t nseg, uint64_t segment, int k, bool cipher, uint64_t off, uint64_t len,
                        int flags, Plan& p) {
    auto u = [](uint64_t v) { return std::to_string((unsigned long long)v); };
    if (k < 1 || k > kMaxData || segment == 0 || segment % (16ull * (uint64_t)k))
        return "segment size " + u(segment) + " must be a non-zero multiple of 16 x " + std::to_string(k) + " data shards";
    if (cipher && !dm_cipher::segment_ok(segment))
        return "segment size " + u(segment) + " has no room for a block and its padding block";
    const uint64_t piece = cipher ? segment - dm_cipher::kBlock : segment;
    if (nseg == 0 || size == 0 || (size - 1) / piece != nseg - 1)
        return "size " + u(size) + " does not end in the last of " + u(nseg) + (cipher ? " pieces" : " segments") + " of " +
               u(piece) + " bytes";
    if (len == 0 || off + len < off || off + len > size)
        return "range of " + u(len) + " bytes at " + u(off) + " is empty or does not lie in the object's " + u(size) + " bytes";
    const uint64_t frag = segment / (uint64_t)k, last = (off + len - 1) / piece;
    p.seg0 = off / piece;
    p.ntouched = last - p.seg0 + 1;
    p.need.assign(p.ntouched * (uint64_t)k, 0);
    p.win.clear();
    p.win.reserve(p.ntouched + 1);
    const uint64_t n = segment / dm_cipher::kBlock;   // blocks of a segment, the padding block among them
    for (uint64_t t = 0; t < p.ntouched; t++) {
        const uint64_t s = p.seg0 + t;
        const uint64_t o0 = t == 0 ? off - s * piece : 0, o1 = s == last ? off + len - s * piece : piece;   // [o0, o1) of the piece
        uint8_t* need = p.need.data() + t * (uint64_t)k;
        auto mark = [&](uint64_t byte0, uint64_t byte1) {   // fragments of segment bytes [byte0, byte1]
            for (uint64_t j = byte0 / frag; j <= byte1 / frag; j++) need[j] = 1;
        };
        if (!cipher) {
            mark(o0, o1 - 1);
            p.win.push_back({s, o0, o1 - o0, 0});
            continue;
        }
        const uint64_t b0 = o0 / 16, b1 = (o1 - 1) / 16, c0 = b0 ? b0 - 1 : 0;
        mark(16 * c0, 16 * b1 + 15);
        const uint32_t iv = b0 == 0 ? kWinPrevIv : 0;
        const bool pad = (t == 0 && !(flags & kNoPaddingCheck)) || need[k - 1];
        if (!pad) {
            p.win.push_back({s, 16 * b0, 16 * (b1 - b0 + 1), iv});
        } else if (b1 == n - 2) {   // ends in the last plaintext block: the padding block follows it
            mark(16 * (n - 1), 16 * n - 1);
            p.win.push_back({s, 16 * b0, 16 * (b1 - b0 + 2), iv | kWinCheckPad});
        } else {
            mark(16 * (n - 2), 16 * n - 1);
            p.win.push_back({s, 16 * b0, 16 * (b1 - b0 + 1), iv});
            p.win.push_back({s, 16 * (n - 2), 32, kWinCheckPad | kWinPadOnly | (n == 2 ? kWinPrevIv : 0u)});
        }
    }
    return "";
}

}  // namespace dm_range
