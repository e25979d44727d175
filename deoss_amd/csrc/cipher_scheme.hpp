// cipher_scheme.hpp -- how FullProcessing / Retrievefile use a cipher; host only, nothing else here.
//
// RECALLED, NOT PINNED: restated from memory of cess-go-sdk core/process and utils.AesCbcEncrypt /
// AesCbcDecrypt; the SDK's source is not at hand, so parity with it is unconfirmed (DESIGN.md
// §6.14).  The AES-CBC core is pinned by FIPS-197 / SP 800-38A vectors; everything SDK-specific is
// in this file, so a correction costs a few lines here:
//   key    the bytes of the cipher string; 16, 24 or 32 of them (AES-128 / -192 / -256);
//   IV     the first 16 key bytes, the same for every segment (each segment its own CBC chain);
//   upload the object is cut into pieces of P = segment - 16 plaintext bytes, the last one
//          zero-padded to P; each piece is CBC-encrypted with PKCS#7 padding, which for a P that is
//          a multiple of 16 is always one block of sixteen 0x10 bytes: the ciphertext is exactly
//          one segment.  Coding, names and the fid are of the ciphertext.
//   download  restore and verify the ciphertext, CBC-decrypt each segment, check and strip its
//          padding block, join the P-byte pieces, cut at the plaintext size.
#pragma once
#include <stdint.h>

#include "aes_host.hpp"

namespace dm_cipher {

constexpr uint64_t kBlock = 16;
constexpr uint8_t kPadByte = 0x10;                  // PKCS#7 padding of a whole block
constexpr uint32_t kPadWord = 0x10101010u;
constexpr const char* kKeyLenError = "cipher must be 16, 24 or 32 bytes";

inline bool key_len_ok(uint64_t n) { return dm_aes::rounds_for(n) != 0; }

// The IV of every segment: the first 16 bytes of the key.
inline void iv_of(const uint8_t* key, uint8_t iv[16]) {
    for (int i = 0; i < 16; i++) iv[i] = key[i];
}

struct Geometry {
    uint64_t segment = 0;   // ciphertext bytes per segment
    uint64_t piece = 0;     // P: plaintext bytes per segment
    uint64_t nseg = 0;
    uint64_t tail = 0;      // plaintext bytes of the last piece that come from the object (1 .. P)
    uint64_t piece_off(uint64_t s) const { return s * piece; }                 // in the object
    uint64_t piece_len(uint64_t s) const { return s + 1 < nseg ? piece : tail; }
};

// Segment sizes a cipher can be used with: room for a padding block and at least one block of data.
inline bool segment_ok(uint64_t segment) { return segment >= 2 * kBlock && segment % kBlock == 0; }

// Geometry of an object of len > 0 plaintext bytes.
inline Geometry geometry(uint64_t len, uint64_t segment) {
    Geometry g;
    g.segment = segment;
    g.piece = segment - kBlock;
    g.nseg = (len + g.piece - 1) / g.piece;
    g.tail = len - (g.nseg - 1) * g.piece;
    return g;
}

// A plaintext size that ends in the last of nseg segments: (nseg - 1) P < size <= nseg P.
inline bool size_ok(uint64_t size, uint64_t nseg, uint64_t segment) {
    const uint64_t p = segment - kBlock;
    return nseg > 0 && size > (nseg - 1) * p && size <= nseg * p;
}

// The file path moves a window in stripes [o, o + w) of the ciphertext segment (o, w multiples of
// 64, o + w <= segment).  On the way in a stripe is plaintext [off, off + len) of each piece, at the
// same offset; the stripe that ends the segment carries 16 bytes less and the padding block, which
// the encrypt kernel writes, is its last one.  w >= 64: never the padding block alone.
struct StripeSpan {
    uint64_t off = 0, len = 0;   // of the piece; both multiples of 16, len > 0
    bool pad = false;            // the stripe ends in the padding block
    uint64_t blk_lo() const { return off / kBlock; }
    uint64_t blk_hi() const { return (off + len) / kBlock; }
};
inline StripeSpan stripe_span(uint64_t o, uint64_t w, uint64_t segment) {
    const uint64_t piece = segment - kBlock, end = o + w < piece ? o + w : piece;
    StripeSpan s;
    s.off = o;
    s.len = end - o;
    s.pad = o + w == segment;
    return s;
}

}  // namespace dm_cipher
