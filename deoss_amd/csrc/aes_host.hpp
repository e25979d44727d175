// aes_host.hpp -- AES (FIPS-197) tables and key schedule, host side; plain C++17, no HIP.
//
// The S-boxes and the T-tables are generated at compile time from the field arithmetic of
// FIPS-197 §4 (no literal tables).  aes_kernels.hpp copies them into LDS; the key schedule runs
// here, on the host, once per call, and the round keys travel to the kernels as arguments.
//
// Word convention everywhere (host and kernels): a state column / round-key word is the
// little-endian load of its four bytes, so byte 0 (row 0) is the low byte.
// Tested without a GPU by tests/cpp/test_cipher_host.cpp (FIPS-197 Appendix A expansions).
#pragma once
#include <stdint.h>

namespace dm_aes {

constexpr int kMaxRounds = 14;
constexpr int kMaxKeyWords = 4 * (kMaxRounds + 1);   // 60 words = 240 bytes

constexpr uint8_t xtime(uint8_t x) { return (uint8_t)((x << 1) ^ ((x & 0x80) ? 0x1b : 0)); }

constexpr uint8_t gmul(uint8_t a, uint8_t b) {
    uint8_t p = 0;
    for (int i = 0; i < 8; i++) {
        if (b & 1) p ^= a;
        a = xtime(a);
        b >>= 1;
    }
    return p;
}

constexpr uint32_t rotl32(uint32_t x, int n) { return n ? (x << n) | (x >> (32 - n)) : x; }

struct Tables {
    uint8_t sbox[256] = {};
    uint8_t inv[256] = {};
    uint32_t te0[256] = {};   // row-0 byte a -> column (2S, S, S, 3S); row r uses rotl(te0, 8 r)
    uint32_t td0[256] = {};   // row-0 byte a -> column (14 Si, 9 Si, 13 Si, 11 Si)
    constexpr Tables() {
        // S-box (FIPS-197 §5.1.1): the affine map of the multiplicative inverse.  p walks the
        // powers of the generator 3 and q those of its inverse 0xf6, so q = p^-1 throughout.
        uint8_t p = 1, q = 1;
        for (int i = 0; i < 255; i++) {
            const uint8_t s = (uint8_t)(q ^ rotl8(q, 1) ^ rotl8(q, 2) ^ rotl8(q, 3) ^ rotl8(q, 4) ^ 0x63);
            sbox[p] = s;
            inv[s] = p;
            p = gmul(p, 3);
            q = gmul(q, 0xf6);
        }
        sbox[0] = 0x63;   // 0 has no inverse: the affine map of 0
        inv[0x63] = 0;
        for (int a = 0; a < 256; a++) {
            const uint8_t s = sbox[a], si = inv[a];
            te0[a] = (uint32_t)gmul(s, 2) | ((uint32_t)s << 8) | ((uint32_t)s << 16) | ((uint32_t)gmul(s, 3) << 24);
            td0[a] = (uint32_t)gmul(si, 14) | ((uint32_t)gmul(si, 9) << 8) | ((uint32_t)gmul(si, 13) << 16) |
                     ((uint32_t)gmul(si, 11) << 24);
        }
    }
    static constexpr uint8_t rotl8(uint8_t x, int n) { return (uint8_t)((x << n) | (x >> (8 - n))); }
};

constexpr Tables kTables{};
static_assert(kTables.sbox[0x00] == 0x63 && kTables.sbox[0x53] == 0xed && kTables.sbox[0xff] == 0x16, "FIPS-197 fig. 7");
static_assert(kTables.inv[0x63] == 0x00 && kTables.inv[0xed] == 0x53, "FIPS-197 fig. 14");

// Rounds for a key of key_len bytes (10 / 12 / 14), 0 for any other length.
constexpr int rounds_for(uint64_t key_len) { return key_len == 16 ? 10 : key_len == 24 ? 12 : key_len == 32 ? 14 : 0; }

struct KeySchedule {
    int rounds = 0;
    uint32_t enc[kMaxKeyWords] = {};   // FIPS-197 §5.2, 4 (rounds + 1) words
    uint32_t dec[kMaxKeyWords] = {};   // equivalent inverse cipher (§5.3.5): dec round r = InvMixColumns(enc round Nr - r)
};

inline uint32_t sub_word(uint32_t w) {
    return (uint32_t)kTables.sbox[w & 0xff] | ((uint32_t)kTables.sbox[(w >> 8) & 0xff] << 8) |
           ((uint32_t)kTables.sbox[(w >> 16) & 0xff] << 16) | ((uint32_t)kTables.sbox[w >> 24] << 24);
}

inline uint32_t inv_mix_column(uint32_t w) {
    uint32_t r = 0;
    for (int row = 0; row < 4; row++) {
        // td0 of the S-box of a byte is the InvMixColumns contribution of that byte in row 0
        r ^= rotl32(kTables.td0[kTables.sbox[(w >> (8 * row)) & 0xff]], 8 * row);
    }
    return r;
}

// False (ks untouched) unless key_len is 16, 24 or 32.
inline bool expand_key(const uint8_t* key, uint64_t key_len, KeySchedule& ks) {
    const int nr = rounds_for(key_len);
    if (!nr) return false;
    const int nk = (int)key_len / 4, nw = 4 * (nr + 1);
    ks.rounds = nr;
    for (int i = 0; i < nk; i++)
        ks.enc[i] = (uint32_t)key[4 * i] | ((uint32_t)key[4 * i + 1] << 8) | ((uint32_t)key[4 * i + 2] << 16) |
                    ((uint32_t)key[4 * i + 3] << 24);
    uint8_t rcon = 1;
    for (int i = nk; i < nw; i++) {
        uint32_t t = ks.enc[i - 1];
        if (i % nk == 0) {
            t = sub_word((t >> 8) | (t << 24)) ^ rcon;   // RotWord on little-endian words, Rcon in byte 0
            rcon = xtime(rcon);
        } else if (nk > 6 && i % nk == 4) {
            t = sub_word(t);
        }
        ks.enc[i] = ks.enc[i - nk] ^ t;
    }
    for (int j = 0; j < 4; j++) {
        ks.dec[j] = ks.enc[4 * nr + j];
        ks.dec[4 * nr + j] = ks.enc[j];
    }
    for (int r = 1; r < nr; r++)
        for (int j = 0; j < 4; j++) ks.dec[4 * r + j] = inv_mix_column(ks.enc[4 * (nr - r) + j]);
    return true;
}

}  // namespace dm_aes
