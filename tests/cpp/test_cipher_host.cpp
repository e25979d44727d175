// CPU test of the cipher host code (no GPU): the AES key schedule of deoss_amd/csrc/aes_host.hpp --
// encrypt keys and the equivalent-inverse-cipher keys -- against the FIPS-197 Appendix A.1 - A.3
// expansions, and the scheme geometry of deoss_amd/csrc/cipher_scheme.hpp around every piece
// boundary.  Built plain (-Wall -Werror) and with ASan/UBSan by tests/test_cipher_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../deoss_amd/csrc/cipher_scheme.hpp"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static std::vector<uint8_t> unhex(const std::string& h) {
    std::vector<uint8_t> v(h.size() / 2);
    for (size_t i = 0; i < v.size(); i++) v[i] = (uint8_t)std::strtoul(h.substr(2 * i, 2).c_str(), nullptr, 16);
    return v;
}

// words (little-endian column words) -> the bytes in order
static std::vector<uint8_t> bytes_of(const uint32_t* w, int n) {
    std::vector<uint8_t> v((size_t)n * 4);
    for (int i = 0; i < n; i++)
        for (int b = 0; b < 4; b++) v[(size_t)4 * i + b] = (uint8_t)(w[i] >> (8 * b));
    return v;
}

struct Expansion {
    const char* key;
    const char* enc;   // w[0 .. 4 (Nr + 1)) as bytes, FIPS-197 Appendix A
    const char* dec;   // dw of §5.3.5: round Nr, InvMixColumns of rounds Nr - 1 .. 1, round 0
};

static const Expansion kExpansions[] = {
    {"2b7e151628aed2a6abf7158809cf4f3c",   // A.1
     "2b7e151628aed2a6abf7158809cf4f3ca0fafe1788542cb123a339392a6c7605"
     "f2c295f27a96b9435935807a7359f67f3d80477d4716fe3e1e237e446d7a883b"
     "ef44a541a8525b7fb671253bdb0bad00d4d1c6f87c839d87caf2b8bc11f915bc"
     "6d88a37a110b3efddbf98641ca0093fd4e54f70e5f5fc9f384a64fb24ea6dc4f"
     "ead27321b58dbad2312bf5607f8d292fac7766f319fadc2128d12941575c006e"
     "d014f9a8c9ee2589e13f0cc8b6630ca6",
     "d014f9a8c9ee2589e13f0cc8b6630ca60c7b5a631319eafeb0398890664cfbb4"
     "df7d925a1f62b09da320626ed675732412c07647c01f22c7bc42d2f37555114a"
     "6efcd876d2df54807c5df034c917c3b96ea30afcbc238cf6ae82a4b4b54a338d"
     "90884413d280860a12a128421bc897397c1f13f74208c219c021ae480969bf7b"
     "cc7505eb3e17d1ee82296c51c94811332b3708a7f262d405bc3ebdbf4b617d62"
     "2b7e151628aed2a6abf7158809cf4f3c"},
    {"8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7b",   // A.2
     "8e73b0f7da0e6452c810f32b809079e562f8ead2522c6b7bfe0c91f72402f5a5"
     "ec12068e6c827f6b0e7a95b95c56fec24db7b4bd69b5411885a74796e92538fd"
     "e75fad44bb095386485af05721efb14fa448f6d94d6dce24aa326360113b30e6"
     "a25e7ed583b1cf9a27f939436a94f767c0a69407d19da4e1ec1786eb6fa64971"
     "485f703222cb8755e26d135233f0b7b340beeb282f18a2596747d26b458c553e"
     "a7e1466c9411f1df821f750aad07d753ca4005388fcc5006282d166abc3ce7b5"
     "e98ba06f448c773c8ecc720401002202",
     "e98ba06f448c773c8ecc720401002202ac491644e55710b746c08a75c89b2cad"
     "a3979ac28e5ba6d8e12cc9e654b272baf3b42258b59ebb5cf8fb64fe491e06f3"
     "4d65dfa2b1e5620dea899c312dcc3c1a5b6cfe3cc745a02bf8b9a572462a9904"
     "c5ddb7f8be933c760b4f46a6fc80bdafb5dc7ad0f7cffb09a7ec43939c295e17"
     "5023b89a3bc51d84d04b19377b4e8b8e41b34544ab0592b9ce92f15e421381d9"
     "659763e78c817087123039436be6a51e9eb149c479d69c5dfeb4a27ceab6d7fd"
     "8e73b0f7da0e6452c810f32b809079e5"},
    {"603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4",   // A.3
     "603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4"
     "9ba354118e6925afa51a8b5f2067fcdea8b09c1a93d194cdbe49846eb75d5b9a"
     "d59aecb85bf3c917fee94248de8ebe96b5a9328a2678a647983122292f6c79b3"
     "812c81addadf48ba24360af2fab8b46498c5bfc9bebd198e268c3ba709e04214"
     "68007bacb2df331696e939e46c518d80c814e20476a9fb8a5025c02d59c58239"
     "de1369676ccc5a71fa2563959674ee155886ca5d2e2f31d77e0af1fa27cf73c3"
     "749c47ab18501ddae2757e4f7401905acafaaae3e4d59b349adf6acebd10190d"
     "fe4890d1e6188d0b046df344706c631e",
     "fe4890d1e6188d0b046df344706c631eada23f4963e23b2455427c8a5c709104"
     "57c96cf6074f07c0706abb07137f9241b668b621ce40046d36a047ae0932ed8e"
     "34ad1e4450866b367725bcc76315294632526c367828b24cf8e043c33f92aa20"
     "c440b289642b757227a3d7f114309581d669a7334a7ade7a80c8f18fc772e9e3"
     "25ba3c22a06bc7fb4388a2833393427054fb808b9c137949cab22ff547ba186c"
     "6c3d632985d1fbd9e3e36578701be0f34a7459f9c8e8f9c256a156bc8d083799"
     "42107758e9ec98f066329ea193f8858b8ec6bff6829ca03b9e49af7edba96125"
     "603deb1015ca71be2b73aef0857d7781"},
};

static void test_tables() {
    const dm_aes::Tables& t = dm_aes::kTables;
    bool seen[256] = {};
    for (int a = 0; a < 256; a++) {
        CHECK(!seen[t.sbox[a]]);
        seen[t.sbox[a]] = true;
        CHECK(t.inv[t.sbox[a]] == a);
        const uint8_t s = t.sbox[a];
        CHECK(t.te0[a] == ((uint32_t)dm_aes::gmul(s, 2) | (uint32_t)s << 8 | (uint32_t)s << 16 |
                           (uint32_t)dm_aes::gmul(s, 3) << 24));
    }
    // FIPS-197 §5.1.1's example {53} -> {ed}, figure 7's corners
    CHECK(t.sbox[0x53] == 0xed && t.sbox[0x00] == 0x63 && t.sbox[0xff] == 0x16 && t.sbox[0x10] == 0xca);
    // §4.2's example {57} x {83} = {c1}
    CHECK(dm_aes::gmul(0x57, 0x83) == 0xc1);
}

static void test_key_schedule() {
    for (const Expansion& e : kExpansions) {
        const std::vector<uint8_t> key = unhex(e.key), enc = unhex(e.enc), dec = unhex(e.dec);
        dm_aes::KeySchedule ks;
        CHECK(dm_aes::expand_key(key.data(), key.size(), ks));
        CHECK(ks.rounds == (int)key.size() / 4 + 6);
        const int nw = 4 * (ks.rounds + 1);
        CHECK(enc.size() == (size_t)4 * nw && dec.size() == (size_t)4 * nw);
        CHECK(bytes_of(ks.enc, nw) == enc);
        CHECK(bytes_of(ks.dec, nw) == dec);
    }
    // FIPS-197 Appendix C.1, equivalent inverse cipher: round[1].ik_sch of key 00 01 .. 0f
    uint8_t k[16];
    for (int i = 0; i < 16; i++) k[i] = (uint8_t)i;
    dm_aes::KeySchedule ks;
    CHECK(dm_aes::expand_key(k, 16, ks));
    CHECK(bytes_of(ks.dec + 4, 4) == unhex("13aa29be9c8faff6f770f58000f7bf03"));
    // any other key length is rejected, and leaves the schedule alone
    uint8_t big[64] = {};
    for (uint64_t n = 0; n <= 64; n++) {
        dm_aes::KeySchedule z;
        const bool ok = dm_aes::expand_key(big, n, z);
        CHECK(ok == (n == 16 || n == 24 || n == 32));
        CHECK(dm_cipher::key_len_ok(n) == ok);
        if (!ok) CHECK(z.rounds == 0);
    }
    CHECK(std::string(dm_cipher::kKeyLenError) == "cipher must be 16, 24 or 32 bytes");
}

static void test_geometry() {
    uint8_t key[32], iv[16];
    for (int i = 0; i < 32; i++) key[i] = (uint8_t)(0xa0 + i);
    dm_cipher::iv_of(key, iv);
    CHECK(std::memcmp(iv, key, 16) == 0);
    CHECK(!dm_cipher::segment_ok(0) && !dm_cipher::segment_ok(16) && dm_cipher::segment_ok(32) &&
          !dm_cipher::segment_ok(40) && dm_cipher::segment_ok(32u << 20));
    for (uint64_t segment : {32ull, 64ull, 256ull, 4096ull, 32ull << 20}) {
        const uint64_t P = segment - 16;
        std::vector<uint64_t> lens = {1, 2, 15, 16, 17};
        for (uint64_t n = 1; n <= 9; n++)
            for (int64_t d = -2; d <= 2; d++)
                if ((int64_t)(n * P) + d > 0) lens.push_back(n * P + d);
        for (uint64_t len : lens) {
            const dm_cipher::Geometry g = dm_cipher::geometry(len, segment);
            CHECK(g.segment == segment && g.piece == P);
            CHECK(g.nseg == (len + P - 1) / P && g.nseg >= 1);
            CHECK((g.nseg - 1) * P < len && len <= g.nseg * P);
            CHECK(g.tail >= 1 && g.tail <= P);
            // the pieces tile the object exactly, in order
            uint64_t at = 0;
            for (uint64_t s = 0; s < g.nseg; s++) {
                CHECK(g.piece_off(s) == at);
                CHECK(g.piece_len(s) == (s + 1 < g.nseg ? P : len - s * P));
                at += g.piece_len(s);
            }
            CHECK(at == len);
            // the size bounds of the download side: exactly the lengths with this segment count
            CHECK(dm_cipher::size_ok(len, g.nseg, segment));
            CHECK(!dm_cipher::size_ok(len, g.nseg + 1, segment));
            if (g.nseg > 1) CHECK(!dm_cipher::size_ok(len, g.nseg - 1, segment));
            CHECK(!dm_cipher::size_ok((g.nseg - 1) * P, g.nseg, segment));
            CHECK(dm_cipher::size_ok((g.nseg - 1) * P + 1, g.nseg, segment));
            CHECK(dm_cipher::size_ok(g.nseg * P, g.nseg, segment));
            CHECK(!dm_cipher::size_ok(g.nseg * P + 1, g.nseg, segment));
            CHECK(!dm_cipher::size_ok(len, 0, segment));
        }
    }
}

int main(int, char**) {
    test_tables();
    test_key_schedule();
    test_geometry();
    std::printf("cipher host OK\n");
    return 0;
}
