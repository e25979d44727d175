// GPU test of the C++ Reed-Solomon mirror (include/deoss_reedsolomon.hpp), built and run by
// tests/test_rs_wide_gpu.py.  The reference is oracle/rs_oracle.c (or_rs_encode), never the library.
//
//  New: klauspost's errors for (0, 4), (4, -1), (255, 2), ErrNotSupported for (4, 0);
//  for (4, 8), (10, 4), (16, 4) and (12, 12): Split of a ragged buffer, Encode == the oracle's
//  parity, Verify true / false after a flipped byte, Reconstruct after losing `parity` shards
//  (data first) gives the originals, one more lost is ErrTooFewShards and changes nothing.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "deoss_reedsolomon.hpp"

extern "C" int or_rs_encode(int data, int parity, const uint8_t* const* dshards, uint8_t* const* pshards, size_t shard,
                            int nthreads);

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

using reedsolomon::Encoder;
using reedsolomon::Shards;

static void check_geometry(dm_ctx* ctx, int k, int m, size_t len, unsigned seed) {
    auto made = Encoder::New(ctx, k, m);
    CHECK(made.first && !made.second, "New(%d, %d): %s", k, m, made.second ? made.second->message.c_str() : "no encoder");
    if (!made.first) return;
    Encoder& enc = *made.first;
    std::mt19937 rng(seed);
    std::vector<uint8_t> buf(len);
    for (auto& b : buf) b = (uint8_t)rng();
    auto split = enc.Split(buf);
    CHECK(!split.second && split.first.size() == (size_t)(k + m), "(%d, %d) Split", k, m);
    Shards shards = split.first;
    const size_t per = (len + k - 1) / k;
    std::vector<uint8_t> joined;
    for (int j = 0; j < k; j++) {
        CHECK(shards[j].size() == per, "(%d, %d) shard %d has %zu bytes", k, m, j, shards[j].size());
        joined.insert(joined.end(), shards[j].begin(), shards[j].end());
    }
    CHECK(std::memcmp(joined.data(), buf.data(), len) == 0, "(%d, %d) Split changed the data", k, m);
    for (size_t i = len; i < joined.size(); i++) CHECK(joined[i] == 0, "(%d, %d) padding byte %zu", k, m, i);
    auto e = enc.Encode(shards);
    CHECK(!e, "(%d, %d) Encode: %s", k, m, e ? e->message.c_str() : "");
    // the oracle's parity
    Shards want((size_t)m, std::vector<uint8_t>(per));
    std::vector<const uint8_t*> dp;
    std::vector<uint8_t*> pp;
    for (int j = 0; j < k; j++) dp.push_back(shards[j].data());
    for (int i = 0; i < m; i++) pp.push_back(want[i].data());
    CHECK(or_rs_encode(k, m, dp.data(), pp.data(), per, 1) == 0, "(%d, %d) oracle", k, m);
    for (int i = 0; i < m; i++) CHECK(shards[k + i] == want[i], "(%d, %d) parity shard %d differs from the oracle's", k, m, i);
    const Shards full = shards;
    auto v = enc.Verify(shards);
    CHECK(!v.second && v.first, "(%d, %d) Verify of a coded set", k, m);
    shards[k + m - 1][per - 1] ^= 1;
    v = enc.Verify(shards);
    CHECK(!v.second && !v.first, "(%d, %d) Verify after a flipped parity byte", k, m);
    shards = full;
    // lose `m` shards, data first
    for (int i = 0; i < m; i++) shards[i].clear();
    e = enc.Reconstruct(shards);
    CHECK(!e && shards == full, "(%d, %d) Reconstruct: %s", k, m, e ? e->message.c_str() : "shards differ");
    shards = full;
    for (int i = 0; i <= m; i++) shards[i].clear();
    const Shards before = shards;
    e = enc.Reconstruct(shards);
    CHECK(e && e->message == "too few shards given" && shards == before, "(%d, %d) m + 1 lost", k, m);
}

int main() {
    dm_ctx* ctx = nullptr;
    if (dm_create(&ctx, nullptr, 0) != DM_OK) {
        std::fprintf(stderr, "dm_create: %s\n", dm_last_error(nullptr));
        return 2;
    }
    auto bad = Encoder::New(ctx, 0, 4);
    CHECK(!bad.first && bad.second && bad.second->message == reedsolomon::ErrInvShardNum().message, "New(0, 4)");
    bad = Encoder::New(ctx, 4, -1);
    CHECK(!bad.first && bad.second && bad.second->message == reedsolomon::ErrInvShardNum().message, "New(4, -1)");
    bad = Encoder::New(ctx, 255, 2);
    CHECK(!bad.first && bad.second && bad.second->message == reedsolomon::ErrMaxShardNum().message, "New(255, 2)");
    bad = Encoder::New(ctx, 4, 0);
    CHECK(!bad.first && bad.second && bad.second->message == reedsolomon::ErrNotSupported().message, "New(4, 0)");
    check_geometry(ctx, 4, 8, 1000, 1);
    check_geometry(ctx, 10, 4, 4099, 2);
    check_geometry(ctx, 16, 4, 16 * 257 + 3, 3);
    check_geometry(ctx, 12, 12, 777, 4);
    dm_destroy(ctx);
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("PASS reedsolomon mirror\n");
    return 0;
}
