// Host test of the keyed AES-CBC launch's slot plan (deoss_amd/csrc/aes_keyed_plan.hpp): group
// sizes drawn from {0, 1, 15, 16, 17, 33} in every combination over the three round counts, the
// chains interleaved in the input.  Every chain appears exactly once, a wave's non-empty slots
// share the wave's round count, the caller's order is kept within a group, the slot count is
// 16 * sum ceil(n_g / 16), and no chains give no slots.  No GPU.
#include <cstdio>
#include <vector>

#include "../../deoss_amd/csrc/aes_keyed_plan.hpp"

static int failures = 0;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            failures++;                                    \
        }                                                  \
    } while (0)

// n10 / n12 / n14 chains interleaved round robin (10, 12, 14, 10, ...) until each group is used up.
static std::vector<int> interleaved(uint64_t n10, uint64_t n12, uint64_t n14) {
    std::vector<int> r;
    uint64_t left[3] = {n10, n12, n14};
    while (left[0] || left[1] || left[2])
        for (int g = 0; g < 3; g++)
            if (left[g]) {
                r.push_back(dm_aes_plan::kRoundCounts[g]);
                left[g]--;
            }
    return r;
}

static void check_case(uint64_t n10, uint64_t n12, uint64_t n14) {
    const std::vector<int> rounds = interleaved(n10, n12, n14);
    const uint64_t n = rounds.size();
    dm_aes_plan::KeyedPlan plan;
    plan.slot.assign(3, 99);   // stale contents must not survive
    plan.wave_rounds.assign(2, 99);
    const bool ok = dm_aes_plan::keyed_plan(rounds.data(), n, plan);
    CHECK(ok, "(%llu, %llu, %llu): refused", (unsigned long long)n10, (unsigned long long)n12, (unsigned long long)n14);
    const uint64_t want = 16 * ((n10 + 15) / 16 + (n12 + 15) / 16 + (n14 + 15) / 16);
    CHECK(plan.slot.size() == want, "slots %zu, want %llu", plan.slot.size(), (unsigned long long)want);
    CHECK(dm_aes_plan::keyed_slot_count(n10, n12, n14) == want, "keyed_slot_count");
    CHECK(plan.wave_rounds.size() * 16 == plan.slot.size(), "waves %zu for %zu slots", plan.wave_rounds.size(), plan.slot.size());
    if (plan.wave_rounds.size() * 16 != plan.slot.size()) return;
    std::vector<int> seen(n, 0);
    int64_t last[3] = {-1, -1, -1};
    int prev_rounds = 0;
    for (uint64_t w = 0; w < plan.wave_rounds.size(); w++) {
        const int nr = plan.wave_rounds[w];
        CHECK(nr == 10 || nr == 12 || nr == 14, "wave %llu has %d rounds", (unsigned long long)w, nr);
        CHECK(nr >= prev_rounds, "groups out of order at wave %llu", (unsigned long long)w);
        prev_rounds = nr;
        uint64_t filled = 0;
        for (uint64_t i = 0; i < 16; i++) {
            const int64_t c = plan.slot[16 * w + i];
            if (c < 0) {
                CHECK(c == -1, "empty slot holds %lld", (long long)c);
                continue;
            }
            filled++;
            CHECK((uint64_t)c < n, "slot names chain %lld of %llu", (long long)c, (unsigned long long)n);
            if ((uint64_t)c >= n) continue;
            seen[c]++;
            CHECK(rounds[c] == nr, "chain %lld (%d rounds) in a wave of %d", (long long)c, rounds[c], nr);
            const int g = (nr - 10) / 2;
            CHECK(c > last[g], "order within the %d-round group: %lld after %lld", nr, (long long)c, (long long)last[g]);
            last[g] = c;
        }
        CHECK(filled > 0, "wave %llu is empty", (unsigned long long)w);
    }
    for (uint64_t c = 0; c < n; c++) CHECK(seen[c] == 1, "chain %llu appears %d times", (unsigned long long)c, seen[c]);
}

int main() {
    const uint64_t sizes[] = {0, 1, 15, 16, 17, 33};
    int cases = 0;
    for (uint64_t a : sizes)
        for (uint64_t b : sizes)
            for (uint64_t c : sizes) {
                check_case(a, b, c);
                cases++;
            }
    // no chains: an empty plan, from a null pointer too
    dm_aes_plan::KeyedPlan plan;
    CHECK(dm_aes_plan::keyed_plan(nullptr, 0, plan) && plan.slot.empty() && plan.wave_rounds.empty(), "n = 0");
    // a round count AES does not have is refused and leaves no plan
    const int bad[3] = {10, 11, 14};
    CHECK(!dm_aes_plan::keyed_plan(bad, 3, plan) && plan.slot.empty() && plan.wave_rounds.empty(), "11 rounds accepted");
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("aes keyed plan OK (%d cases)\n", cases);
    return 0;
}
