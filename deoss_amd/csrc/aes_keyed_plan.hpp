// aes_keyed_plan.hpp -- slot order of a keyed AES-CBC launch; plain C++17, no HIP.
//
// aes_cbc_encrypt_keyed_kernel (aes_kernels.hpp) runs 16 chains per wave and takes ONE round count
// per wave: its round loop is unrolled over a compile-time count, so a wave may not mix key
// lengths.  Given the round count of each chain of a call this orders the chains into slots so that
// the 16 slots of every wave share one count:
//   groups come in the order 10, 12, 14 rounds; the caller's chain order is kept inside a group;
//   every group is padded with empty slots (-1) to a multiple of 16;
//   slots = 16 * sum over groups of ceil(n_g / 16); no chains, no slots.
// Tested without a GPU by tests/cpp/test_aes_keyed_plan.cpp.
#pragma once
#include <stdint.h>

#include <vector>

namespace dm_aes_plan {

constexpr uint64_t kChainsPerWave = 16;
constexpr int kRoundCounts[3] = {10, 12, 14};

struct KeyedPlan {
    std::vector<int64_t> slot;      // chain index, or -1 for an empty slot; size = 16 * wave_rounds.size()
    std::vector<int> wave_rounds;   // round count of wave w = slots [16 w, 16 w + 16)
};

inline uint64_t keyed_slot_count(uint64_t n10, uint64_t n12, uint64_t n14) {
    const uint64_t w = kChainsPerWave;
    return w * ((n10 + w - 1) / w + (n12 + w - 1) / w + (n14 + w - 1) / w);
}

// rounds[c] = 10, 12 or 14 for each of n chains.  False (plan empty) when a chain has another count.
inline bool keyed_plan(const int* rounds, uint64_t n, KeyedPlan& plan) {
    plan.slot.clear();
    plan.wave_rounds.clear();
    for (uint64_t c = 0; c < n; c++)
        if (rounds[c] != 10 && rounds[c] != 12 && rounds[c] != 14) return false;
    for (const int nr : kRoundCounts) {
        for (uint64_t c = 0; c < n; c++) {
            if (rounds[c] != nr) continue;
            if (plan.slot.size() % kChainsPerWave == 0) plan.wave_rounds.push_back(nr);
            plan.slot.push_back((int64_t)c);
        }
        while (plan.slot.size() % kChainsPerWave) plan.slot.push_back(-1);
    }
    return true;
}

}  // namespace dm_aes_plan
