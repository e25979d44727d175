// K1Q's ring and barrier schedule as plain constexpr arithmetic: included by both waves of
// leaf_kernel_quad (merkle_kernels.hpp) and by tests/cpp/test_quad_ring.cpp, which steps a
// producer and a consumer built from these functions on the host.  No HIP in here.
//
// The ring holds `depth` stages of 8 blocks per leaf.  The producer wave runs depth - 1 stages
// ahead of the consumer wave; both execute NI + 1 workgroup barriers for NI stages:
//   producer:  write stages 0 .. depth-2 | barrier 0 | write stage it+depth-1 | barrier it+1 | ...
//   consumer:                            | barrier 0 | read stage it          | barrier it+1 | ...
// After barrier b the stages below b + depth - 1 are complete, and the slot the producer writes in
// the interval after barrier `it` held stage it - 1, whose last read came before that barrier.
// At depth 2 (K1L, K1P, the compact K1Q) the consumer may read stage `it` only; at depth 3 (the
// wide K1Q) stage it + 1 is complete too, which is what lets the step stream and its K+W prefetch
// run across the stage boundary.
#pragma once
#include <cstdint>

namespace dm {
namespace quad_ring {

constexpr int kBlocks = 8;        // blocks per leaf per ring stage
constexpr int kWideDepth = 3;     // ring slots of the wide K1Q
constexpr int kAhead = 2;         // the consumer loads a block's words this many blocks ahead
constexpr int kSets = 4;          // register sets of 64 words; kBlocks % kSets == 0 keeps them static
static_assert(kBlocks % kSets == 0 && kSets > kAhead, "a block's register set must not depend on the stage");

// ---- both waves ----
constexpr uint64_t stages(uint64_t max_blocks) { return (max_blocks + kBlocks - 1) / kBlocks; }
constexpr uint64_t barriers(uint64_t ni) { return ni + 1; }
constexpr uint32_t slot_of(uint64_t stage, int depth) { return (uint32_t)(stage % (uint64_t)depth); }
constexpr uint32_t next_slot(uint32_t slot, int depth) { return slot + 1 == (uint32_t)depth ? 0 : slot + 1; }

// ---- producer ----
constexpr uint64_t stages_before_first_barrier(int depth) { return (uint64_t)depth - 1; }
// the stage written between barrier `it` and barrier it + 1 (nothing if it is >= NI)
constexpr uint64_t stage_written_after_barrier(uint64_t it, int depth) { return it + (uint64_t)depth - 1; }
// after barrier b, stages [0, complete_after_barrier) are complete
constexpr uint64_t complete_after_barrier(uint64_t b, int depth) { return b + (uint64_t)depth - 1; }

// ---- consumer: runs of whole stages ----
// A leaf is running at stage `it` while it has blocks at or beyond it; a run of whole stages ends
// where the first running leaf of the wave ends (min over the wave of leaf_run_end).
constexpr bool leaf_running(bool active, uint64_t nb, uint64_t it) { return active && nb > it * kBlocks; }
constexpr uint64_t leaf_run_end(bool running, uint64_t nb, uint64_t ns) { return running ? nb / kBlocks : ns; }
// the leaf ends strictly inside stage `it`: that stage takes the per-block path
constexpr bool leaf_ends_inside(bool active, uint64_t nb, uint64_t it) {
    return active && nb > it * kBlocks && nb < (it + 1) * kBlocks;
}

// ---- consumer: one stream per run (wide K1Q) ----
// Block k of a stage reads set_of(k), links into set_of(k + 1) and loads block k + kAhead.  For
// k >= kBlocks - kAhead that block is in the NEXT stage (complete since the barrier this stage
// started at, at depth 3), except in the last stage of a run, which loads nothing beyond itself
// and drains at its block 7.
struct BlockRef {
    uint32_t dstage;   // 0: this stage, 1: the next
    uint32_t block;
};
constexpr BlockRef prefetch_of(uint32_t k) { return BlockRef{(k + kAhead) / kBlocks, (k + kAhead) % kBlocks}; }
constexpr uint32_t set_of(uint32_t k) { return k % kSets; }
constexpr bool block_prefetches(uint32_t k, bool last_stage_of_run) {
    return !(last_stage_of_run && k + kAhead >= (uint32_t)kBlocks);
}
constexpr bool block_links(uint32_t k, bool last_stage_of_run) {
    return !(last_stage_of_run && k + 1 == (uint32_t)kBlocks);
}

}  // namespace quad_ring
}  // namespace dm
