"""CPU model of the control flow of the compact K1Q consumer (no GPU code, no digests).

It restates, for one wave of 8 leaves, the COMPACT branch of leaf_kernel_quad in
deoss_amd/csrc/merkle_kernels.hpp:

  leaf_view                 nb = have / 64: full 64-byte blocks (the padded tail goes through
                            leaf_epilogue); a leaf at or beyond nleaves is not active
  NB, NI, NS                NI = ceil(max nb / 8) ring stages, NS the same on the consumer
  for (it = 0; it < NS;)    the consumer's loop
    running                 vq.active && vq.nb > it * kQuadBlocks
    end                     wave_min(running ? vq.nb / kQuadBlocks : NS)
    for (; it < end; it++)  the register run: quad_stage_regs on ring slot it % kLatRing (a ring of
                            two), every lane of the wave, the leaves that ended earlier included;
                            if (running) xf = x after it
    if (it == NS) break
    __any(active && nb > it * 8 && nb < (it + 1) * 8)
                            some leaf ends strictly inside stage it: the per-block path
                            (quad_block_skewed) on slot it % kLatRing, block k only where
                            it * 8 + k < nb; if (nb > it * 8) xf = x; else the next run

walk() names the paths a wave takes through that loop, and with by_slot the ring slot each runs in.
tests/test_quad_compact_shape.py asserts, without a GPU, that the waves
tests/test_quad_compact_gpu.py launches take every one of them.
"""

BLOCKS = 8      # kQuadBlocks: blocks per leaf per ring stage
RING = 2        # kLatRing: stages in the compact ring
LEAVES = 8      # kQuadLeaves: leaves per workgroup, one consumer wave

CLASSES = frozenset(
    ["run1", "run2", "run3+",               # a register run of 1, 2 or >= 3 stages (>= 3 wraps the ring)
     "run_start_slot0", "run_start_slot1",  # ring slot of a run's first stage
     "run_ends_at_leaf_boundary",           # a running leaf's nb is 8 * end: it ends with the run
     "run_after_block",                     # a run after a per-block stage
     "stale_run",                           # a leaf that ended earlier sits through a later run
     "block_slot0", "block_slot1",          # a per-block stage in ring slot it % 2
     "two_ends_one_stage",                  # two leaves end inside one stage at different blocks
     "block_with_full_leaf",                # a per-block stage in which another leaf has all 8 blocks
     "stale_block",                         # a per-block stage with a leaf that ended before it
     "inactive",                            # the wave has a leaf beyond nleaves
     "nb0_beside_long"]                     # a leaf under 64 B beside multi-stage leaves
    + ["ends_k%d" % k for k in range(1, BLOCKS)])   # a leaf ends after k blocks of its per-block stage

# The same paths by ring slot (a wrong slot offset shows only where that path runs in slot 1, or in
# slot 0 again after the ring has wrapped): a run by its length and the slot it starts in, a leaf's
# end by its block and the stage's slot, the stale and full-leaf cases by slot.
SLOT_CLASSES = frozenset(
    ["%s@slot%d" % (c, s) for s in range(RING)
     for c in ["run1", "run2", "run3+", "stale_run", "stale_block", "block_with_full_leaf"]
     + ["ends_k%d" % k for k in range(1, BLOCKS)]])


def walk(lens, by_slot=False):
    """lens: the byte lengths of one wave's leaves, at most 8, None (or a missing entry) for a leaf
    beyond nleaves.  Returns the set of CLASSES the compact consumer takes for that wave; with
    by_slot, the set of SLOT_CLASSES instead."""
    lens = list(lens) + [None] * (LEAVES - len(lens))
    assert len(lens) == LEAVES
    active = [n is not None for n in lens]
    nb = [n // 64 if a else 0 for n, a in zip(lens, active)]
    NS = (max(nb) + BLOCKS - 1) // BLOCKS
    tags, slots = set(), set()
    if not all(active):
        tags.add("inactive")
    if NS > 1 and any(a and n == 0 for a, n in zip(active, nb)):
        tags.add("nb0_beside_long")
    it = 0
    seen_block = False
    while it < NS:
        running = [a and n > it * BLOCKS for a, n in zip(active, nb)]
        end = min(n // BLOCKS if r else NS for r, n in zip(running, nb))
        if end > it:
            tags.add("run%s" % (end - it if end - it < 3 else "3+"))
            tags.add("run_start_slot%d" % (it % RING))
            slots.add("run%s@slot%d" % (end - it if end - it < 3 else "3+", it % RING))
            if any(a and not r and n > 0 for a, r, n in zip(active, running, nb)):
                tags.add("stale_run")
                slots.add("stale_run@slot%d" % (it % RING))
            if seen_block:
                tags.add("run_after_block")
            if any(r and n == end * BLOCKS for r, n in zip(running, nb)):
                tags.add("run_ends_at_leaf_boundary")
            it = end
        if it == NS:
            break
        inside = [a and it * BLOCKS < n < (it + 1) * BLOCKS for a, n in zip(active, nb)]
        if not any(inside):
            continue
        tags.add("block_slot%d" % (it % RING))
        ends = {n - it * BLOCKS for f, n in zip(inside, nb) if f}
        tags.update("ends_k%d" % k for k in ends)
        slots.update("ends_k%d@slot%d" % (k, it % RING) for k in ends)
        if len(ends) > 1:
            tags.add("two_ends_one_stage")
        if any(a and n >= (it + 1) * BLOCKS for a, n in zip(active, nb)):
            tags.add("block_with_full_leaf")
            slots.add("block_with_full_leaf@slot%d" % (it % RING))
        if any(a and 0 < n <= it * BLOCKS for a, n in zip(active, nb)):
            tags.add("stale_block")
            slots.add("stale_block@slot%d" % (it % RING))
        seen_block = True
        it += 1
    assert tags <= CLASSES and slots <= SLOT_CLASSES
    return slots if by_slot else tags


def walk_all(lens, by_slot=False):
    """Union of walk() over consecutive waves of 8 of a leaf list (the last may be partial)."""
    tags = set()
    for i in range(0, len(lens), LEAVES):
        tags |= walk(lens[i:i + LEAVES], by_slot)
    return tags
