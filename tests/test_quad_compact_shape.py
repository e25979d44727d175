"""The inputs of tests/test_quad_compact_gpu.py reach what they claim, checked on the CPU (no GPU,
no library): tests/quad_compact_model.py walks the compact K1Q consumer's loop for each wave."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from quad_compact_model import CLASSES, SLOT_CLASSES, walk, walk_all  # noqa: E402
from test_quad_compact_gpu import CATALOGUE, PARTIAL, UNIFORM, object_lengths, table_lengths  # noqa: E402

CUS = (256, 304, 64)     # MI355X, and two other counts: the layout must not depend on it


def test_model_on_known_waves():
    """The model on waves whose path is plain from the kernel's source."""
    assert walk([1015] * 8) == {"run1", "run_start_slot0", "block_slot1", "ends_k7"}
    assert walk([2039] * 8) == {"run3+", "run_start_slot0", "block_slot1", "ends_k7"}
    assert walk([2039] * 8, by_slot=True) == {"run3+@slot0", "ends_k7@slot1"}
    assert walk([1024] * 8) == {"run2", "run_start_slot0", "run_ends_at_leaf_boundary"}
    assert walk([63] * 8) == set() and walk([64]) == {"inactive", "block_slot0", "ends_k1"}
    # the x-stage test's "mixed lengths" wave: per-block stages only, no register run
    assert not {t for t in walk(CATALOGUE[0]) if t.startswith("run")}
    # a last leaf of 8 blocks beside seven of 31: the first run ends with it after stage 0, a second
    # run of stages 1 and 2 starts in slot 1 with that leaf stale, then stage 3 goes block by block
    assert walk([2039] * 7 + [520]) == {"run1", "run2", "run_start_slot0", "run_start_slot1",
                                         "run_ends_at_leaf_boundary", "stale_run", "stale_block", "block_slot1",
                                         "ends_k7"}
    assert walk([2039] * 7 + [520], by_slot=True) == {"run1@slot0", "run2@slot1", "stale_run@slot1",
                                                       "stale_block@slot1", "ends_k7@slot1"}


def test_catalogue_takes_every_path():
    """(a) the catalogue's waves and the partial last wave take every path class between them, and
    every path in both ring slots; so does the table test's layout, and no less as one-leaf
    objects."""
    assert all(len(w) == 8 for w in CATALOGUE) and 0 < len(PARTIAL) < 8
    union, slots = walk(PARTIAL), walk(PARTIAL, by_slot=True)
    for wave in CATALOGUE:
        union |= walk(wave)
        slots |= walk(wave, by_slot=True)
    assert union == CLASSES, sorted(CLASSES - union)
    assert slots == SLOT_CLASSES, sorted(SLOT_CLASSES - slots)
    for cus in CUS:
        lens, objs = table_lengths(16 * cus + 3), object_lengths(16 * cus + 3)
        assert len(lens) == 16 * cus + 3 and lens[-3:] == PARTIAL
        assert walk_all(lens) == CLASSES and walk_all(lens, by_slot=True) == SLOT_CLASSES
        assert walk_all(objs) == CLASSES and walk_all(objs, by_slot=True) == SLOT_CLASSES and min(objs) == 1
    # the classes do not depend on the lane a leaf sits on
    for wave in CATALOGUE:
        assert all(walk(wave[r:] + wave[:r]) == walk(wave) for r in range(8))


@pytest.mark.parametrize("cus", CUS)
def test_longest_leaf_on_every_lane(cus):
    """(b) over the rotated catalogue as the table test lays it out, the longest leaf of each
    catalogue wave occurs at every lane position 0..7, and so does its shortest."""
    lens = table_lengths(16 * cus + 3)
    nw = len(CATALOGUE)
    single = [i for i, wave in enumerate(CATALOGUE) if wave.count(max(wave)) == 1]
    assert len(single) == nw - 1     # one wave has seven equal leaves and a short one: its shortest moves
    longest, shortest = {}, {}       # catalogue wave -> lanes its longest / shortest leaf sat on
    for w in range(len(lens) // 8):
        wave = lens[8 * w:8 * w + 8]
        assert sorted(wave) == sorted(CATALOGUE[w % nw])
        longest.setdefault(w % nw, set()).add(wave.index(max(wave)))
        shortest.setdefault(w % nw, set()).add(wave.index(min(wave)))
    assert all(longest[i] == set(range(8)) for i in single)
    assert all(shortest[i] == set(range(8)) for i in range(nw))


def test_uniform_lengths():
    """(c) every uniform length has the full blocks and the tail its comment claims."""
    for n, (nb, tail) in UNIFORM.items():
        assert (n // 64, n % 64) == (nb, tail), n
    assert {nb for nb, _ in UNIFORM.values()} == {0, 1, 7, 8, 9, 15, 16, 17, 24, 25}
    assert {tail for _, tail in UNIFORM.values()} == {0, 55, 56, 63}
    aligned = {n for n in UNIFORM if n % 16 == 0}
    assert {UNIFORM[n][0] for n in aligned} >= {1, 8, 9, 16, 17, 24, 25}    # the ALIGNED instance's walk
