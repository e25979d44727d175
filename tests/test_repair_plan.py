"""CPU checks of the repair plan (dm_rs_repair_plan): which fragments a segment's missing ones are
rebuilt from, which are written -- data or parity -- and with which GF(2^8) coding rows.

The runtime builds every descriptor of a repair launch through this same function (repair_plan in
rs_plan.hpp), so what is checked here is what runs.  The reference is oracle/oracle.py's Python
restatement (py_rs_matrix, py_gf_inverse, py_gf_mul, py_rs_code), never the library: the row of a
missing data fragment j is row j of the inverse of the sub-matrix made of the inputs' rows, the row of
a missing parity fragment j is (coding matrix row j) x that inverse.  No GPU.
"""
from __future__ import annotations

import ctypes
import itertools
import random

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from deoss_amd import build as b
    b.build(verbose=False)
    from deoss_amd import load_library
    return load_library()


_MATS, _INVS = {}, {}


def _expected(k, m, present, want):
    """(inputs, outputs, rows) from the oracle's matrix, inverse and product alone."""
    from oracle import py_gf_inverse, py_gf_mul, py_rs_matrix
    if (k, m) not in _MATS:
        _MATS[(k, m)] = py_rs_matrix(k, k + m)
    mat = _MATS[(k, m)]
    inputs = [i for i in range(k + m) if present[i]][:k]
    key = (k, m, tuple(inputs))
    if key not in _INVS:
        _INVS[key] = py_gf_inverse([mat[i] for i in inputs])
    inv = _INVS[key]
    outputs = [j for j in range(k + m) if not present[j] and (want is None or want[j])]
    rows = []
    for j in outputs:
        row = []
        for c in range(k):
            acc = 0
            for q in range(k):
                acc ^= py_gf_mul(mat[j][q], inv[q][c])
            row.append(acc)
        if j < k:
            assert row == inv[j]            # the top of the matrix is the identity
        rows.append(row)
    return inputs, outputs, rows


def _check(lib, k, m, present, want=None):
    from deoss_amd.reedsolomon import repair_plan
    got = repair_plan(present, want, k, m)
    assert got == _expected(k, m, present, want), (k, m, present, want)
    ins, outs, rows = got
    assert ins == [i for i in range(k + m) if present[i]][:k]            # first k present, index order
    assert not any(present[j] for j in outs)                             # a present fragment is never an output
    assert outs == sorted(outs) and len(rows) == len(outs) <= m
    return got


def _frags(k, m, n, seed):
    """k + m random-data fragments of n bytes, coded by the oracle's restatement."""
    from oracle import py_rs_code, py_rs_matrix
    rng = np.random.default_rng(seed)
    data = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for _ in range(k)]
    return data + py_rs_code(py_rs_matrix(k, k + m)[k:], data)


def test_all_495_four_of_twelve_patterns_rebuild_the_other_eight(lib):
    from oracle import py_rs_code
    frags = _frags(4, 8, 48, 495)
    n = 0
    for keep in itertools.combinations(range(12), 4):
        present = [i in keep for i in range(12)]
        ins, outs, rows = _check(lib, 4, 8, present)
        assert ins == list(keep) and outs == [j for j in range(12) if j not in keep] and len(rows) == 8
        # the rows applied to the kept fragments give the original fragments back
        assert py_rs_code(rows, [frags[i] for i in ins]) == [frags[j] for j in outs]
        n += 1
    assert n == 495


def test_4_8_more_present_and_want_subsets(lib):
    from oracle import py_rs_code
    rng = random.Random(0x4e9a)
    frags = _frags(4, 8, 48, 2)
    for _ in range(600):
        keep = set(rng.sample(range(12), rng.randint(5, 12)))
        present = [i in keep for i in range(12)]
        _check(lib, 4, 8, present)
        want = [rng.random() < 0.5 for _ in range(12)]     # present-and-wanted entries among them
        ins, outs, rows = _check(lib, 4, 8, present, want)
        assert set(outs) == {j for j in range(12) if want[j] and not present[j]}
        if outs:
            assert py_rs_code(rows, [frags[i] for i in ins]) == [frags[j] for j in outs]
    # nothing missing, and nothing wanted: no output
    assert _check(lib, 4, 8, [True] * 12)[1:] == ([], [])
    assert _check(lib, 4, 8, [True] * 4 + [False] * 8, [False] * 12)[1:] == ([], [])
    # only parity wanted, one fragment wanted
    ins, outs, rows = _check(lib, 4, 8, [False, True, True, True, True] + [False] * 7, [False] * 4 + [True] * 8)
    assert ins == [1, 2, 3, 4] and outs == [5, 6, 7, 8, 9, 10, 11]
    ins, outs, rows = _check(lib, 4, 8, [False, True, True, True, True] + [False] * 7, [True] + [False] * 11)
    assert outs == [0]


def test_8_8_seeded_500_patterns(lib):
    from oracle import py_rs_code
    rng = random.Random(88)
    frags = _frags(8, 8, 48, 88)
    pats = list(itertools.combinations(range(16), 8))
    assert len(pats) == 12870
    for keep in rng.sample(pats, 500):
        present = [i in keep for i in range(16)]
        ins, outs, rows = _check(lib, 8, 8, present)
        assert ins == list(keep) and len(outs) == 8
        assert py_rs_code(rows, [frags[i] for i in ins]) == [frags[j] for j in outs]
        _check(lib, 8, 8, present, [rng.random() < 0.5 for _ in range(16)])


def test_1_8_and_3_2_every_pattern(lib):
    from oracle import py_rs_code
    f18, f32 = _frags(1, 8, 48, 18), _frags(3, 2, 48, 32)
    for mask in range(1, 1 << 9):
        present = [bool(mask >> i & 1) for i in range(9)]
        ins, outs, rows = _check(lib, 1, 8, present)
        if outs:
            assert py_rs_code(rows, [f18[i] for i in ins]) == [f18[j] for j in outs]
    for mask in range(1 << 5):
        present = [bool(mask >> i & 1) for i in range(5)]
        if sum(present) >= 3:
            ins, outs, rows = _check(lib, 3, 2, present)
            if outs:
                assert py_rs_code(rows, [f32[i] for i in ins]) == [f32[j] for j in outs]
            for wmask in range(1 << 5):
                _check(lib, 3, 2, present, [bool(wmask >> i & 1) for i in range(5)])


def test_three_of_twelve_is_too_few(lib):
    from deoss_amd._lib import DM_ERR_INVALID
    from deoss_amd.reedsolomon import ErrTooFewShards, repair_plan
    present = bytes([0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    ins, outs = (ctypes.c_int * 4)(), (ctypes.c_int * 8)()
    rows = ctypes.create_string_buffer(32)
    nout = ctypes.c_int(-1)
    rc = lib.dm_rs_repair_plan(4, 8, present, None, ins, outs, rows, ctypes.byref(nout))
    assert rc == DM_ERR_INVALID
    assert lib.dm_last_error(None) == b"too few shards given (3 of 4 needed)"
    with pytest.raises(ErrTooFewShards):
        repair_plan(list(present), None, 4, 8)
    # shard counts outside the coder's range
    assert lib.dm_rs_repair_plan(9, 8, present, None, ins, outs, rows, ctypes.byref(nout)) == DM_ERR_INVALID
    assert lib.dm_rs_repair_plan(4, 0, present, None, ins, outs, rows, ctypes.byref(nout)) == DM_ERR_INVALID


def test_repair_fragments_without_a_gpu_fails_the_go_way(lib, tmp_path):
    """No GPU: (0, DeossMerkleError), as FullProcessing.  (Where a GPU is visible the same call fails
    the same way for another reason -- none of the named fragments exists, so the segment has too few
    -- and the test needs no skip.)"""
    from deoss_amd import DeossMerkleError
    from deoss_amd.process import RepairFragments, SegmentDataInfo
    n, err = RepairFragments(str(tmp_path), [SegmentDataInfo("ab" * 32, ["cd" * 32] * 12)])
    assert n == 0 and isinstance(err, DeossMerkleError)
    assert list(tmp_path.iterdir()) == []
