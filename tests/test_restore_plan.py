"""CPU checks of the restore plan (dm_rs_restore_plan): which fragments a segment is rebuilt from,
which data fragments are written and with which GF(2^8) coding rows.

The runtime builds every descriptor of the restore kernel through this same function, so what is
checked here is what runs.  The reference is oracle/oracle.py's Python restatement (py_rs_matrix,
py_gf_inverse), never the library: the rows of data fragment j are row j of the inverse of the
sub-matrix made of the inputs' rows.  No GPU.
"""
from __future__ import annotations

import ctypes
import itertools
import random

import pytest


@pytest.fixture(scope="module")
def lib():
    from deoss_amd import build as b
    b.build(verbose=False)
    from deoss_amd import load_library
    return load_library()


_MATS, _INVS = {}, {}


def _expected(k, m, present, in_place):
    """(inputs, outputs, rows) from the oracle's matrix and inverse alone."""
    from oracle import py_gf_inverse, py_rs_matrix
    if (k, m) not in _MATS:
        _MATS[(k, m)] = py_rs_matrix(k, k + m)
    mat = _MATS[(k, m)]
    inputs = [i for i in range(k + m) if present[i]][:k]
    key = (k, m, tuple(inputs))
    if key not in _INVS:
        _INVS[key] = py_gf_inverse([mat[i] for i in inputs])
    inv = _INVS[key]
    outputs = [j for j in range(k) if not present[j] or not (in_place and in_place[j])]
    return inputs, outputs, [inv[j] for j in outputs]


def _check(lib, k, m, present, in_place=None):
    from deoss_amd.reedsolomon import restore_plan
    ins, outs, rows = restore_plan(present, in_place, k, m)
    want = _expected(k, m, present, in_place)
    assert (ins, outs, rows) == want, (k, m, present, in_place)
    # the properties the issue names, stated directly
    assert ins == [i for i in range(k + m) if present[i]][:k]                 # first k present, index order
    assert all(j in ins for j in range(k) if present[j])                       # a present data fragment is an input
    assert outs == [j for j in range(k) if not present[j] or not (in_place and in_place[j])]
    for j, row in zip(outs, rows):
        if present[j]:                                                         # gather: a unit row
            assert row == [int(ins[q] == j) for q in range(k)]
    return ins, outs, rows


def test_all_495_four_of_twelve_patterns(lib):
    n = 0
    for keep in itertools.combinations(range(12), 4):
        present = [i in keep for i in range(12)]
        ins, outs, rows = _check(lib, 4, 8, present)
        assert ins == list(keep) and outs == [0, 1, 2, 3] and len(rows) == 4
        n += 1
    assert n == 495


def test_4_8_more_than_four_present_with_and_without_in_place(lib):
    rng = random.Random(0x5e57)
    for _ in range(600):
        npres = rng.randint(5, 12)
        keep = set(rng.sample(range(12), npres))
        present = [i in keep for i in range(12)]
        _check(lib, 4, 8, present)
        in_place = [present[j] and rng.random() < 0.6 for j in range(4)]
        ins, outs, rows = _check(lib, 4, 8, present, in_place)
        assert set(outs) == {j for j in range(4) if not (present[j] and in_place[j])}
    # everything in place: nothing to write
    ins, outs, rows = _check(lib, 4, 8, [True] * 12, [True] * 4)
    assert outs == [] and rows == [] and ins == [0, 1, 2, 3]
    # in_place of an absent fragment means nothing
    ins, outs, rows = _check(lib, 4, 8, [False] + [True] * 11, [True] * 4)
    assert outs == [0]


def test_8_8_seeded_500_patterns_with_data_missing(lib):
    rng = random.Random(88)
    pats = [p for p in itertools.combinations(range(16), 8) if any(j not in p for j in range(8))]
    assert len(pats) == 12870 - 1
    for keep in rng.sample(pats, 500):
        present = [i in keep for i in range(16)]
        ins, outs, rows = _check(lib, 8, 8, present)
        assert ins == list(keep)
        in_place = [present[j] and rng.random() < 0.5 for j in range(8)]
        _check(lib, 8, 8, present, in_place)


def test_1_8_every_pattern(lib):
    for mask in range(1, 1 << 9):
        present = [bool(mask >> i & 1) for i in range(9)]
        for in_place in (None, [True], [False]):
            _check(lib, 1, 8, present, in_place)


def test_3_2_every_pattern(lib):
    for mask in range(1 << 5):
        present = [bool(mask >> i & 1) for i in range(5)]
        if sum(present) >= 3:
            _check(lib, 3, 2, present)


def test_three_of_twelve_is_too_few(lib):
    from deoss_amd._lib import DM_ERR_INVALID
    from deoss_amd.reedsolomon import ErrTooFewShards, restore_plan
    present = bytes([0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    ins, outs = (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
    rows = ctypes.create_string_buffer(16)
    nout = ctypes.c_int(-1)
    rc = lib.dm_rs_restore_plan(4, 8, present, None, ins, outs, rows, ctypes.byref(nout))
    assert rc == DM_ERR_INVALID
    assert lib.dm_last_error(None) == b"too few shards given (3 of 4 needed)"
    with pytest.raises(ErrTooFewShards):
        restore_plan(list(present), None, 4, 8)
    # shard counts outside the coder's range
    assert lib.dm_rs_restore_plan(9, 8, present, None, ins, outs, rows, ctypes.byref(nout)) == DM_ERR_INVALID
    assert lib.dm_rs_restore_plan(4, 0, present, None, ins, outs, rows, ctypes.byref(nout)) == DM_ERR_INVALID


def test_fixture_oracle_matches_the_python_restatement(oracle_lib):
    """The C oracle that makes the fragments and names of tests/test_restore_gpu.py, against
    oracle.py's bitwise restatement (a check of the fixtures, not of the library)."""
    import numpy as np
    from oracle import py_full_processing
    buf = np.random.default_rng(1).integers(0, 256, 3 * 256 + 77, dtype=np.uint8).tobytes()
    segd, fragd, fid, raw = oracle_lib.full_processing(buf, 256, 4, 8, want_frags=True)
    segs, frag_h, pfid, frags = py_full_processing(buf, 256, 4, 8)
    assert b"".join(segs) == segd and pfid == fid
    assert b"".join(h for seg in frag_h for h in seg) == fragd
    assert b"".join(f for seg in frags for f in seg) == raw


def test_restore_file_without_a_gpu_fails_the_go_way(lib, tmp_path):
    """No GPU: (False, DeossMerkleError), as FullProcessing.  (Where a GPU is visible the same call
    fails the same way for another reason -- none of the named fragments exists -- so the test
    holds there too and needs no skip.)"""
    from deoss_amd import DeossMerkleError
    from deoss_amd.process import RestoreFile, SegmentDataInfo
    ok, err = RestoreFile(str(tmp_path), [SegmentDataInfo("ab" * 32, ["cd" * 32] * 12)], 1, str(tmp_path / "out"))
    assert ok is False and isinstance(err, DeossMerkleError)
    assert not (tmp_path / "out").exists()
