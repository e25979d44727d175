"""CPU tests of the wide Reed-Solomon coder's host side (any geometry with data + parity <= 256).

dm_rs_coding_matrix (a pure host function of the built library: no GPU, no context) against the
bitwise Python restatement ``oracle.py_rs_matrix``, directly where that is quick and through the
digests of tests/golden/rs_wide_matrices.json (tests/golden/make_rs_wide_matrices.py) where it takes
from 12 s to over a minute; and tests/cpp/test_rs_wide_plan.cpp (inverse, reconstruct plan, nibble
tables of deoss_amd/csrc/rs_plan.hpp), a stand-alone program built plain and with ASan/UBSan.
"""
import ctypes
import hashlib
import json
import os
import subprocess

import pytest

from oracle import py_rs_matrix
from test_fp_host import ROOT, _builds

DM_ERR_INVALID = -2
ORACLE_CHECKED = [(9, 1), (8, 9), (4, 12), (10, 4), (17, 3), (16, 16), (64, 32)]
FIXTURE_CHECKED = [(128, 128), (200, 56), (255, 1), (1, 255)]


@pytest.fixture(scope="module")
def lib():
    from deoss_amd import build as b
    b.build(verbose=False)
    from deoss_amd import load_library
    return load_library()


def _matrix(lib, k, m):
    out = ctypes.create_string_buffer((k + m) * k)
    assert lib.dm_rs_coding_matrix(k, m, out) == 0, (k, m, lib.dm_last_error(None))
    return out.raw


def _rows(raw, k):
    return [raw[i:i + k] for i in range(0, len(raw), k)]


@pytest.mark.parametrize("k, m", ORACLE_CHECKED)
def test_matrix_equals_the_python_restatement(lib, k, m):
    rows = _rows(_matrix(lib, k, m), k)
    assert rows == [bytes(r) for r in py_rs_matrix(k, k + m)]
    assert rows[:k] == [bytes(int(i == j) for j in range(k)) for i in range(k)]


@pytest.mark.parametrize("k, m", FIXTURE_CHECKED)
def test_matrix_equals_the_committed_digest(lib, k, m):
    with open(os.path.join(ROOT, "tests", "golden", "rs_wide_matrices.json")) as f:
        golden = {(g["data"], g["parity"]): g for g in json.load(f)["matrices"]}
    assert set(golden) == set(FIXTURE_CHECKED)
    raw = _matrix(lib, k, m)
    rows = _rows(raw, k)
    assert len(rows) == k + m
    assert rows[:k] == [bytes(int(i == j) for j in range(k)) for i in range(k)]
    assert rows[k].hex() == golden[(k, m)]["first_parity_row"]
    assert hashlib.sha256(raw).hexdigest() == golden[(k, m)]["sha256"]


def test_parity_row_of_255_plus_1_is_all_ones(lib):
    """255 + 1: the single parity shard is the xor of the data shards (row 255 of the Vandermonde
    matrix is 255^j, and the top 255 rows hold every power of every other element)."""
    assert _rows(_matrix(lib, 255, 1), 255)[255] == bytes([1]) * 255
    with open(os.path.join(ROOT, "tests", "golden", "rs_wide_matrices.json")) as f:
        g = [x for x in json.load(f)["matrices"] if (x["data"], x["parity"]) == (255, 1)]
    assert g[0]["first_parity_row"] == "01" * 255


def test_within_8_plus_8_equals_the_golden_matrices(lib):
    with open(os.path.join(ROOT, "tests", "golden", "rs_golden.json")) as f:
        mats = json.load(f)["matrices"]
    assert {(4, 8), (8, 8)} <= {(g["data"], g["parity"]) for g in mats}
    for g in mats:
        k, m = g["data"], g["parity"]
        assert [r.hex() for r in _rows(_matrix(lib, k, m), k)] == g["rows"], (k, m)


def test_invalid_counts(lib):
    out = ctypes.create_string_buffer(256 * 256)
    texts = {}
    for k, m in [(0, 1), (1, 0), (255, 2), (256, 1), (-1, 4), (4, -1)]:
        assert lib.dm_rs_coding_matrix(k, m, out) == DM_ERR_INVALID, (k, m)
        texts[(k, m)] = lib.dm_last_error(None).decode()
    # klauspost's ErrInvShardNum and ErrMaxShardNum
    assert "less than one data shard" in texts[(0, 1)]
    assert texts[(255, 2)] == texts[(256, 1)] == "cannot create Encoder with more than 256 data+parity shards"
    assert lib.dm_rs_coding_matrix(4, 8, None) == DM_ERR_INVALID
    # the edges that are valid
    for k, m in [(1, 1), (255, 1), (1, 255), (254, 2)]:
        assert lib.dm_rs_coding_matrix(k, m, out) == 0, (k, m)


def test_rs_create_keeps_its_limit(lib):
    """dm_rs_create(9, 2) stays DM_ERR_INVALID.  Without a GPU there is no context, and the call is
    invalid for that alone; tests/test_rs_wide_gpu.py repeats it with the limit's own text."""
    import torch
    if not torch.cuda.is_available():
        h = ctypes.c_void_p()
        assert lib.dm_rs_create(None, 9, 2, ctypes.byref(h)) == DM_ERR_INVALID
        assert lib.dm_rs_create_wide(None, 10, 4, ctypes.byref(h)) == DM_ERR_INVALID
        return
    from deoss_amd import MerkleContext
    c = MerkleContext()
    try:
        h = ctypes.c_void_p()
        assert lib.dm_rs_create(c._h, 9, 2, ctypes.byref(h)) == DM_ERR_INVALID and not h.value
        assert "1 <= data <= 8" in lib.dm_last_error(c._h).decode()
    finally:
        c.close()


def test_rs_wide_plan_cpp_plain_and_asan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_rs_wide_plan.cpp")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for name, cc in _builds():
        exe = str(tmp_path / f"test_rs_wide_plan_{name}")
        subprocess.run(cc + [src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, env=env)
        assert out.returncode == 0, (name, out.stdout, out.stderr)
        assert "rs wide plan OK" in out.stdout
