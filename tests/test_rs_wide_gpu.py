"""The wide Reed-Solomon coder (dm_rs_create_wide, rs_code_wide_kernel): any geometry with
data + parity <= 256, through dm_rs_encode, dm_rs_encode_buffer, dm_rs_reconstruct, dm_rs_verify,
dm_rs_encode_device_async and dm_rs_reconstruct_device_async.

Every comparison is bit-exact and the reference is never the library.  With at most 16 data shards
expected parity is oracle.Oracle.rs_encode (oracle/rs_oracle.c, pinned by klauspost's known answer
in tests/test_rs_oracle.py).  Above that it is a numpy table lookup in this module (_gf_matmul)
with a matrix from this module's vectorised Gauss-Jordan (_gj_matrix); both use a product table
built bit by bit, and the matrix is itself checked against oracle.py_rs_matrix at (10,4), (17,3) and
(64,32) and against the digests of tests/golden/rs_wide_matrices.json at the large geometries
(test_reference_matrix_*, no GPU).  Expected reconstructions are the coded originals.

Device buffers are carved out of 0xEE-filled allocations with 64 guard bytes in front and behind
(and gaps between segments), and whole allocations are compared, with the checker of
tests/test_rs_code_kernel_gpu.py.  _wide_grid restates the launch rule (rs_grid plus one z layer per
group of 8 outputs, csrc/rs_capi.inl) only to state each shape's precondition as an assert over the
device's CU count.

Geometries and the edge each one is: (9,1) first input count past rs_code_kernel's template, one
output; (8,9), (4,12) wide by parity only, the second output group has 1 resp. 4 outputs; (10,4),
(17,3) common, oracle-checked; (16,16) two full groups, the oracle's largest data count; (64,32),
(128,128), (200,56) the middle of the range; (255,1), (1,255) the LDS table at its largest, 32
output groups.
"""
from __future__ import annotations

import ctypes
import hashlib
import json
import os
import random
import threading

import numpy as np
import pytest

from oracle import py_rs_matrix
from test_rs_code_kernel_gpu import (FILL, GUARD, THREADS, _ceil_div, _compare, _image, _oracle_parity, _passes, _rs_grid,
                                     _span)

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(9, 1), (8, 9), (4, 12), (10, 4), (17, 3), (16, 16), (64, 32), (128, 128), (200, 56), (255, 1), (1, 255)]
ORACLE_MAX_DATA = 16                       # oracle/rs_oracle.c
HOST_SIZES = [1, 15, 16, 17, 48, 4096 + 16, 256 * 16 - 16, 256 * 16 + 16]
DM_ERR_INVALID = -2
REFUSED = "%s needs a fragment coder of at most 8 + 8 shards"


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _wide_grid(cus, units, nseg, nout):
    """launch_rs_wide's rule: (gx, gy, gz)."""
    return _rs_grid(cus, units, nseg) + (_ceil_div(nout, 8),)


# ---- the reference above 16 data shards: GF(2^8) in numpy ---------------------------------------

def _build_mul():
    """MUL[a][b] = a * b over GF(2^8) mod x^8 + x^4 + x^3 + x^2 + 1, shift and add, no log tables."""
    a = np.arange(256, dtype=np.uint16).reshape(256, 1) * np.ones((1, 256), dtype=np.uint16)
    b = np.arange(256, dtype=np.uint16).reshape(1, 256)
    res = np.zeros((256, 256), dtype=np.uint16)
    for bit in range(8):
        res ^= np.where((b >> bit) & 1, a, 0).astype(np.uint16)
        a = a << 1
        a ^= np.where(a & 0x100, 0x11d, 0).astype(np.uint16)
    assert res.max() < 256
    return res.astype(np.uint8)


MUL = _build_mul()
INV = np.zeros(256, dtype=np.uint8)
INV[1:] = [int(np.flatnonzero(MUL[x] == 1)[0]) for x in range(1, 256)]


def _gf_matmul(a, b):
    """a (n x k) x b (k x p) over GF(2^8): one table lookup per term."""
    out = np.zeros((a.shape[0], b.shape[1]), dtype=np.uint8)
    for t in range(a.shape[1]):
        out ^= MUL[a[:, t].reshape(-1, 1), b[t].reshape(1, -1)]
    return out


def _gf_inverse(mat):
    k = mat.shape[0]
    w = np.concatenate([mat.astype(np.uint8), np.eye(k, dtype=np.uint8)], axis=1)
    for c in range(k):
        p = c + int(np.flatnonzero(w[c:, c])[0])
        if p != c:
            w[[c, p]] = w[[p, c]]
        w[c] = MUL[w[c], INV[w[c, c]]]
        f = w[:, c].copy()
        f[c] = 0
        w ^= MUL[f.reshape(-1, 1), w[c].reshape(1, -1)]
    assert np.array_equal(w[:, :k], np.eye(k, dtype=np.uint8))
    return w[:, k:]


_MATS = {}


def _gj_matrix(k, m):
    """klauspost's default matrix: vandermonde(k + m, k) x inverse(its top k x k)."""
    if (k, m) not in _MATS:
        total = k + m
        vm = np.zeros((total, k), dtype=np.uint8)
        vm[:, 0] = 1
        r = np.arange(total, dtype=np.uint8)
        for j in range(1, k):
            vm[:, j] = MUL[vm[:, j - 1], r]
        mat = _gf_matmul(vm, _gf_inverse(vm[:k]))
        mat.setflags(write=False)
        _MATS[(k, m)] = mat
    return _MATS[(k, m)]


@pytest.mark.parametrize("k, m", [(10, 4), (17, 3), (64, 32)])
def test_reference_matrix_equals_the_python_restatement(k, m):
    assert [bytes(r) for r in _gj_matrix(k, m)] == [bytes(r) for r in py_rs_matrix(k, k + m)]


def test_reference_matrix_equals_the_committed_digests():
    with open(os.path.join(ROOT, "tests", "golden", "rs_wide_matrices.json")) as f:
        golden = json.load(f)["matrices"]
    assert {(g["data"], g["parity"]) for g in golden} == {(128, 128), (200, 56), (255, 1), (1, 255)}
    for g in golden:
        mat = _gj_matrix(g["data"], g["parity"])
        assert hashlib.sha256(mat.tobytes()).hexdigest() == g["sha256"], (g["data"], g["parity"])
        assert bytes(mat[g["data"]]).hex() == g["first_parity_row"]


def test_product_table():
    """The bit-by-bit table against known products of this field (0x11d): 2 * 0x80 = 0x1d,
    3 * 7 = 9, 0x53 * 0xca != 1 here (that pair is inverse under AES's 0x11b), x * inverse = 1."""
    assert MUL[2, 0x80] == 0x1d and MUL[3, 7] == 9 and MUL[0x53, 0xca] != 1
    assert all(MUL[x, INV[x]] == 1 for x in range(1, 256)) and not MUL[0].any() and np.array_equal(MUL, MUL.T)
    assert np.array_equal(MUL[1], np.arange(256, dtype=np.uint8))


# ---- coded sets, computed once per (geometry, size, seed) ---------------------------------------

_CODED = {}


def _coded(oracle_lib, k, m, n, seed):
    """(k + m, n) uint8, read-only: seeded data shards and their parity."""
    key = (k, m, n, seed)
    if key not in _CODED:
        data = np.random.default_rng(seed).integers(0, 256, (k, n), dtype=np.uint8)
        if k <= ORACLE_MAX_DATA:
            par = np.frombuffer(b"".join(oracle_lib.rs_encode([data[j].tobytes() for j in range(k)], m, nthreads=8)),
                                dtype=np.uint8).reshape(m, n)
        else:
            par = _gf_matmul(_gj_matrix(k, m)[k:], data)
        full = np.concatenate([data, par])
        full.setflags(write=False)
        _CODED[key] = full
    return _CODED[key]


def test_numpy_reference_equals_the_oracle(oracle_lib):
    """Where both references apply they agree: (16,16) and (10,4), 100 bytes."""
    for k, m in [(16, 16), (10, 4), (1, 255)]:
        full = _coded(oracle_lib, k, m, 100, 7)
        assert np.array_equal(_gf_matmul(_gj_matrix(k, m)[k:], full[:k]), full[k:]), (k, m)


def _new(ctx, k, m):
    from deoss_amd.reedsolomon import New
    enc = New(ctx, k, m)
    assert (enc.data_shards, enc.parity_shards) == (k, m)
    return enc


# ---- encode: host API at every geometry ---------------------------------------------------------

@gpu
@pytest.mark.parametrize("k, m", GEOMETRIES)
def test_encode_host_sizes_and_matrix(ctx, oracle_lib, k, m):
    """dm_rs_encode at shard sizes 1, 15, 16, 17, 48, 4096 + 16 and 256 x 16 -+ 16 bytes (one
    workgroup, -+ one unit; the padded last unit of an odd size is coded and never copied back),
    dm_rs_encode_buffer, dm_rs_matrix, and one dm_rs_encode_device_async call of 2 segments with gaps."""
    torch = _torch()
    total_n = sum(HOST_SIZES)
    full = _coded(oracle_lib, k, m, total_n, 1000 * k + m)
    enc = _new(ctx, k, m)
    try:
        assert np.array_equal(np.array(enc.matrix(), dtype=np.uint8), _gj_matrix(k, m))
        off = 0
        for n in HOST_SIZES:
            assert _rs_grid(_cus(), _ceil_div(n, 16), 1) == (_ceil_div(_ceil_div(n, 16), THREADS), 1)
            part = full[:, off:off + n]
            got = enc.Encode([part[j].tobytes() for j in range(k)] + [b""] * m)
            assert len(got) == k + m
            for i in range(k + m):
                assert got[i] == part[i].tobytes(), ("shard", i, "size", n, (k, m))
            off += n
        part = full[:, :48]
        assert enc.EncodeBuffer(part[:k].tobytes()) == [part[i].tobytes() for i in range(k + m)]
        # device form: 2 segments of 5 units, gaps of 32 and 48 bytes
        nseg, shard = 2, 80
        assert _wide_grid(_cus(), 5, nseg, m) == (1, 2, _ceil_div(m, 8))
        seg = np.ascontiguousarray(full[:, :nseg * shard].reshape(k + m, nseg, shard).transpose(1, 0, 2))
        dstride, pstride = k * shard + 32, m * shard + 48
        ddev = torch.from_numpy(_image(np.ascontiguousarray(seg[:, :k]), dstride)).cuda()
        pdev = torch.full((2 * GUARD + _span(nseg, m, shard, pstride),), FILL, dtype=torch.uint8, device="cuda")
        enc.encode_device_async(ddev.data_ptr() + GUARD, dstride, pdev.data_ptr() + GUARD, pstride, shard, nseg, 0)
        torch.cuda.synchronize()
        _compare(pdev.cpu().numpy(), np.ascontiguousarray(seg[:, k:]), pstride, ("parity", (k, m)))
        _compare(ddev.cpu().numpy(), np.ascontiguousarray(seg[:, :k]), dstride, ("data", (k, m)))
    finally:
        enc.close()


# ---- encode: the grid and loop edges through dm_rs_encode_device_async --------------------------

def _check_encode(ctx, oracle_lib, k, m, shard, nseg, data_gap, parity_gap, seed):
    torch = _torch()
    dstride = 0 if data_gap is None else k * shard + data_gap
    pstride = 0 if parity_gap is None else m * shard + parity_gap
    data = np.random.default_rng(seed).integers(0, 256, (nseg, k, shard), dtype=np.uint8)
    want = _oracle_parity(oracle_lib, data, m)
    ddev = torch.from_numpy(_image(data, dstride)).cuda()
    pdev = torch.full((2 * GUARD + _span(nseg, m, shard, pstride),), FILL, dtype=torch.uint8, device="cuda")
    assert (ddev.data_ptr() + GUARD) % 16 == 0 and (pdev.data_ptr() + GUARD) % 16 == 0
    enc = _new(ctx, k, m)
    try:
        enc.encode_device_async(ddev.data_ptr() + GUARD, dstride, pdev.data_ptr() + GUARD, pstride, shard, nseg, 0)
        torch.cuda.synchronize()
    finally:
        enc.close()
    tag = (k, m, shard, nseg, dstride, pstride)
    _compare(pdev.cpu().numpy(), want, pstride, ("parity", tag))
    _compare(ddev.cpu().numpy(), data, dstride, ("data", tag))


@gpu
@pytest.mark.parametrize("k, m", [(10, 4), (4, 12)])
def test_encode_stride_loop_runs_twice_for_the_first_lane(ctx, oracle_lib, k, m):
    """One unit more than one pass of the whole x-grid holds: lane 0 of workgroup 0 makes two passes
    of the stride loop, every other lane one."""
    gx0, _ = _rs_grid(_cus(), 1 << 30, 1)
    units = gx0 * THREADS + 1
    gx, gy, gz = _wide_grid(_cus(), units, 1, m)
    assert (gx, gy, gz) == (gx0, 1, _ceil_div(m, 8)) and _passes(units, gx) == (2, 1)
    _check_encode(ctx, oracle_lib, k, m, 16 * units, 1, None, None, 31 * k + m)


@gpu
@pytest.mark.parametrize("k, m", [(10, 4), (4, 12)])
@pytest.mark.parametrize("nseg", [1, 3])
def test_encode_segments_with_gaps(ctx, oracle_lib, k, m, nseg):
    """257 units per shard (two workgroups per grid row, the second with one lane at work), 1 and 3
    segments, strides that leave gaps."""
    units = 257
    assert _wide_grid(_cus(), units, nseg, m) == (2, nseg, _ceil_div(m, 8))
    _check_encode(ctx, oracle_lib, k, m, 16 * units, nseg, 32, 48, 57 * k + m + nseg)


@gpu
@pytest.mark.parametrize("k, m", [(10, 4), (4, 12)])
def test_encode_more_segments_than_grid_rows(ctx, oracle_lib, k, m):
    """One segment more than the y-grid holds, 16-byte shards: the segment loop wraps for the
    workgroups of row 0."""
    nseg = 8 * _cus() + 1
    gx, gy, gz = _wide_grid(_cus(), 1, nseg, m)
    assert gx == 1 and gy == nseg - 1 and gz == _ceil_div(m, 8), (gx, gy, gz)
    _check_encode(ctx, oracle_lib, k, m, 16, nseg, 32, 48, 77 * k + m)


# ---- reconstruct --------------------------------------------------------------------------------

def _lost_sets(k, m, seed):
    """[(name, lost)]: one data, one parity, exactly m, and all data where m >= k."""
    rng = random.Random(seed)
    total = k + m
    sets = [("one data shard", [rng.randrange(k)]), ("one parity shard", [k + rng.randrange(m)]),
            ("exactly parity shards", rng.sample(range(total), m))]
    if m >= k:
        sets.append(("all data", list(range(k))))
    return sets


def test_lost_sets_cover_what_they_claim():
    more_than_8_rebuilt = set()
    for k, m in GEOMETRIES:
        sets = dict(_lost_sets(k, m, 5))
        assert sets["one data shard"][0] < k <= sets["one parity shard"][0] < k + m
        assert len(set(sets["exactly parity shards"])) == m
        assert ("all data" in sets) == (m >= k)
        if "all data" in sets and k > 8:
            more_than_8_rebuilt.add((k, m))
    assert more_than_8_rebuilt == {(16, 16), (128, 128)}


@gpu
@pytest.mark.parametrize("k, m", GEOMETRIES)
def test_reconstruct_host_and_device(ctx, oracle_lib, k, m):
    """dm_rs_reconstruct and dm_rs_reconstruct_device_async at 37 units per shard: nothing missing
    (every byte as it was), one data shard, one parity shard, exactly `parity` shards, all data
    shards where parity >= data; then parity + 1 missing: DM_ERR_INVALID "too few shards given" and
    no byte changed."""
    torch = _torch()
    from deoss_amd.reedsolomon import ErrTooFewShards
    total, shard = k + m, 16 * 37
    full = _coded(oracle_lib, k, m, shard, 3000 + 10 * k + m)
    want = np.ascontiguousarray(full).reshape(1, total, shard)
    clean = torch.from_numpy(_image(want, 0)).cuda()
    L = ctx._L
    enc = _new(ctx, k, m)
    try:
        def device(lost, tag):
            buf = clean.clone()
            base = buf.data_ptr() + GUARD
            assert base % 16 == 0
            for i in lost:
                buf[GUARD + i * shard:GUARD + (i + 1) * shard] = 0x5A
            before = buf.cpu().numpy()
            try:
                enc.reconstruct_device_async([base + i * shard for i in range(total)],
                                             [i not in lost for i in range(total)], shard, 0)
            finally:
                torch.cuda.synchronize()
            return before, buf.cpu().numpy(), tag

        _, after, tag = device([], "nothing missing")
        _compare(after, want, 0, (tag, (k, m)))
        assert enc.Reconstruct([full[i].tobytes() for i in range(total)]) == [full[i].tobytes() for i in range(total)]
        for name, lost in _lost_sets(k, m, 40 * k + m):
            _, after, tag = device(lost, name)
            _compare(after, want, 0, ("device", tag, (k, m), sorted(lost)))
            got = enc.Reconstruct([None if i in lost else full[i].tobytes() for i in range(total)])
            for i in range(total):
                assert got[i] == full[i].tobytes(), ("host", name, (k, m), "shard", i)
        # one more than parity missing
        lost = random.Random(50 * k + m).sample(range(total), m + 1)
        text = "too few shards given (%d of %d needed)" % (k - 1, k)
        with pytest.raises(ErrTooFewShards):
            device(lost, "too few")
        assert text in L.dm_last_error(ctx._h).decode()
        buf = clean.clone()
        for i in lost:
            buf[GUARD + i * shard:GUARD + (i + 1) * shard] = 0x5A
        before = buf.cpu().numpy()
        base = buf.data_ptr() + GUARD
        ptrs = (ctypes.c_void_p * total)(*[base + i * shard for i in range(total)])
        present = bytes(int(i not in lost) for i in range(total))
        assert L.dm_rs_reconstruct_device_async(enc._h, ptrs, present, shard, None) == DM_ERR_INVALID
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), before)
        # host form, raw: the caller's buffers stay as they were
        bufs = [ctypes.create_string_buffer(bytes([0x5A]) * shard if i in lost else full[i].tobytes(), shard)
                for i in range(total)]
        hp = (ctypes.c_void_p * total)(*[ctypes.addressof(b) for b in bufs])
        assert L.dm_rs_reconstruct(enc._h, hp, present, shard) == DM_ERR_INVALID
        assert L.dm_last_error(ctx._h).decode() == text
        for i in range(total):
            assert bufs[i].raw == (bytes([0x5A]) * shard if i in lost else full[i].tobytes()), i
    finally:
        enc.close()


# ---- verify -------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("k, m", GEOMETRIES)
def test_verify(ctx, oracle_lib, k, m):
    total, n = k + m, 100
    full = _coded(oracle_lib, k, m, n, 6000 + 10 * k + m)
    shards = [full[i].tobytes() for i in range(total)]
    enc = _new(ctx, k, m)
    try:
        assert enc.Verify(shards) is True
        bad = list(shards)
        bad[total - 1] = bad[total - 1][:n - 1] + bytes([bad[total - 1][n - 1] ^ 0x01])
        assert enc.Verify(bad) is False
        bad = list(shards)
        bad[0] = bytes([bad[0][0] ^ 0x80]) + bad[0][1:]
        assert enc.Verify(bad) is False
    finally:
        enc.close()


# ---- the constructor's limits; identity within 8 + 8 ---------------------------------------------

@gpu
def test_create_limits(ctx):
    L = ctx._L
    h = ctypes.c_void_p()
    assert L.dm_rs_create(ctx._h, 9, 2, ctypes.byref(h)) == DM_ERR_INVALID and not h.value
    assert L.dm_last_error(ctx._h).decode() == "shard counts: 1 <= data <= 8, 1 <= parity <= 8"
    assert L.dm_rs_create(ctx._h, 2, 9, ctypes.byref(h)) == DM_ERR_INVALID and not h.value
    for k, m, text in [(0, 1, "less than one data shard"), (1, 0, "less than one parity shard"),
                       (255, 2, "more than 256 data+parity shards"), (256, 1, "more than 256 data+parity shards")]:
        assert L.dm_rs_create_wide(ctx._h, k, m, ctypes.byref(h)) == DM_ERR_INVALID and not h.value, (k, m)
        assert text in L.dm_last_error(ctx._h).decode(), (k, m)


@gpu
def test_within_8_plus_8_the_wide_constructor_gives_the_fragment_coder(ctx, oracle_lib):
    """dm_rs_create_wide(4, 8) and dm_rs_create(4, 8): identical parity for 1,000 bytes per shard
    (the oracle's), and the handle passes dm_process_buffer."""
    L = ctx._L
    k, m, n = 4, 8, 1000
    full = _coded(oracle_lib, k, m, n, 48)
    handles = []
    try:
        for create in (L.dm_rs_create_wide, L.dm_rs_create):
            h = ctypes.c_void_p()
            assert create(ctx._h, k, m, ctypes.byref(h)) == 0
            handles.append(h)
        outs = []
        for h in handles:
            ins = [ctypes.create_string_buffer(full[j].tobytes(), n) for j in range(k)]
            par = [ctypes.create_string_buffer(n) for _ in range(m)]
            dp = (ctypes.c_void_p * k)(*[ctypes.addressof(b) for b in ins])
            pp = (ctypes.c_void_p * m)(*[ctypes.addressof(b) for b in par])
            assert L.dm_rs_encode(h, dp, pp, n) == 0
            outs.append([b.raw for b in par])
        assert outs[0] == outs[1] == [full[k + i].tobytes() for i in range(m)]
        segment, length = 4096, 3 * 4096 - 100
        obj = np.random.default_rng(9).integers(0, 256, length, dtype=np.uint8).tobytes()
        want_seg, want_frag, want_fid, raw = oracle_lib.full_processing(obj, segment, k, m, want_frags=True)
        nseg = 3
        frags = ctypes.create_string_buffer(nseg * (k + m) * (segment // k))
        segh, fragh = ctypes.create_string_buffer(nseg * 32), ctypes.create_string_buffer(nseg * (k + m) * 32)
        fid = ctypes.create_string_buffer(32)
        src = ctypes.create_string_buffer(obj, length)
        assert L.dm_process_buffer(handles[0], src, length, segment, frags, segh, fragh, fid) == 0
        assert (frags.raw, segh.raw, fragh.raw, fid.raw) == (bytes(raw), bytes(want_seg), bytes(want_frag), bytes(want_fid))
    finally:
        for h in handles:
            L.dm_rs_destroy(h)


# ---- every other entry point refuses a wide coder -----------------------------------------------

@gpu
def test_other_entry_points_refuse_a_wide_coder(ctx, tmp_path):
    """A (10,4) coder: DM_ERR_INVALID with the stated text from dm_process_buffer, dm_restore_buffer,
    dm_repair_buffer, dm_restore_range_buffer, dm_pstream_open and dm_full_processing; no output
    byte is written and no file appears."""
    L = ctx._L
    k, m = 10, 4
    total, segment = k + m, 1600
    frag = segment // k
    enc = _new(ctx, k, m)
    sent = bytes([0xC3])

    def fresh(n):
        return ctypes.create_string_buffer(sent * n, n)

    def refused(rc, fn, *outs):
        assert rc == DM_ERR_INVALID, (fn, rc)
        assert L.dm_last_error(ctx._h).decode() == REFUSED % fn
        for o in outs:
            assert o.raw == sent * len(o.raw), fn

    try:
        obj = fresh(segment)
        frags_out, segh, fragh, fid = fresh(total * frag), fresh(32), fresh(total * 32), fresh(32)
        refused(L.dm_process_buffer(enc._h, obj, segment, segment, frags_out, segh, fragh, fid), "dm_process_buffer",
                frags_out, segh, fragh, fid)
        held = [fresh(frag) for _ in range(total)]
        fp = (ctypes.c_void_p * total)(*[ctypes.addressof(b) for b in held])
        names = fresh(total * 32)
        out, fst, sst = fresh(segment), fresh(total), fresh(1)
        ok = ctypes.c_int(7)
        refused(L.dm_restore_buffer(enc._h, fp, None, None, None, 1, segment, segment, 0, out, fst, sst, ctypes.byref(ok)),
                "dm_restore_buffer", out, fst, sst)
        assert ok.value == 0
        rebuilt = [fresh(frag) for _ in range(total)]
        op = (ctypes.c_void_p * total)(*[ctypes.addressof(b) for b in rebuilt])
        ok = ctypes.c_int(7)
        refused(L.dm_repair_buffer(enc._h, fp, op, names, 1, segment, fst, sst, ctypes.byref(ok)), "dm_repair_buffer",
                fst, sst, *rebuilt)
        assert ok.value == 0
        ok = ctypes.c_int(7)
        refused(L.dm_restore_range_buffer(enc._h, fp, names, 1, segment, segment, 0, 16, 0, None, 0, out, fst, sst,
                                          ctypes.byref(ok)), "dm_restore_range_buffer", out, fst, sst)
        assert ok.value == 0
        savedir = tmp_path / "save"
        savedir.mkdir()
        ps = ctypes.c_void_p()
        refused(L.dm_pstream_open(enc._h, segment, str(savedir).encode(), 0, ctypes.byref(ps)), "dm_pstream_open")
        assert not ps.value
        src = tmp_path / "object.bin"
        src.write_bytes(bytes(range(256)) * 20)
        nseg_out = ctypes.c_uint64(99)
        refused(L.dm_full_processing(enc._h, str(src).encode(), str(savedir).encode(), segment, 0, segh, fragh, 1,
                                     ctypes.byref(nseg_out), fid), "dm_full_processing", segh, fragh, fid)
        assert nseg_out.value == 0
        assert os.listdir(savedir) == [] and sorted(os.listdir(tmp_path)) == ["object.bin", "save"]
    finally:
        enc.close()


# ---- the C++ mirror ------------------------------------------------------------------------------

@gpu
def test_cpp_reedsolomon_mirror(oracle_lib, tmp_path):
    """Compile and run tests/cpp/test_reedsolomon.cpp: include/deoss_reedsolomon.hpp at (4,8), (10,4),
    (16,4) and (12,12) against oracle/rs_oracle.c, and klauspost's errors from New."""
    import subprocess
    exe = str(tmp_path / "test_reedsolomon")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_reedsolomon.cpp"),
                    "-L", os.path.join(ROOT, "deoss_amd"), "-ldeoss_merkle",
                    "-L", os.path.join(ROOT, "oracle"), "-loracle_merkle",   # the checker's restatement only
                    "-Wl,-rpath," + os.path.join(ROOT, "deoss_amd") + ":" + os.path.join(ROOT, "oracle"),
                    "-lpthread", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr


# ---- two call lanes ------------------------------------------------------------------------------

@gpu
def test_two_geometries_on_two_call_lanes(oracle_lib):
    """Two threads on one MerkleContext(lanes=2), one coding at (10,4) and one at (17,3): host
    encode, host reconstruct with `parity` shards lost and a device encode, three rounds each, at
    the same time.  The references are computed before a thread starts."""
    torch = _torch()
    from deoss_amd import MerkleContext
    jobs = []
    for k, m, n in [(10, 4, 16 * 300 + 5), (17, 3, 16 * 257 + 9)]:
        full = _coded(oracle_lib, k, m, n, 7000 + k)
        shard = 16 * 64
        seg = np.ascontiguousarray(full[:, :2 * shard].reshape(k + m, 2, shard).transpose(1, 0, 2))
        lost = random.Random(k).sample(range(k + m), m)
        jobs.append(dict(k=k, m=m, full=full, seg=seg, shard=shard, lost=lost))
    ctx2 = MerkleContext(lanes=2)
    errors = []
    barrier = threading.Barrier(len(jobs))

    def worker(job):
        try:
            k, m, full, seg, shard = job["k"], job["m"], job["full"], job["seg"], job["shard"]
            total = k + m
            enc = _new(ctx2, k, m)
            stream = torch.cuda.Stream()
            dstride, pstride = k * shard + 32, m * shard + 48
            ddev = torch.from_numpy(_image(np.ascontiguousarray(seg[:, :k]), dstride)).cuda()
            torch.cuda.synchronize()
            barrier.wait()
            for _ in range(3):
                pdev = torch.full((2 * GUARD + _span(2, m, shard, pstride),), FILL, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                enc.encode_device_async(ddev.data_ptr() + GUARD, dstride, pdev.data_ptr() + GUARD, pstride, shard, 2,
                                        stream.cuda_stream)
                got = enc.Encode([full[j].tobytes() for j in range(k)] + [b""] * m)
                assert got == [full[i].tobytes() for i in range(total)], ("encode", k, m)
                got = enc.Reconstruct([None if i in job["lost"] else full[i].tobytes() for i in range(total)])
                assert got == [full[i].tobytes() for i in range(total)], ("reconstruct", k, m)
                stream.synchronize()
                _compare(pdev.cpu().numpy(), np.ascontiguousarray(seg[:, k:]), pstride, ("device parity", (k, m)))
            enc.close()
        except BaseException as e:   # noqa: BLE001 -- reported by the main thread
            errors.append((job["k"], job["m"], repr(e)))
            barrier.abort()

    threads = [threading.Thread(target=worker, args=(j,)) for j in jobs]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert ctx2._L.dm_lane_count(ctx2._h) == 2
    finally:
        ctx2.close()
    assert errors == []
