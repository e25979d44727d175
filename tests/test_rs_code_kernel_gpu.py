"""rs_code_kernel at its grid and loop edges, through dm_rs_encode_device_async,
dm_rs_reconstruct_device_async and dm_process_device_async.

Every comparison is bit-exact.  The reference is never the code under test: expected parity is
oracle.Oracle.rs_encode (oracle/rs_oracle.c, pinned by klauspost's known answer in
tests/test_rs_oracle.py), expected reconstructions are the oracle-coded originals, and
FullProcessing results are Oracle.full_processing(..., want_frags=True).

Every device buffer the kernel reads or writes is carved out of a larger 0xEE-filled allocation
(64 guard bytes in front and behind, gaps between segments where the strides leave them), and the
whole allocation is compared with the image the oracle predicts: a store one unit past a shard,
into a gap or into the input shows as a changed guard byte.

The launch rule (rs_grid, csrc/rs_capi.inl) is restated in _rs_grid only to state each shape's
precondition -- which loop of the kernel it runs -- as an assert over the device's CU count: on a
chip where a shape no longer reaches its edge the test fails instead of covering nothing.
"""
from __future__ import annotations

import random

import numpy as np
import pytest

from oracle import py_rs_encode

gpu = pytest.mark.gpu

THREADS = 256      # kRsThreads
GUARD = 64
FILL = 0xEE


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _cus():
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _ceil_div(a, b):
    return -(-a // b)


def _rs_grid(cus, units, nseg):
    """rs_grid's rule: (gx, gy)."""
    target = 8 * cus
    gy = min(nseg, 65535, target)
    gx = max(1, min(_ceil_div(units, THREADS), _ceil_div(target, gy)))
    return gx, gy


def _passes(units, gx):
    """(most, fewest) passes of the stride loop over the lanes of one grid row."""
    stride = gx * THREADS
    return _ceil_div(units, stride), units // stride


def _rand(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---- the reference: one oracle call for many segments ------------------------------------------

def _oracle_parity(oracle_lib, data, m, nthreads=8):
    """data: (nseg, k, shard) uint8 -> parity (nseg, m, shard).  The code is position-independent,
    so shard j of all segments is concatenated, coded in one call and cut back into segments
    (test_concatenated_encode_equals_per_segment)."""
    nseg, k, shard = data.shape
    cols = [np.ascontiguousarray(data[:, j, :]).tobytes() for j in range(k)]
    par = oracle_lib.rs_encode(cols, m, nthreads=nthreads)
    out = np.empty((nseg, m, shard), dtype=np.uint8)
    for i in range(m):
        out[:, i, :] = np.frombuffer(par[i], dtype=np.uint8).reshape(nseg, shard)
    return out


def test_concatenated_encode_equals_per_segment(oracle_lib):
    """One oracle call over the concatenated shards == one call per segment; and the C oracle ==
    the bitwise Python restatement for every (k, m) in 1..8 x 1..8 at a 48-byte shard."""
    for k, m, nseg, shard in [(4, 8, 7, 48), (3, 2, 5, 16), (8, 8, 3, 80), (1, 8, 4, 32)]:
        data = _rand((nseg, k, shard), 100 * k + m)
        got = _oracle_parity(oracle_lib, data, m)
        for s in range(nseg):
            want = oracle_lib.rs_encode([data[s, j].tobytes() for j in range(k)], m)
            assert [got[s, i].tobytes() for i in range(m)] == want, (k, m, s)
    for k in range(1, 9):
        for m in range(1, 9):
            shards = [_rand(48, 1000 + 10 * k + m + 100 * j).tobytes() for j in range(k)]
            assert oracle_lib.rs_encode(shards, m) == py_rs_encode(shards, m), (k, m)


# ---- the checker: a guarded layout and its comparison -----------------------------------------

def _span(nseg, rows, shard, stride):
    return (nseg - 1) * stride + rows * shard


def _image(shards, stride):
    """The bytes of a whole guarded allocation: shards (nseg, rows, shard) with row r of segment s
    at GUARD + s * stride + r * shard, 0xEE everywhere else."""
    nseg, rows, shard = shards.shape
    assert stride % 16 == 0 and shard % 16 == 0 and (stride >= rows * shard or nseg == 1)
    img = np.full(2 * GUARD + _span(nseg, rows, shard, stride), FILL, dtype=np.uint8)
    if stride == rows * shard or nseg == 1:
        img[GUARD:GUARD + nseg * rows * shard] = shards.reshape(-1)
    else:
        body = img[GUARD:GUARD + (nseg - 1) * stride].reshape(nseg - 1, stride)
        body[:, :rows * shard] = shards[:-1].reshape(nseg - 1, rows * shard)
        img[GUARD + (nseg - 1) * stride:GUARD + (nseg - 1) * stride + rows * shard] = shards[-1].reshape(-1)
    return img


def _compare(got, want_shards, stride, what):
    """got: the whole allocation after the call (host bytes).  Raises AssertionError naming the
    first differing byte: (segment, shard, unit) inside a shard, or the offset of a guard byte
    (head, gap or tail)."""
    nseg, rows, shard = want_shards.shape
    want = _image(want_shards, stride)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return
    at = int(bad[0])
    off = at - GUARD
    span = _span(nseg, rows, shard, stride)
    if off < 0 or off >= span:
        where = ("guard byte", "head" if off < 0 else "tail", at)
    else:
        seg = off // stride if stride else 0
        within = off - seg * stride
        if within >= rows * shard:
            where = ("guard byte", "gap after segment", seg, at)
        else:
            where = ("segment", seg, "shard", within // shard, "unit", within % shard // 16)
    raise AssertionError((what, "first differing byte", where, "got", int(got[at]), "want", int(want[at]),
                          "differing bytes", int(bad.size)))


def test_checker_reports_a_flipped_byte_and_a_touched_guard():
    """Negative control of the compare step (no GPU): a wrong byte in the last unit of the last
    segment and an altered guard byte each fail, and are named."""
    nseg, rows, shard, stride = 3, 2, 32, 2 * 32 + 48
    good = _rand((nseg, rows, shard), 1)
    got = _image(good, stride)
    _compare(got, good, stride, "control")                      # equal: passes
    flipped = good.copy()
    flipped[nseg - 1, rows - 1, shard - 1] ^= 0x01
    with pytest.raises(AssertionError) as e:
        _compare(got, flipped, stride, "control")
    assert e.value.args[0][2] == ("segment", 2, "shard", 1, "unit", 1) and e.value.args[0][-1] == 1
    for at, name in [(GUARD - 1, "head"), (got.size - GUARD, "tail"), (GUARD + rows * shard, "gap after segment"),
                     (GUARD + stride + rows * shard + 47, "gap after segment")]:
        touched = got.copy()
        touched[at] = 0x00
        with pytest.raises(AssertionError) as e:
            _compare(touched, good, stride, "control")
        assert e.value.args[0][2][0] == "guard byte" and e.value.args[0][2][1] == name, (at, e.value.args[0])
    # a store one unit past the last parity shard of a segment lands in the gap
    touched = got.copy()
    touched[GUARD + rows * shard:GUARD + rows * shard + 16] = 7
    with pytest.raises(AssertionError) as e:
        _compare(touched, good, stride, "control")
    assert e.value.args[0][2] == ("guard byte", "gap after segment", 0, GUARD + rows * shard)


def test_grid_rule_at_256_cus():
    """The shapes below on an MI355X (256 CUs): (gx, gy), (most, fewest) passes per lane, most
    segments per workgroup.  Pure arithmetic over the restated launch rule."""
    def row(units, nseg):
        gx, gy = _rs_grid(256, units, nseg)
        return gx, gy, _passes(units, gx), _ceil_div(nseg, gy)
    assert row(1, 5000) == (1, 2048, (1, 0), 3)
    assert row(517, 2100) == (1, 2048, (3, 2), 2)
    assert row(2 * 8192 + 257, 64) == (32, 64, (3, 2), 1)
    assert row(257, 3) == (2, 3, (1, 0), 1)
    assert row(37, 3) == (1, 3, (1, 0), 1)
    assert row(257, 1) == (2, 1, (1, 0), 1)
    assert row((8 << 20) // 16 + 257, 1) == (2048, 1, (2, 1), 1)
    assert row(300, 1) == (2, 1, (1, 0), 1)


def _check_encode(ctx, oracle_lib, k, m, shard, nseg, data_gap=32, parity_gap=48, seed=0):
    """One dm_rs_encode_device_async call over guarded buffers.  Data rows at
    data_stride = k * shard + data_gap, parity rows at parity_stride = m * shard + parity_gap
    (a gap of None: stride 0, one segment)."""
    torch = _torch()
    from deoss_amd.reedsolomon import New
    if data_gap is None:
        assert nseg == 1
    dstride = 0 if data_gap is None else k * shard + data_gap
    pstride = 0 if parity_gap is None else m * shard + parity_gap
    data = _rand((nseg, k, shard), seed or (k * 1000 + m * 10 + nseg))
    want = _oracle_parity(oracle_lib, data, m)
    dimg = _image(data, dstride)
    ddev = torch.from_numpy(dimg).cuda()
    pdev = torch.full((2 * GUARD + _span(nseg, m, shard, pstride),), FILL, dtype=torch.uint8, device="cuda")
    assert (ddev.data_ptr() + GUARD) % 16 == 0 and (pdev.data_ptr() + GUARD) % 16 == 0
    enc = New(ctx, k, m)
    try:
        enc.encode_device_async(ddev.data_ptr() + GUARD, dstride, pdev.data_ptr() + GUARD, pstride, shard, nseg, 0)
        torch.cuda.synchronize()
    finally:
        enc.close()
    tag = (k, m, shard, nseg, dstride, pstride)
    _compare(pdev.cpu().numpy(), want, pstride, ("parity", tag))
    _compare(ddev.cpu().numpy(), data, dstride, ("data", tag))


# ---- encode shapes ------------------------------------------------------------------------------

@gpu
def test_encode_more_segments_than_grid_rows(ctx, oracle_lib):
    """4 + 8, one unit per shard, 5,000 segments: a workgroup codes segments s, s + gy, s + 2 gy,
    and 255 of its lanes have no unit."""
    nseg, units = 5000, 1
    gx, gy = _rs_grid(_cus(), units, nseg)
    assert gx == 1 and _ceil_div(nseg, gy) >= 3, (gx, gy)
    _check_encode(ctx, oracle_lib, 4, 8, 16 * units, nseg)


@gpu
def test_encode_segment_walk_and_stride_loop(ctx, oracle_lib):
    """4 + 8, 517 units per shard, 2,100 segments: one workgroup per grid row (stride 256 units), so
    lanes 0..4 make three passes and the rest two -- the prefetch guard is taken and not taken in
    the same wave -- and the first nseg - gy workgroups start a second segment."""
    nseg, units = 2100, 517
    gx, gy = _rs_grid(_cus(), units, nseg)
    assert gx == 1 and gy < nseg <= 2 * gy, (gx, gy)
    assert _passes(units, gx) == (3, 2) and units % THREADS == 5
    _check_encode(ctx, oracle_lib, 4, 8, 16 * units, nseg)


@gpu
def test_encode_stride_loop_across_workgroups(ctx, oracle_lib):
    """4 + 8, 2 x 8,192 + 257 units per shard, 64 segments: a grid row of 32 workgroups strides
    8,192 units; the third pass covers 257 lanes: one workgroup and one lane of the next."""
    nseg = 64
    gx0, gy = _rs_grid(_cus(), 1 << 30, nseg)          # gx for a shard long enough to need the loop
    units = 2 * gx0 * THREADS + 257
    gx, gy = _rs_grid(_cus(), units, nseg)
    assert gx == gx0 and gx > 1 and gy == nseg, (gx, gy)
    assert _passes(units, gx) == (3, 2) and units - 2 * gx * THREADS == THREADS + 1
    assert units == 2 * 8192 + 257, ("the shape the issue names, at 256 CUs", units)
    _check_encode(ctx, oracle_lib, 4, 8, 16 * units, nseg)


@gpu
@pytest.mark.parametrize("layout", ["gaps", "contiguous", "stride0"])
def test_encode_257_units(ctx, oracle_lib, layout):
    """257 units per shard: no multiple of the workgroup size, two workgroups per grid row.  With
    gaps between the segments, with the contiguous strides the product uses (k x shard, m x shard),
    and as one segment with both strides 0 (the host path's call)."""
    units = 257
    nseg = 1 if layout == "stride0" else 3
    gx, gy = _rs_grid(_cus(), units, nseg)
    assert (gx, gy) == (2, nseg)
    gaps = {"gaps": (32, 48), "contiguous": (0, 0), "stride0": (None, None)}[layout]
    _check_encode(ctx, oracle_lib, 4, 8, 16 * units, nseg, *gaps)


@gpu
@pytest.mark.parametrize("k", range(1, 9))
def test_encode_every_instance(ctx, oracle_lib, k):
    """All eight template instances (NIN = k) with every nout = m in 1..8, 37 units, 3 segments."""
    units, nseg = 37, 3
    assert _rs_grid(_cus(), units, nseg) == (1, nseg)
    for m in range(1, 9):
        _check_encode(ctx, oracle_lib, k, m, 16 * units, nseg)


# ---- reconstruct shapes -------------------------------------------------------------------------

def _coded_shards(oracle_lib, k, m, shard, seed):
    data = _rand((1, k, shard), seed)
    par = _oracle_parity(oracle_lib, data, m)
    return np.concatenate([data[0], par[0]])        # (k + m, shard)


def _check_reconstruct(ctx, full, k, m, lost_sets):
    """dm_rs_reconstruct_device_async per lost set: every shard in its own guarded allocation, the
    lost ones overwritten with 0x5A; afterwards every shard equals the oracle's and every guard
    byte is intact."""
    torch = _torch()
    from deoss_amd.reedsolomon import New
    total, shard = full.shape
    assert total == k + m
    clean = [torch.from_numpy(_image(full[i].reshape(1, 1, shard), 0)).cuda() for i in range(total)]
    enc = New(ctx, k, m)
    try:
        for lost in lost_sets:
            assert 1 <= len(lost) <= m and all(0 <= i < total for i in lost), lost
            bufs = [c.clone() for c in clean]
            for i in lost:
                bufs[i][GUARD:GUARD + shard] = 0x5A
            ptrs = [b.data_ptr() + GUARD for b in bufs]
            assert all(p % 16 == 0 for p in ptrs)
            enc.reconstruct_device_async(ptrs, [i not in lost for i in range(total)], shard, 0)
            torch.cuda.synchronize()
            for i in range(total):
                _compare(bufs[i].cpu().numpy(), full[i].reshape(1, 1, shard), 0,
                         ("reconstruct", (k, m, shard), "lost", sorted(lost), "buffer of shard", i))
    finally:
        enc.close()


def _lost_sets_4_8():
    """For every count 1..8: data-only (while it fits), parity-only and mixed losses, and from two
    lost on a set with both shard 0 and shard 11 (one lost: each of them alone)."""
    rng = random.Random(48)
    sets = []
    for n in range(1, 9):
        if n <= 4:
            sets.append(rng.sample(range(4), n))
        sets.append(rng.sample(range(4, 12), n))
        if n == 1:
            sets += [[0], [11]]
            continue
        nd = rng.randint(1, min(4, n - 1))
        sets.append(rng.sample(range(4), nd) + rng.sample(range(4, 12), n - nd))
        sets.append([0, 11] + rng.sample(range(1, 11), n - 2))
    return sets


def test_lost_sets_cover_what_they_claim():
    sets = _lost_sets_4_8()
    for n in range(1, 9):
        mine = [set(s) for s in sets if len(s) == n]
        assert all(len(s) == n for s in mine)
        assert any(s <= set(range(4)) for s in mine) == (n <= 4)
        assert any(s <= set(range(4, 12)) for s in mine)
        if n == 1:
            assert {0} in mine and {11} in mine
        else:
            assert any(s & set(range(4)) and s & set(range(4, 12)) for s in mine)
            assert any({0, 11} <= s for s in mine)


@gpu
def test_reconstruct_4_8_every_count(ctx, oracle_lib):
    """4 + 8 at 300 units per shard (two workgroups, the second partly idle): 1 to 8 lost."""
    units = 300
    assert _rs_grid(_cus(), units, 1) == (2, 1)
    full = _coded_shards(oracle_lib, 4, 8, 16 * units, 480)
    _check_reconstruct(ctx, full, 4, 8, _lost_sets_4_8())


@gpu
def test_reconstruct_stride_loop_above_8_mib(ctx, oracle_lib):
    """4 + 8, shard = 8 MiB + 257 units, 8 lost: with one segment the grid row is 8 x CUs workgroups
    wide, so only a shard above that many x 256 units makes a lane take a second pass (257 lanes
    do, with the prefetch)."""
    gx0, _ = _rs_grid(_cus(), 1 << 30, 1)
    units = gx0 * THREADS + 257
    gx, gy = _rs_grid(_cus(), units, 1)
    assert (gx, gy) == (gx0, 1) and _passes(units, gx) == (2, 1)
    assert 16 * units == (8 << 20) + 16 * 257, ("the shape the issue names, at 256 CUs", units)
    full = _coded_shards(oracle_lib, 4, 8, 16 * units, 481)
    _check_reconstruct(ctx, full, 4, 8, [[0, 2, 3, 5, 6, 8, 10, 11]])


@gpu
def test_reconstruct_8_8_high_half_and_narrow_instances(ctx, oracle_lib):
    """8 + 8 with 5, 6, 7 and 8 lost: outputs 4..7 come from the high half of the table entry.
    1 + 8 and 3 + 2: the narrowest instance, and nout < 4 with an odd k."""
    rng = random.Random(88)
    sets = [list(range(8)), list(range(8, 16)), [0, 15, 3, 4, 8, 9, 12, 7]]
    for n in (5, 6, 7, 8):
        nd = rng.randint(1, n - 1)
        sets.append(rng.sample(range(8), nd) + rng.sample(range(8, 16), n - nd))
        sets.append([0, 15] + rng.sample(range(1, 15), n - 2))
    assert {len(s) for s in sets} == {5, 6, 7, 8}
    _check_reconstruct(ctx, _coded_shards(oracle_lib, 8, 8, 16 * 37, 882), 8, 8, sets)
    sets = [[0], [8], [0, 8], [0, 1, 2, 3, 4, 5, 6, 7], [1, 2, 3, 4, 5, 6, 7, 8], [0, 1, 2, 3, 5, 6, 7, 8]]
    _check_reconstruct(ctx, _coded_shards(oracle_lib, 1, 8, 16 * 37, 183), 1, 8, sets)
    sets = [[0], [4], [0, 1], [3, 4], [0, 4], [2, 3], [1, 2]]
    _check_reconstruct(ctx, _coded_shards(oracle_lib, 3, 2, 16 * 37, 324), 3, 2, sets)


# ---- FullProcessing on the device at small segments --------------------------------------------

def _check_process(ctx, oracle_lib, k, m, segment, length, seed):
    """dm_process_device_async (auto leaf kernel) over a guarded object buffer whose last segment's
    padding holds 0xA5, and a guarded parity buffer."""
    torch = _torch()
    from deoss_amd.process import Processor
    total, frag = k + m, segment // k
    nseg = _ceil_div(length, segment)
    assert (nseg - 1) * segment < length <= nseg * segment and segment % (16 * k) == 0
    buf = _rand(length, seed)
    stale = np.full((nseg * segment,), 0xA5, dtype=np.uint8)
    stale[:length] = buf
    odev = torch.from_numpy(_image(stale.reshape(nseg, k, frag), segment)).cuda()
    pdev = torch.full((2 * GUARD + nseg * m * frag,), FILL, dtype=torch.uint8, device="cuda")
    segh = torch.full((2 * GUARD + nseg * 32,), FILL, dtype=torch.uint8, device="cuda")
    fragh = torch.full((2 * GUARD + nseg * total * 32,), FILL, dtype=torch.uint8, device="cuda")
    fid = torch.full((2 * GUARD + 32,), FILL, dtype=torch.uint8, device="cuda")
    p = Processor(ctx, k, m, segment)
    try:
        p.process_device_async(odev.data_ptr() + GUARD, length, pdev.data_ptr() + GUARD, segh.data_ptr() + GUARD,
                               fragh.data_ptr() + GUARD, fid.data_ptr() + GUARD)
        torch.cuda.synchronize()
    finally:
        p.close()
    want_seg, want_frag, want_fid, raw = oracle_lib.full_processing(buf.tobytes(), segment, k, m, want_frags=True,
                                                                   nthreads=8)
    frags = np.frombuffer(raw, dtype=np.uint8).reshape(nseg, total, frag)
    tag = (k, m, segment, length)
    padded = np.zeros((nseg * segment,), dtype=np.uint8)
    padded[:length] = buf
    assert np.array_equal(frags[:, :k, :].reshape(-1), padded)      # the oracle's data fragments are the object
    _compare(odev.cpu().numpy(), padded.reshape(nseg, k, frag), segment, ("object, padding zeroed", tag))
    _compare(pdev.cpu().numpy(), np.ascontiguousarray(frags[:, k:, :]), m * frag, ("parity", tag))
    for name, dev, want in (("segment hashes", segh, want_seg), ("fragment hashes", fragh, want_frag),
                            ("fid", fid, want_fid)):
        w = np.frombuffer(want, dtype=np.uint8)
        _compare(dev.cpu().numpy(), w.reshape(1, 1, w.size), 0, (name, tag))


@gpu
def test_process_device_5000_segments_of_64_bytes(ctx, oracle_lib):
    """segment = 64 (one unit per fragment), 5,000 segments, ragged: the coding kernel's workgroups
    walk three segments under FullProcessing's strides."""
    nseg = 5000
    gx, gy = _rs_grid(_cus(), 1, nseg)
    assert gx == 1 and _ceil_div(nseg, gy) >= 3, (gx, gy)
    _check_process(ctx, oracle_lib, 4, 8, 64, nseg * 64 - 21, 5064)


@gpu
def test_process_device_2100_segments_stride_loop(ctx, oracle_lib):
    """segment = 4 x 16 x 517, 2,100 segments, ragged: segment walk and stride loop together."""
    nseg, units = 2100, 517
    gx, gy = _rs_grid(_cus(), units, nseg)
    assert gx == 1 and gy < nseg and _passes(units, gx) == (3, 2), (gx, gy)
    segment = 4 * 16 * units
    _check_process(ctx, oracle_lib, 4, 8, segment, nseg * segment - segment // 3 - 5, 2100)


@gpu
def test_process_device_2_3(ctx, oracle_lib):
    """2 + 3, segment = 2 x 16 x 5, 7 segments, ragged."""
    assert _rs_grid(_cus(), 5, 7) == (1, 7)
    _check_process(ctx, oracle_lib, 2, 3, 2 * 16 * 5, 7 * 160 - 33, 23)
