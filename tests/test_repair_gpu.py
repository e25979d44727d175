"""GPU checks of the repair path (the storage side): rs_repair_kernel and the choice between it and
rs_restore_kernel through dm_rs_repair_device_async, dm_repair_buffer and dm_repair_files.

Every comparison is bit-exact.  The reference is never the code under test: fragments and names come
from oracle/ (process_oracle.c / rs_oracle.c through oracle.Oracle, cross-checked against the
pure-Python restatement in tests/test_restore_plan.py), and a repaired fragment must equal the
oracle's fragment of the same (segment, index).
"""
from __future__ import annotations

import ctypes
import itertools
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ABSENT, USED, SPARE, BAD, REBUILT = 0, 1, 2, 3, 4
FILL = 0xA5


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


class Coded:
    """An object and what FullProcessing makes of it, from the CPU oracle."""

    def __init__(self, oracle_lib, buf, segment, k, m):
        self.buf, self.segment, self.k, self.m, self.total = buf, segment, k, m, k + m
        self.frag = segment // k
        self.nseg = (len(buf) + segment - 1) // segment
        self.segd, self.fragd, self.fid, raw = oracle_lib.full_processing(buf, segment, k, m, want_frags=True)
        self.raw = raw                                    # nseg x total x frag
        f = self.frag
        self.frags = [[raw[(s * self.total + j) * f:(s * self.total + j + 1) * f] for j in range(self.total)]
                      for s in range(self.nseg)]

    def name(self, s, j):
        return self.fragd[32 * (s * self.total + j):32 * (s * self.total + j + 1)]


# ---- kernels through dm_rs_repair_device_async ------------------------------------------------

def _device_repair(ctx, oracle_lib, k, m, frag, present, want, seed):
    """Repair len(present) segments on the device.  present[s]: the fragment indices held;
    want[s]: the indices wanted (None: every missing one).  Every slot that is not held starts as
    0xA5.  Asserts: every wanted fragment equals the oracle's, every held one is unchanged, every
    slot that is neither is untouched."""
    torch = _torch()
    from deoss_amd.reedsolomon import New
    nseg, total, segment = len(present), k + m, k * frag
    size = nseg * segment - (segment // 3 if segment > 3 else 0)   # the last segment is zero-padded
    c = Coded(oracle_lib, _bytes(size, seed), segment, k, m)
    pres = np.zeros((nseg, total), dtype=bool)
    tgt = np.zeros((nseg, total), dtype=bool)
    for s in range(nseg):
        pres[s, present[s]] = True
        if want is None or want[s] is None:
            tgt[s] = ~pres[s]
        else:
            tgt[s, want[s]] = True
            tgt[s] &= ~pres[s]
    truth = torch.frombuffer(bytearray(c.raw), dtype=torch.uint8).cuda().view(nseg, total, frag)
    pres_t, tgt_t = torch.from_numpy(pres).cuda(), torch.from_numpy(tgt).cuda()
    work = torch.full((nseg, total, frag), FILL, dtype=torch.uint8, device="cuda")
    work[pres_t] = truth[pres_t]
    expect = work.clone()
    expect[tgt_t] = truth[tgt_t]
    base = work.data_ptr()
    given = (pres | tgt).reshape(-1)
    ptrs = [base + i * frag if given[i] else 0 for i in range(nseg * total)]
    enc = New(ctx, k, m)
    try:
        enc.repair_device_async(ptrs, pres.reshape(-1).tolist(), nseg, frag, 0)
        torch.cuda.synchronize()
    finally:
        enc.close()
    bad = torch.nonzero((work != expect).reshape(-1))
    assert bad.numel() == 0, ("first differing byte", int(bad[0]), "segment", int(bad[0]) // (total * frag),
                              "fragment", int(bad[0]) // frag % total)
    return tgt


def _mixed_5000(rng, narrow_only):
    """5,000 patterns: every fifth complete (nout 0), the others missing 1-4 and -- unless
    narrow_only -- 5-8 in turn, so consecutive segments of a workgroup differ in table width."""
    pats = []
    for s in range(5000):
        if s % 5 == 2:
            nmiss = 0
        elif narrow_only or s % 2 == 0:
            nmiss = rng.randint(1, 4)
        else:
            nmiss = rng.randint(5, 8)
        pats.append(sorted(rng.sample(range(12), 12 - nmiss)))
    return pats


def test_kernel_5000_tiny_segments_narrow_and_wide_tables_alternating(ctx, oracle_lib):
    """One 16-byte unit per fragment, 5,000 segments: more segments than grid rows, so one
    workgroup walks segments with nout 0, nout <= 4 and nout > 4 in turn (the wide kernel runs)."""
    pats = _mixed_5000(random.Random(5001), narrow_only=False)
    tgt = _device_repair(ctx, oracle_lib, 4, 8, 16, pats, None, 21)
    nout = tgt.sum(axis=1)
    assert (nout == 0).sum() == 1000 and (nout > 4).sum() > 1500 and ((nout > 0) & (nout <= 4)).sum() > 1500


def test_kernel_5000_tiny_segments_at_most_four_missing(ctx, oracle_lib):
    """The same shape with at most 4 missing everywhere: the restore kernel is the one launched,
    also for missing parity fragments."""
    pats = _mixed_5000(random.Random(5002), narrow_only=True)
    tgt = _device_repair(ctx, oracle_lib, 4, 8, 16, pats, None, 22)
    assert tgt.sum(axis=1).max() == 4 and tgt[:, 4:].any()


def test_kernel_all_495_patterns_eight_outputs_each(ctx, oracle_lib):
    pats = [list(p) for p in itertools.combinations(range(12), 4)]
    assert len(pats) == 495
    tgt = _device_repair(ctx, oracle_lib, 4, 8, 4096, pats, None, 23)
    assert (tgt.sum(axis=1) == 8).all()


def test_kernel_257_units_per_fragment(ctx, oracle_lib):
    """257 units per fragment: no multiple of the 256 threads; wide and narrow segments."""
    pats = [[1, 5, 6, 11], [0, 2, 9, 10, 11], [3, 4, 7, 8], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]]
    _device_repair(ctx, oracle_lib, 4, 8, 16 * 257, pats, None, 24)


def test_kernel_stride_loop_and_prefetch(ctx, oracle_lib):
    """Fragments of 160 KiB, 64 segments: 10,240 units per fragment against the 8,192 one grid row
    covers, so the stride loop and its prefetch run, with 1-8 missing per segment."""
    rng = random.Random(64)
    pats = [sorted(rng.sample(range(12), rng.randint(4, 11))) for _ in range(64)]
    _device_repair(ctx, oracle_lib, 4, 8, 160 * 1024, pats, None, 25)


def test_kernel_8_8_1_8_and_3_2(ctx, oracle_lib):
    """8 + 8 with 8 missing in seeded data / parity mixes (nout == k: the restore kernel, high half
    of the table); 1 + 8 and 3 + 2 (nout > k: the wide kernel with fewer than 4 inputs)."""
    rng = random.Random(88)
    pats = [sorted(rng.sample(range(16), 8)) for _ in range(24)]
    _device_repair(ctx, oracle_lib, 8, 8, 16 * 37, pats, None, 26)
    pats = [[j] for j in range(9)] + [[0, 3], [2, 8], list(range(9))]
    _device_repair(ctx, oracle_lib, 1, 8, 16 * 300, pats, None, 27)
    _device_repair(ctx, oracle_lib, 3, 2, 16 * 5, [[0, 1, 2], [2, 3, 4], [0, 3, 4], [1, 2, 4], [0, 1, 2, 3]], None, 28)


def test_kernel_want_subsets(ctx, oracle_lib):
    """Only parity wanted, one fragment wanted, a wanted fragment that is held (not written), and
    nothing wanted at all (nothing is launched)."""
    pats = [[0, 1, 2, 3], [1, 2, 3, 4, 5], [4, 5, 6, 7], [0, 5, 6, 11]]
    want = [list(range(4, 12)), [0], [0, 1, 2, 3, 4, 8], [11, 1]]
    tgt = _device_repair(ctx, oracle_lib, 4, 8, 16 * 33, pats, want, 29)
    assert tgt.sum(axis=1).tolist() == [8, 1, 5, 1]
    tgt = _device_repair(ctx, oracle_lib, 4, 8, 16 * 33, pats, [[], [], [4], [0, 5]], 29)
    assert not tgt.any()


def _mixed_missing(rng, k, counts):
    """Per count n the held fragments of a k + 8 segment that misses n, data and parity mixed (a
    single missing one is either)."""
    pats = []
    for n in counts:
        nd = rng.randint(max(1, n - 8), min(k, n - 1)) if n >= 2 else rng.randint(0, min(n, 1))
        gone = set(rng.sample(range(k), nd)) | set(rng.sample(range(k, k + 8), n - nd))
        pats.append(sorted(set(range(k + 8)) - gone))
    return pats


@pytest.mark.parametrize("k,call", [(k, "restore_kernel") for k in range(1, 9)] +
                         [(k, "repair_kernel") for k in range(1, 8)])
def test_kernel_every_instance(ctx, oracle_lib, k, call):
    """Every rs_restore_kernel<k> and rs_repair_kernel<k>, k + 8, at 257 units per fragment: two
    workgroups in x, the second with one live lane, so the prefetch guard and the loop bound are at
    their edge.  Seven segments, one of them complete (nout 0).
    restore_kernel: 1 .. k missing everywhere, so no segment has more outputs than inputs and
    rs_restore_kernel<k> runs; one segment has nout == k, the last store its bound lets through, and
    from k = 5 on segments on both sides of nout > 4 (with and without the entries' high half).
    repair_kernel: one segment missing k + 1 and one missing 8 next to segments missing 1 .. 4, so
    rs_repair_kernel<k> runs and takes both sides of its nout > 4 branch in one launch.  There is
    no such case for k = 8: of 8 + 8 fragments at most 8 can be missing, never more than k, so
    rs_repair_kernel<8> is unreachable."""
    rng = random.Random(800 + k)
    if call == "restore_kernel":
        counts = [k, 1, max(1, k // 2), min(k, 4), max(1, k - 1), 0, min(k, 3)]
    else:
        counts = [1, k + 1, 3, 0, 8, 2, 4]
    tgt = _device_repair(ctx, oracle_lib, k, 8, 16 * 257, _mixed_missing(rng, k, counts), None, 30 + k)
    nout = tgt.sum(axis=1).tolist()
    assert nout == counts
    assert tgt[:, :k].any() and tgt[:, k:].any()
    if call == "restore_kernel":
        assert max(nout) == k and min(nout) == 0
        assert k < 5 or (max(nout) > 4 and any(0 < n <= 4 for n in nout))
    else:
        assert k + 1 in nout and 8 in nout and any(0 < n <= 4 for n in nout)


def test_device_repair_too_few_fails_before_any_launch(ctx):
    torch = _torch()
    from deoss_amd import DeossMerkleError
    from deoss_amd.reedsolomon import ErrTooFewShards, New
    enc = New(ctx, 4, 8)
    pool = torch.full((2 * 12 * 16,), FILL, dtype=torch.uint8, device="cuda")
    ptrs = [pool.data_ptr() + 16 * i for i in range(24)]
    present = [1, 1, 1, 1] + [0] * 8 + [0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1]   # segment 1 keeps 3 of 12
    with pytest.raises(ErrTooFewShards):
        enc.repair_device_async(ptrs, present, 2, 16, 0)
    torch.cuda.synchronize()
    assert bool((pool == FILL).all())              # segment 0 was not repaired either
    with pytest.raises(DeossMerkleError):          # unaligned fragment
        enc.repair_device_async([p + 1 for p in ptrs[:12]], present[:12], 1, 16, 0)
    with pytest.raises(DeossMerkleError):          # fragment size no multiple of 16
        enc.repair_device_async(ptrs[:12], present[:12], 1, 24, 0)
    with pytest.raises(DeossMerkleError):
        enc.repair_device_async(ptrs[:12], present[:12], 1, 0, 0)
    enc.close()


# ---- dm_repair_buffer -------------------------------------------------------------------------

SEG = 4096


@pytest.fixture(scope="module")
def proc(ctx):
    from deoss_amd.process import Processor
    p = Processor(ctx, 4, 8, SEG)
    yield p
    p.close()


_CODED = {}


def _coded(oracle_lib, size):
    """The object of `size` bytes at SEG / 4 + 8, computed once and left unchanged."""
    if size not in _CODED:
        _CODED[size] = Coded(oracle_lib, _bytes(size, size), SEG, 4, 8)
    return _CODED[size]


def _flip(b, at=None):
    at = len(b) // 2 if at is None else at
    return b[:at] + bytes([b[at] ^ 0x40]) + b[at + 1:]


def _outs(c, frag=None):
    f = frag or c.frag
    return [ctypes.create_string_buffer(bytes([FILL]) * f, f) for _ in range(c.nseg * c.total)]


def _delete(c, rng, lo=1, hi=8):
    kept = [sorted(rng.sample(range(c.total), c.total - rng.randint(lo, hi))) for _ in range(c.nseg)]
    return [[c.frags[s][j] if j in kept[s] else None for j in range(c.total)] for s in range(c.nseg)], kept


def _assert_outs(c, outs, fst):
    """A delivered fragment (status 4) is the oracle's; every other out buffer is untouched."""
    for i, o in enumerate(outs):
        s, j = divmod(i, c.total)
        if fst[i] == REBUILT:
            assert o.raw == c.frags[s][j], (s, j)
        else:
            assert o.raw == bytes([FILL]) * c.frag, (s, j, fst[i])


@pytest.mark.parametrize("size", [1, SEG - 1, SEG, SEG + 17, 9 * SEG + 12345])
def test_repair_buffer(ctx, proc, oracle_lib, size):
    rng = random.Random(size)
    c = _coded(oracle_lib, size)
    total = c.total
    # 1-8 of 12 deleted: every one comes back, the first four kept are the inputs; one repair
    # launch and one leaf launch (one timing record per round)
    frags, kept = _delete(c, rng)
    outs = _outs(c)
    ctx.set_timing(True)
    try:
        ok, got, fst, sst = proc.repair_buffer(frags, c.fragd, out=outs)
        rounds = ctx.timing_summary()[0]
    finally:
        ctx.set_timing(False)
    assert ok and sst == bytes(c.nseg) and rounds == 1
    for s in range(c.nseg):
        want = [REBUILT] * total
        for n, j in enumerate(kept[s]):
            want[j] = USED if n < 4 else ABSENT           # a kept fragment beyond the inputs is not read
        assert list(fst[s * total:(s + 1) * total]) == want
        for j in range(total):
            if j not in kept[s]:
                assert got[s * total + j] == c.frags[s][j]
    _assert_outs(c, outs, fst)
    # a corrupted input (one flipped bit) is bad, the next candidate is used, the result is exact
    frags, kept = _delete(c, rng, 1, 7)
    hit = []
    for s in range(c.nseg):
        j = kept[s][rng.randrange(4)]
        frags[s][j] = _flip(frags[s][j], rng.randrange(c.frag))
        hit.append(j)
    outs = _outs(c)
    ctx.set_timing(True)
    try:
        ok, got, fst, sst = proc.repair_buffer(frags, c.fragd, out=outs)
        rounds = ctx.timing_summary()[0]
    finally:
        ctx.set_timing(False)
    assert ok and sst == bytes(c.nseg) and rounds == 2
    for s in range(c.nseg):
        row = list(fst[s * total:(s + 1) * total])
        assert row[hit[s]] == BAD                           # not wanted: it stays bad
        assert [j for j in range(total) if row[j] == USED] == [j for j in kept[s] if j != hit[s]][:4]
        assert all(row[j] == REBUILT for j in range(total) if j not in kept[s])
    _assert_outs(c, outs, fst)
    # a corrupted input and only 4 present: too few, that segment's out untouched, the others delivered
    frags, kept = _delete(c, rng, 8, 8)
    s_bad = rng.randrange(c.nseg)
    j_bad = kept[s_bad][2]
    frags[s_bad][j_bad] = _flip(frags[s_bad][j_bad])
    outs = _outs(c)
    ok, got, fst, sst = proc.repair_buffer(frags, c.fragd, out=outs)
    assert not ok and list(sst) == [1 if s == s_bad else 0 for s in range(c.nseg)]
    assert sorted(fst[s_bad * total:(s_bad + 1) * total]) == [ABSENT] * 8 + [SPARE] * 3 + [BAD]
    for s in range(c.nseg):
        if s != s_bad:
            assert list(fst[s * total:(s + 1) * total]).count(REBUILT) == 8
    _assert_outs(c, outs, fst)
    # a wrong name for a wanted fragment: every input verifies, that output does not -> mismatch,
    # not delivered; the segment's other outputs prove themselves and are
    frags, kept = _delete(c, rng, 2, 8)
    s_bad = rng.randrange(c.nseg)
    j_bad = next(j for j in range(total) if j not in kept[s_bad])
    names = bytearray(c.fragd)
    names[32 * (s_bad * total + j_bad) + 5] ^= 1
    outs = _outs(c)
    ok, got, fst, sst = proc.repair_buffer(frags, bytes(names), out=outs)
    assert not ok and list(sst) == [2 if s == s_bad else 0 for s in range(c.nseg)]
    assert fst[s_bad * total + j_bad] == ABSENT and got[s_bad * total + j_bad] is None
    assert list(fst).count(REBUILT) == sum(total - len(kp) for kp in kept) - 1
    _assert_outs(c, outs, fst)
    # a corrupted present fragment with out set is rebuilt (3 -> 4), wherever it stands
    frags, kept = _delete(c, rng, 1, 7)
    hit = []
    for s in range(c.nseg):
        j = rng.choice(kept[s])
        frags[s][j] = _flip(frags[s][j], 0)
        hit.append(j)
    want = [[frags[s][j] is None or j == hit[s] for j in range(total)] for s in range(c.nseg)]
    outs = _outs(c)
    ok, got, fst, sst = proc.repair_buffer(frags, c.fragd, want=want, out=outs)
    assert ok and sst == bytes(c.nseg)
    for s in range(c.nseg):
        assert fst[s * total + hit[s]] == REBUILT and got[s * total + hit[s]] == c.frags[s][hit[s]]
        assert all(fst[s * total + j] == REBUILT for j in range(total) if j not in kept[s])
    _assert_outs(c, outs, fst)
    # a good present fragment with out set is checked and left alone; nothing missing elsewhere
    frags = [list(f) for f in c.frags]
    want = [[j == 9 for j in range(total)] for _ in range(c.nseg)]
    outs = _outs(c)
    ok, got, fst, sst = proc.repair_buffer(frags, c.fragd, want=want, out=outs)
    assert ok and all(g is None for g in got) and list(fst).count(REBUILT) == 0
    _assert_outs(c, outs, fst)


def test_repair_buffer_argument_errors(proc, oracle_lib):
    from deoss_amd import DeossMerkleError
    c = _coded(oracle_lib, SEG + 17)
    with pytest.raises(DeossMerkleError) as e:   # nseg == 0
        proc.repair_buffer([], b"")
    assert e.value.code == -1
    L = proc.ctx._L
    ok = ctypes.c_int(7)
    ptrs = (ctypes.c_void_p * 24)()
    assert L.dm_repair_buffer(proc.enc._h, ptrs, ptrs, None, 2, SEG, None, None, ctypes.byref(ok)) == -2
    assert ok.value == 0
    assert L.dm_repair_buffer(proc.enc._h, ptrs, ptrs, c.fragd, 2, SEG + 16, None, None, ctypes.byref(ok)) == -2
    # nothing given and nothing wanted: nothing to do
    assert L.dm_repair_buffer(proc.enc._h, ptrs, ptrs, c.fragd, 2, SEG, None, None, ctypes.byref(ok)) == 0
    assert ok.value == 1
    # wanted, and nothing to rebuild it from: a result, not an error
    outs = _outs(c)
    ok_, got, fst, sst = proc.repair_buffer([None] * 24, c.fragd, out=outs)
    assert not ok_ and list(sst) == [1, 1] and fst == bytes(24)
    _assert_outs(c, outs, fst)


@pytest.mark.parametrize("mode", ["auto", "wide", "latency", "pair", "quad"])
def test_repair_full_size_segment_under_every_leaf_kernel(ctx, oracle_lib, mode):
    """One 32 MiB segment, 4 + 8 (chain.SegmentSize / DataShards / ParShards), 3 fragments missing,
    one of them parity: 8 MiB chains for the inputs and the outputs in one leaf launch."""
    from deoss_amd.process import Processor
    seg = 32 << 20
    if "full" not in _CODED:
        _CODED["full"] = Coded(oracle_lib, _bytes(seg - 777, 32), seg, 4, 8)
    c = _CODED["full"]
    frags = [[None if j in (1, 3, 6) else c.frags[0][j] for j in range(12)]]
    p = Processor(ctx)
    ctx.set_leaf_kernel(mode)
    try:
        ok, got, fst, sst = p.repair_buffer(frags, c.fragd)
    finally:
        ctx.set_leaf_kernel("auto")
        p.close()
    assert ok and sst == bytes(1)
    assert list(fst) == [USED, REBUILT, USED, REBUILT, USED, USED, REBUILT, 0, 0, 0, 0, 0]
    for j in (1, 3, 6):
        assert got[j] == c.frags[0][j]


def test_repair_buffer_fuzz_100_cases(ctx, oracle_lib):
    """Seeded shapes 4 + 8 / 8 + 8 / 3 + 2 with tiny segments, random deletions, corruptions and
    want sets, each against the oracle's fragments and the status rules."""
    from deoss_amd.process import Processor
    rng = random.Random(0xF022)
    procs, coded = {}, {}
    try:
        for case in range(100):
            k, m = rng.choice([(4, 8), (8, 8), (3, 2)])
            segment = k * 16 * rng.choice([1, 2, 5])
            nseg = rng.randint(1, 6)
            key = (k, m, segment, nseg)
            if key not in coded:
                size = nseg * segment - rng.randrange(segment)
                coded[key] = Coded(oracle_lib, _bytes(size, case), segment, k, m)
                procs.setdefault((k, m, segment), Processor(ctx, k, m, segment))
            c, p, total = coded[key], procs[(k, m, segment)], k + m
            frags = [list(f) for f in c.frags]
            want = [[False] * total for _ in range(nseg)]
            state = [["good"] * total for _ in range(nseg)]
            for s in range(nseg):
                for j in range(total):
                    r = rng.random()
                    if r < 0.35:
                        frags[s][j], state[s][j] = None, "missing"
                    elif r < 0.5:
                        frags[s][j], state[s][j] = _flip(frags[s][j], rng.randrange(c.frag)), "corrupt"
                    want[s][j] = rng.random() < (0.8 if state[s][j] != "good" else 0.3)
            outs = _outs(c)
            ok, got, fst, sst = p.repair_buffer(frags, c.fragd, want=want, out=outs)
            _assert_outs(c, outs, fst)
            all_ok = True
            for s in range(nseg):
                row = list(fst[s * total:(s + 1) * total])
                ngood = sum(1 for j in range(total) if state[s][j] == "good")
                looked = sum(1 for j in range(total) if state[s][j] != "missing") >= k   # else nothing is even loaded
                needs = any(want[s][j] for j in range(total))       # missing and wanted, or given and checked
                for j in range(total):
                    if state[s][j] == "missing":
                        assert row[j] in (ABSENT, REBUILT), (case, s, j, row)
                        assert (row[j] == REBUILT) == (want[s][j] and ngood >= k), (case, s, j, row, state[s])
                    elif state[s][j] == "good":
                        assert row[j] in (ABSENT, USED, SPARE), (case, s, j, row)
                        if want[s][j]:
                            assert row[j] in ((USED, SPARE) if looked else (ABSENT,))   # checked
                    else:
                        if want[s][j]:                               # checked: bad, rebuilt when possible
                            assert row[j] == (REBUILT if ngood >= k else BAD if looked else ABSENT), (case, s, j, row, state[s])
                        else:
                            assert row[j] in (ABSENT, BAD), (case, s, j, row)
                    if want[s][j] and state[s][j] != "good" and row[j] != REBUILT:
                        all_ok = False
                if not needs:
                    assert row == [ABSENT] * total and sst[s] == 0
                elif ngood >= k:
                    assert sst[s] == 0 and row.count(USED) == k, (case, s, row, state[s])
                    used = [j for j in range(total) if row[j] == USED]
                    assert used == [j for j in range(total) if state[s][j] == "good"][:k]
                else:
                    assert sst[s] == 1 and row.count(USED) == 0 and row.count(REBUILT) == 0
                    assert looked or row == [ABSENT] * total
            assert ok == all_ok, (case, list(fst), list(sst))
    finally:
        for p in procs.values():
            p.close()


# ---- dm_repair_files --------------------------------------------------------------------------

FSEG = 16384
FFRAG = FSEG // 4


@pytest.fixture(scope="module")
def stored(ctx, tmp_path_factory):
    """A 10-segment object run through full_processing_file into a directory of fragment files, and a
    pristine copy of every file's bytes (the last segment is mostly padding: its data fragments 1-3
    are all zero and share one name and one file)."""
    from deoss_amd.process import Processor
    d = tmp_path_factory.mktemp("repair")
    size = 9 * FSEG + 2345
    buf = _bytes(size, 99)
    src = d / "object"
    src.write_bytes(buf)
    p = Processor(ctx, 4, 8, FSEG)
    segd, fragd, fid = p.full_processing_file(str(src), str(d / "frags"), segment_files=False)
    pristine = {n: (d / "frags" / n).read_bytes() for n in os.listdir(d / "frags")}
    yield p, buf, segd, fragd, fid, pristine
    p.close()


def _name(fragd, s, j):
    return fragd[32 * (12 * s + j):32 * (12 * s + j + 1)].hex()


def _fresh_dir(stored, tmp_path, sub="have"):
    fd = tmp_path / sub
    fd.mkdir()
    for n, b in stored[5].items():
        (fd / n).write_bytes(b)
    return fd


def _assert_whole(stored, fd):
    """Every name exists with the original bytes and nothing else is in the directory."""
    pristine = stored[5]
    assert sorted(os.listdir(fd)) == sorted(pristine)
    for n, b in pristine.items():
        assert (fd / n).read_bytes() == b, n


def test_repair_files_deleted_and_truncated(stored, tmp_path):
    p, buf, segd, fragd, fid, pristine = stored
    fd = _fresh_dir(stored, tmp_path)
    rng = random.Random(10)
    gone = set()
    for s in range(9):                                      # segment 9 is the padded one (its own test)
        pool = range(1, 12) if s == 4 else range(12)        # fragment 0 of segment 4 is the truncated one
        for j in rng.sample(pool, rng.randint(0, 7 if s == 4 else 8)):
            gone.add(_name(fragd, s, j))
    for n in gone:
        os.unlink(fd / n)
    short = _name(fragd, 4, 0)                              # a truncated file is replaced
    (fd / short).write_bytes(pristine[short][:-1])
    before = {n: (os.stat(fd / n).st_ino, os.stat(fd / n).st_mtime_ns) for n in os.listdir(fd) if n != short}
    ok, n, fst, sst = p.repair_files(str(fd), fragd)
    assert ok and sst == bytes(10) and n == len(gone) + 1
    _assert_whole(stored, fd)
    for name, (ino, mtime) in before.items():               # untouched files are not rewritten
        st = os.stat(fd / name)
        assert (st.st_ino, st.st_mtime_ns) == (ino, mtime), name
    for s in range(10):
        row = list(fst[12 * s:12 * s + 12])
        lost = [j for j in range(12) if _name(fragd, s, j) in gone or _name(fragd, s, j) == short]
        if not lost:
            assert row == [ABSENT] * 12                     # a whole segment is not read at all
            continue
        assert [j for j in range(12) if row[j] == REBUILT] == lost
        assert [j for j in range(12) if row[j] == USED] == [j for j in range(12) if j not in lost][:4]
        assert row.count(ABSENT) == 12 - 4 - len(lost)      # an existing file that is no input is not read
    # a second call finds nothing to do
    ok, n, fst, sst = p.repair_files(str(fd), fragd)
    assert ok and n == 0 and fst == bytes(120)


def test_repair_files_segment_with_three_files_left(stored, tmp_path):
    p, buf, segd, fragd, fid, pristine = stored
    fd = _fresh_dir(stored, tmp_path)
    for s, js in ((2, range(3, 12)), (5, (0, 7)), (7, (11,))):
        for j in js:
            os.unlink(fd / _name(fragd, s, j))
    ok, n, fst, sst = p.repair_files(str(fd), fragd)
    assert not ok and list(sst) == [1 if s == 2 else 0 for s in range(10)] and n == 3
    assert list(fst[24:36]) == [ABSENT] * 12
    left = set(os.listdir(fd))
    assert left == set(pristine) - {_name(fragd, 2, j) for j in range(3, 12)}   # the others repaired, no temporary
    for name in left:
        assert (fd / name).read_bytes() == pristine[name]
    from deoss_amd.process import SegmentDataInfo
    info = [SegmentDataInfo(segd[32 * s:32 * s + 32].hex(), [_name(fragd, s, j) for j in range(12)]) for s in range(10)]
    n, err = p.RepairFragments(str(fd), info)
    assert n == 0 and err is not None and "segment(s) 2" in str(err)


def test_repair_files_three_windows_and_slot_reuse(stored, tmp_path, monkeypatch):
    """Windows of 24 fragments (loaded + rebuilt) and slots of 3 fragments: every segment loses
    files, several lose an input's replacement candidate too (a corrupt first input: reloads)."""
    p, buf, segd, fragd, fid, pristine = stored
    fd = _fresh_dir(stored, tmp_path)
    rng = random.Random(3)
    gone = set()
    for s in range(9):
        for j in rng.sample(range(4, 12), 4):
            gone.add(_name(fragd, s, j))
    for n in gone:
        os.unlink(fd / n)
    bad = [_name(fragd, s, 0) for s in (1, 6)]               # an input that fails its name
    for n in bad:
        (fd / n).write_bytes(_flip(pristine[n]))
    monkeypatch.setenv("DEOSS_REPAIR_WINDOW_BYTES", str(24 * FFRAG))   # 3 segments of 4 + 4 per window
    monkeypatch.setenv("DEOSS_FP_SLOT_BYTES", str(3 * FFRAG))
    ok, n, fst, sst = p.repair_files(str(fd), fragd)
    assert ok and sst == bytes(10) and n == len(gone) + len(bad)
    _assert_whole(stored, fd)
    for s in (1, 6):
        row = list(fst[12 * s:12 * s + 12])
        assert row[0] == REBUILT and row.count(USED) == 4 and row.count(REBUILT) == 5


def test_repair_files_scrub(stored, tmp_path):
    p, buf, segd, fragd, fid, pristine = stored
    fd = _fresh_dir(stored, tmp_path)
    rot = _name(fragd, 3, 10)                                # no plan reads it: segment 3 is whole
    (fd / rot).write_bytes(_flip(pristine[rot], 17))
    os.unlink(fd / _name(fragd, 5, 1))
    ok, n, fst, sst = p.repair_files(str(fd), fragd)         # without the flag it is left as it is
    assert ok and n == 1 and (fd / rot).read_bytes() != pristine[rot]
    assert list(fst[36:48]) == [ABSENT] * 12
    ok, n, fst, sst = p.repair_files(str(fd), fragd, scrub=True)
    assert ok and n == 1 and sst == bytes(10)
    _assert_whole(stored, fd)
    assert list(fst[36:48]) == [USED] * 4 + [SPARE] * 6 + [REBUILT, SPARE]
    assert fst.count(BAD) == 0 and fst.count(REBUILT) == 1 and fst.count(ABSENT) == 0


def test_repair_files_equal_names_in_the_padded_segment(stored, tmp_path):
    p, buf, segd, fragd, fid, pristine = stored
    zero = _name(fragd, 9, 1)
    assert zero == _name(fragd, 9, 2) == _name(fragd, 9, 3) and pristine[zero] == bytes(FFRAG)
    fd = _fresh_dir(stored, tmp_path)
    os.unlink(fd / zero)
    os.unlink(fd / _name(fragd, 9, 8))
    ok, n, fst, sst = p.repair_files(str(fd), fragd)
    assert ok and n == 2                                     # one file for the three owners, one for parity 8
    assert list(fst[108:120]) == [USED, REBUILT, REBUILT, REBUILT, USED, USED, USED, ABSENT, REBUILT, 0, 0, 0]
    _assert_whole(stored, fd)
    # the file there: it serves all three owners as an input
    for j in (0, 4, 5):
        os.unlink(fd / _name(fragd, 9, j))
    ok, n, fst, sst = p.repair_files(str(fd), fragd)
    assert ok and n == 3
    assert list(fst[108:120]) == [REBUILT, USED, USED, USED, REBUILT, REBUILT, USED, 0, 0, 0, 0, 0]
    _assert_whole(stored, fd)


def test_round_trip_with_the_mirrors(ctx, tmp_path):
    """FullProcessing -> delete -> RepairFragments -> RestoreFile gives the object back."""
    from deoss_amd.process import Processor
    p = Processor(ctx, 4, 8, FSEG)
    try:
        buf = _bytes(3 * FSEG + 99, 5)
        src = tmp_path / "object"
        src.write_bytes(buf)
        info, fid, err = p.FullProcessing(str(src), "", str(tmp_path / "frags"))
        assert err is None and len(info) == 4
        rng = random.Random(5)
        lost = {info[s].FragmentHash[j] for s in range(4) for j in rng.sample(range(12), 5)}
        for path in lost:
            os.unlink(path)
        n, err = p.RepairFragments(str(tmp_path / "frags"), info)
        assert err is None and n == len(lost)
        assert all(os.path.getsize(f) == FFRAG for s in info for f in s.FragmentHash)
        for s in range(3):                                   # restore from rebuilt files: the survivors go
            for f in info[s].FragmentHash:
                if f not in lost:
                    os.unlink(f)
        ok, err = p.RestoreFile(str(tmp_path / "frags"), info, len(buf), str(tmp_path / "back"))
        assert ok and err is None and (tmp_path / "back").read_bytes() == buf
    finally:
        p.close()
