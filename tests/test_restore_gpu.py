"""GPU checks of the restore path (the download side): rs_restore_kernel through
dm_rs_restore_device_async, dm_restore_buffer and dm_retrieve_file.

Every comparison is bit-exact.  The reference is never the code under test: it is the original
object bytes, and oracle/ (process_oracle.c / rs_oracle.c through oracle.Oracle, cross-checked
against the pure-Python restatement in tests/test_restore_plan.py) makes the fragments and names.
"""
from __future__ import annotations

import ctypes
import itertools
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VF, VS, VID, VALL = 1, 2, 4, 7   # DM_RESTORE_VERIFY_*
ABSENT, USED, SPARE, BAD = 0, 1, 2, 3


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
        self.padded = buf + bytes(self.nseg * segment - len(buf))
        self.segd, self.fragd, self.fid, raw = oracle_lib.full_processing(buf, segment, k, m, want_frags=True)
        self.raw = raw                                    # nseg x total x frag
        f = self.frag
        self.frags = [[raw[(s * self.total + j) * f:(s * self.total + j + 1) * f] for j in range(self.total)]
                      for s in range(self.nseg)]


# ---- kernel edges through dm_rs_restore_device_async ------------------------------------------

def _device_restore(ctx, oracle_lib, k, m, segment, patterns, in_place, seed):
    """Restore len(patterns) segments on the device.  patterns[s]: the fragment indices present;
    in_place[s]: of those, the data fragments that already lie at their final address (the others
    are given at addresses outside the object).  The object buffer starts as 0xA5 everywhere else.
    Returns nothing: asserts dev_obj == the zero-padded original."""
    torch = _torch()
    from deoss_amd.reedsolomon import New
    nseg, total, frag = len(patterns), k + m, segment // k
    size = nseg * segment - (segment // 3 if segment > 3 else 0)   # the last segment is zero-padded
    c = Coded(oracle_lib, _bytes(size, seed), segment, k, m)
    pool = torch.frombuffer(bytearray(c.raw), dtype=torch.uint8).cuda()
    want = torch.frombuffer(bytearray(c.padded), dtype=torch.uint8).cuda()
    obj = torch.full((nseg * segment,), 0xA5, dtype=torch.uint8, device="cuda")
    ptrs = [0] * (nseg * total)
    for s in range(nseg):
        for j in patterns[s]:
            if j < k and j in in_place[s]:
                at = s * segment + j * frag
                obj[at:at + frag] = want[at:at + frag]
                ptrs[s * total + j] = obj.data_ptr() + at
            else:
                ptrs[s * total + j] = pool.data_ptr() + (s * total + j) * frag
    enc = New(ctx, k, m)
    try:
        enc.restore_device_async(ptrs, nseg, segment, obj.data_ptr(), 0)
        torch.cuda.synchronize()
    finally:
        enc.close()
    bad = torch.nonzero(obj != want)
    assert bad.numel() == 0, ("first differing byte", int(bad[0]), "segment", int(bad[0]) // segment)


def _random_patterns(rng, nseg, k, total, lo=None):
    return [sorted(rng.sample(range(total), rng.randint(lo or k, total))) for _ in range(nseg)]


def test_kernel_5000_tiny_segments_with_differing_tables(ctx, oracle_lib):
    """segment = 64 (one 16-byte unit per fragment), 5,000 segments: more segments than grid rows,
    so one workgroup walks segments whose tables differ; every fifth segment has all its data
    fragments in place (nout == 0), in between the others."""
    rng = random.Random(5000)
    pats = _random_patterns(rng, 5000, 4, 12)
    inpl = []
    for s, p in enumerate(pats):
        if s % 5 == 2:
            pats[s] = sorted(set(p) | {0, 1, 2, 3})
            inpl.append({0, 1, 2, 3})
        else:
            inpl.append({j for j in p if j < 4 and rng.random() < 0.3})
    assert sum(1 for s in range(5000) if inpl[s] == {0, 1, 2, 3}) >= 1000
    _device_restore(ctx, oracle_lib, 4, 8, 64, pats, inpl, 11)


def test_kernel_257_units_per_fragment(ctx, oracle_lib):
    """257 units per fragment: no multiple of the 256 threads."""
    pats = [[1, 5, 6, 11], [0, 2, 9, 10, 11], [3, 4, 7, 8]]
    _device_restore(ctx, oracle_lib, 4, 8, 4 * 16 * 257, pats, [set(), {0}, set()], 12)


def test_kernel_stride_loop_and_prefetch(ctx, oracle_lib):
    """segment = 4 x 160 KiB, 64 segments: 10,240 units per fragment against the 8,192 one grid row
    covers, so the stride loop and its prefetch run."""
    rng = random.Random(64)
    pats = _random_patterns(rng, 64, 4, 12)
    _device_restore(ctx, oracle_lib, 4, 8, 4 * 160 * 1024, pats, [set()] * 64, 13)


def test_kernel_all_495_patterns_in_one_call(ctx, oracle_lib):
    pats = [list(p) for p in itertools.combinations(range(12), 4)]
    assert len(pats) == 495
    _device_restore(ctx, oracle_lib, 4, 8, 4 * 4096, pats, [set()] * 495, 14)


def test_kernel_8_8_high_half_of_the_table_and_1_8(ctx, oracle_lib):
    """8 + 8 with 5-8 data fragments missing (outputs 4-7 come from the high half of a table entry)
    and 1 + 8."""
    rng = random.Random(88)
    pats = []
    for nmiss in (5, 6, 7, 8) * 6:
        data = rng.sample(range(8), 8 - nmiss)
        par = rng.sample(range(8, 16), rng.randint(nmiss, 8))
        pats.append(sorted(data + par))
    _device_restore(ctx, oracle_lib, 8, 8, 8 * 16 * 37, pats, [set()] * len(pats), 15)
    pats = [[j] for j in range(9)] + [[0, 3], [2, 8], list(range(9))]
    _device_restore(ctx, oracle_lib, 1, 8, 16 * 300, pats, [set()] * 9 + [{0}, set(), {0}], 16)
    _device_restore(ctx, oracle_lib, 3, 2, 3 * 16 * 5, [[0, 1, 2], [2, 3, 4], [0, 3, 4], [1, 2, 4]],
                    [set()] * 4, 17)


def test_kernel_in_place_and_pure_gather(ctx, oracle_lib):
    """Data fragments already in place: no output at all (every nout == 0: nothing is launched);
    the same fragments at other addresses: a pure gather (unit rows)."""
    pats = [[0, 1, 2, 3], [0, 1, 2, 3, 7], list(range(12))]
    _device_restore(ctx, oracle_lib, 4, 8, 4 * 16 * 33, pats, [{0, 1, 2, 3}] * 3, 18)
    _device_restore(ctx, oracle_lib, 4, 8, 4 * 16 * 33, pats, [set()] * 3, 18)
    _device_restore(ctx, oracle_lib, 4, 8, 4 * 16 * 33, pats, [{1, 3}, {0}, {2}], 18)


def test_device_restore_too_few_fails_before_any_launch(ctx):
    torch = _torch()
    from deoss_amd import DeossMerkleError
    from deoss_amd.reedsolomon import ErrTooFewShards, New
    enc = New(ctx, 4, 8)
    pool = torch.zeros(2 * 12 * 16, dtype=torch.uint8, device="cuda")
    obj = torch.full((128,), 0xA5, dtype=torch.uint8, device="cuda")
    ptrs = [pool.data_ptr() + 16 * i for i in range(24)]
    for j in (0, 1, 2, 3, 4, 5, 6, 8, 9):        # segment 1 keeps 3 of 12
        ptrs[12 + j] = 0
    with pytest.raises(ErrTooFewShards):
        enc.restore_device_async(ptrs, 2, 64, obj.data_ptr(), 0)
    torch.cuda.synchronize()
    assert bool((obj == 0xA5).all())              # segment 0 was not restored either
    with pytest.raises(DeossMerkleError):          # unaligned fragment
        enc.restore_device_async([p + 1 for p in ptrs[:12]], 1, 64, obj.data_ptr(), 0)
    with pytest.raises(DeossMerkleError):          # segment no multiple of 16 x data
        enc.restore_device_async(ptrs[:12], 1, 48, obj.data_ptr(), 0)
    enc.close()


# ---- dm_restore_buffer ------------------------------------------------------------------------

SEG = 4096


@pytest.fixture(scope="module")
def proc(ctx):
    from deoss_amd.process import Processor
    p = Processor(ctx, 4, 8, SEG)
    yield p
    p.close()


def _keep(c, rng, n):
    """Fragments with a seeded n of every segment's kept, the rest None; the kept index lists."""
    kept = [sorted(rng.sample(range(c.total), n)) for _ in range(c.nseg)]
    return [[c.frags[s][j] if j in kept[s] else None for j in range(c.total)] for s in range(c.nseg)], kept


def _flip(b, at=None):
    at = len(b) // 2 if at is None else at
    return b[:at] + bytes([b[at] ^ 0x40]) + b[at + 1:]


@pytest.mark.parametrize("size", [1, SEG - 1, SEG, SEG + 17, 9 * SEG + 12345])
def test_restore_buffer(proc, oracle_lib, size):
    rng = random.Random(size)
    c = Coded(oracle_lib, _bytes(size, size), SEG, 4, 8)
    total = c.total
    # any 4 of 12
    frags, kept = _keep(c, rng, 4)
    ok, out, fst, sst = proc.restore_buffer(frags, size, c.fragd, c.segd, c.fid, VALL)
    assert ok and out == c.buf and sst == bytes(c.nseg)
    for s in range(c.nseg):
        assert list(fst[s * total:(s + 1) * total]) == [USED if j in kept[s] else ABSENT for j in range(total)]
    # 5 of 12, one used fragment corrupted: it is bad, the spare takes its place, the output is exact
    frags, kept = _keep(c, rng, 5)
    hit = []
    for s in range(c.nseg):
        j = kept[s][rng.randrange(4)]
        frags[s][j] = _flip(frags[s][j], rng.randrange(c.frag))
        hit.append(j)
    ok, out, fst, sst = proc.restore_buffer(frags, size, c.fragd, c.segd, c.fid, VALL)
    assert ok and out == c.buf and sst == bytes(c.nseg)
    for s in range(c.nseg):
        want = [BAD if j == hit[s] else USED if j in kept[s] else ABSENT for j in range(total)]
        assert list(fst[s * total:(s + 1) * total]) == want
    # 7 of 12, nothing corrupted: the first four are used, the rest spare
    frags, kept = _keep(c, rng, 7)
    ok, out, fst, sst = proc.restore_buffer(frags, size, c.fragd, c.segd, c.fid, VALL)
    assert ok and out == c.buf
    for s in range(c.nseg):
        want = [ABSENT] * total
        for n, j in enumerate(kept[s]):
            want[j] = USED if n < 4 else SPARE
        assert list(fst[s * total:(s + 1) * total]) == want
    # 4 of 12 and one corrupted: no spare left -> not ok, segment "too few", out untouched
    frags, kept = _keep(c, rng, 4)
    s_bad = rng.randrange(c.nseg)
    j_bad = kept[s_bad][2]
    frags[s_bad][j_bad] = _flip(frags[s_bad][j_bad])
    out_buf = ctypes.create_string_buffer(b"\x5a" * size, size)
    ok, out, fst, sst = proc.restore_buffer(frags, size, c.fragd, c.segd, c.fid, VALL, out=out_buf)
    assert not ok and out is None and out_buf.raw == b"\x5a" * size
    assert list(sst) == [1 if s == s_bad else 0 for s in range(c.nseg)]
    assert fst[s_bad * total + j_bad] == BAD
    assert sorted(fst[s_bad * total:(s_bad + 1) * total]) == [ABSENT] * 8 + [SPARE] * 3 + [BAD]
    # a wrong segment name
    frags, kept = _keep(c, rng, 4)
    s_bad = rng.randrange(c.nseg)
    segn = bytearray(c.segd)
    segn[32 * s_bad + 5] ^= 1
    out_buf = ctypes.create_string_buffer(b"\x5a" * size, size)
    ok, out, fst, sst = proc.restore_buffer(frags, size, c.fragd, bytes(segn), None, VF | VS, out=out_buf)
    assert not ok and out_buf.raw == b"\x5a" * size
    assert list(sst) == [2 if s == s_bad else 0 for s in range(c.nseg)]
    # a wrong fid
    fid = bytes([c.fid[0] ^ 0x80]) + c.fid[1:]
    out_buf = ctypes.create_string_buffer(b"\x5a" * size, size)
    ok, out, fst, sst = proc.restore_buffer(frags, size, c.fragd, c.segd, fid, VALL, out=out_buf)
    assert not ok and out_buf.raw == b"\x5a" * size and sst == bytes(c.nseg)
    ok, out, fst, sst = proc.restore_buffer(frags, size, None, None, c.fid, VID)
    assert ok and out == c.buf
    # flags = 0: corrupted input is used as given (documented): the output is what klauspost's
    # Reconstruct makes of those bytes, and the names are not consulted
    frags, kept = _keep(c, rng, 4)
    s_bad = c.nseg - 1
    j_bad = kept[s_bad][1]
    frags[s_bad][j_bad] = _flip(frags[s_bad][j_bad], 0)
    ok, out, fst, sst = proc.restore_buffer(frags, size, c.fragd, c.segd, c.fid, 0)
    rebuilt = oracle_lib.rs_reconstruct(4, 8, frags[s_bad], c.frag)
    want = (c.padded[:s_bad * SEG] + b"".join(rebuilt[:4]))[:size]
    assert ok and out == want and fst[s_bad * total + j_bad] == USED
    # the same with the checks on is caught
    ok, out, fst, sst = proc.restore_buffer(frags, size, c.fragd, c.segd, c.fid, VALL)
    assert not ok and fst[s_bad * total + j_bad] == BAD and sst[s_bad] == 1


def test_restore_buffer_argument_errors(proc, oracle_lib):
    from deoss_amd import DeossMerkleError
    c = Coded(oracle_lib, _bytes(SEG + 1, 3), SEG, 4, 8)
    for size in (SEG, 2 * SEG + 1, 0):           # must end inside the last segment
        with pytest.raises(DeossMerkleError) as e:
            proc.restore_buffer(c.frags, size, c.fragd, c.segd, c.fid)
        assert e.value.code == -2
    with pytest.raises(DeossMerkleError) as e:   # nseg == 0
        proc.restore_buffer([], 1, b"", b"", c.fid)
    assert e.value.code == -1


def test_restore_buffer_full_size_segments(ctx, oracle_lib):
    """3 segments of 32 MiB, 4 + 8 (chain.SegmentSize / DataShards / ParShards): 5 fragments of
    each segment given, one of the first four corrupted."""
    from deoss_amd.process import Processor
    seg = 32 << 20
    size = 3 * seg - 12345
    c = Coded(oracle_lib, _bytes(size, 32), seg, 4, 8)
    rng = random.Random(32)
    frags, kept = _keep(c, rng, 5)
    frags[1][kept[1][0]] = _flip(frags[1][kept[1][0]], c.frag - 1)
    p = Processor(ctx)
    try:
        ok, out, fst, sst = p.restore_buffer(frags, size, c.fragd, c.segd, c.fid, VALL)
    finally:
        p.close()
    assert ok and out == c.buf and sst == bytes(3)
    assert fst[12 + kept[1][0]] == BAD and fst[12 + kept[1][4]] == USED
    assert list(fst[:12]).count(USED) == 4 and list(fst[:12]).count(SPARE) == 1


@pytest.mark.parametrize("mode", ["auto", "wide", "latency", "pair", "quad"])
def test_fragment_verify_under_every_leaf_kernel(ctx, proc, oracle_lib, mode):
    size = 5 * SEG + 100
    c = Coded(oracle_lib, _bytes(size, 77), SEG, 4, 8)
    rng = random.Random(77)
    frags, kept = _keep(c, rng, 6)
    frags[2][kept[2][1]] = _flip(frags[2][kept[2][1]])
    ctx.set_leaf_kernel(mode)
    try:
        ok, out, fst, sst = proc.restore_buffer(frags, size, c.fragd, c.segd, c.fid, VALL)
    finally:
        ctx.set_leaf_kernel("auto")
    assert ok and out == c.buf
    assert fst[2 * 12 + kept[2][1]] == BAD and list(fst).count(BAD) == 1
    assert fst[2 * 12 + kept[2][4]] == USED and fst[2 * 12 + kept[2][5]] == SPARE


# ---- dm_retrieve_file -------------------------------------------------------------------------

FSEG = 16384


@pytest.fixture(scope="module")
def stored(ctx, tmp_path_factory):
    """An object run through full_processing_file into a directory of fragment files."""
    from deoss_amd.process import Processor
    d = tmp_path_factory.mktemp("restore")
    size = 9 * FSEG + 12345
    buf = _bytes(size, 99)
    src = d / "object"
    src.write_bytes(buf)
    p = Processor(ctx, 4, 8, FSEG)
    segd, fragd, fid = p.full_processing_file(str(src), str(d / "frags"), segment_files=False)
    yield p, buf, segd, fragd, fid, d
    p.close()


def _fragment_dir(stored, tmp_path, keep_of):
    """A copy of the stored fragments with only keep_of(s) of segment s's 12 files."""
    p, buf, segd, fragd, fid, d = stored
    fd = tmp_path / "have"
    fd.mkdir()
    for s in range(len(segd) // 32):
        for j in keep_of(s):
            name = fragd[32 * (12 * s + j):32 * (12 * s + j + 1)].hex()
            (fd / name).write_bytes((d / "frags" / name).read_bytes())
    return fd


def test_retrieve_file_round_trip(stored, tmp_path, monkeypatch):
    """8 of every segment's 12 fragment files deleted; several windows and reused pinned slots."""
    p, buf, segd, fragd, fid, d = stored
    rng = random.Random(8)
    kept = [sorted(rng.sample(range(12), 4)) for _ in range(10)]
    fd = _fragment_dir(stored, tmp_path, lambda s: kept[s])
    outdir = tmp_path / "out"
    outdir.mkdir()
    monkeypatch.setenv("DEOSS_RT_WINDOW_BYTES", str(4 * FSEG))     # 3 windows
    monkeypatch.setenv("DEOSS_FP_SLOT_BYTES", str(3 * (FSEG // 4)))   # 3 fragments per slot
    ok, fst, sst = p.retrieve_file(str(fd), fragd, len(buf), str(outdir / "object"), segd, fid)
    assert ok and sst == bytes(10)
    assert (outdir / "object").read_bytes() == buf
    assert os.listdir(outdir) == ["object"]
    for s in range(10):
        assert list(fst[12 * s:12 * s + 12]) == [USED if j in kept[s] else ABSENT for j in range(12)]


def test_retrieve_file_wrong_length_and_corrupt_fragments(stored, tmp_path):
    p, buf, segd, fragd, fid, d = stored
    kept = [[0, 2, 5, 7, 9, 11]] * 10
    fd = _fragment_dir(stored, tmp_path, lambda s: kept[s])
    name = lambda s, j: fragd[32 * (12 * s + j):32 * (12 * s + j + 1)].hex()   # noqa: E731
    (fd / name(3, 2)).write_bytes((fd / name(3, 2)).read_bytes()[:-1])          # wrong length: bad
    (fd / name(6, 0)).write_bytes(_flip((fd / name(6, 0)).read_bytes()))        # wrong bytes: bad
    (fd / name(6, 5)).write_bytes(_flip((fd / name(6, 5)).read_bytes(), 1))
    out = tmp_path / "object"
    ok, fst, sst = p.retrieve_file(str(fd), fragd, len(buf), str(out), segd, fid)
    assert ok and out.read_bytes() == buf
    row = lambda s: list(fst[12 * s:12 * s + 12])                               # noqa: E731
    # only as many files as needed are read: the rest stay "absent" (never looked at)
    assert row(0) == [USED, 0, USED, 0, 0, USED, 0, USED, 0, 0, 0, 0]
    assert row(3) == [USED, 0, BAD, 0, 0, USED, 0, USED, 0, USED, 0, 0]
    assert row(6) == [BAD, 0, USED, 0, 0, BAD, 0, USED, 0, USED, 0, USED]
    # without fragment verification the corrupt bytes are caught by the segment names instead
    out2 = tmp_path / "object2"
    ok, fst, sst = p.retrieve_file(str(fd), fragd, len(buf), str(out2), segd, fid, flags=VS)
    assert not ok and list(sst) == [2 if s == 6 else 0 for s in range(10)]
    assert not out2.exists()


def test_retrieve_file_segment_without_fragments_leaves_nothing_behind(stored, tmp_path):
    p, buf, segd, fragd, fid, d = stored
    fd = _fragment_dir(stored, tmp_path, lambda s: [] if s == 4 else [1, 3, 8, 10])
    outdir = tmp_path / "out"
    outdir.mkdir()
    ok, fst, sst = p.retrieve_file(str(fd), fragd, len(buf), str(outdir / "object"), segd, fid)
    assert not ok and list(sst) == [1 if s == 4 else 0 for s in range(10)]
    assert list(fst[48:60]) == [ABSENT] * 12
    assert os.listdir(outdir) == []               # no output file, no temporary file
    # an output directory that does not exist: Go's text, nothing created
    from deoss_amd import DeossMerkleError
    with pytest.raises(DeossMerkleError) as e:
        p.retrieve_file(str(fd), fragd, len(buf), str(tmp_path / "nowhere" / "object"), segd, fid)
    assert e.value.code == -6 and "no such file or directory" in str(e.value)


def _three_windows(monkeypatch):
    monkeypatch.setenv("DEOSS_RT_WINDOW_BYTES", str(4 * FSEG))   # segments 0-3, 4-7, 8-9


def test_retrieve_file_failed_middle_window(stored, tmp_path, monkeypatch):
    """A segment of the second of three windows has no fragment files: that window is not rebuilt,
    the windows before and after it still report their fragments, nothing is left behind."""
    p, buf, segd, fragd, fid, d = stored
    kept = [2, 4, 7, 11]
    fd = _fragment_dir(stored, tmp_path, lambda s: [] if s == 5 else kept)
    outdir = tmp_path / "out"
    outdir.mkdir()
    _three_windows(monkeypatch)
    ok, fst, sst = p.retrieve_file(str(fd), fragd, len(buf), str(outdir / "object"), segd, fid)
    assert not ok and list(sst) == [1 if s == 5 else 0 for s in range(10)]
    for s in (0, 1, 2, 3, 8, 9):
        assert list(fst[12 * s:12 * s + 12]) == [USED if j in kept else ABSENT for j in range(12)], s
    assert list(fst[60:72]) == [ABSENT] * 12
    assert os.listdir(outdir) == []


def test_retrieve_file_wrong_fid_across_windows(stored, tmp_path, monkeypatch):
    """Only the fid is checked, over the digests of three windows: one flipped bit fails the call
    after every window was rebuilt; the right fid gives the object back."""
    p, buf, segd, fragd, fid, d = stored
    fd = _fragment_dir(stored, tmp_path, lambda s: [0, 3, 5, 10])
    outdir = tmp_path / "out"
    outdir.mkdir()
    _three_windows(monkeypatch)
    wrong = fid[:17] + bytes([fid[17] ^ 0x04]) + fid[18:]
    ok, fst, sst = p.retrieve_file(str(fd), fragd, len(buf), str(outdir / "object"), None, wrong, flags=VID)
    assert not ok and sst == bytes(10)
    assert os.listdir(outdir) == []
    ok, fst, sst = p.retrieve_file(str(fd), fragd, len(buf), str(outdir / "object"), None, fid, flags=VID)
    assert ok and sst == bytes(10)
    assert (outdir / "object").read_bytes() == buf
    assert os.listdir(outdir) == ["object"]


def test_retrieve_file_segment_mismatch_in_first_window(stored, tmp_path, monkeypatch):
    """Segment names only: a corrupt used fragment of segment 1 shows as that segment's mismatch;
    the later windows still load and report their fragments, and nothing is written."""
    p, buf, segd, fragd, fid, d = stored
    kept = [1, 6, 8, 9]
    fd = _fragment_dir(stored, tmp_path, lambda s: kept)
    name = fragd[32 * (12 * 1 + 6):32 * (12 * 1 + 7)].hex()
    (fd / name).write_bytes(_flip((fd / name).read_bytes()))
    outdir = tmp_path / "out"
    outdir.mkdir()
    _three_windows(monkeypatch)
    ok, fst, sst = p.retrieve_file(str(fd), fragd, len(buf), str(outdir / "object"), segd, None, flags=VS)
    assert not ok and list(sst) == [2 if s == 1 else 0 for s in range(10)]
    for s in range(10):
        assert list(fst[12 * s:12 * s + 12]) == [USED if j in kept else ABSENT for j in range(12)], s
    assert os.listdir(outdir) == []


def test_retrieve_file_candidate_reload_across_slots(stored, tmp_path, monkeypatch):
    """6 files per segment, the first kept one of two segments corrupt, 3 fragments per pinned slot:
    the replacements are loaded in a second round through reused slots."""
    p, buf, segd, fragd, fid, d = stored
    kept = [1, 2, 4, 7, 9, 10]
    fd = _fragment_dir(stored, tmp_path, lambda s: kept)
    for s in (2, 7):
        name = fragd[32 * (12 * s + 1):32 * (12 * s + 2)].hex()
        (fd / name).write_bytes(_flip((fd / name).read_bytes(), s))
    monkeypatch.setenv("DEOSS_FP_SLOT_BYTES", str(3 * (FSEG // 4)))
    out = tmp_path / "object"
    ok, fst, sst = p.retrieve_file(str(fd), fragd, len(buf), str(out), segd, fid)
    assert ok and sst == bytes(10) and out.read_bytes() == buf
    for s in range(10):
        if s in (2, 7):   # the fifth kept file takes the corrupt one's place, the sixth is never read
            want = [0, BAD, USED, 0, USED, 0, 0, USED, 0, USED, 0, 0]
        else:
            want = [0, USED, USED, 0, USED, 0, 0, USED, 0, 0, 0, 0]
        assert list(fst[12 * s:12 * s + 12]) == want, s


def test_restore_file_inverts_full_processing(tmp_path):
    """The module-level mirrors at chain sizes: FullProcessing, 8 of 12 fragment files deleted,
    RestoreFile gives the file back."""
    from deoss_amd.process import FullProcessing, RestoreFile
    buf = _bytes((25 << 20) + 321, 5)   # past the third data fragment: no two fragments alike
    src = tmp_path / "upload"
    src.write_bytes(buf)
    info, fid, err = FullProcessing(str(src), "", str(tmp_path / "frags"))
    assert err is None and len(info) == 1
    for j in (0, 1, 3, 4, 6, 7, 10, 11):
        os.unlink(info[0].FragmentHash[j])
    ok, err = RestoreFile(str(tmp_path / "frags"), info, len(buf), str(tmp_path / "download"))
    assert ok and err is None and (tmp_path / "download").read_bytes() == buf
    os.unlink(info[0].FragmentHash[2])
    ok, err = RestoreFile(str(tmp_path / "frags"), info, len(buf), str(tmp_path / "download2"))
    assert not ok and err is not None and not (tmp_path / "download2").exists()


# ---- fuzz ---------------------------------------------------------------------------------------

def test_restore_fuzz_100_cases(ctx, oracle_lib):
    """k, m, segment, size, erasure patterns and corruptions varied; against the original bytes
    and, for every rebuilt fragment, against the oracle's Reconstruct of the same good fragments."""
    from deoss_amd.process import Processor
    rng = random.Random(0xF022)
    for case in range(100):
        k, m = rng.randint(1, 8), rng.randint(1, 8)
        total = k + m
        segment = 16 * k * rng.choice([1, 2, 3, 17, 64, 257, 300])
        nseg = rng.randint(1, 6)
        size = (nseg - 1) * segment + rng.randint(1, segment)
        c = Coded(oracle_lib, _bytes(size, 1000 + case), segment, k, m)
        frags, corrupt = [], []
        doomed = rng.random() < 0.2      # one segment is left with too few good fragments
        s_doom = rng.randrange(nseg)
        for s in range(nseg):
            n = rng.randint(k, total)
            kept = sorted(rng.sample(range(total), n))
            nbad = 0
            if doomed and s == s_doom:
                nbad = n - k + 1
            elif n > k and rng.random() < 0.5:
                nbad = rng.randint(1, n - k)
            bad = set(rng.sample(kept, nbad))
            row = [None] * total
            for j in kept:
                row[j] = _flip(c.frags[s][j], rng.randrange(c.frag)) if j in bad else c.frags[s][j]
            frags.append(row)
            corrupt.append(bad)
        p = Processor(ctx, k, m, segment)
        try:
            ok, out, fst, sst = p.restore_buffer(frags, size, c.fragd, c.segd, c.fid, VALL)
        finally:
            p.close()
        tag = (case, k, m, segment, nseg, size)
        for s in range(nseg):
            good = [j for j in range(total) if frags[s][j] is not None and j not in corrupt[s]]
            want = [ABSENT] * total
            for j in corrupt[s]:
                want[j] = BAD
            for n, j in enumerate(good):
                want[j] = SPARE if (len(good) < k or n >= k) else USED
            assert list(fst[s * total:(s + 1) * total]) == want, tag
            assert sst[s] == (1 if len(good) < k else 0), tag
        if doomed:
            assert not ok and out is None, tag
            continue
        assert ok and out == c.buf, tag
        for s in range(nseg):
            used = [j for j in range(total) if fst[s * total + j] == USED]
            shards = [frags[s][j] if j in used else None for j in range(total)]
            rebuilt = oracle_lib.rs_reconstruct(k, m, shards, c.frag)
            assert (b"".join(rebuilt[:k]))[:max(0, min(segment, size - s * segment))] == \
                out[s * segment:(s + 1) * segment], tag
