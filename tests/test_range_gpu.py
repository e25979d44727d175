"""GPU checks of the ranged restore: aes_cbc_decrypt_window_kernel through
dm_aes_cbc_decrypt_windows_device_async, dm_restore_range_buffer / Processor.restore_range, and
dm_retrieve_range / RestoreRange.

Every comparison is bit-exact.  Expected plaintext is the object's own bytes; expected decryptions
come from tests/cipher_ref.py (plain-Python AES); fragments and names come from oracle/ (the Coded
class of test_restore_gpu.py).  The ranged result is also compared with restore_buffer(...)[off:off+len]
of the same inputs.  SEG = 4096, 4 + 8: a fragment is 1,024 bytes = 64 blocks, P = 4080.
"""
from __future__ import annotations

import ctypes
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cipher_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

VF = 1                                    # DM_RESTORE_VERIFY_FRAGMENTS
NO_PAD = 8                                # DM_RANGE_NO_PADDING_CHECK
ABSENT, USED, SPARE, BAD, REBUILT = 0, 1, 2, 3, 4
SEG, K, M, TOTAL = 4096, 4, 8, 12
FRAG, P = SEG // K, SEG - 16
KEYS = {n: bytes((37 * i + 11 * n + 5) & 0xFF for i in range(n)) for n in (16, 24, 32)}
IV = bytes((91 * i + 7) & 0xFF for i in range(16))
SENTINEL = 0xEE
SIZE_PLAIN, SIZE_CIPHER = 9 * SEG + 12345, 9 * P + 1234
FUZZ_SEED = 0x5EEC


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _flip(b, at=None):
    at = len(b) // 2 if at is None else at
    return b[:at] + bytes([b[at] ^ 0x40]) + b[at + 1:]


def fuzz_cases():
    """The 200 seeded cases of test_range_fuzz_200_cases: (cipher, off, len, kept fragment indices per
    segment).  Needs no GPU and no oracle: tests/test_range_plan.py checks on the CPU that none is
    degenerate."""
    rng = random.Random(FUZZ_SEED)
    cases = []
    for _ in range(200):
        cipher = rng.random() < 0.5
        size, piece = (SIZE_CIPHER, P) if cipher else (SIZE_PLAIN, SEG)
        nseg = (size + piece - 1) // piece
        shape = rng.randrange(4)
        if shape == 0:      # a few bytes anywhere
            length = rng.randint(1, 40)
        elif shape == 1:    # up to a few fragments
            length = rng.randint(1, 3 * FRAG)
        elif shape == 2:    # across segments
            length = rng.randint(1, 3 * SEG)
        else:
            length = rng.randint(1, size)
        off = rng.randint(0, size - length)
        kept = [sorted(rng.sample(range(TOTAL), rng.randint(K, TOTAL))) for _ in range(nseg)]
        cases.append((cipher, off, length, kept))
    return cases


# ---- the window kernel through dm_aes_cbc_decrypt_windows_device_async ---------------------------

NB = 10240 + 64       # ciphertext blocks of the kernel tests' shared buffer
_kref = {}


def _kernel_ref(klen):
    """(random "ciphertext" blocks C (NB, 16), D = the bare inverse cipher of every block): the
    plaintext of block i after predecessor q is D[i] ^ q.  Computed once per key length, read-only."""
    if klen not in _kref:
        C = np.random.default_rng(7000 + klen).integers(0, 256, size=(NB, 16), dtype=np.uint8)
        D = R.decrypt_blocks(R.expand_key(KEYS[klen]), C)
        C.setflags(write=False)
        D.setflags(write=False)
        _kref[klen] = (C, D)
    return _kref[klen]


def _expect(C, D, b0, n, first_prev):
    prevs = np.concatenate([np.frombuffer(first_prev, dtype=np.uint8).reshape(1, 16), C[b0:b0 + n - 1]])
    return D[b0:b0 + n] ^ prevs


def _run_windows(ctx, klen, specs, C, extra=None):
    """specs: [(first block in C, nblk, prev: 'iv' | 'in' (the block before, in C) | 'x' (a block in
    another allocation), check_pad)].  Every window gets its own output region with a sentinel block
    behind it.  Returns (outputs per window incl. the sentinel block, verdict bytes)."""
    torch = _torch()
    dC = torch.from_numpy(np.array(C)).cuda()
    X = np.frombuffer(_bytes(16, 99), dtype=np.uint8)
    dX = torch.from_numpy(X.copy()).cuda()
    offs, total = [], 0
    for _, n, _, _ in specs:
        offs.append(total)
        total += 16 * (n + 1)
    out = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    verdict = torch.full((len(specs),), 7, dtype=torch.uint8, device="cuda")
    wins = []
    for (b0, n, prev, pad), o in zip(specs, offs):
        pp = 0 if prev == "iv" else dX.data_ptr() if prev == "x" else dC.data_ptr() + 16 * (b0 - 1)
        wins.append((dC.data_ptr() + 16 * b0, pp, out.data_ptr() + o, n, pad))
    ctx.aes_cbc_decrypt_windows_device_async(KEYS[klen], IV, wins, verdict.data_ptr())
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    return [host[o:o + 16 * (n + 1)].reshape(n + 1, 16) for (_, n, _, _), o in zip(specs, offs)], verdict.cpu().numpy(), X


def _check_windows(specs, outs, verdict, C, D, X, tag):
    for w, ((b0, n, prev, pad), got) in enumerate(zip(specs, outs)):
        first = IV if prev == "iv" else X.tobytes() if prev == "x" else C[b0 - 1].tobytes()
        want = _expect(C, D, b0, n, first)
        keep = n - 1 if pad else n
        assert (got[:keep] == want[:keep]).all(), (tag, w)
        assert (got[keep:] == SENTINEL).all(), (tag, w)          # a padding block is not stored; nothing beyond
        if pad:
            assert verdict[w] == int((want[n - 1] == 0x10).all()), (tag, w)
        else:
            assert verdict[w] == 7, (tag, w)                     # written for check_pad windows only


@pytest.mark.parametrize("klen", (16, 24, 32))
def test_window_kernel_every_shape_in_one_call(ctx, klen):
    C0, _ = _kernel_ref(klen)
    # a good padding block at block 520: E(0x10 x 16 ^ C[519]), so the buffer differs per key there
    C = C0.copy()
    rk = R.expand_key(KEYS[klen])
    C[520] = R.encrypt_blocks(rk, (np.full((1, 16), 0x10, dtype=np.uint8) ^ C[519:520]))[0]
    D = R.decrypt_blocks(rk, C)
    specs = [(0, 5, "iv", 0), (1, 7, "in", 0),                  # from block 0 (IV) and from block 1
             (100, 1, "in", 0), (200, 1, "iv", 0),              # nblk = 1
             (500, 21, "in", 1),                                # check_pad, good: blocks 500 .. 520
             (300, 10, "in", 1),                                # check_pad, bad
             (519, 2, "in", 1), (2, 2, "iv", 1),                # the two-block windows of the padding check
             (400, 4, "x", 0),                                  # prev in another allocation than in
             (0, 10240, "iv", 0), (700, 1, "in", 0)]            # a long window beside a short one
    specs += [(1 + i, 10240, "in", 0) for i in range(64)]       # 64 x 10,240 blocks: beyond one grid row's 8,192
    outs, verdict, X = _run_windows(ctx, klen, specs, C)
    _check_windows(specs, outs, verdict, C, D, X, klen)
    assert verdict[4] == 1 and verdict[5] == 0 and verdict[6] == 1 and verdict[7] == 0


@pytest.mark.parametrize("klen", (16, 24, 32))
def test_window_kernel_5000_short_windows(ctx, klen):
    """More windows than grid rows (y is capped at 8 x CUs = 2,048)."""
    C, D = _kernel_ref(klen)
    rng = random.Random(klen)
    specs = []
    for _ in range(5000):
        n = rng.randint(1, 3)
        pad = 1 if n >= 2 and rng.random() < 0.2 else 0
        specs.append((rng.randint(1, NB - 4), n, rng.choice(["iv", "in", "x"]), pad))
    outs, verdict, X = _run_windows(ctx, klen, specs, C)
    _check_windows(specs, outs, verdict, C, D, X, klen)


def test_window_kernel_argument_checks(ctx):
    from deoss_amd import DeossMerkleError
    torch = _torch()
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    out = torch.zeros(256, dtype=torch.uint8, device="cuda")
    a, o = buf.data_ptr(), out.data_ptr()
    ctx.aes_cbc_decrypt_windows_device_async(KEYS[16], IV, [], 0)          # nwin == 0 launches nothing
    for key, win, pad in ((bytes(15), [(a, 0, o, 1, 0)], 0), (KEYS[16], [(a + 8, 0, o, 1, 0)], 0),
                          (KEYS[16], [(a, a + 4, o, 1, 0)], 0), (KEYS[16], [(a, 0, o + 1, 1, 0)], 0),
                          (KEYS[16], [(a, 0, o, 0, 0)], 0), (KEYS[16], [(a, 0, o, 1, 1)], o + 64),
                          (KEYS[16], [(a, 0, o, 2, 1)], 0), (KEYS[16], [(a, 0, 0, 1, 0)], 0)):
        with pytest.raises(DeossMerkleError) as e:
            ctx.aes_cbc_decrypt_windows_device_async(key, IV, win, pad)
        assert e.value.code == -2, win
    torch.cuda.synchronize()
    assert not out.any().item()   # nothing ran


# ---- dm_restore_range_buffer / Processor.restore_range --------------------------------------------

@pytest.fixture(scope="module")
def proc(ctx):
    from deoss_amd.process import Processor
    p = Processor(ctx, K, M, SEG)
    yield p
    p.close()


class Obj:
    """An object, its fragments and names (from the CPU oracle; with a cipher over the reference
    ciphertext), shared by the tests and never changed."""

    def __init__(self, oracle_lib, size, key):
        from test_restore_gpu import Coded
        self.size, self.key = size, key
        self.buf = _bytes(size, size)
        self.piece = P if key else SEG
        c = Coded(oracle_lib, R.scheme_encrypt(self.buf, key, SEG) if key else self.buf, SEG, K, M)
        self.nseg, self.fragd, self.frags = c.nseg, c.fragd, c.frags

    def given(self, kept=None):
        """Fragment rows; kept: per segment the indices given (None: all)."""
        return [[f if kept is None or j in kept[s] else None for j, f in enumerate(row)]
                for s, row in enumerate(self.frags)]


@pytest.fixture(scope="module")
def plain_obj(oracle_lib):
    return Obj(oracle_lib, SIZE_PLAIN, b"")


@pytest.fixture(scope="module")
def cipher_obj(oracle_lib):
    return Obj(oracle_lib, SIZE_CIPHER, KEYS[32])


def _rows(fst):
    return [list(fst[TOTAL * s:TOTAL * (s + 1)]) for s in range(len(fst) // TOTAL)]


def _need_rows(proc, o, off, length, padding_check=True):
    seg0, nt, need, _ = proc.range_plan(o.size, off, length, cipher=o.key, padding_check=padding_check)
    rows = [[ABSENT] * TOTAL for _ in range(o.nseg)]
    for t in range(nt):
        rows[seg0 + t][:K] = need[t]
    return rows


def _ranges(o):
    size, piece = o.size, o.piece
    tail0 = (o.nseg - 1) * piece
    return [(0, 1), (size - 1, 1), (1023, 2), (SEG - 1, 2), (P - 1, 2), (5, 3 * SEG), (0, size), (tail0, size - tail0),
            (2 * piece + 7, 333), (3 * piece + 1024 + 13, 2 * FRAG + 5)]


@pytest.mark.parametrize("which", ["plain", "cipher"])
def test_fixed_ranges_every_fragment_given(proc, plain_obj, cipher_obj, which):
    o = plain_obj if which == "plain" else cipher_obj
    frags = o.given()
    ok, whole, _, _ = proc.restore_buffer(frags, o.size, o.fragd, None, None, VF, cipher=o.key)
    assert ok and whole == o.buf
    for off, length in _ranges(o):
        ok, out, fst, sst = proc.restore_range(frags, o.size, off, length, o.fragd, cipher=o.key)
        assert ok and out == o.buf[off:off + length] == whole[off:off + length], (which, off, length)
        assert sst == bytes(o.nseg)
        # used exactly where the plan needs it, nothing else was looked at: what the feature is for
        assert _rows(fst) == _need_rows(proc, o, off, length), (which, off, length)
        # the same through the C entry point's other face: names absent, nothing verified
        ok, out, fst2, _ = proc.restore_range(frags, o.size, off, length, None, cipher=o.key)
        assert ok and out == o.buf[off:off + length] and fst2 == fst


def test_cipher_edges(proc, cipher_obj):
    o = cipher_obj
    frags = o.given()
    # piece offset 1,024: the first block of fragment 1 needs the last block of fragment 0
    off = 4 * P + 1024
    ok, out, fst, _ = proc.restore_range(frags, o.size, off, 10, o.fragd, cipher=o.key, padding_check=False)
    assert ok and out == o.buf[off:off + 10] and _rows(fst)[4] == [USED, USED] + [ABSENT] * 10
    assert list(fst).count(USED) == 2
    ok, out, fst, _ = proc.restore_range(frags, o.size, off, 10, o.fragd, cipher=o.key)
    assert ok and out == o.buf[off:off + 10] and _rows(fst)[4] == [USED, USED, ABSENT, USED] + [ABSENT] * 8
    # the last plaintext block of a piece (the padding block follows it)
    off = 5 * P + P - 16
    for length in (16, 7):
        ok, out, fst, _ = proc.restore_range(frags, o.size, off, length, o.fragd, cipher=o.key)
        assert ok and out == o.buf[off:off + length] and _rows(fst)[5] == [ABSENT] * 3 + [USED] + [ABSENT] * 8
    # inside fragment 0: the padding check brings fragment 3 of the first touched segment, the flag leaves it out
    off = 2 * P + 100
    ok, out, fst, _ = proc.restore_range(frags, o.size, off, 600, o.fragd, cipher=o.key)
    assert ok and out == o.buf[off:off + 600] and _rows(fst)[2] == [USED, ABSENT, ABSENT, USED] + [ABSENT] * 8
    ok, out, fst, _ = proc.restore_range(frags, o.size, off, 600, o.fragd, cipher=o.key, padding_check=False)
    assert ok and out == o.buf[off:off + 600] and _rows(fst)[2] == [USED] + [ABSENT] * 11
    # only the first touched segment gets the extra fragment
    off = 2 * P + 4000
    ok, out, fst, _ = proc.restore_range(frags, o.size, off, 200, o.fragd, cipher=o.key)
    assert ok and out == o.buf[off:off + 200]
    assert _rows(fst)[2][:4] == [ABSENT, ABSENT, ABSENT, USED] and _rows(fst)[3][:4] == [USED, ABSENT, ABSENT, ABSENT]
    # a wrong cipher: bad padding, nothing released
    wrong = bytes([o.key[0] ^ 1]) + o.key[1:]
    for off, length in ((2 * P + 100, 600), (5, 3 * SEG)):
        dst = ctypes.create_string_buffer(bytes([0x5A]) * length, length)
        ok, out, fst, sst = proc.restore_range(frags, o.size, off, length, o.fragd, cipher=wrong, out=dst)
        assert not ok and out is None and dst.raw == bytes([0x5A]) * length
        assert sst[off // P] == 3 and set(sst) <= {0, 3}
    # ... which the flag trades for garbage when the range does not reach a padding block
    ok, out, _, _ = proc.restore_range(frags, o.size, 2 * P + 100, 600, o.fragd, cipher=wrong, padding_check=False)
    assert ok and out != o.buf[2 * P + 100:2 * P + 700]


@pytest.mark.parametrize("which", ["plain", "cipher"])
def test_erasures(proc, plain_obj, cipher_obj, which):
    o = plain_obj if which == "plain" else cipher_obj
    pc = False                              # the padding flag off: need is fragment 1 alone
    off, length = 2 * o.piece + 1024 + 40, 500    # inside fragment 1 of segment 2
    want = o.buf[off:off + length]

    def run(frags, flags=VF, out=None, names=o.fragd):
        return proc.restore_range(frags, o.size, off, length, names, cipher=o.key, padding_check=pc, flags=flags,
                                  out=out)
    every = [list(range(TOTAL)) for _ in range(o.nseg)]
    # a needed data fragment is missing: rebuilt from the first 4 given, no other data fragment is
    kept = [list(r) for r in every]
    kept[2] = [0, 2, 4, 5, 7, 11]           # 1 (needed) and 3 (not needed) are gone
    ok, out, fst, sst = run(o.given(kept))
    assert ok and out == want and sst == bytes(o.nseg)
    assert _rows(fst)[2] == [USED, REBUILT, USED, ABSENT, USED, USED] + [ABSENT] * 6
    assert sum(map(sum, _rows(fst)[:2] + _rows(fst)[3:])) == 0
    # a needed data fragment is corrupt: bad, replaced by a rebuilt one
    frags = o.given()
    frags[2][1] = _flip(frags[2][1])
    ok, out, fst, sst = run(frags)
    assert ok and out == want and _rows(fst)[2] == [USED, BAD, USED, USED, USED] + [ABSENT] * 7
    # a corrupt input is replaced by the next given one in a second round
    frags = o.given(kept)
    frags[2][2] = _flip(frags[2][2], 3)
    ok, out, fst, sst = run(frags)
    assert ok and out == want and _rows(fst)[2] == [USED, REBUILT, BAD, ABSENT, USED, USED, ABSENT, USED] + [ABSENT] * 4
    # too few good fragments in a touched segment
    kept3 = [list(r) for r in every]
    kept3[2] = [0, 4, 9]
    dst = ctypes.create_string_buffer(bytes([0x5A]) * length, length)
    ok, out, fst, sst = run(o.given(kept3), out=dst)
    assert not ok and out is None and dst.raw == bytes([0x5A]) * length
    assert list(sst) == [1 if s == 2 else 0 for s in range(o.nseg)]
    frags = o.given(kept)                   # 6 given, 3 of them corrupt: 3 good ones left
    for j in (0, 5, 11):
        frags[2][j] = _flip(frags[2][j], j)
    dst = ctypes.create_string_buffer(bytes([0x5A]) * length, length)
    ok, out, fst, sst = run(frags, out=dst)
    assert not ok and dst.raw == bytes([0x5A]) * length and sst[2] == 1
    assert _rows(fst)[2] == [BAD, ABSENT, SPARE, ABSENT, SPARE, BAD, ABSENT, SPARE, ABSENT, ABSENT, ABSENT, BAD]
    # a missing fragment, or none at all, in an untouched segment changes nothing
    kept5 = [list(r) for r in every]
    kept5[5], kept5[0] = [], [3]
    ok, out, fst, sst = run(o.given(kept5))
    assert ok and out == want and _rows(fst)[2] == [ABSENT, USED] + [ABSENT] * 10 and list(fst).count(USED) == 1
    # flags = 0: fragments are used as given, the names are not consulted
    frags = o.given()
    frags[2][1] = _flip(frags[2][1], 300)
    ok, out, fst, sst = run(frags, flags=0)
    assert ok and _rows(fst)[2] == [ABSENT, USED] + [ABSENT] * 10
    if not o.key:
        assert out == _flip(want, 300 - 40)
    else:
        assert out != want
    ok, out, fst, sst = run(frags)          # with the check on it is caught and replaced
    assert ok and out == want and fst[2 * TOTAL + 1] == BAD
    # a rebuilt fragment that is not its name: good inputs, another output
    names = bytearray(o.fragd)
    names[32 * (2 * TOTAL + 1)] ^= 1
    dst = ctypes.create_string_buffer(bytes([0x5A]) * length, length)
    ok, out, fst, sst = run(o.given(kept), out=dst, names=bytes(names))
    assert not ok and dst.raw == bytes([0x5A]) * length and sst[2] == 2


def test_range_fuzz_200_cases(proc, plain_obj, cipher_obj):
    """Seed FUZZ_SEED: random ranges, random erasure patterns with at least k fragments kept per
    segment, cipher on or off, against the object's bytes (tests/test_range_plan.py checks on the CPU
    that no case is degenerate; none is skipped here)."""
    whole = {}
    ran = 0
    for cipher, off, length, kept in fuzz_cases():
        o = cipher_obj if cipher else plain_obj
        if cipher not in whole:
            ok, whole[cipher], _, _ = proc.restore_buffer(o.given(), o.size, o.fragd, None, None, VF, cipher=o.key)
            assert ok
        frags = o.given(kept)
        ok, out, fst, sst = proc.restore_range(frags, o.size, off, length, o.fragd, cipher=o.key)
        tag = (cipher, off, length)
        assert ok and out == o.buf[off:off + length] == whole[cipher][off:off + length], tag
        assert sst == bytes(o.nseg), tag
        need = _need_rows(proc, o, off, length)
        for s, row in enumerate(_rows(fst)):
            if not any(need[s]):
                assert row == [ABSENT] * TOTAL, tag      # untouched: never looked at
                continue
            lost = [j for j in range(K) if need[s][j] and j not in kept[s]]
            if not lost:
                assert row == need[s], tag
            else:                                         # the first k given are the inputs, only the lost needed ones rebuilt
                want = [ABSENT] * TOTAL
                for j in kept[s][:K]:
                    want[j] = USED
                for j in lost:
                    want[j] = REBUILT
                assert row == want, tag
        ran += 1
    assert ran == 200


def test_restore_range_argument_errors(proc, plain_obj, cipher_obj):
    """Mirrors test_restore_buffer_argument_errors, plus the range's own."""
    from deoss_amd import DeossMerkleError
    o = plain_obj
    frags = o.given()
    for size in ((o.nseg - 1) * SEG, o.nseg * SEG + 1, 0):           # must end inside the last segment
        with pytest.raises(DeossMerkleError) as e:
            proc.restore_range(frags, size, 0, 1, o.fragd)
        assert e.value.code == -2
    with pytest.raises(DeossMerkleError) as e:                        # nseg == 0
        proc.restore_range([], 1, 0, 1, b"")
    assert e.value.code == -1
    for off, length in ((0, 0), (o.size, 1), (o.size - 1, 2), (2**64 - 1, 2)):
        with pytest.raises(DeossMerkleError) as e:
            proc.restore_range(frags, o.size, off, length, o.fragd)
        assert e.value.code == -2 and "does not lie in the object" in str(e.value)
    c = cipher_obj
    for size in (9 * P, 10 * P + 1):
        with pytest.raises(DeossMerkleError) as e:
            proc.restore_range(c.given(), size, 0, 1, c.fragd, cipher=c.key)
        assert e.value.code == -2 and "pieces" in str(e.value)
    with pytest.raises(DeossMerkleError) as e:
        proc.restore_range(c.given(), c.size, 0, 1, c.fragd, cipher=b"short")
    assert e.value.code == -2 and "16, 24 or 32" in str(e.value)


def test_ranged_calls_are_timed(ctx, proc, plain_obj):
    """With dm_set_timing a ranged call adds a record per round to dm_timing_summary."""
    o = plain_obj
    ctx.set_timing(True)
    try:
        proc.restore_range(o.given(), o.size, 5, 3 * SEG, o.fragd)
        n = ctx.timing_summary()[0]
    finally:
        ctx.set_timing(False)
    assert n >= 1


# ---- dm_retrieve_range / RestoreRange ---------------------------------------------------------------

FSEG = 16384


@pytest.fixture(scope="module")
def stored(ctx, tmp_path_factory):
    """An object run through full_processing_file into a directory of fragment files (as the `stored`
    fixture of test_restore_gpu.py)."""
    from deoss_amd.process import Processor
    d = tmp_path_factory.mktemp("range")
    size = 9 * FSEG + 12345
    buf = _bytes(size, 99)
    src = d / "object"
    src.write_bytes(buf)
    p = Processor(ctx, 4, 8, FSEG)
    segd, fragd, fid = p.full_processing_file(str(src), str(d / "frags"), segment_files=False)
    yield p, buf, fragd, d
    p.close()


def _fragment_dir(stored, tmp_path, keep_of=lambda s: range(12)):
    p, buf, fragd, d = stored
    fd = tmp_path / "have"
    fd.mkdir()
    for s in range(len(fragd) // (32 * 12)):
        for j in keep_of(s):
            name = fragd[32 * (12 * s + j):32 * (12 * s + j + 1)].hex()
            (fd / name).write_bytes((d / "frags" / name).read_bytes())
    return fd


def _name(fragd, s, j):
    return fragd[32 * (12 * s + j):32 * (12 * s + j + 1)].hex()


def test_retrieve_range_files(stored, tmp_path, monkeypatch):
    p, buf, fragd, d = stored
    fd = _fragment_dir(stored, tmp_path)
    before = sorted(os.listdir(fd))
    monkeypatch.setenv("TMPDIR", str(tmp_path / "tmp"))
    (tmp_path / "tmp").mkdir()
    ffrag = FSEG // 4
    size = len(buf)
    for off, length in ((0, 1), (size - 1, 1), (ffrag - 1, 2), (FSEG - 1, 2), (5, 3 * FSEG), (0, size),
                        (2 * FSEG + ffrag + 3, 1000)):
        ok, out, fst, sst = p.retrieve_range(str(fd), fragd, size, off, length)
        assert ok and out == buf[off:off + length] and sst == bytes(10), (off, length)
        seg0, nt, need, _ = p.range_plan(size, off, length)
        want = [[0] * 12 for _ in range(10)]
        for t in range(nt):
            want[seg0 + t][:4] = need[t]
        assert _rows(fst) == want, (off, length)
    off, length = 2 * FSEG + ffrag + 3, 1000            # fragment 1 of segment 2
    # a needed file deleted: rebuilt from the first four that exist
    os.unlink(fd / _name(fragd, 2, 1))
    os.unlink(fd / _name(fragd, 2, 3))
    ok, out, fst, sst = p.retrieve_range(str(fd), fragd, size, off, length)
    assert ok and out == buf[off:off + length]
    assert _rows(fst)[2] == [USED, REBUILT, USED, ABSENT, USED, USED] + [ABSENT] * 6
    # a needed file truncated: bad, rebuilt
    (tmp_path / "b").mkdir()
    fd2 = _fragment_dir(stored, tmp_path / "b")
    path = fd2 / _name(fragd, 2, 1)
    path.write_bytes(path.read_bytes()[:-1])
    ok, out, fst, sst = p.retrieve_range(str(fd2), fragd, size, off, length)
    assert ok and out == buf[off:off + length]
    assert _rows(fst)[2] == [USED, BAD, USED, USED, USED] + [ABSENT] * 7
    # nothing was created or left, in fragdir or the temp dir
    assert sorted(os.listdir(fd) + [_name(fragd, 2, 1), _name(fragd, 2, 3)]) == before
    assert os.listdir(tmp_path / "tmp") == []
    os.unlink(path)
    os.mkdir(path)                                       # a directory in a fragment's place: wrong shape, bad
    ok, out, fst, sst = p.retrieve_range(str(fd2), fragd, size, off, length)
    assert ok and out == buf[off:off + length] and fst[2 * 12 + 1] == BAD
    # a directory that does not exist: every file is absent
    ok, out, fst, sst = p.retrieve_range(str(tmp_path / "nowhere"), fragd, size, off, length)
    assert not ok and out is None and sst[2] == 1 and fst == bytes(120)


def test_retrieve_range_three_windows_failed_middle(stored, tmp_path, monkeypatch):
    """A range over segments 1 .. 9 in windows of 4, 4 and 1 touched segments; a segment of the middle
    window has too few files: the caller's buffer is untouched, the other windows still report."""
    p, buf, fragd, d = stored
    size = len(buf)
    off, length = FSEG + 100, 8 * FSEG + 200
    monkeypatch.setenv("DEOSS_RT_WINDOW_BYTES", str(4 * FSEG))
    monkeypatch.setenv("DEOSS_FP_SLOT_BYTES", str(3 * (FSEG // 4)))   # 3 fragments per slot: slots are reused
    fd = _fragment_dir(stored, tmp_path)
    ok, out, fst, sst = p.retrieve_range(str(fd), fragd, size, off, length)
    assert ok and out == buf[off:off + length] and sst == bytes(10)
    for j in range(3, 12):
        os.unlink(fd / _name(fragd, 6, j))
    dst = ctypes.create_string_buffer(bytes([0x5A]) * length, length)
    ok, out, fst, sst = p.retrieve_range(str(fd), fragd, size, off, length, out=dst)
    assert not ok and out is None and dst.raw == bytes([0x5A]) * length
    assert list(sst) == [1 if s == 6 else 0 for s in range(10)]
    rows = _rows(fst)
    assert rows[0] == [ABSENT] * 12 and rows[1] == [USED] * 4 + [ABSENT] * 8 and rows[9][0] == USED
    assert len(os.listdir(fd)) == len(set(_name(fragd, s, j) for s in range(10) for j in range(12))) - 9


def test_restore_range_mirror_with_a_cipher(ctx, tmp_path):
    """Processor.FullProcessingWindows(file, cipher, savedir), then RestoreRange of ranges of the
    plaintext, with needed files deleted; a wrong cipher is an error, not bytes."""
    from deoss_amd.process import Processor
    key = "k" * 24
    p = Processor(ctx, 4, 8, FSEG)
    try:
        size = 5 * (FSEG - 16) + 777
        buf = _bytes(size, 24)
        src = tmp_path / "upload"
        src.write_bytes(buf)
        info, fid, err = p.FullProcessingWindows(str(src), key, str(tmp_path / "frags"))
        assert err is None and len(info) == 6
        for off, length in ((0, 1), (size - 1, 1), (3 * (FSEG - 16) - 5, 4100), (0, size)):
            data, err = p.RestoreRange(str(tmp_path / "frags"), info, size, off, length, key)
            assert err is None and data == buf[off:off + length], (off, length)
        os.unlink(info[2].FragmentHash[0])
        os.unlink(info[2].FragmentHash[5])
        off = 2 * (FSEG - 16) + 50
        data, err = p.RestoreRange(str(tmp_path / "frags"), info, size, off, 300, key)
        assert err is None and data == buf[off:off + 300]
        data, err = p.RestoreRange(str(tmp_path / "frags"), info, size, off, 300, "w" * 24)
        assert data is None and "wrong cipher" in str(err)
        data, err = p.RestoreRange(str(tmp_path / "frags"), info, size, size, 1, key)
        assert data is None and err.code == -2
        left = set(os.listdir(tmp_path / "frags"))
        assert left == {os.path.basename(f) for s in info for f in s.FragmentHash + [s.SegmentHash]} - {
            os.path.basename(info[2].FragmentHash[0]), os.path.basename(info[2].FragmentHash[5])}
    finally:
        p.close()


def test_module_level_restore_range(tmp_path):
    """The module-level mirrors at chain sizes: FullProcessing, then RestoreRange of 1 MiB inside a data
    fragment whose file is gone."""
    from deoss_amd.process import FullProcessing, RestoreRange
    buf = _bytes((25 << 20) + 321, 5)
    src = tmp_path / "upload"
    src.write_bytes(buf)
    info, fid, err = FullProcessing(str(src), "", str(tmp_path / "frags"))
    assert err is None and len(info) == 1
    off = (9 << 20) + 17
    data, err = RestoreRange(str(tmp_path / "frags"), info, len(buf), off, 1 << 20)
    assert err is None and data == buf[off:off + (1 << 20)]
    os.unlink(info[0].FragmentHash[1])
    data, err = RestoreRange(str(tmp_path / "frags"), info, len(buf), off, 1 << 20)
    assert err is None and data == buf[off:off + (1 << 20)]
    for j in range(4, 12):
        os.unlink(info[0].FragmentHash[j])
    data, err = RestoreRange(str(tmp_path / "frags"), info, len(buf), off, 1 << 20)
    assert data is None and err is not None
