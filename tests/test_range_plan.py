"""CPU tests of the range plan through the library (dm_range_plan loads and runs without a GPU; the
rule is deoss_amd/csrc/range_plan.hpp, the same one dm_restore_range_buffer and dm_retrieve_range
use), and of how the ranged restore fails without a GPU.

The plan is compared with a brute-force model written here: every plaintext byte of the range is
mapped to its segment, its ciphertext block, that block's predecessor and the data fragments that
hold them.  Geometry small enough to be exhaustive: segment = 128, k = 4 (32-byte fragments, two AES
blocks each), every size of SIZES with the segment count it ends in, with and without a cipher, both
settings of DM_RANGE_NO_PADDING_CHECK, every (off, len) with off + len <= size."""
import ctypes

import pytest

SEG, K = 128, 4
FRAG, NBLK = SEG // K, SEG // 16
SIZES = (1, 112, 113, 128, 129, 300, 384)
NO_PAD, PREV_IV, CHECK_PAD, PAD_ONLY = 8, 1, 2, 4


@pytest.fixture(scope="module")
def lib():
    from deoss_amd import build as b
    b.build(verbose=False)
    from deoss_amd import load_library
    return load_library()


class Planner:
    """dm_range_plan with arrays large enough for every case here, one call per plan."""

    def __init__(self, lib):
        from deoss_amd._lib import RangeWindow
        self.lib = lib
        self.need = ctypes.create_string_buffer(64)
        self.win = (RangeWindow * 16)()
        self.seg0, self.nt, self.nw = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()

    def __call__(self, size, nseg, cipher, off, length, flags, segment=SEG, k=K):
        rc = self.lib.dm_range_plan(size, nseg, segment, k, int(cipher), off, length, flags, ctypes.byref(self.seg0),
                                    ctypes.byref(self.nt), self.need, 64, self.win, 16, ctypes.byref(self.nw))
        if rc != 0:
            return rc, (self.lib.dm_last_error(None) or b"").decode()
        nt = self.nt.value
        return 0, (self.seg0.value, nt, self.need.raw[:nt * k],
                   [(w.seg, w.first, w.bytes, w.flags) for w in self.win[:self.nw.value]])


def expected(need, blocks, seg0, cipher, flags):
    """The plan the model's per-byte findings amount to.  need: {segment: set of fragments}; blocks:
    {segment: set of plaintext blocks (cipher) or bytes (none)} of the range."""
    segs = sorted(need)
    need = {s: set(v) for s, v in need.items()}
    wins = []
    for s in segs:
        lo, hi = min(blocks[s]), max(blocks[s])
        assert blocks[s] == set(range(lo, hi + 1))      # a range is contiguous within a segment
        if not cipher:
            wins.append((s, lo, hi - lo + 1, 0))
            continue
        iv = PREV_IV if lo == 0 else 0
        # the padding block (the segment's last) is checked on the first touched segment, and wherever
        # the range reaches the last data fragment anyway
        if (s == seg0 and not flags & NO_PAD) or (K - 1) in need[s]:
            need[s].add(16 * (NBLK - 1) // FRAG)
            if hi == NBLK - 2:      # the padding block follows the range's last block
                wins.append((s, 16 * lo, 16 * (hi - lo + 2), iv | CHECK_PAD))
                continue
            need[s].add(16 * (NBLK - 2) // FRAG)   # its predecessor block
            wins.append((s, 16 * lo, 16 * (hi - lo + 1), iv))
            wins.append((s, 16 * (NBLK - 2), 32, CHECK_PAD | PAD_ONLY))
        else:
            wins.append((s, 16 * lo, 16 * (hi - lo + 1), iv))
    mask = bytes(int(j in need[s]) for s in segs for j in range(K))
    return segs[0], len(segs), mask, wins


@pytest.mark.parametrize("cipher", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_plan_matches_the_brute_force_model(lib, size, cipher):
    plan = Planner(lib)
    piece = SEG - 16 if cipher else SEG
    nseg = (size + piece - 1) // piece
    cases = 0
    for off in range(size):
        need, blocks = {}, {}
        for length in range(1, size - off + 1):
            # the model, one more byte: plaintext byte x -> segment, block, predecessor, fragments
            x = off + length - 1
            s, o = divmod(x, piece)
            if cipher:
                b = o // 16
                blocks.setdefault(s, set()).add(b)
                need.setdefault(s, set()).add(16 * b // FRAG)
                if b > 0:                                   # block 0's predecessor is the IV
                    need[s].add(16 * (b - 1) // FRAG)
            else:
                blocks.setdefault(s, set()).add(o)
                need.setdefault(s, set()).add(o // FRAG)
            for flags in (0, NO_PAD):
                rc, got = plan(size, nseg, cipher, off, length, flags)
                assert rc == 0, (off, length, flags, got)
                want = expected(need, blocks, off // piece, cipher, flags)
                assert got == want, (size, cipher, off, length, flags)
                cases += 1
    assert cases == size * (size + 1)   # every (off, len), both flag settings: none skipped


def test_a_range_starting_in_a_fragments_first_block_needs_the_fragment_before(lib):
    """The case the predecessor rule exists for, spelled out: piece offset 32 is the first block of
    fragment 1; decrypting it needs the last block of fragment 0."""
    plan = Planner(lib)
    rc, (seg0, nt, need, wins) = plan(300, 3, True, 112 + 32, 4, NO_PAD)
    assert (rc, seg0, nt) == (0, 1, 1) and need == bytes([1, 1, 0, 0]) and wins == [(1, 32, 16, 0)]
    rc, (_, _, need, wins) = plan(300, 3, False, 128 + 32, 4, 0)
    assert need == bytes([0, 1, 0, 0]) and wins == [(1, 32, 4, 0)]
    # with the padding check the first touched segment also gets its last fragment and a two-block window
    rc, (_, _, need, wins) = plan(300, 3, True, 112 + 32, 4, 0)
    assert need == bytes([1, 1, 0, 1]) and wins == [(1, 32, 16, 0), (1, 96, 32, CHECK_PAD | PAD_ONLY)]


def test_first_call_learns_the_counts(lib):
    seg0, nt, nw = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    rc = lib.dm_range_plan(300, 3, SEG, K, 1, 5, 250, 0, ctypes.byref(seg0), ctypes.byref(nt), None, 0, None, 0,
                           ctypes.byref(nw))
    assert (rc, seg0.value, nt.value, nw.value) == (0, 0, 3, 3)
    need = ctypes.create_string_buffer(12)
    rc = lib.dm_range_plan(300, 3, SEG, K, 1, 5, 250, 0, ctypes.byref(seg0), ctypes.byref(nt), need, 11, None, 0,
                           ctypes.byref(nw))
    assert rc == -2 and b"do not fit" in lib.dm_last_error(None)
    from deoss_amd.merkle import range_plan
    assert range_plan(300, 3, SEG, K, 5, 250, cipher=True)[:2] == (0, 3)


def test_plan_errors(lib):
    plan = Planner(lib)
    for cipher in (False, True):
        piece = SEG - 16 if cipher else SEG
        for args in ((300, 3, cipher, 5, 0, 0), (300, 3, cipher, 299, 2, 0), (300, 3, cipher, 300, 1, 0),
                     (300, 3, cipher, 2**64 - 2, 5, 0), (300, 3, cipher, 5, 2**64 - 3, 0)):
            rc, msg = plan(*args)
            assert rc == -2 and "is empty or does not lie in the object's 300 bytes" in msg, (args, msg)
        # a size that does not end in the last of nseg pieces (restore_check's text)
        for size in SIZES:
            right = (size + piece - 1) // piece
            for nseg in range(0, 6):
                rc, msg = plan(size, nseg, cipher, 0, 1, 0)
                if nseg == right:
                    assert rc == 0
                else:
                    assert rc == -2 and msg == "size %d does not end in the last of %d %s of %d bytes" % (
                        size, nseg, "pieces" if cipher else "segments", piece), msg
    rc, msg = plan(1, 1, True, 0, 1, 0, segment=16, k=1)
    assert rc == -2 and msg == "segment size 16 has no room for a block and its padding block"
    assert plan(1, 1, False, 0, 1, 0, segment=16, k=1)[0] == 0
    for segment, k in ((100, 4), (0, 4), (128, 0), (144, 9), (48, 2)):
        rc, msg = plan(1, 1, False, 0, 1, 0, segment=segment, k=k)
        assert rc == -2 and "must be a non-zero multiple of 16 x" in msg, (segment, k, msg)
    assert lib.dm_range_plan(1, 1, SEG, K, 0, 0, 1, 0, None, None, None, 0, None, 0, None) == -2


def test_ranged_restore_fails_loudly_without_a_gpu(lib):
    """Without a visible GPU RestoreRange and Processor() fail with DeossMerkleError (no CPU path),
    as the other mirrors do (test_capi_symbols.py::test_no_gpu_fails_loudly)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from deoss_amd import DeossMerkleError
    from deoss_amd.process import Processor, RestoreRange, SegmentDataInfo
    with pytest.raises(DeossMerkleError):
        Processor()
    seg = SegmentDataInfo("ab" * 32, ["cd" * 32] * 12)
    data, err = RestoreRange("/nonexistent-fragdir", [seg], 100, 5, 10)
    assert data is None and isinstance(err, DeossMerkleError)


def test_the_gpu_fuzz_inputs_are_not_degenerate():
    """The 200 seeded cases of tests/test_range_gpu.py::test_range_fuzz_200_cases, checked here without
    a GPU: every range is non-empty and inside its object, every segment keeps at least k fragments
    (so every pattern can be rebuilt), both cipher settings occur, and a fair share of the cases
    really rebuild a needed data fragment."""
    import test_range_gpu as G
    cases = G.fuzz_cases()
    assert len(cases) == 200 and cases == G.fuzz_cases()      # seeded: the same every time
    rebuilds = 0
    for cipher, off, length, kept in cases:
        size, piece = (G.SIZE_CIPHER, G.P) if cipher else (G.SIZE_PLAIN, G.SEG)
        assert length >= 1 and 0 <= off and off + length <= size
        assert len(kept) == (size + piece - 1) // piece
        assert all(len(set(row)) == len(row) >= G.K and set(row) <= set(range(G.TOTAL)) for row in kept)
        first, last = off // piece, (off + length - 1) // piece
        rebuilds += any(j not in kept[s] for s in range(first, last + 1) for j in range(G.K))
    assert 50 <= sum(c[0] for c in cases) <= 150
    assert rebuilds >= 50
