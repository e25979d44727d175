"""K1Q's register path runs the blocks of a ring stage as one step stream: the a-triple's last two
rounds of a block share their steps with the e-triple's first two of the next, and the stream
fills and drains once per stage (deoss_amd/csrc/merkle_kernels.hpp, DM_QS_LINKQ).  These tests
walk the block counts at which that path starts, links, drains and hands over to the per-block
path, nb = (len + 8) // 64 + 1:

  nb = 8          one stage: fill and drain only
  nb = 16, 24     two and three stages: the chaining words carried across the stage barrier
  nb = 9, 17      a run of whole stages followed by the per-block path
  nb = 7          the per-block path only

in full and partly empty workgroups, alone and mixed in one wave, through uniform and table mode,
aligned and unaligned pointers, the host-buffer path (whose stripes enter a run mid-leaf with the
chaining state from HBM) and the compact kernel.  Every leaf digest is checked against
hashlib.sha256 and every root against the CPU oracle.
"""
import hashlib

import pytest

from oracle import py_root_chunks, split_chunks

pytestmark = pytest.mark.gpu

# len -> nb; the second of each pair is the longest length with that block count, and the third
# a multiple of 16 (the ALIGNED kernels need chunk % 16 == 0)
LENS = {7: (376, 439, 384), 8: (440, 503, 448), 9: (504, 567, 512), 16: (952, 1015, 1008),
        17: (1016, 1079, 1024), 24: (1464, 1527, 1472)}


for _nb, _lens in LENS.items():
    assert all((n + 8) // 64 + 1 == _nb for n in _lens) and _lens[2] % 16 == 0


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _dev(data: bytes, offset: int = 0):
    import numpy as np
    torch = _torch()
    t = torch.zeros(len(data) + 64 + offset, dtype=torch.uint8, device="cuda")
    t[offset:offset + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    return t, t.data_ptr() + offset


def _root_dev(ctx, ptr, length, chunk):
    torch = _torch()
    n = (length + chunk - 1) // chunk
    r = torch.zeros(32, dtype=torch.uint8, device="cuda")
    lv = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    ctx.root_device_async(ptr, length, chunk, r.data_ptr(), lv.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return bytes(lv.cpu().numpy()), bytes(r.cpu().numpy())


def _want(chunks):
    leaves, root = py_root_chunks(chunks)
    assert leaves == [hashlib.sha256(c).digest() for c in chunks]
    return b"".join(leaves), root


@pytest.fixture
def quad(ctx):
    ctx.set_leaf_kernel("quad")
    yield ctx
    ctx.set_leaf_kernel("auto")


@pytest.mark.parametrize("nb", sorted(LENS))
def test_uniform_objects(quad, oracle_lib, nb):
    """1, 8 and 9 leaves of one length: a partly empty, a full and a second workgroup; device
    pointers 16-byte aligned (ALIGNED for the chunk that is a multiple of 16) and off by 1."""
    for chunk in LENS[nb]:
        for nleaves in (1, 8, 9):
            data = oracle_lib.splitmix_bytes(chunk * nleaves, 7100 + nb)
            want = _want([data[i * chunk:(i + 1) * chunk] for i in range(nleaves)])
            for offset in (0, 1):
                keep, ptr = _dev(data, offset)
                assert _root_dev(quad, ptr, len(data), chunk) == want, (chunk, nleaves, offset)


@pytest.mark.parametrize("chunk", [1015, 1008, 1527, 567])
def test_short_last_chunk(quad, oracle_lib, chunk):
    """A uniform object whose last chunk is shorter, so one wave mixes two lengths: the last
    leaf ends in an earlier stage (or on the per-block path) and must keep its result."""
    for nleaves in (8, 9, 12):
        for last in (1, 439, 440, 503, 504, 952, 1000):
            if last >= chunk:
                continue
            data = oracle_lib.splitmix_bytes(chunk * (nleaves - 1) + last, 7200 + last)
            chunks = [data[i * chunk:(i + 1) * chunk] for i in range(nleaves)]
            assert len(chunks[-1]) == last
            keep, ptr = _dev(data)
            assert _root_dev(quad, ptr, len(data), chunk) == _want(chunks), (chunk, nleaves, last)


# every block-count class in one wave (8 leaves per wave), in several orders, with empty and
# one-block leaves among them
MIXED = [503, 1015, 1527, 567, 1079, 439, 440, 952,
         376, 1464, 1016, 504, 1527, 0, 1, 1015,
         1527, 1527, 1527, 1527, 1527, 1527, 1527, 440,
         439, 1079, 55, 503, 2047, 2039, 4095, 1015,
         1015]


def test_mixed_lengths_table_mode(quad, oracle_lib):
    """Table mode (one address per leaf), host and device entry points: a ragged batch."""
    torch = _torch()
    chunks = [oracle_lib.splitmix_bytes(n, 7300 + i) for i, n in enumerate(MIXED)]
    want_leaves, want_root = _want(chunks)
    assert quad.root_chunks(chunks) == (want_leaves, want_root)
    # each as an object of its own: root_batch and its device twin (a one-leaf object's root is
    # its leaf paired with itself)
    objs = [c for c in chunks if c]
    roots = [hashlib.sha256(2 * hashlib.sha256(c).digest()).digest() for c in objs]
    assert [oracle_lib.root_buffer(o, 1 << 20)[1] for o in objs] == roots   # the oracle agrees with hashlib
    assert quad.root_batch(objs, 1 << 20) == roots
    keep = [_dev(o, i % 3) for i, o in enumerate(objs)]
    out = torch.zeros(32 * len(objs), dtype=torch.uint8, device="cuda")
    quad.root_batch_device_async([p for _, p in keep], [len(o) for o in objs], 1 << 20, out.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = bytes(out.cpu().numpy())
    assert [got[32 * i:32 * i + 32] for i in range(len(objs))] == roots
    # multi-leaf objects of mixed sizes through root_batch: leaves of several objects share a wave
    sizes = [1015 * 3 + 440, 503, 1527 * 2, 1015 * 8, 567 * 5 + 1, 1079, 1015 * 9 + 952]
    multi = [oracle_lib.splitmix_bytes(n, 7400 + i) for i, n in enumerate(sizes)]
    for chunk in (1015, 1008, 1527):
        # roots only come back: each must be the tree over the hashlib digests of the object's leaves
        want = [_want(split_chunks(o, chunk))[1] for o in multi]
        assert want == [oracle_lib.root_buffer(o, chunk)[1] for o in multi]
        assert quad.root_batch(multi, chunk) == want, chunk


def test_host_buffer(quad, oracle_lib):
    """root_buffer: one contiguous step for a small buffer; above the stripe budget (256 MiB) each
    leaf advances a stripe at a time, its chaining state carried in HBM, so a run of whole stages
    starts mid-leaf from a loaded state (stripe widths are whole blocks, not whole stages)."""
    small = oracle_lib.splitmix_bytes(1015 * 9 + 503, 7500)
    for chunk in (1015, 1008):
        want = _want(split_chunks(small, chunk))
        assert want == oracle_lib.root_buffer(small, chunk)
        assert quad.root_buffer(small, chunk) == want
    chunk = (30 << 20) + 1015          # odd: the unaligned kernels
    big = oracle_lib.splitmix_bytes(8 * chunk + (3 << 20) + 440, 7501)   # 9 leaves, 273 MiB
    leaves, root = quad.root_buffer(big, chunk)
    want_leaves, want_root = oracle_lib.root_buffer(big, chunk, nthreads=8)
    assert (leaves, root) == (want_leaves, want_root)
    view = memoryview(big)
    assert leaves == b"".join(hashlib.sha256(view[i * chunk:(i + 1) * chunk]).digest() for i in range(9))


def test_compact_kernel(quad, oracle_lib):
    """4,104 leaves of 1,015 B: 513 workgroups, more than two per CU, so the compact ring."""
    chunk, nleaves = 1015, 4104
    data = oracle_lib.splitmix_bytes(chunk * nleaves, 7600)
    chunks = [data[i * chunk:(i + 1) * chunk] for i in range(nleaves)]
    want_leaves = b"".join(hashlib.sha256(c).digest() for c in chunks)
    want_root = oracle_lib.root_buffer(data, chunk, nthreads=8)[1]
    for offset in (0, 1):
        keep, ptr = _dev(data, offset)
        assert _root_dev(quad, ptr, len(data), chunk) == (want_leaves, want_root), offset
    chunk = 1008                       # ALIGNED
    data = data[:chunk * nleaves]
    chunks = [data[i * chunk:(i + 1) * chunk] for i in range(nleaves)]
    keep, ptr = _dev(data)
    assert _root_dev(quad, ptr, len(data), chunk) == (
        b"".join(hashlib.sha256(c).digest() for c in chunks), oracle_lib.root_buffer(data, chunk, nthreads=8)[1])
