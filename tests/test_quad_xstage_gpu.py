"""The wide K1Q carries its step stream and its K+W prefetch across ring stages: a run of whole
stages is one stream, the boundary between two stages a DM_QS_LINKQ, the ring three stages deep
with the producer two ahead (deoss_amd/csrc/quad_ring.hpp, quad_run_xstage in merkle_kernels.hpp).
tests/test_quad_overlap_gpu.py covers one to three stages; these tests walk the block counts
nb = (len + 8) // 64 + 1 at which the ring of three wraps:

  nb = 25         three stages then the per-block path
  nb = 32         four stages: the fourth is written into the first one's slot
  nb = 33         the wrap, then the per-block path
  nb = 40         five stages

in full and partly empty workgroups, aligned and unaligned, with a short last chunk that ends in
each stage of a four-stage wave, with eight different lengths in one wave (table mode), and once on
the compact kernel, whose code is unchanged.  Every leaf digest is checked against hashlib.sha256
and every root against the CPU oracle.
"""
import hashlib

import pytest

from oracle import py_root_chunks

pytestmark = pytest.mark.gpu

# nb: (shortest, longest, a multiple of 16 -- the ALIGNED kernels need chunk % 16 == 0)
LENS = {25: (1528, 1591, 1536), 32: (1976, 2039, 1984), 33: (2040, 2103, 2048), 40: (2488, 2551, 2496)}

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
    pointers 16-byte aligned and off by 1."""
    for chunk in LENS[nb]:
        for nleaves in (1, 8, 9):
            data = oracle_lib.splitmix_bytes(chunk * nleaves, 8100 + nb)
            want = _want([data[i * chunk:(i + 1) * chunk] for i in range(nleaves)])
            for offset in (0, 1):
                keep, ptr = _dev(data, offset)
                assert _root_dev(quad, ptr, len(data), chunk) == want, (chunk, nleaves, offset)


@pytest.mark.parametrize("last", [1, 440, 503, 504, 1015, 1016, 1527, 1528, 2000])
def test_short_last_chunk(quad, oracle_lib, last):
    """Chunks of 2,039 B (four stages) and a shorter last one that ends in stage 0, 1, 2 or 3, at a
    stage boundary or inside a stage: the wave's runs end there, and the last leaf keeps its result
    while the others run on."""
    chunk = 2039
    for nleaves in (8, 9):
        data = oracle_lib.splitmix_bytes(chunk * (nleaves - 1) + last, 8200 + last)
        chunks = [data[i * chunk:(i + 1) * chunk] for i in range(nleaves)]
        assert len(chunks[-1]) == last
        keep, ptr = _dev(data)
        assert _root_dev(quad, ptr, len(data), chunk) == _want(chunks), (nleaves, last)


# one wave: its runs end at four different stages, one leaf is empty
MIXED = [2039, 2551, 1527, 1015, 503, 2103, 0, 1591]


def test_mixed_lengths_table_mode(quad, oracle_lib):
    chunks = [oracle_lib.splitmix_bytes(n, 8300 + i) for i, n in enumerate(MIXED)]
    assert quad.root_chunks(chunks) == _want(chunks)


def test_compact_kernel(quad, oracle_lib):
    """4,104 leaves of 2,039 B: 513 workgroups, more than two per CU, so the compact kernel (a ring of
    two stages, one stream per stage)."""
    chunk, nleaves = 2039, 4104
    data = oracle_lib.splitmix_bytes(chunk * nleaves, 8400)
    chunks = [data[i * chunk:(i + 1) * chunk] for i in range(nleaves)]
    want_leaves = b"".join(hashlib.sha256(c).digest() for c in chunks)
    want_root = oracle_lib.root_buffer(data, chunk, nthreads=8)[1]
    keep, ptr = _dev(data)
    assert _root_dev(quad, ptr, len(data), chunk) == (want_leaves, want_root)
