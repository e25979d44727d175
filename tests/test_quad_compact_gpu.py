"""The compact K1Q leaf kernel, leaf_kernel_quad<TABLE, ALIGNED, COMPACT = true>
(deoss_amd/csrc/merkle_kernels.hpp), at its stage, mix and entry edges.

launch_leaves_t takes the compact kernel when K1Q is chosen and the grid has more than two
workgroups per CU: 16 x CUs < leaves <= 32 x CUs in auto mode.  It has a ring of two stages, its own
producer loop and its own run / per-block arithmetic, none of which the host test of quad_ring.hpp
steps.  Every case here has its leaf count in that range (taken from the device's CU count, never a
literal), every leaf digest is checked against hashlib.sha256 and every root against the CPU oracle.

Which entry reaches which of the four compact instances <TABLE, ALIGNED>:

  <false, true>    root_device_async, a chunk that is a multiple of 16 at a 16-byte aligned pointer
                   (test_uniform_walk at offset 0); root_buffer_ptr, a chunk that is a multiple of
                   16 (test_from_chaining_state[aligned])
  <false, false>   root_device_async, any other chunk or a pointer off by 1 (test_uniform_walk,
                   test_partial_last_workgroup, test_short_last_chunk); root_buffer_ptr with an odd
                   chunk (test_from_chaining_state[unaligned])
  <true, true>     root_chunks (host chunks are packed at 256-byte starts: test_table_mixed_waves);
                   Processor.process_buffer (test_full_processing); root_batch_device_async with
                   every object 16-byte aligned (test_table_one_leaf_objects[*-aligned])
  <true, false>    root_batch_device_async with object i at offset i % 16
                   (test_table_one_leaf_objects[*-unaligned])

The mixed waves of the table-mode cases are CATALOGUE below; tests/test_quad_compact_shape.py
checks on the CPU, with the model of the consumer's loop in tests/quad_compact_model.py, that they
take every path of that loop, and that the uniform lengths have the block counts claimed here.
"""
import hashlib

import pytest

from oracle import py_root_chunks

pytestmark = pytest.mark.gpu

# Uniform walk: len -> (len // 64 full blocks, len % 64 tail bytes).  Full blocks 0, 1, 7, 8, 9, 15,
# 16, 17, 24, 25: no stage, the per-block path alone, one / two / three whole stages (the third in
# ring slot 0 again), each followed by no, one or seven blocks.  Tails 0 (padding block alone), 55
# (the longest tail with the length in the same block), 56 (the shortest with a second padding
# block) and 63.  The multiples of 16 run the ALIGNED instance at pointer offset 0.
UNIFORM = {63: (0, 63), 64: (1, 0), 119: (1, 55), 120: (1, 56), 503: (7, 55), 512: (8, 0), 575: (8, 63),
           576: (9, 0), 1015: (15, 55), 1024: (16, 0), 1079: (16, 55), 1088: (17, 0), 1536: (24, 0),
           1591: (24, 55), 1592: (24, 56), 1600: (25, 0)}

# Table mode: one wave (8 leaves, one workgroup) per row, bytes per leaf.
CATALOGUE = [
    [2039, 2551, 1527, 1015, 503, 2103, 0, 1591],      # the x-stage test's wave: no register run at all
    [503, 1015, 1527, 567, 1079, 439, 440, 952],
    [64, 128, 192, 256, 320, 384, 448, 512],           # 1..8 blocks
    [1024, 1089, 1207, 1272, 1343, 1352, 1424, 1512],  # 16..23 blocks, tails 0, 1, 55, 56, 63, 8, 16, 40
    [4160, 1088, 1088, 1024, 1024, 576, 575, 0],
    [1, 55, 56, 63, 64, 119, 120, 2560],
    [1600, 1600, 1600, 1600, 1600, 1600, 1600, 520],
    [3000, 1536, 1537, 700, 2999, 100, 1471, 2048],
    # 9..16 blocks: one stage, then leaves end after 1..7 blocks of a stage in ring slot 1
    [577, 695, 760, 831, 832, 904, 976, 1064],
    # a run of three stages from slot 0 in a mixed wave, leaves that end after 3, 4 and 5 blocks in slot 1,
    # then runs of one and two stages for the two long leaves
    [1536, 1729, 1847, 1912, 2623, 1544, 3600, 0],
]
PARTIAL = [1015, 700, 64]                               # the last workgroup: 3 leaves, 5 lanes beyond nleaves


def table_lengths(nleaves):
    """The leaf lengths of the table-mode cases: the catalogue cycled over nleaves // 8 waves, wave
    w rotated left by (w + cycle) % 8 lanes -- so each catalogue wave comes back in every rotation
    and its longest leaf sits on every lane position in turn -- then the partial last wave."""
    full, rest = divmod(nleaves, 8)
    assert rest == len(PARTIAL)
    out = []
    for w in range(full):
        wave = CATALOGUE[w % len(CATALOGUE)]
        r = (w % len(CATALOGUE) + w // len(CATALOGUE)) % 8
        out += wave[r:] + wave[:r]
    return out + PARTIAL


def object_lengths(nleaves):
    """The same waves as one-leaf objects: an object cannot be empty, so an empty leaf becomes one
    byte (no full block either: the same path through the consumer's loop)."""
    return [max(n, 1) for n in table_lengths(nleaves)]


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _cus():
    """The attribute init_device reads (hipDeviceAttributeMultiprocessorCount)."""
    return _torch().cuda.get_device_properties(0).multi_processor_count


def _compact(ctx, nleaves, auto=False):
    """nleaves is in the compact kernel's range: more than two, at most four workgroups per CU."""
    assert 16 * _cus() < nleaves <= 32 * _cus(), (nleaves, _cus())
    if auto:
        assert ctx.leaf_kernel_for(nleaves) == "quad"
    return nleaves


def _one_device(ctx):
    """A host-memory call ran whole on one device (sharded, each device would see fewer leaves)."""
    assert len(ctx.last_call_devices()[0]) == 1


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


def _sha(data, chunk):
    view = memoryview(data)
    return b"".join(hashlib.sha256(view[o:o + chunk]).digest() for o in range(0, len(data), chunk))


def _want(oracle_lib, data, chunk):
    """(leaf digests by hashlib, root by the oracle, whose leaves must be hashlib's)."""
    leaves, root = oracle_lib.root_buffer(data, chunk, nthreads=8)
    assert leaves == _sha(data, chunk)
    return leaves, root


@pytest.fixture
def quad(ctx):
    ctx.set_leaf_kernel("quad")
    yield ctx
    ctx.set_leaf_kernel("auto")


@pytest.fixture(params=["quad", "auto"])
def either(ctx, request):
    """K1Q forced, then chosen by the library (both take the compact kernel in this range)."""
    ctx.set_leaf_kernel(request.param)
    yield ctx
    ctx.set_leaf_kernel("auto")


# ------------------------------------------------------------------------------- uniform mode
@pytest.mark.parametrize("chunk", sorted(UNIFORM))
def test_uniform_walk(quad, oracle_lib, chunk):
    """16 x CUs + 9 leaves of one length (a last workgroup of one leaf), at pointer offsets 0 and 1."""
    nleaves = _compact(quad, 16 * _cus() + 9)
    data = oracle_lib.splitmix_bytes(chunk * nleaves, 9100 + chunk)
    want = _want(oracle_lib, data, chunk)
    for offset in (0, 1):
        keep, ptr = _dev(data, offset)
        assert _root_dev(quad, ptr, len(data), chunk) == want, (chunk, offset)


@pytest.fixture(scope="module")
def run_and_tail(oracle_lib):
    """16 x CUs + 8 leaves of 1,079 B (two whole stages, then the padded tail) on the device."""
    chunk = 1079
    data = oracle_lib.splitmix_bytes(chunk * (16 * _cus() + 8), 9200)
    keep, ptr = _dev(data)
    yield chunk, data, ptr
    del keep


@pytest.mark.parametrize("r", [1, 2, 3, 5, 6, 7, 8])
def test_partial_last_workgroup(quad, oracle_lib, run_and_tail, r):
    """A last workgroup of r leaves: 8 - r consumer groups beyond nleaves, and the fused tree levels
    (lds_reduce) over 1..8 nodes, odd counts duplicated."""
    chunk, data, ptr = run_and_tail
    nleaves = _compact(quad, 16 * _cus() + r)
    part = data[:chunk * nleaves]
    assert _root_dev(quad, ptr, len(part), chunk) == _want(oracle_lib, part, chunk)


@pytest.fixture(scope="module")
def four_stages(oracle_lib):
    """16 x CUs + 9 leaves of 2,039 B (31 full blocks: three stages and seven blocks) on the device."""
    chunk = 2039
    data = oracle_lib.splitmix_bytes(chunk * (16 * _cus() + 9), 9300)
    keep, ptr = _dev(data)
    yield chunk, data, ptr, _sha(data, chunk)
    del keep


@pytest.mark.parametrize("last", [1, 63, 64, 503, 512, 520, 1527, 2038])
def test_short_last_chunk(quad, oracle_lib, four_stages, last):
    """A shorter last chunk that ends in stage 0, 1, 2 or 3, at a stage boundary or inside a stage:
    as the eighth leaf of a full last workgroup (the wave's runs end where it ends, and it keeps
    its result while seven leaves run on) and alone in the last workgroup."""
    chunk, data, ptr, digests = four_stages
    for extra in (8, 9):
        nleaves = _compact(quad, 16 * _cus() + extra)
        part = data[:chunk * (nleaves - 1) + last]
        want_leaves = digests[:32 * (nleaves - 1)] + hashlib.sha256(part[chunk * (nleaves - 1):]).digest()
        want_root = oracle_lib.root_buffer(part, chunk, nthreads=8)[1]
        assert _root_dev(quad, ptr, len(part), chunk) == (want_leaves, want_root), (extra, last)


# --------------------------------------------------------------------------------- table mode
@pytest.fixture(scope="module")
def mixed_waves(oracle_lib):
    """The rotated catalogue cycled to 16 x CUs + 3 leaves (the last wave is the partial one), as
    chunks (empty ones included) and as one-leaf objects (one byte for an empty one)."""
    nleaves = 16 * _cus() + 3
    lens, olens = table_lengths(nleaves), object_lengths(nleaves)
    data = oracle_lib.splitmix_bytes(sum(olens), 9400)
    chunks, objs, at = [], [], 0
    for n, m in zip(lens, olens):
        chunks.append(data[at:at + n])
        objs.append(data[at:at + m])
        at += m
    leaves = b"".join(hashlib.sha256(c).digest() for c in chunks)
    got_leaves, root = oracle_lib.root_chunks(chunks, nthreads=8)
    assert got_leaves == leaves
    small = py_root_chunks(chunks[:11])     # the C oracle against the plain-Python one on a short list
    assert oracle_lib.root_chunks(chunks[:11]) == (b"".join(small[0]), small[1])
    roots = [hashlib.sha256(2 * hashlib.sha256(o).digest()).digest() for o in objs]
    return chunks, leaves, root, objs, roots


def test_table_mixed_waves(either, mixed_waves):
    """root_chunks over the mixed waves: every leaf digest and the root."""
    chunks, leaves, root, _, _ = mixed_waves
    _compact(either, len(chunks), auto=True)
    assert either.root_chunks(chunks) == (leaves, root)
    _one_device(either)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
def test_table_one_leaf_objects(either, mixed_waves, aligned):
    """The same waves as one-leaf objects packed into one device tensor, addressed by pointer
    arithmetic: every start 16-byte aligned, then object i at offset i % 16.  A one-leaf object's
    root is its leaf digest paired with itself."""
    import numpy as np
    torch = _torch()
    _, _, _, objs, roots = mixed_waves
    _compact(either, len(objs), auto=True)
    starts, at = [], 0
    for i, o in enumerate(objs):
        at = (at + 15) // 16 * 16 + (0 if aligned else i % 16)
        starts.append(at)
        at += len(o)
    host = np.zeros(at + 64, dtype=np.uint8)
    for s, o in zip(starts, objs):
        host[s:s + len(o)] = np.frombuffer(o, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 16 == 0
    out = torch.zeros(32 * len(objs), dtype=torch.uint8, device="cuda")
    either.root_batch_device_async([dev.data_ptr() + s for s in starts], [len(o) for o in objs], 1 << 20,
                                   out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = bytes(out.cpu().numpy())
    assert [got[32 * i:32 * i + 32] for i in range(len(objs))] == roots


# ------------------------------------------------------------------------------ FullProcessing
@pytest.mark.parametrize("segment", [1984, 2048, 2112, 4096])
def test_full_processing(ctx, oracle_lib, segment):
    """The production route, auto mode: process_segments hashes nseg segments and their 12 x nseg
    fragments in one table-mode launch.  Segment / fragment full blocks 31 / 7, 32 / 8, 33 / 8 and
    64 / 16; nseg % 8 in {2, 5}, so one workgroup holds the last segments beside the first
    fragments; the object ends 17 B into its last segment."""
    from deoss_amd.process import Processor
    cus = _cus()
    nseg = next(n for n in range((16 * cus) // 13 + 1, (32 * cus) // 13 + 1) if n % 8 in (2, 5))
    assert 13 * nseg > 16 * cus and (segment // 64, segment // 4 // 64) in ((31, 7), (32, 8), (33, 8), (64, 16))
    _compact(ctx, 13 * nseg, auto=True)
    buf = oracle_lib.splitmix_bytes((nseg - 1) * segment + 17, 9500 + segment)
    want = oracle_lib.full_processing(buf, segment, 4, 8, want_frags=True, nthreads=8)
    view = memoryview(buf)
    assert want[0][:32 * (nseg - 1)] == b"".join(
        hashlib.sha256(view[s * segment:(s + 1) * segment]).digest() for s in range(nseg - 1))
    p = Processor(ctx, 4, 8, segment)
    try:
        seg, frag, fid, frags = p.process_buffer(buf, want_frags=True)
    finally:
        p.close()
    _one_device(ctx)
    assert seg == want[0]          # segment names
    assert frag == want[1]         # fragment names
    assert fid == want[2]
    assert frags == want[3]        # fragment bytes


# ---------------------------------------------------------------------- chaining state in HBM
@pytest.fixture(scope="module")
def host_buffer(oracle_lib):
    """A pageable host buffer just above 256 MiB of splitmix64 bytes."""
    torch = _torch()
    n = 16 * _cus() + 9
    cap = (n * (((1 << 28) // n) // 64 * 64 + 64 * 9 + 55) + 7) // 8 * 8
    t = torch.empty(cap, dtype=torch.uint8)
    oracle_lib.fill_splitmix_ptr(t.data_ptr(), 0, cap, 9600)
    return t


@pytest.mark.parametrize("tail", [55, 48], ids=["unaligned", "aligned"])
def test_from_chaining_state(quad, oracle_lib, host_buffer, tail):
    """root_buffer_ptr above the stripe budget (kStripeBudget, 256 MiB): every launch absorbs one
    stripe of whole blocks of every leaf, and every launch after the first starts from the leaf's
    chaining state in HBM (la.state, byte_off != 0).  The chunk is larger than the stripe width
    W = (2^28 / n) // 64 * 64 and no multiple of 64; odd for the unaligned instance, a multiple of
    16 for the ALIGNED one.  The last leaf (1,000 B) ends in the first stripe and sits through the
    rest."""
    n = _compact(quad, 16 * _cus() + 9)
    W = ((1 << 28) // n) // 64 * 64
    chunk = W + 64 * 9 + tail
    length = (n - 1) * chunk + 1000
    assert chunk > W and chunk % 64 and (chunk % 16 == 0) == (tail == 48)
    assert (1 << 28) < length <= host_buffer.numel()
    want = oracle_lib.root_buffer_ptr(host_buffer.data_ptr(), length, chunk, nthreads=8, want_leaves=True)
    got = quad.root_buffer_ptr(host_buffer.data_ptr(), length, chunk, want_leaves=True)
    _one_device(quad)
    assert got == want
