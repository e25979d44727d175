"""GPU tests of restoring many objects in one pass: the keyed AES-CBC decrypt kernel (a key per
chain, ONE launch: dm_aes_cbc_decrypt_keyed_device_async), dm_restore_batch, the DM_BATCH_RESTORE
batcher (dm_batcher_restore) and the Python and C++ mirrors.

Every comparison is bit-exact and the reference is never the code under test: the original object
bytes, oracle_lib.full_processing for fragments and names, tests/cipher_ref.py (plain-Python AES from
FIPS-197: scheme_encrypt, decrypt_blocks, cbc_decrypt_many) for the cipher, the fixtures in
tests/golden/aes_kat.json, and the existing single-object calls as a second witness.

Shapes are the smallest that reach every path of the kernel: 2 blocks (the minimum), 3, and 256 /
257 / 258 around one workgroup's 256 lanes; 10,241 blocks at 64 chains, where rs_grid gives a row 32
workgroups (8,192 blocks), so the stride loop and its prefetch run; 2,049 and 5,000 chains, more
than rs_grid's 8 x CU rows, so a workgroup walks chains whose key and round count change."""
from __future__ import annotations

import ctypes
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cipher_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "aes_kat.json")
KLENS = (16, 24, 32)
SENTINEL = 0xEE
PAD = np.full(16, 0x10, dtype=np.uint8)
VF, VS, VID, VALL = 1, 2, 4, 7   # DM_RESTORE_VERIFY_*
BAD_FRAG, SEG_TOO_FEW, SEG_MISMATCH, SEG_BAD_PADDING = 3, 1, 2, 3


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _key(tag: int, klen: int) -> bytes:
    return bytes((tag * 29 + 37 * i + 11 * klen + 5) & 0xFF for i in range(klen))


def _iv(tag: int) -> bytes:
    return bytes((tag * 53 + 91 * i + 7) & 0xFF for i in range(16))


# ---- the keyed decrypt kernel through the device-level call ----------------------------------------

_rk_cache = {}


def _rk(key: bytes) -> np.ndarray:
    if key not in _rk_cache:
        _rk_cache[key] = R.expand_key(key)
    return _rk_cache[key]


def _decrypt_rows(keys, kidx, blocks: np.ndarray) -> np.ndarray:
    """InvCipher of blocks (n, nb, 16), row c under keys[kidx[c]][0]: cipher_ref.decrypt_blocks with
    the rows of one key length stacked, each row's round keys broadcast over its blocks."""
    n, nb, _ = blocks.shape
    out = np.empty_like(blocks)
    kidx = np.asarray(kidx)
    if len(keys) <= 4:   # few keys: one plain call per key
        for k, (key, _) in enumerate(keys):
            rows = np.flatnonzero(kidx == k)
            if len(rows):
                out[rows] = R.decrypt_blocks(_rk(key), blocks[rows].reshape(-1, 16)).reshape(len(rows), nb, 16)
        return out
    for klen in KLENS:
        rows = np.array([c for c in range(n) if len(keys[kidx[c]][0]) == klen], dtype=np.int64)
        if not len(rows):
            continue
        rk = np.stack([_rk(keys[kidx[c]][0]) for c in rows])            # (rows, nr + 1, 16)
        rk = np.repeat(rk.transpose(1, 0, 2), nb, axis=1)                # (nr + 1, rows * nb, 16)
        out[rows] = R.decrypt_blocks(rk, blocks[rows].reshape(-1, 16)).reshape(len(rows), nb, 16)
    return out


def _make_chains(keys, kidx, nb: int, seed: int):
    """Random ciphertext (n, nb, 16) whose even chains end in a valid padding block without a serial
    encryption -- C_{nb-2} = D(C_{nb-1}) ^ 0x10..10 (the IV takes C_{-1}'s place at nb == 1, never
    here: nb >= 2) -- and whose odd chains do not; the reference plaintext and verdicts."""
    n = len(kidx)
    ct = np.random.default_rng(seed).integers(0, 256, size=(n, nb, 16), dtype=np.uint8)
    even = np.arange(0, n, 2)
    last = _decrypt_rows(keys, kidx, ct[:, nb - 1:nb, :])[:, 0, :]
    ct[even, nb - 2, :] = last[even] ^ PAD
    d = _decrypt_rows(keys, kidx, ct)
    prev = np.empty_like(ct)
    prev[:, 0, :] = np.stack([np.frombuffer(keys[k][1], dtype=np.uint8) for k in kidx])
    prev[:, 1:, :] = ct[:, :-1, :]
    plain = d ^ prev
    ok = (plain[:, nb - 1, :] == PAD).all(axis=1).astype(np.uint8)
    assert ok[even].all() and not ok[1::2].any()
    return ct.reshape(n, nb * 16), plain[:, :nb - 1, :].reshape(n, (nb - 1) * 16), ok


def _layout(n: int, nbytes: int, seed: int):
    """Offsets of n ranges of nbytes in one buffer: placed in a shuffled order with gaps of 16, 32 or
    48 sentinel bytes between them."""
    rng = np.random.default_rng(seed)
    off = np.zeros(n, dtype=np.int64)
    pos = 16 * int(rng.integers(1, 4))
    for c in rng.permutation(n):
        off[c] = pos
        pos += nbytes + 16 * int(rng.integers(1, 4))
    return off, pos


def _scatter(rows: np.ndarray, off, size: int) -> np.ndarray:
    host = np.full(size, SENTINEL, dtype=np.uint8)
    idx = (np.asarray(off)[:, None] + np.arange(rows.shape[1])[None, :]).reshape(-1)
    host[idx] = rows.reshape(-1)
    return host


def _pattern(name: str, n: int):
    """(keys, key index of every chain) of a pattern at n chains."""
    if name == "one":
        return [(_key(100, 24), _iv(100))], [0] * n
    if name == "own":
        return [(_key(c, KLENS[c % 3]), _iv(c)) for c in range(n)], list(range(n))
    # "runs": two long runs of one key separated by a single chain of another length.  Beyond
    # rs_grid's 2,048 rows the odd chain sits in the second lap, so the workgroup of row 7 walks
    # key 0, key 1, key 0 (two forced re-reads) while every other row skips the re-read.
    keys = [(_key(101, 32), _iv(101)), (_key(102, 16), _iv(102))]
    at = 2048 + 7 if n > 2048 + 7 else n // 2
    return keys, [1 if c == at else 0 for c in range(n)]


def _run_keyed(ctx, keys, kidx, nb: int, seed: int):
    torch = _torch()
    n = len(kidx)
    ct, want, want_ok = _make_chains(keys, kidx, nb, seed)
    in_off, in_size = _layout(n, 16 * nb, seed + 1)
    out_off, out_size = _layout(n, 16 * (nb - 1), seed + 2)
    src = torch.from_numpy(_scatter(ct, in_off, in_size)).cuda()
    dst = torch.full((out_size + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    pad = torch.full((n + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    chains = [(src.data_ptr() + int(in_off[c]), dst.data_ptr() + int(out_off[c]), kidx[c]) for c in range(n)]
    ctx.aes_cbc_decrypt_keyed_device_async(keys, chains, 16 * nb, pad.data_ptr())
    torch.cuda.synchronize()
    got, got_pad = dst.cpu().numpy(), pad.cpu().numpy()
    expect = np.concatenate([_scatter(want, out_off, out_size), np.full(64, SENTINEL, dtype=np.uint8)])
    if not (got == expect).all():
        bad = int(np.flatnonzero(got != expect)[0])
        raise AssertionError(f"n={n} nb={nb}: first differing output byte at {bad}")
    assert (got_pad[:n] == want_ok).all(), (n, nb, np.flatnonzero(got_pad[:n] != want_ok)[:8])
    assert (got_pad[n:] == SENTINEL).all(), (n, nb)
    assert (src.cpu().numpy() == _scatter(ct, in_off, in_size)).all()   # out of place: the input is untouched


@pytest.mark.parametrize("pattern", ("one", "own", "runs"))
def test_keyed_decrypt_small_shapes(ctx, pattern):
    for n in (1, 2, 3, 64):
        keys, kidx = _pattern(pattern, n)
        for nb in (2, 3, 256, 257, 258):
            _run_keyed(ctx, keys, kidx, nb, 1000 * n + nb)


@pytest.mark.parametrize("pattern", ("own", "runs"))
def test_keyed_decrypt_stride_loop(ctx, pattern):
    keys, kidx = _pattern(pattern, 64)
    _run_keyed(ctx, keys, kidx, 10241, 77)


@pytest.mark.parametrize("pattern", ("one", "own", "runs"))
@pytest.mark.parametrize("n, nb", ((2049, 2), (2049, 3), (5000, 2), (5000, 3)))
def test_keyed_decrypt_more_chains_than_rows(ctx, pattern, n, nb):
    keys, kidx = _pattern(pattern, n)
    _run_keyed(ctx, keys, kidx, nb, n + nb)


def test_keyed_decrypt_sp800_38a_three_keys_one_launch(ctx):
    """SP 800-38A F.2.2 / F.2.4 / F.2.6 (CBC-AES128 / 192 / 256 decrypt) as three chains of one
    launch; a fifth block makes each chain end in a padding block (valid for the first two)."""
    torch = _torch()
    with open(KAT) as f:
        k = json.load(f)["sp800_38a_cbc"]
    iv, pt = bytes.fromhex(k["iv"]), bytes.fromhex("".join(k["plaintext"]))
    cases = k["cases"]
    assert sorted(len(bytes.fromhex(c["key"])) for c in cases) == [16, 24, 32]
    keys = [(bytes.fromhex(c["key"]), iv) for c in cases]
    host = np.zeros((3, 96), dtype=np.uint8)
    for i, c in enumerate(cases):
        ct = np.frombuffer(bytes.fromhex("".join(c["ciphertext"])), dtype=np.uint8)
        host[i, :64] = ct
        host[i, 64:80] = np.frombuffer(R.cbc_encrypt(keys[i][0], iv, pt, pkcs7=True)[64:80], dtype=np.uint8)
    host[2, 64] ^= 1   # the third chain's padding block is damaged
    src = torch.from_numpy(host).cuda()
    dst = torch.full((3, 80), SENTINEL, dtype=torch.uint8, device="cuda")
    pad = torch.full((8,), SENTINEL, dtype=torch.uint8, device="cuda")
    ctx.aes_cbc_decrypt_keyed_device_async(
        keys, [(src.data_ptr() + 96 * i, dst.data_ptr() + 80 * i, i) for i in range(3)], 80, pad.data_ptr())
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    for i, c in enumerate(cases):
        assert got[i, :64].tobytes() == pt, c["section"]
        assert (got[i, 64:] == SENTINEL).all()
    assert pad.cpu().numpy().tolist() == [1, 1, 0] + [SENTINEL] * 5


@pytest.mark.parametrize("nb", (2, 3, 257, 1025))
def test_keyed_decrypt_equals_single_key_kernel(ctx, nb):
    """Per key byte-identical to dm_aes_cbc_decrypt_device_async on the same buffers, three key
    lengths in one keyed launch against three single-key launches."""
    torch = _torch()
    per = 11
    keys = [(_key(110 + i, klen), _iv(110 + i)) for i, klen in enumerate(KLENS)]
    kidx = [c % 3 for c in range(3 * per)]
    ct, _, want_ok = _make_chains(keys, kidx, nb, 5 + nb)
    order = sorted(range(3 * per), key=lambda c: kidx[c])   # chains of one key side by side, a common stride
    src = torch.from_numpy(np.ascontiguousarray(ct[order])).cuda()
    cb, pb = 16 * nb, 16 * (nb - 1)
    a = torch.full((3 * per, pb), SENTINEL, dtype=torch.uint8, device="cuda")
    b = torch.full((3 * per, pb), SENTINEL, dtype=torch.uint8, device="cuda")
    pa = torch.full((3 * per,), SENTINEL, dtype=torch.uint8, device="cuda")
    pbk = torch.full((3 * per,), SENTINEL, dtype=torch.uint8, device="cuda")
    for k in range(3):
        ctx.aes_cbc_decrypt_device_async(keys[k][0], keys[k][1], src.data_ptr() + k * per * cb, cb, cb, per,
                                         a.data_ptr() + k * per * pb, pb, pa.data_ptr() + k * per)
    chains = [(src.data_ptr() + i * cb, b.data_ptr() + i * pb, kidx[order[i]]) for i in range(3 * per)]
    ctx.aes_cbc_decrypt_keyed_device_async(keys, chains, cb, pbk.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(pa, pbk), nb
    assert (pbk.cpu().numpy() == want_ok[order]).all()


def test_keyed_decrypt_argument_checks(ctx):
    from deoss_amd import DeossMerkleError
    from deoss_amd._lib import DM_ERR_INVALID
    torch = _torch()
    src = torch.full((512,), SENTINEL, dtype=torch.uint8, device="cuda")
    dst = torch.full((512,), SENTINEL, dtype=torch.uint8, device="cuda")
    pad = torch.full((16,), SENTINEL, dtype=torch.uint8, device="cuda")
    s, d, p = src.data_ptr(), dst.data_ptr(), pad.data_ptr()
    good = [(_key(1, 16), _iv(1)), (_key(2, 32), _iv(2))]
    with pytest.raises(DeossMerkleError) as e:
        ctx.aes_cbc_decrypt_keyed_device_async([good[0], (bytes(15), _iv(0)), good[1]], [(s, d, 0)], 64, p)
    assert e.value.code == DM_ERR_INVALID
    assert "key 1" in str(e.value) and "cipher must be 16, 24 or 32 bytes" in str(e.value)
    bad_calls = (
        dict(chains=[(s, d, 0), (s + 136, d + 128, 1)]),        # misaligned in
        dict(chains=[(s, d, 0), (s + 128, d + 136, 1)]),        # misaligned out
        dict(chains=[(s, d, 0), (0, d + 128, 1)]),              # null
        dict(chains=[(s, d, 0), (s + 128, d + 128, 2)]),        # key_index == nkeys
        dict(chains=[(s, d, 0), (s + 128, d + 128, 1)], cb=16),  # no room for a padding block
        dict(chains=[(s, d, 0), (s + 128, d + 128, 1)], cb=40),  # not whole blocks
    )
    for bad in bad_calls:
        with pytest.raises(DeossMerkleError) as e:
            ctx.aes_cbc_decrypt_keyed_device_async(good, bad["chains"], bad.get("cb", 64), p)
        assert e.value.code == DM_ERR_INVALID, bad
    # no chains: accepted, with or without keys
    ctx.aes_cbc_decrypt_keyed_device_async(good, [], 64, p)
    ctx.aes_cbc_decrypt_keyed_device_async([], [], 64, 0)
    torch.cuda.synchronize()
    for t in (src, dst, pad):
        assert (t == SENTINEL).all().item()   # nothing ran


# ---- dm_restore_batch ------------------------------------------------------------------------------

GEOMETRIES = ((4, 8, 64), (4, 8, 4 * 16 * 257), (4, 8, 4 * 4096), (8, 8, 8 * 16 * 37))
C16, C24, C32, C32B = _key(200, 16), _key(201, 24), _key(202, 32), _key(203, 32)


def _bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


class Obj:
    """One object of a batch: what the uploader made of it (reference), what the downloader has."""

    def __init__(self, oracle_lib, k, m, segment, nseg, cipher, seed, flags=VALL, size=None, keep=None):
        self.k, self.m, self.total, self.segment, self.cipher, self.flags = k, m, k + m, segment, cipher, flags
        piece = segment - 16 if cipher else segment
        self.size = size if size is not None else (nseg - 1) * piece + 1 + seed * 7919 % piece
        self.buf = _bytes(self.size, seed)
        stored = R.scheme_encrypt(self.buf, cipher, segment) if cipher else self.buf
        self.segd, self.fragd, self.fid, raw = oracle_lib.full_processing(stored, segment, k, m, want_frags=True)
        self.nseg, f = nseg, segment // k
        assert len(self.segd) == 32 * nseg
        rng = np.random.default_rng(seed + 1)
        self.frags = []
        for s in range(nseg):   # an erasure pattern drawn per segment: `keep` of the fragments, at least k
            have = set(rng.permutation(self.total)[:keep if keep else int(rng.integers(k, self.total + 1))].tolist())
            self.frags.append([raw[(s * self.total + j) * f:(s * self.total + j + 1) * f] if j in have else None
                               for j in range(self.total)])
        self.use_cipher = cipher
        self.holds = True   # what the reference says: restored and equal to buf

    def args(self):
        return dict(frags=self.frags, size=self.size, frag_names=self.fragd, seg_names=self.segd, fid=self.fid,
                    flags=self.flags, cipher=self.use_cipher)


def _mixed(oracle_lib, k, m, segment):
    """About 20 objects: nseg 1, 2 and 5, plain and three key lengths (two objects sharing a cipher),
    flags 0, 1, 3 and 7, and every way an object can fail."""
    def mk(nseg, cipher, seed, **kw):
        return Obj(oracle_lib, k, m, segment, nseg, cipher, seed, **kw)
    total, piece = k + m, segment - 16
    o = [mk(1, b"", 1), mk(2, b"", 2, flags=0), mk(5, b"", 3, flags=VF | VS), mk(1, C16, 4), mk(2, C24, 5, flags=VF),
         mk(5, C32, 6), mk(2, C16, 7, flags=VF | VS), mk(2, b"", 8, keep=k + 1), mk(5, b"", 9), mk(2, b"", 10),
         mk(2, C24, 11), mk(2, C32, 12), mk(2, b"", 13, keep=total), mk(1, _key(204, 16), 14, flags=0, keep=total),
         mk(1, b"", 15, flags=VID),
         mk(5, C32, 16, flags=VS), mk(1, C24, 17), mk(1, b"", 18, size=1), mk(2, C16, 19, size=2 * piece),
         mk(2, b"", 20, size=2 * segment)]
    # 7: one corrupt fragment that has a spare -- it is the first one given, so it would be used
    j = next(j for j in range(total) if o[7].frags[1][j] is not None)
    o[7].frags[1][j] = bytes(b ^ 0x55 for b in o[7].frags[1][j])
    o[7].corrupt = (1, j)
    # 8: too few fragments in its middle segment
    given = [j for j in range(total) if o[8].frags[2][j] is not None]
    for j in given[k - 1:]:
        o[8].frags[2][j] = None
    o[8].holds = False
    # 9: a wrong segment name; 10: a wrong fid; 11: a wrong cipher
    o[9].segd = o[9].segd[:32] + bytes(32)
    o[9].holds = False
    o[10].fid = bytes(31) + b"\x01"
    o[10].holds = False
    o[11].use_cipher = C32B
    o[11].holds = False
    # 12, 13: no parity given; 19: parity only
    for x in (o[12], o[13]):
        x.frags = [[f if j < k else None for j, f in enumerate(seg)] for seg in x.frags]
    raw19 = Obj(oracle_lib, k, m, segment, 2, b"", 20, size=2 * segment, keep=total)
    o[19].frags = [[f if k <= j < 2 * k else None for j, f in enumerate(seg)] for seg in raw19.frags]
    # 16: too few fragments in its only segment, with a cipher
    given = [j for j in range(total) if o[16].frags[0][j] is not None]
    for j in given[k - 1:]:
        o[16].frags[0][j] = None
    o[16].holds = False
    return o


_sets = {}


@pytest.fixture(scope="module", params=GEOMETRIES, ids=lambda g: f"{g[0]}+{g[1]}x{g[2]}")
def batch_case(request, ctx, oracle_lib):
    """The mixed set of a geometry and what the single-object calls give for each object, once."""
    from deoss_amd.process import Processor
    k, m, segment = request.param
    if request.param not in _sets:
        objs = _mixed(oracle_lib, k, m, segment)
        proc = Processor(ctx, k, m, segment)
        alone = [proc.restore_buffer(**x.args()) for x in objs]
        proc.close()
        _sets[request.param] = (objs, alone)
    return request.param, _sets[request.param][0], _sets[request.param][1]


def test_single_object_calls_agree_with_the_reference(batch_case):
    """The second witness is sound: alone, every object gives what the reference says."""
    _, objs, alone = batch_case
    for i, (x, (ok, data, fst, sst)) in enumerate(zip(objs, alone)):
        assert ok == x.holds, i
        if ok:
            assert data == x.buf, i
    assert alone[7][2][objs[7].corrupt[0] * objs[7].total + objs[7].corrupt[1]] == BAD_FRAG
    assert alone[8][3][2] == SEG_TOO_FEW and alone[9][3][1] == SEG_MISMATCH
    assert set(alone[11][3]) == {SEG_BAD_PADDING} and alone[16][3][0] == SEG_TOO_FEW


def test_restore_batch_of_one_equals_single_calls(ctx, batch_case):
    from deoss_amd.process import Processor
    (k, m, segment), objs, alone = batch_case
    proc = Processor(ctx, k, m, segment)
    for i in (0, 2, 3, 5, 7, 8, 11):   # plain and cipher, held and failed
        assert proc.restore_batch([objs[i].args()]) == [alone[i]], i
    proc.close()


def test_restore_batch_mixed(ctx, batch_case):
    from deoss_amd.process import Processor, RestoreObject
    (k, m, segment), objs, alone = batch_case
    proc = Processor(ctx, k, m, segment)
    got = proc.restore_batch([RestoreObject(**x.args()) for x in objs])
    assert len(got) == len(objs) == 20
    for i, (g, a, x) in enumerate(zip(got, alone, objs)):
        assert g[0] == a[0], ("ok", i)
        assert g[2] == a[2], ("fragment statuses", i)
        assert g[3] == a[3], ("segment statuses", i)
        assert g[1] == a[1], ("bytes", i)
        assert g[0] == x.holds and (not g[0] or g[1] == x.buf), ("reference", i)
    # the order of a batch changes nothing for any object
    rev = proc.restore_batch([x.args() for x in reversed(objs)])
    assert rev == list(reversed(got))
    assert proc.restore_batch([]) == []
    proc.close()


def _raw_batch(proc, objs, segment=None):
    """dm_restore_batch through ctypes with every output buffer full of sentinel bytes: (rc, error
    text, ok list, parts) where parts[i] = (out, fst, sst) ctypes buffers."""
    from deoss_amd._lib import RestoreObj
    from deoss_amd._lib import restore_obj_fields
    from deoss_amd.process import _cipher_bytes
    n = len(objs)
    arr = (RestoreObj * n)()
    parts = []
    for i, a in enumerate(objs):
        f = restore_obj_fields(a["frags"], a["size"], a["frag_names"], a["seg_names"], a["fid"], a["flags"],
                                _cipher_bytes(a["cipher"]), proc.k + proc.m, proc.frag)
        for b in f[2:5]:
            ctypes.memset(b, SENTINEL, len(b))
        if "nseg" in a:
            f[0].nseg = a["nseg"]
        arr[i] = f[0]
        parts.append(f)
    ok = (ctypes.c_int * n)(*([SENTINEL] * n))
    L = proc.ctx._L
    rc = L.dm_restore_batch(proc.enc._h, arr, n, segment or proc.segment, ok)
    return rc, L.dm_last_error(proc.ctx._h).decode(), list(ok), [p[2:5] for p in parts]


def _untouched(b) -> bool:
    return b.raw == bytes([SENTINEL]) * len(b.raw)


def test_restore_batch_failed_objects_keep_their_out(ctx, batch_case):
    from deoss_amd.process import Processor
    (k, m, segment), objs, alone = batch_case
    proc = Processor(ctx, k, m, segment)
    rc, _, ok, parts = _raw_batch(proc, [x.args() for x in objs])
    assert rc == 0
    for i, (x, (out, fst, sst)) in enumerate(zip(objs, parts)):
        assert ok[i] == int(x.holds), i
        assert (out.raw[:x.size] == x.buf) if x.holds else _untouched(out), i
        assert fst.raw[:x.nseg * x.total] == alone[i][2] and sst.raw[:x.nseg] == alone[i][3], i
    proc.close()


def test_restore_batch_argument_errors_name_the_object_and_write_nothing(ctx, batch_case):
    from deoss_amd import DeossMerkleError
    from deoss_amd._lib import DM_ERR_EMPTY, DM_ERR_INVALID
    from deoss_amd.process import Processor
    (k, m, segment), objs, _ = batch_case
    proc = Processor(ctx, k, m, segment)
    base = [objs[i].args() for i in (0, 3, 5, 2)]
    piece = segment - 16

    def broken(at, **change):
        return [dict(a, **change) if i == at else a for i, a in enumerate(base)]

    cases = (
        (broken(2, size=5 * piece + 1), DM_ERR_INVALID, "object 2", "does not end in the last of"),
        (broken(3, size=4 * segment), DM_ERR_INVALID, "object 3", "does not end in the last of"),
        (broken(1, cipher=bytes(15)), DM_ERR_INVALID, "object 1", "cipher must be 16, 24 or 32 bytes"),
        (broken(0, nseg=0), DM_ERR_EMPTY, "object 0", "Empty data"),
    )
    for batch, code, who, text in cases:
        rc, msg, ok, parts = _raw_batch(proc, batch)
        assert rc == code and who in msg and text in msg, (who, rc, msg)
        assert all(_untouched(b) for p in parts for b in p), who
        assert ok == [SENTINEL] * 4, who   # nothing is written, the verdicts included
    with pytest.raises(DeossMerkleError) as e:
        proc.restore_batch(broken(1, cipher=bytes(15)))
    assert e.value.code == DM_ERR_INVALID and "object 1" in str(e.value)
    proc.close()


def test_restore_batch_cipher_needs_room_for_a_padding_block(ctx, oracle_lib):
    """A 16-byte segment (1 + 2 shards) serves plain objects and has no room for a cipher's padding
    block: the encrypted object is named, the plain one beside it untouched."""
    from deoss_amd._lib import DM_ERR_INVALID
    from deoss_amd.process import Processor
    proc = Processor(ctx, 1, 2, 16)
    plain = Obj(oracle_lib, 1, 2, 16, 2, b"", 30)
    ok_alone = proc.restore_batch([plain.args()])
    assert ok_alone[0][0] and ok_alone[0][1] == plain.buf
    rc, msg, ok, parts = _raw_batch(proc, [plain.args(), dict(plain.args(), cipher=C16)])
    assert rc == DM_ERR_INVALID and "object 1" in msg and "no room for a block and its padding block" in msg
    assert all(_untouched(b) for p in parts for b in p)
    proc.close()


# ---- dm_batcher_restore ----------------------------------------------------------------------------

def test_batcher_restore_coalesces_24_threads(ctx, oracle_lib):
    from deoss_amd import DeossMerkleError
    from deoss_amd._lib import DM_ERR_INVALID
    from deoss_amd.batcher import RESTORE, Batcher
    from deoss_amd.process import Processor
    k, m, segment, nthreads = 4, 8, 4 * 4096, 24
    if (k, m, segment) not in _sets:
        objs = _mixed(oracle_lib, k, m, segment)
        proc = Processor(ctx, k, m, segment)
        _sets[(k, m, segment)] = (objs, [proc.restore_buffer(**x.args()) for x in objs])
        proc.close()
    objs, alone = _sets[(k, m, segment)]
    pick = list(range(20)) + [3, 5, 8, 11]
    got = [None] * (nthreads + 1)
    start = threading.Barrier(nthreads + 1)
    with Batcher(RESTORE, segment, k, m, device=0, linger_us=200_000) as b:
        def run(i):
            start.wait()
            try:
                if i == nthreads:   # one client's bad cipher: refused at submit, alone
                    got[i] = b.restore(**dict(objs[3].args(), cipher=bytes(15)))
                else:
                    got[i] = b.restore(**objs[pick[i]].args())
            except Exception as e:   # noqa: BLE001
                got[i] = e
        ts = [threading.Thread(target=run, args=(i,)) for i in range(nthreads + 1)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        requests, batches, largest = b.stats()
    for i in range(nthreads):
        assert got[i] == alone[pick[i]], (i, pick[i])
    bad = got[nthreads]
    assert isinstance(bad, DeossMerkleError) and bad.code == DM_ERR_INVALID
    assert "cipher must be 16, 24 or 32 bytes" in str(bad)
    assert requests == nthreads            # the refused request was never queued
    assert largest >= 2 and batches < requests, (requests, batches, largest)


def test_batcher_restore_wrong_mode_and_submit_checks(ctx, oracle_lib):
    from deoss_amd import DeossMerkleError
    from deoss_amd._lib import DM_ERR_EMPTY, DM_ERR_INVALID
    from deoss_amd.batcher import PROCESS, RESTORE, Batcher
    k, m, segment = 4, 8, 64
    x = Obj(oracle_lib, k, m, segment, 2, C24, 40)
    with Batcher(PROCESS, segment, k, m, device=0) as b:
        with pytest.raises(DeossMerkleError) as e:
            b.restore(**x.args())
        assert e.value.code == DM_ERR_INVALID and "not a RESTORE batcher" in str(e.value)
    with Batcher(RESTORE, segment, k, m, device=0) as b:
        with pytest.raises(DeossMerkleError) as e:
            b.process(b"x" * 100)
        assert e.value.code == DM_ERR_INVALID and "not a PROCESS batcher" in str(e.value)
        with pytest.raises(DeossMerkleError) as e:
            b.restore(**dict(x.args(), size=2 * (segment - 16) + 1))
        assert e.value.code == DM_ERR_INVALID and "does not end in the last of" in str(e.value)
        with pytest.raises(DeossMerkleError) as e:
            b.restore(**dict(x.args(), frags=[]))
        assert e.value.code == DM_ERR_EMPTY
        ok, data, fst, sst = b.restore(**x.args())   # the batcher still serves
        assert ok and data == x.buf
        assert b.stats()[0] == 1
    with Batcher(RESTORE, 16, 1, 2, device=0) as b:   # no room for a padding block: refused at submit
        y = Obj(oracle_lib, 1, 2, 16, 1, b"", 41)
        assert b.restore(**y.args())[1] == y.buf
        with pytest.raises(DeossMerkleError) as e:
            b.restore(**dict(y.args(), cipher=C16))
        assert e.value.code == DM_ERR_INVALID and "no room for a block and its padding block" in str(e.value)


def test_batcher_restore_virtual_devices(ctx, oracle_lib):
    """device=[0, 0]: two sets of slots on one GPU, requests spread over both."""
    from deoss_amd.batcher import RESTORE, Batcher
    from deoss_amd.process import Processor
    k, m, segment = 4, 8, 64
    objs = [Obj(oracle_lib, k, m, segment, 1 + i % 3, (b"", C16, C32)[i % 3], 50 + i) for i in range(8)]
    proc = Processor(ctx, k, m, segment)
    alone = [proc.restore_buffer(**x.args()) for x in objs]
    proc.close()
    got = [None] * len(objs)
    with Batcher(RESTORE, segment, k, m, device=[0, 0], slots=1) as b:
        def run(i):
            got[i] = b.restore(**objs[i].args())
        ts = [threading.Thread(target=run, args=(i,)) for i in range(len(objs))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert b.stats()[0] == len(objs)
    assert got == alone and all(g[0] and g[1] == x.buf for g, x in zip(got, objs))


# ---- the C++ mirror --------------------------------------------------------------------------------

def test_cpp_mirror_restore_batch(ctx, oracle_lib, tmp_path):
    """tests/cpp/test_restore_batch_mirror.cpp: process::RestoreBatch on objects written to files,
    against the original bytes and the reference's verdicts."""
    k, m, segment = 4, 8, 4 * 4096
    objs = [Obj(oracle_lib, k, m, segment, 1, b"", 60), Obj(oracle_lib, k, m, segment, 2, C24, 61),
            Obj(oracle_lib, k, m, segment, 5, C32, 62, flags=VF | VS), Obj(oracle_lib, k, m, segment, 2, C16, 63),
            Obj(oracle_lib, k, m, segment, 2, b"", 64)]
    objs[3].use_cipher = _key(205, 16)           # a wrong cipher
    objs[4].segd = bytes(32) + objs[4].segd[32:]  # a wrong segment name
    exe = str(tmp_path / "test_restore_batch_mirror")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_restore_batch_mirror.cpp"),
                    "-L", os.path.join(ROOT, "deoss_amd"), "-ldeoss_merkle",
                    "-Wl,-rpath," + os.path.join(ROOT, "deoss_amd"), "-lpthread", "-o", exe], check=True)
    lines = []
    for o, x in enumerate(objs):
        blob = bytearray()
        present = []
        for seg in x.frags:
            for f in seg:
                present.append("1" if f is not None else "0")
                blob += f if f is not None else b""
        (tmp_path / f"frags{o}.bin").write_bytes(bytes(blob))
        (tmp_path / f"names{o}.bin").write_bytes(x.fragd + x.segd + x.fid)
        lines.append(f"{tmp_path / f'frags{o}.bin'} {tmp_path / f'names{o}.bin'} {''.join(present)} {x.nseg} {x.size} "
                     f"{x.flags} {x.use_cipher.hex() if x.use_cipher else '-'}")
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(manifest), str(segment)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-2000:] + r.stderr
    res = [ln.split(" ")[1:] for ln in r.stdout.splitlines() if ln.startswith("OBJ ")]
    assert len(res) == len(objs)
    for o, (ok, data, sst) in enumerate(res):
        want_ok = o < 3
        assert ok == ("1" if want_ok else "0"), o
        assert (bytes.fromhex(data) == objs[o].buf) if want_ok else data == "-", o
    assert set(bytes.fromhex(res[3][2])) == {SEG_BAD_PADDING} and bytes.fromhex(res[4][2])[0] == SEG_MISMATCH
