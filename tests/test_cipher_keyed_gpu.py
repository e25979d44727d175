"""GPU tests of encrypted uploads in batches: the keyed AES-CBC kernel (a key per chain, ONE launch:
dm_aes_cbc_encrypt_keyed_device_async), FullProcessing of many objects with a cipher each
(dm_process_cipher_batch), the coalescing executor with a cipher (dm_batcher_process_cipher) and the
Python and C++ mirrors -- bit-exact against tests/cipher_ref.py (plain-Python AES from FIPS-197, the
recalled scheme over oracle.py_full_processing), the fixtures in tests/golden/aes_kat.json and the
existing single-object calls.

Shapes are the smallest that reach every path: blocks per chain around the kernel's prefetch depth
(8) and its multiples, chain counts around one wave's 16 chains, key-length groups of exactly 16 and
17 chains beside a single chain of another length (the plan pads every group to whole waves)."""
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
BLOCKS = (1, 7, 8, 9, 17, 33)
NCHAINS = (1, 2, 15, 16, 17, 33, 65)
MAXB, MAXC = max(BLOCKS), max(NCHAINS)
KLENS = (16, 24, 32)
SENTINEL = 0xEE


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _key(tag: int, klen: int) -> bytes:
    return bytes((tag * 29 + 37 * i + 11 * klen + 5) & 0xFF for i in range(klen))


def _iv(tag: int) -> bytes:
    return bytes((tag * 53 + 91 * i + 7) & 0xFF for i in range(16))


# the keys of every pattern: two shared ones per length, and one of its own for every chain index
# with the length cycling 16 / 24 / 32
SHARED = {(klen, i): (_key(100 + i, klen), _iv(100 + i)) for klen in KLENS for i in (0, 1)}
OWN = [(_key(c, KLENS[c % 3]), _iv(c)) for c in range(MAXC)]

_plain = None
_ref_cache = {}


def _plain_rows() -> np.ndarray:
    """Chain c's plaintext is the head of row c: (65, 33 blocks), fixed."""
    global _plain
    if _plain is None:
        _plain = np.random.default_rng(20260).integers(0, 256, size=(MAXC, 16 * MAXB), dtype=np.uint8)
        _plain.setflags(write=False)
    return _plain


def _ref(key: bytes, iv: bytes, rows):
    """{blocks: ciphertext with its padding block} of the given plaintext rows under one key, by
    ``cbc_encrypt_many``: for every block count the row's head, the padding block and filler (CBC
    is causal: what follows the padding block does not reach it).  Computed once per (key, rows)."""
    rows = tuple(rows)
    if (key, iv, rows) not in _ref_cache:
        plain = _plain_rows()[list(rows)]
        stack = np.zeros((len(BLOCKS), len(rows), 16 * (MAXB + 1)), dtype=np.uint8)
        for t, nb in enumerate(BLOCKS):
            stack[t, :, :16 * nb] = plain[:, :16 * nb]
            stack[t, :, 16 * nb:16 * (nb + 1)] = 16
        ct = R.cbc_encrypt_many(key, iv, stack.reshape(-1, 16 * (MAXB + 1))).reshape(stack.shape)
        out = {nb: np.ascontiguousarray(ct[t, :, :16 * (nb + 1)]) for t, nb in enumerate(BLOCKS)}
        for a in out.values():
            a.setflags(write=False)
        _ref_cache[(key, iv, rows)] = out
    return _ref_cache[(key, iv, rows)]


def _pattern(name: str, n: int):
    """(keys, key index of every chain) of a pattern at n chains."""
    if name == "one":
        return [SHARED[(32, 0)]], [0] * n
    if name == "own":
        return OWN[:n], list(range(n))
    # "group": n - 1 chains of one key length (two keys, alternating) beside 1 of another: at 17 a
    # group of exactly 16, at 18 one of 17; which length is the large group changes with n
    a, b = KLENS[n % 3], KLENS[(n + 1) % 3]
    keys = [SHARED[(a, 0)], SHARED[(a, 1)], SHARED[(b, 0)]]
    return keys, [c % 2 for c in range(n - 1)] + [2]


def _want(keys, kidx, nb):
    """Reference ciphertext (n, 16 (nb + 1)): chain c is row c under keys[kidx[c]]."""
    n = len(kidx)
    want = np.zeros((n, 16 * (nb + 1)), dtype=np.uint8)
    for k, (key, iv) in enumerate(keys):
        rows = [c for c in range(n) if kidx[c] == k]
        if rows:
            want[rows] = _ref(key, iv, rows)[nb]
    return want


def _layout(n: int, nb: int, seed: int):
    """Offsets of n chains of nb blocks in one buffer: placed in a shuffled order (so offsets are not
    monotone in the chain index) with gaps of 16, 32 or 48 sentinel bytes between them."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n)
    off = np.zeros(n, dtype=np.int64)
    pos = 16 * int(rng.integers(1, 4))
    for c in order:
        off[c] = pos
        pos += 16 * (nb + 1) + 16 * int(rng.integers(1, 4))
    return off, pos


CASES = [(p, n) for p in ("one", "own", "group") for n in NCHAINS] + [("group", 18)]


@pytest.mark.parametrize("pattern, n", CASES)
def test_keyed_encrypt_device(ctx, pattern, n):
    torch = _torch()
    keys, kidx = _pattern(pattern, n)
    plain = _plain_rows()
    for nb in BLOCKS:
        want = _want(keys, kidx, nb)
        off, size = _layout(n, nb, 1000 * n + nb)
        host = np.full(size, SENTINEL, dtype=np.uint8)
        gap = np.ones(size, dtype=bool)
        for c in range(n):
            host[off[c]:off[c] + 16 * nb] = plain[c, :16 * nb]
            gap[off[c]:off[c] + 16 * (nb + 1)] = False
        results = []
        # the chain list in the caller's order, then permuted: the same bytes
        for order in (list(range(n)), list(np.random.default_rng(n + nb).permutation(n))):
            buf = torch.from_numpy(host.copy()).cuda()
            chains = [(buf.data_ptr() + int(off[c]), kidx[c]) for c in order]
            ctx.aes_cbc_encrypt_keyed_device_async(keys, chains, 16 * nb)
            torch.cuda.synchronize()
            results.append(buf.cpu().numpy())
        got = results[0]
        for c in range(n):
            assert (got[off[c]:off[c] + 16 * (nb + 1)] == want[c]).all(), (pattern, n, nb, c)
        assert (got[gap] == SENTINEL).all(), (pattern, n, nb)
        assert (results[1] == got).all(), (pattern, n, nb)


@pytest.mark.parametrize("klen", KLENS)
def test_keyed_equals_single_key_kernel(ctx, klen):
    """One key and a common stride: byte-identical to dm_aes_cbc_encrypt_device_async."""
    torch = _torch()
    key, iv = SHARED[(klen, 1)]
    n = 33
    for nb in BLOCKS:
        stride = 16 * (nb + 1) + 32
        host = np.full((n, stride), SENTINEL, dtype=np.uint8)
        host[:, :16 * nb] = _plain_rows()[:n, :16 * nb]
        a = torch.from_numpy(host.copy()).cuda()
        b = torch.from_numpy(host.copy()).cuda()
        ctx.aes_cbc_encrypt_device_async(key, iv, a.data_ptr(), stride, 16 * nb, n)
        ctx.aes_cbc_encrypt_keyed_device_async([(key, iv)], [(b.data_ptr() + c * stride, 0) for c in range(n)], 16 * nb)
        torch.cuda.synchronize()
        assert torch.equal(a, b), (klen, nb)
        assert not (a.cpu().numpy()[:, :16 * nb] == host[:, :16 * nb]).all()


def test_keyed_sp800_38a_three_keys_one_launch(ctx):
    """SP 800-38A F.2.1 / F.2.3 / F.2.5 (CBC-AES128 / 192 / 256) as three chains of one launch."""
    torch = _torch()
    with open(KAT) as f:
        k = json.load(f)["sp800_38a_cbc"]
    iv, pt = bytes.fromhex(k["iv"]), bytes.fromhex("".join(k["plaintext"]))
    cases = k["cases"]
    assert sorted(len(bytes.fromhex(c["key"])) for c in cases) == [16, 24, 32]
    host = np.zeros((3, 96), dtype=np.uint8)
    host[:, :64] = np.frombuffer(pt, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    keys = [(bytes.fromhex(c["key"]), iv) for c in cases]
    ctx.aes_cbc_encrypt_keyed_device_async(keys, [(buf.data_ptr() + 96 * i, i) for i in range(3)], 64)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    for i, c in enumerate(cases):
        assert got[i, :64].tobytes() == bytes.fromhex("".join(c["ciphertext"])), c["section"]
        assert got[i, :80].tobytes() == R.cbc_encrypt(keys[i][0], iv, pt, pkcs7=True), c["section"]
        assert not got[i, 80:].any()


def test_keyed_argument_checks(ctx):
    from deoss_amd import DeossMerkleError
    from deoss_amd._lib import DM_ERR_INVALID
    torch = _torch()
    buf = torch.full((512,), SENTINEL, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    good = [SHARED[(16, 0)], SHARED[(32, 0)]]
    with pytest.raises(DeossMerkleError) as e:
        ctx.aes_cbc_encrypt_keyed_device_async([good[0], (bytes(15), _iv(0)), good[1]], [(p, 0)], 64)
    assert e.value.code == DM_ERR_INVALID
    assert "key 1" in str(e.value) and "cipher must be 16, 24 or 32 bytes" in str(e.value)
    bad_calls = (
        dict(chains=[(p, 0), (p + 136, 1)]),            # misaligned
        dict(chains=[(p, 0), (0, 1)]),                  # null
        dict(chains=[(p, 0), (p + 128, 2)]),            # key index out of range
        dict(chains=[(p, 0), (p + 128, 1)], plain=72),  # plain % 16 != 0
    )
    for bad in bad_calls:
        with pytest.raises(DeossMerkleError) as e:
            ctx.aes_cbc_encrypt_keyed_device_async(good, bad["chains"], bad.get("plain", 64))
        assert e.value.code == DM_ERR_INVALID, bad
    # no chains: accepted, with or without keys
    ctx.aes_cbc_encrypt_keyed_device_async(good, [], 64)
    ctx.aes_cbc_encrypt_keyed_device_async([], [], 64)
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all().item()   # nothing ran


# ---- dm_process_cipher_batch ---------------------------------------------------------------------

CIPHERS = {0: b"", 16: _key(200, 16), 24: _key(201, 24), 32: _key(202, 32)}


def _processor(ctx, segment, k=4, m=8):
    from deoss_amd.process import Processor
    return Processor(ctx, k, m, segment)


def _object(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def _flat(ref):
    segs, fragh, fid, frags = ref
    return b"".join(segs), b"".join(h for s in fragh for h in s), fid, b"".join(f for s in frags for f in s)


@pytest.fixture(scope="module")
def small_batch():
    """Segment 256 (P = 240), 4 + 8 shards: lengths {1, 239, 240, 241, 480, 481} x ciphers {none, 16,
    24, 32 bytes} and every object's reference, computed once."""
    from oracle import py_full_processing
    bufs, ciphers, want = [], [], []
    for n in (1, 239, 240, 241, 480, 481):
        for klen in (0, 16, 24, 32):
            buf = _object(n, 31 * n + klen)
            bufs.append(buf)
            ciphers.append(CIPHERS[klen])
            want.append(_flat(R.scheme_full_processing(buf, CIPHERS[klen], 256) if klen else py_full_processing(buf, 256)))
    return bufs, ciphers, want


def test_process_cipher_batch_small(ctx, small_batch):
    bufs, ciphers, want = small_batch
    p = _processor(ctx, 256)
    got = p.process_batch(bufs, want_frags=True, ciphers=ciphers)
    assert len(got) == len(bufs) == 24
    for o, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], ("fid", o, len(bufs[o]), len(ciphers[o]))
        assert g[0] == w[0], ("segment names", o, len(bufs[o]), len(ciphers[o]))
        assert g[1] == w[1], ("fragment names", o, len(bufs[o]), len(ciphers[o]))
        assert g[3] == w[3], ("fragments", o, len(bufs[o]), len(ciphers[o]))
    p.close()


def test_process_cipher_batch_1mib(ctx):
    segment = 1 << 20
    P = segment - 16
    p = _processor(ctx, segment)
    bufs = [_object(segment + 5, 1), _object(P, 2), _object(P + 1, 3), _object(100_000, 4)]
    ciphers = [b"", _key(210, 16), _key(211, 24), _key(212, 32)]
    got = p.process_batch(bufs, want_frags=True, ciphers=ciphers)
    for o in range(4):
        alone = p.process_buffer(bufs[o], want_frags=True, cipher=ciphers[o])
        assert got[o] == alone, o
    assert [len(g[0]) // 32 for g in got] == [2, 1, 2, 1]
    p.close()


def test_process_cipher_batch_all_plain_equals_process_batch(ctx, small_batch):
    bufs = [b for b, c in zip(*small_batch[:2]) if not c]
    p = _processor(ctx, 256)
    want = p.process_batch(bufs, want_frags=True)
    assert p.process_batch(bufs, want_frags=True, ciphers=[b""] * len(bufs)) == want
    assert p.process_batch(bufs, want_frags=True, ciphers=[None] * len(bufs)) == want
    p.close()


def test_process_cipher_batch_bad_cipher_names_object_and_writes_nothing(ctx):
    from deoss_amd import DeossMerkleError
    from deoss_amd._lib import DM_ERR_EMPTY, DM_ERR_INVALID
    p = _processor(ctx, 256)
    L = ctx._L
    n = 4
    bufs = [ctypes.create_string_buffer(_object(300, 50 + o), 300) for o in range(n)]
    keys = [ctypes.create_string_buffer(k, 32) for k in (CIPHERS[16], CIPHERS[24], bytes(17), CIPHERS[32])]

    def call(lens, key_lens):
        seg = [ctypes.create_string_buffer(bytes([0x5A]) * 64, 64) for _ in range(n)]
        frag = [ctypes.create_string_buffer(bytes([0x5A]) * 768, 768) for _ in range(n)]
        frags = [ctypes.create_string_buffer(bytes([0x5A]) * 1536, 1536) for _ in range(n)]
        fids = ctypes.create_string_buffer(bytes([0x5A]) * 32 * n, 32 * n)
        arr = lambda xs: (ctypes.c_void_p * n)(*[ctypes.addressof(x) for x in xs])  # noqa: E731
        rc = L.dm_process_cipher_batch(p.enc._h, arr(bufs), (ctypes.c_uint64 * n)(*lens), arr(keys),
                                       (ctypes.c_uint64 * n)(*key_lens), n, 256, arr(frags), arr(seg), arr(frag), fids)
        clean = all(x.raw == bytes([0x5A]) * len(x.raw) for x in seg + frag + frags + [fids])
        return rc, L.dm_last_error(ctx._h).decode(), clean

    rc, msg, clean = call([300] * n, [16, 24, 17, 32])
    assert rc == DM_ERR_INVALID and "object 2" in msg and "cipher must be 16, 24 or 32 bytes" in msg and clean
    rc, msg, clean = call([300, 0, 300, 300], [16, 24, 32, 32])
    assert rc == DM_ERR_EMPTY and "object 1" in msg and clean
    rc, msg, clean = call([300] * n, [16, 24, 32, 0])
    assert rc == 0 and not clean
    # the Python wrapper raises the same error
    with pytest.raises(DeossMerkleError) as e:
        p.process_batch([b"x" * 300] * 4, ciphers=[CIPHERS[16], b"", bytes(17), CIPHERS[32]])
    assert e.value.code == DM_ERR_INVALID and "object 2" in str(e.value)
    p.close()


# ---- dm_batcher_process_cipher -------------------------------------------------------------------

def test_batcher_process_cipher_coalesces_mixed_keys(ctx):
    from deoss_amd import DeossMerkleError
    from deoss_amd._lib import DM_ERR_INVALID
    from deoss_amd.batcher import PROCESS, Batcher
    segment, nthreads = 64 << 10, 24
    P = segment - 16
    lens = [1, P - 1, P, P + 1, 2 * P, 2 * P + 5, 3 * P, 70_000]
    bufs = [_object(lens[i % len(lens)] + (i // len(lens)), 900 + i) for i in range(nthreads)]
    ciphers = [b"" if i % 4 == 0 else _key(300 + i, KLENS[i % 3]) for i in range(nthreads)]
    p = _processor(ctx, segment)
    want = [p.process_buffer(bufs[i], want_frags=True, cipher=ciphers[i]) for i in range(nthreads)]
    p.close()
    got = [None] * (nthreads + 1)
    start = threading.Barrier(nthreads + 1)
    with Batcher(PROCESS, segment, 4, 8, device=0, linger_us=200_000) as b:
        def run(i):
            start.wait()
            try:
                if i == nthreads:   # one client's bad cipher: refused at submit, alone
                    got[i] = b.process(bufs[0], want_frags=True, cipher=bytes(15))
                else:
                    got[i] = b.process(bufs[i], want_frags=True, cipher=ciphers[i])
            except Exception as e:   # noqa: BLE001
                got[i] = e
        ts = [threading.Thread(target=run, args=(i,)) for i in range(nthreads + 1)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        requests, batches, largest = b.stats()
    for i in range(nthreads):
        assert got[i] == want[i], (i, len(bufs[i]), len(ciphers[i]))
    bad = got[nthreads]
    assert isinstance(bad, DeossMerkleError) and bad.code == DM_ERR_INVALID
    assert "cipher must be 16, 24 or 32 bytes" in str(bad)
    assert requests == nthreads            # the refused request was never queued
    assert batches < requests and largest > 1, (requests, batches, largest)


# ---- the C++ mirror ------------------------------------------------------------------------------

def test_cpp_mirror_batch(small_batch, tmp_path):
    """tests/cpp/test_cipher_batch_mirror.cpp: process::FullProcessingCipherBatch at the segment-256
    shapes, against the same reference."""
    bufs, ciphers, want = small_batch
    exe = str(tmp_path / "test_cipher_batch_mirror")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_cipher_batch_mirror.cpp"),
                    "-L", os.path.join(ROOT, "deoss_amd"), "-ldeoss_merkle",
                    "-Wl,-rpath," + os.path.join(ROOT, "deoss_amd"), "-lpthread", "-o", exe], check=True)
    lines = []
    for o, (buf, key) in enumerate(zip(bufs, ciphers)):
        path = tmp_path / f"obj{o}.bin"
        path.write_bytes(buf)
        lines.append(f"{path} {key.hex() if key else '-'}")
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(manifest), "256"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-2000:] + r.stderr
    objs = [ln.split(" ")[1:] for ln in r.stdout.splitlines() if ln.startswith("OBJ ")]
    assert len(objs) == len(bufs)
    for o, (fid, segs, fragh, frags) in enumerate(objs):
        w = want[o]
        assert (bytes.fromhex(segs), bytes.fromhex(fragh), bytes.fromhex(fid), bytes.fromhex(frags)) == w, o
