"""GPU tests of the cipher through the file path: the resumable encrypt kernel
(dm_aes_cbc_encrypt_range_device_async) and dm_full_processing_cipher with its Python and C++
mirrors, bit-exact against tests/cipher_ref.py (plain-Python AES from FIPS-197 + the recalled scheme
over oracle.py_full_processing), the fixtures in tests/golden/aes_kat.json and, at 32 MiB segments,
dm_process_cipher_buffer on the same bytes.

Shapes are the smallest that reach every loop tail: blocks per chain around the kernel's prefetch
depth (8) and its multiples, cut at every block; segment counts around one wave's 16 chains; files
around one piece and around the striped pass's threshold of 4 segments."""
from __future__ import annotations

import ctypes
import hashlib
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cipher_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "aes_kat.json")
BLOCKS = (1, 2, 7, 8, 9, 16, 17, 33)
NSEGS = (1, 16, 17)
KEYS = {n: bytes((37 * i + 11 * n + 5) & 0xFF for i in range(n)) for n in (16, 24, 32)}
IV = bytes((91 * i + 7) & 0xFF for i in range(16))
SENTINEL = 0xEE
GAP = 48


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _dev(torch, arr: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


# ---- the range kernel ------------------------------------------------------------------------------

_ref_cache = {}


def _ref(klen: int, blocks: int):
    """(plaintext (17, 16 blocks), ciphertext with its padding block (17, 16 (blocks + 1))); fewer
    segments are its first rows.  Computed once per (key, blocks)."""
    if (klen, blocks) not in _ref_cache:
        rng = np.random.default_rng(7000 * klen + blocks)
        plain = rng.integers(0, 256, size=(max(NSEGS), 16 * blocks), dtype=np.uint8)
        padded = np.concatenate([plain, np.full((max(NSEGS), 16), 16, dtype=np.uint8)], axis=1)
        ct = R.cbc_encrypt_many(KEYS[klen], IV, padded)
        plain.setflags(write=False)
        ct.setflags(write=False)
        _ref_cache[(klen, blocks)] = (plain, ct)
    return _ref_cache[(klen, blocks)]


def _splits(B: int):
    """Cut lists of a chain of B blocks: every single cut, B one-block calls, and three pieces whose
    first two are 7, 8 or 9 blocks (below, at and above the prefetch depth), in every order."""
    out = [[c] for c in range(1, B)]
    if B > 2:
        out.append(list(range(1, B)))
    out += [[a, a + b] for a, b in itertools.product((7, 8, 9), repeat=2) if a + b < B]
    return out or [[]]


@pytest.mark.parametrize("nseg", NSEGS)
@pytest.mark.parametrize("klen", (16, 24, 32))
def test_encrypt_range_device(ctx, klen, nseg):
    torch = _torch()
    key = KEYS[klen]
    for B in BLOCKS:
        plain, ct = _ref(klen, B)
        n = 16 * B
        stride = n + 16 + GAP   # larger than plain + 16: the gap holds a sentinel
        host = np.full((nseg, stride), SENTINEL, dtype=np.uint8)
        host[:, :n] = plain[:nseg]
        whole = _dev(torch, host)
        ctx.aes_cbc_encrypt_device_async(key, IV, whole.data_ptr(), stride, n, nseg)
        torch.cuda.synchronize()
        whole = whole.cpu().numpy()
        for cuts in _splits(B):
            buf = _dev(torch, host)
            edges = [0] + cuts + [B]
            for lo, hi in zip(edges[:-1], edges[1:]):
                ctx.aes_cbc_encrypt_range_device_async(key, IV, buf.data_ptr(), stride, n, nseg, lo, hi)
                torch.cuda.synchronize()
                got = buf.cpu().numpy()
                what = (klen, nseg, B, cuts, lo, hi)
                assert (got[:, :16 * hi] == ct[:nseg, :16 * hi]).all(), what
                if hi < B:   # the rest is still plaintext; padding slot and gap untouched
                    assert (got[:, 16 * hi:n] == plain[:nseg, 16 * hi:]).all(), what
                    assert (got[:, n:] == SENTINEL).all(), what
            assert (got[:, :n + 16] == ct[:nseg]).all(), (klen, nseg, B, cuts)
            assert (got[:, n + 16:] == SENTINEL).all(), (klen, nseg, B, cuts)
            assert (got == whole).all(), (klen, nseg, B, cuts)


def test_encrypt_range_sp800_38a(ctx):
    """SP 800-38A F.2.1 / F.2.3 / F.2.5 (CBC-AES128 / 192 / 256 encrypt), cut after block 2."""
    torch = _torch()
    with open(KAT) as f:
        k = json.load(f)["sp800_38a_cbc"]
    iv, pt = bytes.fromhex(k["iv"]), bytes.fromhex("".join(k["plaintext"]))
    assert [c["section"] for c in k["cases"]] == ["F.2.1", "F.2.3", "F.2.5"]
    for c in k["cases"]:
        key, want = bytes.fromhex(c["key"]), bytes.fromhex("".join(c["ciphertext"]))
        host = np.zeros((3, 96), dtype=np.uint8)
        host[:, :64] = np.frombuffer(pt, dtype=np.uint8)
        buf = _dev(torch, host)
        ctx.aes_cbc_encrypt_range_device_async(key, iv, buf.data_ptr(), 96, 64, 3, 0, 2)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        for s in range(3):
            assert got[s, :32].tobytes() == want[:32] and got[s, 32:64].tobytes() == pt[32:], c["section"]
            assert not got[s, 64:].any(), c["section"]
        ctx.aes_cbc_encrypt_range_device_async(key, iv, buf.data_ptr(), 96, 64, 3, 2, 4)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        for s in range(3):
            assert got[s, :64].tobytes() == want, c["section"]
            assert got[s, :80].tobytes() == R.cbc_encrypt(key, iv, pt, pkcs7=True), c["section"]
            assert not got[s, 80:].any(), c["section"]


def test_encrypt_range_argument_checks(ctx):
    from deoss_amd import DeossMerkleError
    from deoss_amd._lib import DM_ERR_INVALID
    torch = _torch()
    host = np.arange(272, dtype=np.uint8)
    buf = _dev(torch, host)
    good = dict(key=KEYS[16], ptr=buf.data_ptr(), stride=128, plain=64, lo=1, hi=3)
    bads = (dict(lo=2, hi=2), dict(lo=3, hi=2), dict(lo=0, hi=5), dict(lo=4, hi=5), dict(key=bytes(15)),
            dict(ptr=buf.data_ptr() + 8), dict(plain=24, hi=1, lo=0), dict(plain=120, stride=128), dict(stride=72))
    for bad in bads:
        a = dict(good)
        a.update(bad)
        with pytest.raises(DeossMerkleError) as e:
            ctx.aes_cbc_encrypt_range_device_async(a["key"], IV, a["ptr"], a["stride"], a["plain"], 2, a["lo"], a["hi"])
        assert e.value.code == DM_ERR_INVALID, bad
        if "key" in bad:
            assert "cipher must be 16, 24 or 32 bytes" in str(e.value)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == host).all()   # nothing ran


# ---- dm_full_processing_cipher at segment 4,096 (4 + 8, P = 4,080) -------------------------------------

SEG = 4096
P = SEG - 16
SIZES = (10 * P + 999, 1, P - 1, P, P + 1, 4 * P, 4 * P + 1)
# name: (key length, DEOSS_FP_STRIPES, DEOSS_FP_SLOT_BYTES, DEOSS_FP_WINDOW_BYTES)
# (with a cipher the striped pass runs when DEOSS_FP_STRIPES asks for it: DESIGN.md §6.14)
CONFIGS = {
    "striped16": (16, "1", None, None),             # one striped window
    "striped24": (24, "1", None, None),
    "striped32": (32, "1", None, None),
    "default": (16, None, None, None),              # encrypt whole chains, then hash
    "nostripes": (16, "0", None, None),
    "unstriped_windows": (16, "1", 8192, 3 * 4096),   # 2-segment windows: never striped, fid over all
    "narrow_stripes": (16, "1", 2 * 4096, 40 * 4096),   # stripes of 4, 8, 12 ... blocks
    "window_boundary": (16, "1", 8192, 6 * 4096),
}


def _processor(ctx, segment=SEG, k=4, m=8):
    from deoss_amd.process import Processor
    return Processor(ctx, k, m, segment)


def _body(n: int) -> bytes:
    return np.random.default_rng(0xC1F0 + n).integers(0, 256, size=n, dtype=np.uint8).tobytes()


_file_ref = {}


def _reference(n: int, klen: int):
    """(body, segment digests, fragment digests per segment, fid, fragments per segment) of the
    scheme over a body of n bytes; computed once per (size, key) and shared."""
    if (n, klen) not in _file_ref:
        body = _body(n)
        _file_ref[(n, klen)] = (body,) + tuple(R.scheme_full_processing(body, KEYS[klen], SEG))
    return _file_ref[(n, klen)]


def _set_config(monkeypatch, name):
    klen, stripes, slot, window = CONFIGS[name]
    if stripes is not None:
        monkeypatch.setenv("DEOSS_FP_STRIPES", stripes)
    if slot:
        monkeypatch.setenv("DEOSS_FP_SLOT_BYTES", str(slot))
        monkeypatch.setenv("DEOSS_FP_WINDOW_BYTES", str(window))
    return klen


@pytest.mark.parametrize("config", list(CONFIGS))
def test_full_processing_cipher_files(ctx, tmp_path, monkeypatch, config):
    """The fid, every name and every byte of every fragment and segment file, for files around one
    piece, around the striped threshold and of 11 segments; no temporary is left."""
    klen = _set_config(monkeypatch, config)
    p = _processor(ctx)
    for n in SIZES:
        body, segs, fragh, fid, frags = _reference(n, klen)
        f = tmp_path / f"object_{n}.bin"
        f.write_bytes(body)
        savedir = tmp_path / f"cache_{n}" / "deeper"
        gseg, gfrag, gfid = p.full_processing_file(str(f), str(savedir), segment_files=True, cipher=KEYS[klen])
        nseg = R.scheme_nseg(n, SEG)
        assert len(segs) == nseg and len(gseg) == 32 * nseg, (config, n)
        assert gfid == fid, (config, n)
        assert gseg == b"".join(segs), (config, n)
        assert gfrag == b"".join(h for row in fragh for h in row), (config, n)
        want_files = {}
        for s in range(nseg):
            want_files[segs[s].hex()] = b"".join(frags[s][:4])   # the data fragments in order: the ciphertext
            for j in range(12):
                want_files[fragh[s][j].hex()] = frags[s][j]
        assert sorted(os.listdir(savedir)) == sorted(want_files), (config, n)
        for name, want in want_files.items():
            assert (savedir / name).read_bytes() == want, (config, n, name)
    p.close()


@pytest.mark.parametrize("config", ("striped16", "default", "nostripes", "window_boundary"))
def test_full_processing_cipher_round_trip(ctx, tmp_path, monkeypatch, capfd, config):
    """FullProcessing(file, cipher, savedir) -> two data fragments of every segment dropped ->
    RestoreFile with the cipher gives the body back; with a wrong cipher it fails on padding.
    The phase trace says which pass ran: the striped one only where DEOSS_FP_STRIPES=1 asks for it."""
    klen = _set_config(monkeypatch, config)
    monkeypatch.setenv("DEOSS_FP_TRACE", "1")
    cipher = KEYS[klen]
    p = _processor(ctx)
    n = SIZES[0]
    body, segs, fragh, fid, _ = _reference(n, klen)
    f = tmp_path / "object.bin"
    f.write_bytes(body)
    savedir = tmp_path / "frags"
    info, gfid, err = p.FullProcessing(str(f), cipher, str(savedir))
    assert err is None, err
    assert gfid == fid.hex() and len(info) == len(segs)
    trace = capfd.readouterr().err
    assert ("stripes read" in trace) == (CONFIGS[config][1] == "1"), trace
    assert trace.count("leaf pass done") == (2 if config == "window_boundary" else 1), trace
    assert [os.path.basename(s.SegmentHash) for s in info] == [h.hex() for h in segs]
    assert [[os.path.basename(x) for x in s.FragmentHash] for s in info] == [[h.hex() for h in row] for row in fragh]
    assert not [x for x in os.listdir(savedir) if x.startswith(".")]
    wrong = bytes(b ^ 0x55 for b in cipher)
    ok, err = p.RestoreFile(str(savedir), info, n, str(tmp_path / "wrong.bin"), wrong)
    assert not ok and "padding" in str(err) and not os.path.exists(tmp_path / "wrong.bin")
    for s, seg in enumerate(info):
        for j in (s % 4, (s + 2) % 4):
            os.unlink(seg.FragmentHash[j])
    ok, err = p.RestoreFile(str(savedir), info, n, str(tmp_path / "restored.bin"), cipher)
    assert ok and err is None, err
    assert (tmp_path / "restored.bin").read_bytes() == body
    p.close()


def test_full_processing_cipher_errors(ctx, tmp_path):
    from deoss_amd._lib import DM_ERR_INVALID
    p = _processor(ctx)
    body = _body(4 * P + 1)
    f = tmp_path / "object.bin"
    f.write_bytes(body)
    # a cipher of the wrong length: the message, and savedir is not created
    for bad in (bytes(15), bytes(17), bytes(33)):
        info, fid, err = p.FullProcessing(str(f), bad, str(tmp_path / "bad"))
        assert info is None and fid == "" and err.code == DM_ERR_INVALID
        assert "cipher must be 16, 24 or 32 bytes" in str(err)
        assert not os.path.exists(tmp_path / "bad")
    empty = tmp_path / "empty.bin"
    empty.write_bytes(b"")
    info, fid, err = p.FullProcessing(str(empty), KEYS[16], str(tmp_path / "e"))
    assert info is None and fid == "" and str(err) == "Empty data"
    info, fid, err = p.FullProcessing(str(tmp_path / "missing"), KEYS[16], str(tmp_path / "m"))
    assert info is None and fid == "" and str(err) == f"open {tmp_path / 'missing'}: no such file or directory"
    # cipher_len == 0 through the C call is dm_full_processing
    L = ctx._L
    outs = []
    for name in ("with_len0", "plain"):
        seg, frag = ctypes.create_string_buffer(32 * 5), ctypes.create_string_buffer(32 * 5 * 12)
        fid, nseg = ctypes.create_string_buffer(32), ctypes.c_uint64(0)
        d = tmp_path / name
        if name == "plain":
            rc = L.dm_full_processing(p.enc._h, os.fsencode(str(f)), os.fsencode(str(d)), SEG, 1, seg, frag, 5,
                                      ctypes.byref(nseg), fid)
        else:
            rc = L.dm_full_processing_cipher(p.enc._h, os.fsencode(str(f)), os.fsencode(str(d)), SEG, None, 0, 1, seg,
                                             frag, 5, ctypes.byref(nseg), fid)
        assert rc == 0, name
        outs.append((nseg.value, seg.raw, frag.raw, fid.raw, {x: (d / x).read_bytes() for x in sorted(os.listdir(d))}))
    assert outs[0] == outs[1] and outs[0][0] == 4   # ceil((4 P + 1) / 4096): plain segments, not the 5 pieces
    assert outs[0][4][outs[0][1][:32].hex()] == body[:SEG]
    # digest arrays too small for the pieces: the count comes back, nothing is written
    seg, frag = ctypes.create_string_buffer(32 * 4), ctypes.create_string_buffer(32 * 4 * 12)
    fid, nseg = ctypes.create_string_buffer(32), ctypes.c_uint64(0)
    rc = L.dm_full_processing_cipher(p.enc._h, os.fsencode(str(f)), os.fsencode(str(tmp_path / "small")), SEG, KEYS[16], 16,
                                     0, seg, frag, 4, ctypes.byref(nseg), fid)
    assert rc == DM_ERR_INVALID and nseg.value == 5 and not os.path.exists(tmp_path / "small")
    p.close()


# ---- once at chain.SegmentSize ---------------------------------------------------------------------

BIG = 32 << 20
BIG_P = BIG - 16


@pytest.fixture(scope="module")
def big_case(ctx, tmp_path_factory):
    """A body of 5 P + 12,345 bytes (6 segments of 32 MiB), its file, and the digests and fid of
    dm_process_cipher_buffer over it; computed once."""
    from oracle import splitmix64_bytes
    body = splitmix64_bytes(5 * BIG_P + 12345, 0xC1F0B16)
    d = tmp_path_factory.mktemp("cipher_file_big")
    path = d / "object.bin"
    path.write_bytes(body)
    p = _processor(ctx, BIG)
    segd, fragd, fid, _ = p.process_buffer(body, want_frags=False, cipher=KEYS[16])
    p.close()
    assert len(segd) == 32 * 6
    return dict(body=body, path=str(path), segd=segd, fragd=fragd, fid=fid)


@pytest.mark.parametrize("stripes", ("1", "0"))
def test_full_processing_cipher_full_segments(ctx, big_case, tmp_path, monkeypatch, stripes):
    """dm_full_processing_cipher at 32 MiB segments, striped and not: the digests and the fid of
    dm_process_cipher_buffer, every file on disk hashes to its name, and the head and the tail of a
    ciphertext segment file decrypt under the reference to the body's bytes and the padding block."""
    monkeypatch.setenv("DEOSS_FP_STRIPES", stripes)
    c = big_case
    key = KEYS[16]
    p = _processor(ctx, BIG)
    savedir = tmp_path / "cache"
    segd, fragd, fid = p.full_processing_file(c["path"], str(savedir), segment_files=True, cipher=key)
    p.close()
    assert (segd, fragd, fid) == (c["segd"], c["fragd"], c["fid"])
    names = sorted(os.listdir(savedir))
    assert names == sorted({fragd[32 * t:32 * t + 32].hex() for t in range(len(fragd) // 32)} |
                           {segd[32 * s:32 * s + 32].hex() for s in range(len(segd) // 32)})
    for n in names:
        assert hashlib.sha256((savedir / n).read_bytes()).hexdigest() == n
    for s in (2, 5):   # a full piece, and the zero-padded last one
        ct = np.frombuffer((savedir / segd[32 * s:32 * s + 32].hex()).read_bytes(), dtype=np.uint8)
        piece = c["body"][s * BIG_P:(s + 1) * BIG_P]
        piece = np.frombuffer(piece + bytes(BIG_P - len(piece)), dtype=np.uint8)
        head = R.cbc_decrypt_many(key, R.scheme_iv(key), ct[:4096].reshape(1, -1))[0]
        assert (head == piece[:4096]).all(), s
        tail = R.cbc_decrypt_many(key, ct[-4112:-4096].tobytes(), ct[-4096:].reshape(1, -1))[0]
        assert (tail[:-16] == piece[-4080:]).all() and (tail[-16:] == 16).all(), s


# ---- the C++ mirror ---------------------------------------------------------------------------------

MIRROR_CIPHER = "0123456789abcdef0123456789abcdef"


def test_cpp_mirror_full_processing_file(ctx, tmp_path):
    """tests/cpp/test_cipher_file_mirror.cpp: process::FullProcessing(file, cipher, savedir) takes
    the one call; names and fid are the reference's and its fragments restore through the Python
    mirror."""
    from deoss_amd.process import SegmentDataInfo
    n = SIZES[0]
    body = _body(n)
    segs, fragh, fid, _ = R.scheme_full_processing(body, MIRROR_CIPHER.encode(), SEG)
    path = tmp_path / "object.bin"
    path.write_bytes(body)
    exe = str(tmp_path / "test_cipher_file_mirror")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_cipher_file_mirror.cpp"),
                    "-L", os.path.join(ROOT, "deoss_amd"), "-ldeoss_merkle",
                    "-Wl,-rpath," + os.path.join(ROOT, "deoss_amd"), "-lpthread", "-o", exe], check=True)
    savedir = tmp_path / "frags"
    r = subprocess.run([exe, str(path), MIRROR_CIPHER, str(savedir), str(SEG)], capture_output=True, text=True)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    lines = r.stdout.split()
    assert lines[lines.index("FID") + 1] == fid.hex()
    assert lines[lines.index("NSEG") + 1] == str(len(segs))
    info = []
    for ln in r.stdout.splitlines():
        if ln.startswith("SEG "):
            info.append(SegmentDataInfo(ln[4:], []))
        elif ln.startswith("FRAG "):
            info[-1].FragmentHash.append(ln[5:])
    assert [os.path.basename(s.SegmentHash) for s in info] == [h.hex() for h in segs]
    assert [[os.path.basename(x) for x in s.FragmentHash] for s in info] == [[h.hex() for h in row] for row in fragh]
    assert not [x for x in os.listdir(savedir) if x.startswith(".")]
    for s, seg in enumerate(info):
        assert os.path.dirname(seg.SegmentHash) == str(savedir) and os.path.getsize(seg.SegmentHash) == SEG
        for j in (s % 4, (s + 2) % 4, 4 + s % 8):
            os.unlink(seg.FragmentHash[j])
    p = _processor(ctx)
    ok, err = p.RestoreFile(str(savedir), info, n, str(tmp_path / "restored.bin"), MIRROR_CIPHER)
    assert ok and err is None, err
    assert (tmp_path / "restored.bin").read_bytes() == body
    p.close()
