"""GPU tests of the cipher branch: the AES-CBC kernels (dm_aes_cbc_*_device_async), FullProcessing
and restore with a cipher (dm_process_cipher_buffer, dm_restore_cipher_buffer) and the Python and
C++ mirrors, bit-exact against tests/cipher_ref.py (plain-Python AES from FIPS-197 + the recalled
scheme over oracle.py_full_processing) and the fixtures in tests/golden/aes_kat.json.

Shapes are the smallest that reach every loop tail: blocks per segment around the encrypt kernel's
prefetch depth (8) and its multiples, segment counts around one wave's 16 chains of 4 lanes."""
from __future__ import annotations

import ctypes
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
BLOCKS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 255, 257)
NSEGS = (1, 2, 15, 16, 17, 65)
KEYS = {n: bytes((37 * i + 11 * n + 5) & 0xFF for i in range(n)) for n in (16, 24, 32)}
IV = bytes((91 * i + 7) & 0xFF for i in range(16))
SENTINEL = 0xEE


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def kat():
    with open(KAT) as f:
        return json.load(f)


_ref_cache = {}


def _ref(klen: int, blocks: int):
    """(plaintext (65, 16 blocks), ciphertext with its padding block (65, 16 (blocks + 1))) for the
    largest segment count; fewer segments are its first rows.  Computed once per (key, blocks)."""
    if (klen, blocks) not in _ref_cache:
        rng = np.random.default_rng(1000 * klen + blocks)
        plain = rng.integers(0, 256, size=(max(NSEGS), 16 * blocks), dtype=np.uint8)
        padded = np.concatenate([plain, np.full((max(NSEGS), 16), 16, dtype=np.uint8)], axis=1)
        ct = R.cbc_encrypt_many(KEYS[klen], IV, padded)
        plain.setflags(write=False)
        ct.setflags(write=False)
        _ref_cache[(klen, blocks)] = (plain, ct)
    return _ref_cache[(klen, blocks)]


def _dev(torch, arr: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


# ---- device-level encrypt ------------------------------------------------------------------------

@pytest.mark.parametrize("nseg", NSEGS)
@pytest.mark.parametrize("klen", (16, 24, 32))
def test_encrypt_device(ctx, klen, nseg):
    torch = _torch()
    for blocks in BLOCKS:
        plain, ct = _ref(klen, blocks)
        n = 16 * blocks
        stride = n + 16 + 48   # larger than plain + 16: the bytes beyond must stay
        host = np.full((nseg, stride), SENTINEL, dtype=np.uint8)
        host[:, :n] = plain[:nseg]
        buf = _dev(torch, host)
        ctx.aes_cbc_encrypt_device_async(KEYS[klen], IV, buf.data_ptr(), stride, n, nseg)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:, :n + 16] == ct[:nseg]).all(), (klen, nseg, blocks)
        assert (got[:, n + 16:] == SENTINEL).all(), (klen, nseg, blocks)


def test_encrypt_device_sp800_38a(ctx, kat):
    torch = _torch()
    k = kat["sp800_38a_cbc"]
    iv, pt = bytes.fromhex(k["iv"]), bytes.fromhex("".join(k["plaintext"]))
    for c in k["cases"]:
        key, want = bytes.fromhex(c["key"]), bytes.fromhex("".join(c["ciphertext"]))
        host = np.zeros((3, 96), dtype=np.uint8)
        host[:, :64] = np.frombuffer(pt, dtype=np.uint8)
        buf = _dev(torch, host)
        ctx.aes_cbc_encrypt_device_async(key, iv, buf.data_ptr(), 96, 64, 3)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        for s in range(3):
            assert got[s, :64].tobytes() == want, c["section"]
        # the padding block that follows is the next CBC block of sixteen 0x10 bytes
        assert got[0, :80].tobytes() == R.cbc_encrypt(key, iv, pt, pkcs7=True), c["section"]


def test_device_fips197_appendix_c(ctx, kat):
    """One block with a zero IV is the bare cipher: FIPS-197 Appendix C, both directions."""
    torch = _torch()
    pt = bytes.fromhex(kat["fips197_appendix_c"]["plaintext"])
    for c in kat["fips197_appendix_c"]["cases"]:
        key, want = bytes.fromhex(c["key"]), bytes.fromhex(c["ciphertext"])
        buf = _dev(torch, np.frombuffer(pt + bytes(16), dtype=np.uint8).copy())
        ctx.aes_cbc_encrypt_device_async(key, bytes(16), buf.data_ptr(), 32, 16, 1)
        out = torch.zeros(16, dtype=torch.uint8, device="cuda")
        ok = torch.zeros(16, dtype=torch.uint8, device="cuda")
        ctx.aes_cbc_decrypt_device_async(key, bytes(16), buf.data_ptr(), 32, 32, 1, out.data_ptr(), 16, ok.data_ptr())
        torch.cuda.synchronize()
        assert buf.cpu().numpy()[:16].tobytes() == want, len(key)
        assert out.cpu().numpy().tobytes() == pt and ok.cpu().tolist()[0] == 1, len(key)


def test_device_argument_checks(ctx):
    from deoss_amd import DeossMerkleError
    from deoss_amd._lib import DM_ERR_INVALID
    torch = _torch()
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    out = torch.zeros(256, dtype=torch.uint8, device="cuda")
    for bad in (dict(key=bytes(15)), dict(plain=24), dict(plain=64, stride=64), dict(stride=72)):
        a = dict(key=KEYS[16], stride=128, plain=64)
        a.update(bad)
        with pytest.raises(DeossMerkleError) as e:
            ctx.aes_cbc_encrypt_device_async(a["key"], IV, buf.data_ptr(), a["stride"], a["plain"], 2)
        assert e.value.code == DM_ERR_INVALID, bad
    for bad in (dict(key=bytes(33)), dict(cipher_bytes=16), dict(cipher_bytes=40)):
        a = dict(key=KEYS[16], cipher_bytes=64)
        a.update(bad)
        with pytest.raises(DeossMerkleError) as e:
            ctx.aes_cbc_decrypt_device_async(a["key"], IV, buf.data_ptr(), 128, a["cipher_bytes"], 2, out.data_ptr(), 128,
                                             out.data_ptr() + 240)
        assert e.value.code == DM_ERR_INVALID, bad
    torch.cuda.synchronize()
    assert not buf.any().item() and not out.any().item()   # nothing ran


# ---- device-level decrypt ------------------------------------------------------------------------

@pytest.mark.parametrize("nseg", NSEGS)
@pytest.mark.parametrize("klen", (16, 24, 32))
def test_decrypt_device(ctx, klen, nseg):
    torch = _torch()
    for blocks in BLOCKS:
        plain, ct = _ref(klen, blocks)
        n = 16 * blocks
        in_stride = n + 16 + 32
        host = np.full((nseg, in_stride), 0x33, dtype=np.uint8)
        host[:, :n + 16] = ct[:nseg]
        src = _dev(torch, host)
        for out_stride in (n, n + 48):   # joined object / a larger stride whose gaps must stay
            dst = torch.full((nseg * out_stride + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
            ok = torch.full((nseg + 16,), 7, dtype=torch.uint8, device="cuda")
            ctx.aes_cbc_decrypt_device_async(KEYS[klen], IV, src.data_ptr(), in_stride, n + 16, nseg, dst.data_ptr(),
                                             out_stride, ok.data_ptr())
            torch.cuda.synchronize()
            got = dst.cpu().numpy()
            rows = got[:nseg * out_stride].reshape(nseg, out_stride)
            assert (rows[:, :n] == plain[:nseg]).all(), (klen, nseg, blocks, out_stride)
            assert (rows[:, n:] == SENTINEL).all() and (got[nseg * out_stride:] == SENTINEL).all()
            okh = ok.cpu().numpy()
            assert (okh[:nseg] == 1).all() and (okh[nseg:] == 7).all(), (klen, nseg, blocks)


@pytest.mark.parametrize("klen", (16, 24, 32))
def test_decrypt_flipped_padding_bit(ctx, klen):
    """One flipped bit in one segment's last ciphertext block: that segment's padding is bad, its
    plaintext (which depends on the earlier blocks only) and every other segment are as before."""
    torch = _torch()
    blocks, nseg, hit = 9, 5, 3
    plain, ct = _ref(klen, blocks)
    n = 16 * blocks
    host = np.array(ct[:nseg])
    host[hit, n + 5] ^= 0x10
    src = _dev(torch, host)
    dst = torch.zeros(nseg * n, dtype=torch.uint8, device="cuda")
    ok = torch.full((nseg,), 7, dtype=torch.uint8, device="cuda")
    ctx.aes_cbc_decrypt_device_async(KEYS[klen], IV, src.data_ptr(), n + 16, n + 16, nseg, dst.data_ptr(), n, ok.data_ptr())
    torch.cuda.synchronize()
    assert ok.cpu().tolist() == [1, 1, 1, 0, 1]
    assert (dst.cpu().numpy().reshape(nseg, n) == plain[:nseg]).all()


@pytest.mark.parametrize("nbytes, nseg, klen", [(1 << 20, 8, 16), (1 << 20, 8, 32), (4 << 20, 3, 24)])
def test_round_trip_large(ctx, nbytes, nseg, klen):
    torch = _torch()
    g = torch.Generator(device="cuda")
    g.manual_seed(nbytes + klen)
    plain = torch.randint(0, 256, (nseg, nbytes), dtype=torch.uint8, device="cuda", generator=g)
    stride = nbytes + 16
    buf = torch.zeros((nseg, stride), dtype=torch.uint8, device="cuda")
    buf[:, :nbytes] = plain
    ctx.aes_cbc_encrypt_device_async(KEYS[klen], IV, buf.data_ptr(), stride, nbytes, nseg)
    out = torch.zeros((nseg, nbytes), dtype=torch.uint8, device="cuda")
    ok = torch.zeros(nseg, dtype=torch.uint8, device="cuda")
    ctx.aes_cbc_decrypt_device_async(KEYS[klen], IV, buf.data_ptr(), stride, stride, nseg, out.data_ptr(), nbytes,
                                     ok.data_ptr())
    torch.cuda.synchronize()
    assert ok.cpu().tolist() == [1] * nseg
    assert torch.equal(out, plain)
    assert not torch.equal(buf[:, :nbytes], plain)
    # the ciphertext is AES-CBC, not merely self-consistent: the reference decrypts the head and the
    # tail of the last segment (CBC decryption needs only the block before)
    ct = buf[nseg - 1].cpu().numpy()
    head = R.cbc_decrypt_many(KEYS[klen], IV, ct[:4096].reshape(1, -1))[0]
    assert (head == plain[nseg - 1, :4096].cpu().numpy()).all()
    tail = R.cbc_decrypt_many(KEYS[klen], ct[-4112:-4096].tobytes(), ct[-4096:].reshape(1, -1))[0]
    assert (tail[:-16] == plain[nseg - 1, -4080:].cpu().numpy()).all() and (tail[-16:] == 16).all()


# ---- process_buffer / restore_buffer with a cipher -------------------------------------------------

def _processor(ctx, segment, k=4, m=8):
    from deoss_amd.process import Processor
    return Processor(ctx, k, m, segment)


def _object(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def _lens(segment):
    P = segment - 16
    return (1, P - 1, P, P + 1, 2 * P, 2 * P + 5)


@pytest.mark.parametrize("klen", (16, 24, 32))
@pytest.mark.parametrize("segment", (256, 4096))
def test_process_buffer_cipher(ctx, segment, klen):
    p = _processor(ctx, segment)
    total, fsz = 12, segment // 4
    for n in _lens(segment):
        buf = _object(n, 10 * segment + n)
        segs, fragh, fid, frags = R.scheme_full_processing(buf, KEYS[klen], segment)
        gseg, gfrag, gfid, gfrags = p.process_buffer(buf, want_frags=True, cipher=KEYS[klen])
        nseg = R.scheme_nseg(n, segment)
        assert len(segs) == nseg and len(gseg) == 32 * nseg, (segment, klen, n)
        assert gseg == b"".join(segs), (segment, klen, n)
        assert gfrag == b"".join(h for s in fragh for h in s), (segment, klen, n)
        assert gfid == fid, (segment, klen, n)
        assert len(gfrags) == nseg * total * fsz
        assert gfrags == b"".join(f for s in frags for f in s), (segment, klen, n)
    p.close()


def test_process_buffer_scheme_vector(ctx, kat):
    s = kat["scheme"]
    p = _processor(ctx, s["segment"])
    want = bytes.fromhex("".join(s["ciphertext"]))
    for n in (s["object_zero_bytes"][0], 17, s["object_zero_bytes"][1]):
        seg, frag, fid, frags = p.process_buffer(bytes(n), want_frags=True, cipher=s["cipher_ascii"])
        assert frags[:s["segment"]] == want, n   # the data fragments in order are the segment's ciphertext
        assert len(seg) == 32
    p.close()


def test_process_buffer_cipher_errors_and_plain_unchanged(ctx):
    from deoss_amd import DeossMerkleError
    from deoss_amd._lib import DM_ERR_INVALID
    from oracle import py_full_processing
    p = _processor(ctx, 256)
    buf = _object(700, 3)
    for bad in (bytes(15), bytes(17), bytes(31), bytes(33), bytes(1)):
        with pytest.raises(DeossMerkleError) as e:
            p.process_buffer(buf, cipher=bad)
        assert e.value.code == DM_ERR_INVALID
        assert "cipher must be 16, 24 or 32 bytes" in str(e.value)
    # no cipher: exactly today's results (the plain oracle), through either spelling
    segs, fragh, fid, frags = py_full_processing(buf, 256)
    want = (b"".join(segs), b"".join(h for s in fragh for h in s), fid, b"".join(f for s in frags for f in s))
    assert p.process_buffer(buf) == want
    assert p.process_buffer(buf, cipher=b"") == want
    assert p.process_buffer(buf, True, "") == want
    p.close()


@pytest.mark.parametrize("klen", (16, 24, 32))
@pytest.mark.parametrize("segment", (256, 4096))
def test_restore_buffer_cipher(ctx, segment, klen):
    from deoss_amd import DeossMerkleError
    from deoss_amd._lib import DM_ERR_INVALID
    from deoss_amd.process import SEG_BAD_PADDING
    p = _processor(ctx, segment)
    key, total, fsz, P = KEYS[klen], 12, segment // 4, segment - 16
    for n in _lens(segment):
        buf = _object(n, 20 * segment + n)
        seg, fragn, fid, frags = p.process_buffer(buf, want_frags=True, cipher=key)
        nseg = len(seg) // 32
        full = [[frags[(s * total + j) * fsz:(s * total + j + 1) * fsz] for j in range(total)] for s in range(nseg)]
        # two data fragments dropped per segment (a different pair each)
        have = [[None if j in (s % 4, (s + 1) % 4) else f for j, f in enumerate(row)]
                for s, row in enumerate(full)]
        ok, data, fst, sst = p.restore_buffer(have, n, frag_names=fragn, seg_names=seg, fid=fid, cipher=key)
        assert ok and data == buf and set(sst) == {0}, (segment, klen, n)
        # one corrupted fragment: bad, and the next good one takes its place
        bad = [list(row) for row in have]
        j0 = next(j for j in range(total) if bad[0][j] is not None)
        bad[0][j0] = bytes([bad[0][j0][0] ^ 1]) + bad[0][j0][1:]
        ok, data, fst, sst = p.restore_buffer(bad, n, frag_names=fragn, seg_names=seg, fid=fid, cipher=key)
        assert ok and data == buf, (segment, klen, n)
        assert fst[j0] == 3 and list(fst[:total]).count(1) == 4
        # the right names with the wrong cipher: every padding is bad, nothing leaves the device
        wrong = bytes(b ^ 0x55 for b in key)
        out = ctypes.create_string_buffer(bytes([0x5A]) * max(n, 1), max(n, 1))
        ok, data, fst, sst = p.restore_buffer(have, n, frag_names=fragn, seg_names=seg, fid=fid, cipher=wrong, out=out)
        assert not ok and data is None and list(sst) == [SEG_BAD_PADDING] * nseg, (segment, klen, n)
        assert out.raw == bytes([0x5A]) * max(n, 1)
        # a size outside the last piece
        for size in ((nseg - 1) * P, nseg * P + 1):
            with pytest.raises(DeossMerkleError) as e:
                p.restore_buffer(have, size, frag_names=fragn, seg_names=seg, fid=fid, cipher=key)
            assert e.value.code == DM_ERR_INVALID, (segment, klen, n, size)
    p.close()


def test_restore_buffer_cipher_with_and_without_a_spare(ctx):
    """5 of 12 fragments with one used fragment corrupt: the spare takes its place and the plaintext
    is exact.  4 of 12 with one corrupt: too few, and nothing is written to the caller's buffer."""
    segment, key, total = 256, KEYS[16], 12
    fsz, n = segment // 4, 3 * (segment - 16) + 7
    p = _processor(ctx, segment)
    buf = _object(n, 4242)
    seg, fragn, fid, frags = p.process_buffer(buf, want_frags=True, cipher=key)
    nseg = len(seg) // 32
    full = [[frags[(s * total + j) * fsz:(s * total + j + 1) * fsz] for j in range(total)] for s in range(nseg)]
    kept = [[1, 3, 6, 8, 11], [0, 5, 7, 9, 10], [2, 3, 4, 5, 6], [0, 1, 2, 3, 4]]
    assert nseg == len(kept)
    have = [[f if j in kept[s] else None for j, f in enumerate(row)] for s, row in enumerate(full)]
    for s in range(nseg):
        j = kept[s][s % 4]
        h = have[s][j]
        have[s][j] = h[:5] + bytes([h[5] ^ 0x20]) + h[6:]
    ok, data, fst, sst = p.restore_buffer(have, n, frag_names=fragn, seg_names=seg, fid=fid, cipher=key)
    assert ok and data == buf and sst == bytes(nseg)
    for s in range(nseg):
        want = [3 if j == kept[s][s % 4] else 1 if j in kept[s] else 0 for j in range(total)]
        assert list(fst[s * total:(s + 1) * total]) == want, s
    few = [[f if j in kept[s][:4] else None for j, f in enumerate(row)] for s, row in enumerate(full)]
    few[2][kept[2][1]] = bytes([few[2][kept[2][1]][0] ^ 1]) + few[2][kept[2][1]][1:]
    out = ctypes.create_string_buffer(bytes([0x5A]) * n, n)
    ok, data, fst, sst = p.restore_buffer(few, n, frag_names=fragn, seg_names=seg, fid=fid, cipher=key, out=out)
    assert not ok and data is None and list(sst) == [0, 0, 1, 0]
    assert out.raw == bytes([0x5A]) * n and fst[2 * total + kept[2][1]] == 3
    p.close()


# ---- the mirrors -----------------------------------------------------------------------------------

MIRROR_CIPHER = "0123456789abcdef0123456789abcdef"


@pytest.fixture(scope="module")
def mirror_case(tmp_path_factory):
    """A file of 2 windows + 1 piece + 3 bytes at segment 4,096 and its reference, computed once."""
    from deoss_amd.process import WINDOW_SEGMENTS
    segment = 4096
    n = (2 * WINDOW_SEGMENTS + 1) * (segment - 16) + 3
    body = _object(n, 77)
    d = tmp_path_factory.mktemp("cipher_mirror")
    path = str(d / "object.bin")
    with open(path, "wb") as f:
        f.write(body)
    segs, fragh, fid, _ = R.scheme_full_processing(body, MIRROR_CIPHER.encode(), segment)
    return dict(segment=segment, body=body, path=path, dir=d, segs=segs, fragh=fragh, fid=fid)


def _check_names(case, info, savedir):
    assert [os.path.basename(s.SegmentHash) for s in info] == [h.hex() for h in case["segs"]]
    assert [[os.path.basename(f) for f in s.FragmentHash] for s in info] == [[h.hex() for h in row] for row in case["fragh"]]
    for s in info:
        for f in s.FragmentHash:
            assert os.path.getsize(f) == case["segment"] // 4 and os.path.dirname(f) == str(savedir)


def _drop_and_restore(p, case, info, savedir, out_path):
    for s, seg in enumerate(info):   # two data fragments and some parity of every segment are "not downloaded"
        for j in (s % 4, (s + 2) % 4, 4 + s % 8):
            if os.path.exists(seg.FragmentHash[j]):
                os.unlink(seg.FragmentHash[j])
    ok, err = p.RestoreFile(str(savedir), info, len(case["body"]), out_path, MIRROR_CIPHER)
    assert ok and err is None, err
    with open(out_path, "rb") as f:
        assert f.read() == case["body"]


def test_python_mirror_full_processing_and_restore(ctx, mirror_case, tmp_path):
    c = mirror_case
    p = _processor(ctx, c["segment"])
    savedir = tmp_path / "frags"
    info, fid, err = p.FullProcessing(c["path"], MIRROR_CIPHER, str(savedir))
    assert err is None, err
    assert fid == c["fid"].hex() and len(info) == 18
    _check_names(c, info, savedir)
    # a wrong cipher restores nothing and writes nothing
    ok, err = p.RestoreFile(str(savedir), info, len(c["body"]), str(tmp_path / "wrong.bin"), MIRROR_CIPHER[::-1])
    assert not ok and "padding" in str(err) and not os.path.exists(tmp_path / "wrong.bin")
    _drop_and_restore(p, c, info, savedir, str(tmp_path / "restored.bin"))
    # without its cipher the same object has another fid, and a 15-byte cipher is an error
    _, plain_fid, err = p.FullProcessingWindows(c["path"], "", str(tmp_path / "plain"))
    assert err is None and plain_fid != fid
    info, fid, err = p.FullProcessing(c["path"], "fifteen-bytes-x", str(tmp_path / "bad"))
    assert info is None and fid == "" and "cipher must be 16, 24 or 32 bytes" in str(err)
    p.close()


def test_cpp_mirror_full_processing(ctx, mirror_case, tmp_path):
    """tests/cpp/test_cipher_mirror.cpp: process::FullProcessingCipher over the same file; its
    fragments restore through the Python mirror."""
    from deoss_amd.process import SegmentDataInfo
    c = mirror_case
    exe = str(tmp_path / "test_cipher_mirror")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_cipher_mirror.cpp"),
                    "-L", os.path.join(ROOT, "deoss_amd"), "-ldeoss_merkle",
                    "-Wl,-rpath," + os.path.join(ROOT, "deoss_amd"), "-lpthread", "-o", exe], check=True)
    savedir = tmp_path / "frags"
    r = subprocess.run([exe, c["path"], MIRROR_CIPHER, str(savedir), str(c["segment"])], capture_output=True, text=True)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout + r.stderr
    lines = r.stdout.split()
    assert lines[lines.index("FID") + 1] == c["fid"].hex()
    assert lines[lines.index("NSEG") + 1] == "18"
    info = []
    for ln in r.stdout.splitlines():
        if ln.startswith("SEG "):
            info.append(SegmentDataInfo(ln[4:], []))
        elif ln.startswith("FRAG "):
            info[-1].FragmentHash.append(ln[5:])
    _check_names(c, info, savedir)
    p = _processor(ctx, c["segment"])
    _drop_and_restore(p, c, info, savedir, str(tmp_path / "restored.bin"))
    p.close()
