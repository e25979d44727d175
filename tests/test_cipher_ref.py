"""CPU tests of the cipher reference (tests/cipher_ref.py): every fixture in tests/golden/aes_kat.json
(FIPS-197 Appendix C, SP 800-38A F.2.1 / F.2.3 / F.2.5, one vector of the recalled scheme), and,
where the machine has OpenSSL's libcrypto, EVP_aes_*_cbc on seeded random cases.  No GPU."""
import ctypes
import ctypes.util
import json
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cipher_ref as R  # noqa: E402

KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aes_kat.json")


@pytest.fixture(scope="module")
def kat():
    with open(KAT) as f:
        return json.load(f)


def test_sbox_corners():
    # FIPS-197 figure 7 / figure 14
    assert (R.SBOX[0x00], R.SBOX[0x53], R.SBOX[0xff]) == (0x63, 0xed, 0x16)
    assert (R.INV_SBOX[0x63], R.INV_SBOX[0xed]) == (0x00, 0x53)
    assert sorted(R.SBOX.tolist()) == list(range(256))


def test_fips197_appendix_c(kat):
    pt = bytes.fromhex(kat["fips197_appendix_c"]["plaintext"])
    for c in kat["fips197_appendix_c"]["cases"]:
        key, ct = bytes.fromhex(c["key"]), bytes.fromhex(c["ciphertext"])
        rk = R.expand_key(key)
        assert R.encrypt_blocks(rk, np.frombuffer(pt, dtype=np.uint8).reshape(1, 16)).tobytes() == ct
        assert R.decrypt_blocks(rk, np.frombuffer(ct, dtype=np.uint8).reshape(1, 16)).tobytes() == pt


def test_sp800_38a_cbc(kat):
    k = kat["sp800_38a_cbc"]
    iv, pt = bytes.fromhex(k["iv"]), bytes.fromhex("".join(k["plaintext"]))
    for c in k["cases"]:
        key, ct = bytes.fromhex(c["key"]), bytes.fromhex("".join(c["ciphertext"]))
        assert R.cbc_encrypt(key, iv, pt) == ct, c["section"]
        assert R.cbc_decrypt(key, iv, ct) == pt, c["section"]


def test_scheme_vector(kat):
    s = kat["scheme"]
    cipher, ct = s["cipher_ascii"].encode(), bytes.fromhex("".join(s["ciphertext"]))
    lo, hi = s["object_zero_bytes"]
    for n in range(lo, hi + 1):
        assert R.scheme_nseg(n, s["segment"]) == 1
        assert R.scheme_encrypt(bytes(n), cipher, s["segment"]) == ct
        assert R.scheme_decrypt(ct, cipher, s["segment"], n) == bytes(n)
    # a piece is exactly the CBC encryption with PKCS#7 of its 48 bytes
    assert R.cbc_encrypt(cipher, cipher[:16], bytes(48), pkcs7=True) == ct
    assert R.scheme_nseg(49, s["segment"]) == 2
    with pytest.raises(ValueError):
        R.scheme_decrypt(ct, cipher[::-1], s["segment"], 5)   # wrong cipher: bad padding
    with pytest.raises(ValueError):
        R.scheme_encrypt(bytes(5), b"x" * 15, s["segment"])


def test_many_rows_equal_single_rows():
    rng = random.Random(7)
    key, iv = rng.randbytes(24), rng.randbytes(16)
    rows = np.frombuffer(rng.randbytes(5 * 80), dtype=np.uint8).reshape(5, 80)
    ct = R.cbc_encrypt_many(key, iv, rows)
    for i in range(5):
        assert ct[i].tobytes() == R.cbc_encrypt(key, iv, rows[i].tobytes())
    assert (R.cbc_decrypt_many(key, iv, ct) == rows).all()


def _openssl():
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        L = ctypes.CDLL(name)
        for f in ("EVP_CIPHER_CTX_new", "EVP_aes_128_cbc", "EVP_aes_192_cbc", "EVP_aes_256_cbc"):
            getattr(L, f).restype = ctypes.c_void_p
        L.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]
        L.EVP_EncryptInit_ex.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_char_p, ctypes.c_char_p]
        L.EVP_EncryptUpdate.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int),
                                        ctypes.c_char_p, ctypes.c_int]
        L.EVP_EncryptFinal_ex.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
        return L
    except (OSError, AttributeError):
        return None


def _evp_cbc(L, key, iv, plain):
    """EVP_aes_*_cbc with PKCS#7 padding (the EVP default)."""
    cipher = {16: L.EVP_aes_128_cbc, 24: L.EVP_aes_192_cbc, 32: L.EVP_aes_256_cbc}[len(key)]()
    ctx = L.EVP_CIPHER_CTX_new()
    try:
        out, last = ctypes.create_string_buffer(len(plain) + 32), ctypes.create_string_buffer(32)
        n, m = ctypes.c_int(0), ctypes.c_int(0)
        assert L.EVP_EncryptInit_ex(ctx, cipher, None, key, iv) == 1
        assert L.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), plain, len(plain)) == 1
        assert L.EVP_EncryptFinal_ex(ctx, last, ctypes.byref(m)) == 1
        return out.raw[:n.value] + last.raw[:m.value]
    finally:
        L.EVP_CIPHER_CTX_free(ctx)


def test_reference_equals_openssl():
    L = _openssl()
    if L is None:
        pytest.skip("no OpenSSL libcrypto on this machine")
    rng = random.Random(0xAE5)
    for _ in range(200):
        key = rng.randbytes(rng.choice((16, 24, 32)))
        iv = rng.randbytes(16)
        plain = rng.randbytes(rng.randrange(0, 400))
        want = _evp_cbc(L, key, iv, plain)
        assert R.cbc_encrypt(key, iv, plain, pkcs7=True) == want
        assert R.cbc_decrypt(key, iv, want, pkcs7=True) == plain
