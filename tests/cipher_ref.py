"""CPU reference for the cipher branch: AES (FIPS-197) with CBC (SP 800-38A) in plain Python / numpy,
and the recalled upload / download scheme (deoss_amd/csrc/cipher_scheme.hpp) built
on ``oracle.py_full_processing`` applied to the ciphertext.  Test infrastructure only.

Written from FIPS-197 alone, by another route than the product: SubBytes / ShiftRows / MixColumns
on a byte state (no T-tables, no equivalent inverse cipher), the S-box from the multiplicative
inverse by exhaustive search.  CBC encryption is vectorised across segments (each segment is its
own chain), CBC decryption across all blocks.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

BLOCK = 16
PAD = bytes([16]) * 16   # PKCS#7 padding of a plaintext that is a whole number of blocks


def _gmul(a: int, b: int) -> int:
    """GF(2^8) product modulo x^8 + x^4 + x^3 + x + 1 (FIPS-197 §4.2)."""
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= 0x11B
        b >>= 1
    return r


def _make_sbox() -> np.ndarray:
    inv = [0] * 256
    for a in range(1, 256):
        if inv[a]:
            continue
        for b in range(1, 256):
            if _gmul(a, b) == 1:
                inv[a], inv[b] = b, a
                break
    s = np.zeros(256, dtype=np.uint8)
    for a in range(256):
        x = inv[a]
        y = x
        for sh in range(1, 5):   # affine transformation, FIPS-197 eq. 5.1
            y ^= ((x << sh) | (x >> (8 - sh))) & 0xFF
        s[a] = y ^ 0x63
    return s


SBOX = _make_sbox()
INV_SBOX = np.zeros(256, dtype=np.uint8)
INV_SBOX[SBOX] = np.arange(256, dtype=np.uint8)
_MUL = {c: np.array([_gmul(a, c) for a in range(256)], dtype=np.uint8) for c in (2, 3, 9, 11, 13, 14)}
# state byte index = 4 * column + row (the block's bytes in order, FIPS-197 §3.4)
_SHIFT = np.array([4 * ((c + r) % 4) + r for c in range(4) for r in range(4)])
_INV_SHIFT = np.array([4 * ((c - r) % 4) + r for c in range(4) for r in range(4)])


def expand_key(key: bytes) -> np.ndarray:
    """KeyExpansion (FIPS-197 §5.2): (Nr + 1, 16) round-key bytes."""
    nk = len(key) // 4
    if len(key) not in (16, 24, 32):
        raise ValueError("cipher must be 16, 24 or 32 bytes")
    nr = nk + 6
    w = [list(key[4 * i:4 * i + 4]) for i in range(nk)]
    rcon = 1
    for i in range(nk, 4 * (nr + 1)):
        t = list(w[i - 1])
        if i % nk == 0:
            t = t[1:] + t[:1]
            t = [int(SBOX[b]) for b in t]
            t[0] ^= rcon
            rcon = _gmul(rcon, 2)
        elif nk > 6 and i % nk == 4:
            t = [int(SBOX[b]) for b in t]
        w.append([a ^ b for a, b in zip(w[i - nk], t)])
    return np.array(w, dtype=np.uint8).reshape(nr + 1, 16)


def _mix(st: np.ndarray, coef: Sequence[int]) -> np.ndarray:
    """MixColumns with the circulant matrix whose first row is ``coef``; st: (n, 16)."""
    s = st.reshape(-1, 4, 4)   # [n, column, row]
    out = np.zeros_like(s)
    for r in range(4):
        for j in range(4):
            c = coef[(j - r) % 4]
            out[:, :, r] ^= s[:, :, j] if c == 1 else _MUL[c][s[:, :, j]]
    return out.reshape(-1, 16)


def encrypt_blocks(rk: np.ndarray, blocks: np.ndarray) -> np.ndarray:
    """Cipher (FIPS-197 §5.1) on every row of blocks (n, 16)."""
    nr = len(rk) - 1
    st = blocks ^ rk[0]
    for r in range(1, nr):
        st = _mix(SBOX[st][:, _SHIFT], (2, 3, 1, 1)) ^ rk[r]
    return SBOX[st][:, _SHIFT] ^ rk[nr]


def decrypt_blocks(rk: np.ndarray, blocks: np.ndarray) -> np.ndarray:
    """InvCipher (FIPS-197 §5.3, the straightforward one) on every row of blocks (n, 16)."""
    nr = len(rk) - 1
    st = blocks ^ rk[nr]
    for r in range(nr - 1, 0, -1):
        st = _mix(INV_SBOX[st[:, _INV_SHIFT]] ^ rk[r], (14, 11, 13, 9))
    return INV_SBOX[st[:, _INV_SHIFT]] ^ rk[0]


def cbc_encrypt_many(key: bytes, iv: bytes, plains: np.ndarray) -> np.ndarray:
    """CBC encryption (SP 800-38A §6.2) of every row of plains (nseg, nbytes), nbytes % 16 == 0,
    all with the same key and IV; no padding.  One Python step per block, all rows at once."""
    rk = expand_key(key)
    nseg, n = plains.shape
    assert n % BLOCK == 0
    out = np.empty_like(plains)
    prev = np.tile(np.frombuffer(iv, dtype=np.uint8), (nseg, 1))
    for b in range(n // BLOCK):
        prev = encrypt_blocks(rk, plains[:, BLOCK * b:BLOCK * (b + 1)] ^ prev)
        out[:, BLOCK * b:BLOCK * (b + 1)] = prev
    return out


def cbc_decrypt_many(key: bytes, iv: bytes, ciphers: np.ndarray) -> np.ndarray:
    """CBC decryption of every row of ciphers (nseg, nbytes); no padding handling."""
    rk = expand_key(key)
    nseg, n = ciphers.shape
    assert n % BLOCK == 0
    d = decrypt_blocks(rk, np.ascontiguousarray(ciphers).reshape(-1, BLOCK)).reshape(nseg, n)
    prev = np.empty_like(ciphers)
    prev[:, :BLOCK] = np.frombuffer(iv, dtype=np.uint8)
    prev[:, BLOCK:] = ciphers[:, :-BLOCK]
    return d ^ prev


def cbc_encrypt(key: bytes, iv: bytes, plain: bytes, pkcs7: bool = False) -> bytes:
    if pkcs7:
        n = BLOCK - len(plain) % BLOCK
        plain = bytes(plain) + bytes([n]) * n
    return cbc_encrypt_many(key, iv, np.frombuffer(plain, dtype=np.uint8).reshape(1, -1)).tobytes()


def cbc_decrypt(key: bytes, iv: bytes, cipher: bytes, pkcs7: bool = False) -> bytes:
    p = cbc_decrypt_many(key, iv, np.frombuffer(cipher, dtype=np.uint8).reshape(1, -1)).tobytes()
    if pkcs7:
        n = p[-1]
        if not 1 <= n <= BLOCK or p[-n:] != bytes([n]) * n:
            raise ValueError("bad padding")
        p = p[:-n]
    return p


# ---- the scheme (recalled; cipher_scheme.hpp) ---------------------------------------------------

def scheme_iv(cipher: bytes) -> bytes:
    return bytes(cipher[:16])


def scheme_nseg(length: int, segment: int) -> int:
    return -(-length // (segment - BLOCK))


def scheme_encrypt(buf: bytes, cipher: bytes, segment: int) -> bytes:
    """The object's ciphertext: nseg segments of `segment` bytes, each the CBC encryption (PKCS#7)
    of one zero-padded piece of segment - 16 plaintext bytes."""
    if len(cipher) not in (16, 24, 32):
        raise ValueError("cipher must be 16, 24 or 32 bytes")
    piece = segment - BLOCK
    nseg = scheme_nseg(len(buf), segment)
    plain = np.zeros((nseg, segment), dtype=np.uint8)
    flat = np.frombuffer(bytes(buf) + bytes(nseg * piece - len(buf)), dtype=np.uint8).reshape(nseg, piece)
    plain[:, :piece] = flat
    plain[:, piece:] = 16
    return cbc_encrypt_many(cipher, scheme_iv(cipher), plain).tobytes()


def scheme_decrypt(ct: bytes, cipher: bytes, segment: int, size: int) -> bytes:
    """The object back from its ciphertext; ValueError on a bad padding block."""
    piece = segment - BLOCK
    nseg = len(ct) // segment
    if not (nseg - 1) * piece < size <= nseg * piece:
        raise ValueError("size does not end in the last piece")
    p = cbc_decrypt_many(cipher, scheme_iv(cipher), np.frombuffer(ct, dtype=np.uint8).reshape(nseg, segment))
    if not (p[:, piece:] == 16).all():
        raise ValueError("bad padding")
    return p[:, :piece].tobytes()[:size]


def scheme_full_processing(buf: bytes, cipher: bytes, segment: int, data: int = 4, parity: int = 8
                           ) -> Tuple[List[bytes], List[List[bytes]], bytes, List[List[bytes]]]:
    """FullProcessing(file, cipher, savedir) restated: py_full_processing over the ciphertext."""
    from oracle import py_full_processing
    return py_full_processing(scheme_encrypt(buf, cipher, segment), segment, data, parity)
