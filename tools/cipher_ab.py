#!/usr/bin/env python3
"""Measure the cipher branch on one MI355X: medians of 5 repeats after a warm-up.

  python tools/cipher_ab.py [--out profiles/cipher] [--parts encrypt,decrypt,process,restore]
                            [--segments 1,8,256] [--repeats 5]

Writes <out>/cipher_ab.jsonl (one JSON record per measurement, appended per part so a run may be
split) and <out>/README.md (a table of whatever the jsonl holds).  No threshold is fixed here.

  encrypt  aes_cbc_encrypt_kernel, ns per AES block on one chain, keys of 16 / 24 / 32 bytes, 1 and
           256 segments of 32 MiB (HIP events), beside the model of ~90 cycles per round;
  decrypt  aes_cbc_decrypt_kernel, GiB/s over 256 x 32 MiB, beside dm_read_probe_async over the same
           buffer in the same run (HIP events);
  process  dm_process_cipher_buffer against dm_process_buffer of the same build (pinned source, no
           fragment copy-out; host clock around the synchronous call), and one CPU core doing the
           same AES-CBC through OpenSSL's EVP when libcrypto is there;
  restore  dm_restore_cipher_buffer against dm_restore_buffer (two data fragments per segment
           missing, every check on; pinned fragments; host clock).
"""
from __future__ import annotations

import argparse
import ctypes
import ctypes.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEGMENT = 32 << 20
PIECE = SEGMENT - 16
KEYS = {n: bytes((37 * i + 11 * n + 5) & 0xFF for i in range(n)) for n in (16, 24, 32)}
MODEL_CYCLES_PER_ROUND = 90.0


def median_ms(fn, repeats):
    fn()   # warm-up
    return statistics.median(fn() for _ in range(repeats))


def event_ms(torch, launch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    launch()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_ms(call):
    t = time.perf_counter()
    call()
    return (time.perf_counter() - t) * 1e3


def clock_mhz(torch):
    khz = getattr(torch.cuda.get_device_properties(0), "clock_rate", 0)
    return khz / 1e3 if khz else 2400.0


def part_encrypt(torch, ctx, args, emit):
    mhz = clock_mhz(torch)
    nmax = max(s for s in args.encrypt_segments)
    buf = torch.empty(nmax * SEGMENT, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.fill_synthetic_async(buf.data_ptr(), 0, buf.numel(), 0xC1F4E5, stream)
    nblk = PIECE // 16 + 1   # the padding block is encrypted too
    for nseg in args.encrypt_segments:
        for klen, key in KEYS.items():
            ms = median_ms(lambda: event_ms(torch, lambda: ctx.aes_cbc_encrypt_device_async(
                key, key[:16], buf.data_ptr(), SEGMENT, PIECE, nseg, stream)), args.repeats)
            rounds = klen // 4 + 6
            ns_block = ms * 1e6 / nblk
            model = rounds * MODEL_CYCLES_PER_ROUND / mhz * 1e3
            emit(dict(part="encrypt", key_bytes=klen, segments=nseg, segment_bytes=SEGMENT, ms=round(ms, 3),
                      ns_per_block=round(ns_block, 1), cycles_per_round=round(ns_block * mhz / 1e3 / rounds, 1),
                      model_ns_per_block=round(model, 1), over_model=round(ns_block / model, 3), clock_mhz=mhz,
                      gib_per_s=round(nseg * SEGMENT / 2**30 / (ms / 1e3), 2)))


def part_decrypt(torch, ctx, args, emit):
    nseg = 256
    src = torch.empty(nseg * SEGMENT, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nseg * PIECE, dtype=torch.uint8, device="cuda")
    ok = torch.zeros(nseg, dtype=torch.uint8, device="cuda")
    x8 = torch.zeros(8, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.fill_synthetic_async(src.data_ptr(), 0, src.numel(), 0xDEC0DE, stream)
    gib = nseg * SEGMENT / 2**30
    for klen, key in KEYS.items():
        ms = median_ms(lambda: event_ms(torch, lambda: ctx.aes_cbc_decrypt_device_async(
            key, key[:16], src.data_ptr(), SEGMENT, SEGMENT, nseg, dst.data_ptr(), PIECE, ok.data_ptr(), stream)),
            args.repeats)
        probe = median_ms(lambda: event_ms(torch, lambda: ctx.read_probe_async(
            src.data_ptr(), src.numel(), x8.data_ptr(), stream)), args.repeats)
        emit(dict(part="decrypt", key_bytes=klen, segments=nseg, segment_bytes=SEGMENT, ms=round(ms, 3),
                  gib_per_s=round(gib / (ms / 1e3), 1), read_probe_ms=round(probe, 3),
                  read_probe_gib_per_s=round(gib / (probe / 1e3), 1)))


def openssl_gib_per_s(key, nbytes=64 << 20):
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        L = ctypes.CDLL(name)
        for f in ("EVP_CIPHER_CTX_new", "EVP_aes_128_cbc", "EVP_aes_192_cbc", "EVP_aes_256_cbc"):
            getattr(L, f).restype = ctypes.c_void_p
        L.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]
        L.EVP_EncryptInit_ex.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_char_p, ctypes.c_char_p]
        L.EVP_EncryptUpdate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                                        ctypes.c_void_p, ctypes.c_int]
        cipher = {16: L.EVP_aes_128_cbc, 24: L.EVP_aes_192_cbc, 32: L.EVP_aes_256_cbc}[len(key)]()
        src, dst = ctypes.create_string_buffer(nbytes), ctypes.create_string_buffer(nbytes + 32)
        n = ctypes.c_int(0)

        def once():
            c = L.EVP_CIPHER_CTX_new()
            L.EVP_EncryptInit_ex(c, cipher, None, key, key[:16])
            t = time.perf_counter()
            L.EVP_EncryptUpdate(c, dst, ctypes.byref(n), src, nbytes)
            dt = time.perf_counter() - t
            L.EVP_CIPHER_CTX_free(c)
            return dt
        once()
        return nbytes / 2**30 / statistics.median(once() for _ in range(5))
    except (OSError, AttributeError):
        return None


class Pinned:
    def __init__(self, L, nbytes):
        self.L, self.p = L, ctypes.c_void_p()
        rc = L.dm_host_alloc(nbytes, ctypes.byref(self.p))
        if rc != 0:
            raise RuntimeError(f"dm_host_alloc({nbytes}): {rc}")

    def free(self):
        self.L.dm_host_free(self.p)


def part_process(torch, ctx, args, emit):
    from deoss_amd.process import Processor
    p = Processor(ctx)
    L, h = ctx._L, p.enc._h
    nmax = max(args.segments)
    src = Pinned(L, nmax * SEGMENT)
    ctypes.memset(src.p, 0x5C, nmax * SEGMENT)
    seg = ctypes.create_string_buffer(32 * nmax)
    frag = ctypes.create_string_buffer(32 * 12 * nmax)
    fid = ctypes.create_string_buffer(32)
    cpu = {klen: openssl_gib_per_s(key) for klen, key in KEYS.items()}

    def check(rc):
        if rc != 0:
            raise RuntimeError((L.dm_last_error(None) or b"").decode())
    for nseg in args.segments:
        plain = median_ms(lambda: wall_ms(lambda: check(L.dm_process_buffer(
            h, src.p, nseg * SEGMENT, SEGMENT, None, seg, frag, fid))), args.repeats)
        for klen, key in KEYS.items():
            # the same number of segments: nseg pieces of plaintext
            ms = median_ms(lambda: wall_ms(lambda: check(L.dm_process_cipher_buffer(
                h, src.p, nseg * PIECE, SEGMENT, key, klen, None, seg, frag, fid))), args.repeats)
            rec = dict(part="process", key_bytes=klen, segments=nseg, segment_bytes=SEGMENT, cipher_ms=round(ms, 2),
                       plain_ms=round(plain, 2), cipher_cost_ms=round(ms - plain, 2))
            if cpu[klen]:
                rec["openssl_one_core_gib_per_s"] = round(cpu[klen], 3)
                rec["openssl_one_core_ms"] = round(nseg * PIECE / 2**30 / cpu[klen] * 1e3, 2)
            emit(rec)
    src.free()
    p.close()


def part_restore(torch, ctx, args, emit):
    from deoss_amd.process import Processor
    p = Processor(ctx)
    L, h = ctx._L, p.enc._h
    nmax = max(args.segments)
    total, fsz = 12, SEGMENT // 4
    src = Pinned(L, nmax * SEGMENT)
    ctypes.memset(src.p, 0x5C, nmax * SEGMENT)
    frags = Pinned(L, nmax * total * fsz)
    out = Pinned(L, nmax * SEGMENT)
    seg = ctypes.create_string_buffer(32 * nmax)
    fragn = ctypes.create_string_buffer(32 * total * nmax)
    fid = ctypes.create_string_buffer(32)
    ok = ctypes.c_int(0)

    def check(rc):
        if rc != 0:
            raise RuntimeError((L.dm_last_error(None) or b"").decode())

    def pointers(nseg):   # data fragments 0 and 1 of every segment are missing; 2, 3 and two parity are there
        ptrs = (ctypes.c_void_p * (nseg * total))()
        for s in range(nseg):
            for j in (2, 3, 4, 5):
                ptrs[s * total + j] = frags.p.value + (s * total + j) * fsz
        return ptrs
    for nseg in args.segments:
        ptrs = pointers(nseg)
        check(L.dm_process_buffer(h, src.p, nseg * SEGMENT, SEGMENT, frags.p, seg, fragn, fid))

        def plain_call():
            check(L.dm_restore_buffer(h, ptrs, fragn, seg, fid, nseg, nseg * SEGMENT, SEGMENT, 7, out.p, None, None,
                                      ctypes.byref(ok)))
            assert ok.value == 1
        plain = median_ms(lambda: wall_ms(plain_call), args.repeats)
        for klen, key in KEYS.items():
            check(L.dm_process_cipher_buffer(h, src.p, nseg * PIECE, SEGMENT, key, klen, frags.p, seg, fragn, fid))

            def cipher_call():
                check(L.dm_restore_cipher_buffer(h, ptrs, fragn, seg, fid, nseg, nseg * PIECE, SEGMENT, 7, key, klen,
                                                 out.p, None, None, ctypes.byref(ok)))
                assert ok.value == 1
            ms = median_ms(lambda: wall_ms(cipher_call), args.repeats)
            assert ctypes.string_at(out.p, 64) == bytes([0x5C]) * 64
            emit(dict(part="restore", key_bytes=klen, segments=nseg, segment_bytes=SEGMENT, cipher_ms=round(ms, 2),
                      plain_ms=round(plain, 2), cipher_cost_ms=round(ms - plain, 2)))
    for b in (src, frags, out):
        b.free()
    p.close()


def write_readme(out_dir, records):
    lines = ["# Cipher branch measurements (tools/cipher_ab.py)", "",
             "One MI355X; medians of 5 repeats after a warm-up.  Device-level parts are timed with HIP events,",
             "the host calls with the host clock around the synchronous call.  Records: cipher_ab.jsonl.", ""]
    enc = [r for r in records if r["part"] == "encrypt"]
    if enc:
        lines += ["## aes_cbc_encrypt_kernel: one chain per 32 MiB segment", "",
                  "| key bytes | segments | ms | ns / block | cycles / round | model ns / block | measured / model | GiB/s |",
                  "|---|---|---|---|---|---|---|---|"]
        lines += [f"| {r['key_bytes']} | {r['segments']} | {r['ms']} | {r['ns_per_block']} | {r['cycles_per_round']} | "
                  f"{r['model_ns_per_block']} | {r['over_model']} | {r['gib_per_s']} |" for r in enc]
        lines.append("")
    dec = [r for r in records if r["part"] == "decrypt"]
    if dec:
        lines += ["## aes_cbc_decrypt_kernel over 256 x 32 MiB, beside dm_read_probe_async", "",
                  "| key bytes | ms | GiB/s | read probe ms | read probe GiB/s |", "|---|---|---|---|---|"]
        lines += [f"| {r['key_bytes']} | {r['ms']} | {r['gib_per_s']} | {r['read_probe_ms']} | {r['read_probe_gib_per_s']} |"
                  for r in dec]
        lines.append("")
    for part, a, b in (("process", "dm_process_cipher_buffer", "dm_process_buffer"),
                       ("restore", "dm_restore_cipher_buffer", "dm_restore_buffer")):
        rs = [r for r in records if r["part"] == part]
        if not rs:
            continue
        lines += [f"## {a} against {b}", "",
                  "| key bytes | segments | cipher ms | plain ms | cipher cost ms | one OpenSSL core ms |", "|---|---|---|---|---|---|"]
        lines += [f"| {r['key_bytes']} | {r['segments']} | {r['cipher_ms']} | {r['plain_ms']} | {r['cipher_cost_ms']} | "
                  f"{r.get('openssl_one_core_ms', 'n/a')} |" for r in rs]
        lines.append("")
    with open(os.path.join(out_dir, "README.md"), "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cipher"))
    ap.add_argument("--parts", default="encrypt,decrypt,process,restore")
    ap.add_argument("--segments", default="1,8,256")
    ap.add_argument("--encrypt-segments", default="1,256")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    args.segments = [int(x) for x in args.segments.split(",")]
    args.encrypt_segments = [int(x) for x in args.encrypt_segments.split(",")]
    import torch
    from deoss_amd import MerkleContext
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "cipher_ab.jsonl")
    parts = args.parts.split(",")
    records = []
    if os.path.exists(path):   # a split run: keep the other parts' records
        records = [json.loads(ln) for ln in open(path) if ln.strip()]
        records = [r for r in records if r["part"] not in parts]

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)
        with open(path, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in records)
    with MerkleContext() as ctx:
        for part in parts:
            {"encrypt": part_encrypt, "decrypt": part_decrypt, "process": part_process,
             "restore": part_restore}[part](torch, ctx, args, emit)
    write_readme(args.out, records)


if __name__ == "__main__":
    main()
