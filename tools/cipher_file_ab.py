#!/usr/bin/env python3
"""Measure FullProcessing(file, cipher, savedir) from the file path on one MI355X.

  python tools/cipher_file_ab.py [--out profiles/cipher] [--pieces 1,8,64,257] [--repeats 5]
                                 [--variants a,b,c,d] [--windows-repeats N] [--dir DIR]

A file of N pieces of 32 MiB - 16 bytes (N segments of ciphertext) in /dev/shm (page cache), savedir
beside it, emptied (untimed) before every call; the host clock around the call; medians after one
warm-up call.  16-byte key, and a 32-byte key at the largest file.

  a  Processor.FullProcessing(file, cipher, savedir) with DEOSS_FP_STRIPES=1: one
     dm_full_processing_cipher call, each stripe encrypted as it lands, the hash chains behind it;
  b  Processor.FullProcessingWindows, same file and key: the window path (8 pieces per
     dm_process_cipher_buffer call, fragments written from Python);
  c  the same call with DEOSS_FP_STRIPES=0: whole chains encrypted, then hashed -- what the
     stripes buy (this order is the call's default with a cipher);
  d  dm_full_processing on the same file without a cipher -- what the cipher costs.

Appends its records (part "file") to <out>/cipher_file_ab.jsonl and writes <out>/FILE_PATH.md, a
table of whatever the jsonl holds.  --windows-repeats bounds the repeats of (b), whose every run at
257 pieces is about a minute.  No threshold is fixed here.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEGMENT = 32 << 20
PIECE = SEGMENT - 16
KEYS = {n: bytes((37 * i + 11 * n + 5) & 0xFF for i in range(n)) for n in (16, 32)}


def write_file(path, pieces):
    """pieces x PIECE + 12,345 bytes less than a whole last piece: the last one is zero-padded."""
    import numpy as np
    rng = np.random.default_rng(0xF11E + pieces)
    left = pieces * PIECE - 12345 if pieces > 1 else PIECE - 12345
    with open(path, "wb") as f:
        while left:
            n = min(left, 64 << 20)
            f.write(rng.integers(0, 256, size=n, dtype=np.uint8).tobytes())
            left -= n
    return os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cipher"))
    ap.add_argument("--pieces", default="1,8,64,257")
    ap.add_argument("--variants", default="a,b,c,d")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--windows-repeats", type=int, default=None)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    pieces = [int(x) for x in args.pieces.split(",")]
    variants = args.variants.split(",")
    import torch
    from deoss_amd import MerkleContext
    from deoss_amd.process import Processor
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "cipher_file_ab.jsonl")
    records = [json.loads(ln) for ln in open(path) if ln.strip()] if os.path.exists(path) else []
    need = max(pieces) * SEGMENT * 5 + (1 << 30)   # the file, 12 fragments of a quarter segment and the segment file
    base = args.dir or ("/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > need else None)
    d = tempfile.mkdtemp(prefix="deoss_cfab_", dir=base)
    savedir = os.path.join(d, "frags")

    def emit(rec):
        records[:] = [r for r in records if (r["variant"], r["pieces"], r["key_bytes"]) !=
                      (rec["variant"], rec["pieces"], rec["key_bytes"])] + [rec]
        print(json.dumps(rec), flush=True)
        with open(path, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in records)

    def timed(call):
        shutil.rmtree(savedir, ignore_errors=True)
        t = time.perf_counter()
        info, fid, err = call()
        ms = (time.perf_counter() - t) * 1e3
        if err is not None:
            raise RuntimeError(str(err))
        return ms, fid, len(info)

    try:
        with MerkleContext() as ctx:
            p = Processor(ctx)
            for n in pieces:
                f = os.path.join(d, "object.bin")
                size = write_file(f, n)
                keys = [16, 32] if n == max(pieces) and len(pieces) > 1 else [16]
                for klen in keys:
                    key = KEYS[klen]
                    fids = {}
                    for v in variants:
                        if v == "d" and klen != 16:
                            continue
                        os.environ.pop("DEOSS_FP_STRIPES", None)
                        if v in ("a", "c"):
                            os.environ["DEOSS_FP_STRIPES"] = "1" if v == "a" else "0"
                        call = {"a": lambda: p.FullProcessing(f, key, savedir),
                                "b": lambda: p.FullProcessingWindows(f, key, savedir),
                                "c": lambda: p.FullProcessing(f, key, savedir),
                                "d": lambda: p.FullProcessing(f, "", savedir)}[v]
                        reps = args.repeats if v != "b" or args.windows_repeats is None else args.windows_repeats
                        warm, fids[v], nseg = timed(call)
                        runs = [timed(call)[0] for _ in range(reps)] or [warm]
                        os.environ.pop("DEOSS_FP_STRIPES", None)
                        emit(dict(part="file", variant=v, pieces=n, key_bytes=klen, file_bytes=size, segments=nseg,
                                  segment_bytes=SEGMENT, repeats=reps, warmup_ms=round(warm, 1),
                                  median_ms=round(statistics.median(runs), 1), min_ms=round(min(runs), 1),
                                  max_ms=round(max(runs), 1), runs_ms=[round(x, 1) for x in runs],
                                  gib_per_s=round(size / 2**30 / (statistics.median(runs) / 1e3), 3),
                                  dir=base or "the temp dir"))
                    same = {fids[v] for v in ("a", "b", "c") if v in fids}
                    assert len(same) <= 1, f"the cipher paths disagree on the fid at {n} pieces: {fids}"
                os.unlink(f)
            p.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    what = {"a": "one call, DEOSS_FP_STRIPES=1", "b": "window path", "c": "one call, DEOSS_FP_STRIPES=0", "d": "plain dm_full_processing"}
    lines = ["# FullProcessing(file, cipher, savedir) from the file path (tools/cipher_file_ab.py)", "",
             "One MI355X; the file and savedir in the page cache; host clock around the call; medians after one",
             "warm-up call.  Records: cipher_file_ab.jsonl.", "",
             "| pieces | key bytes | variant | repeats | median ms | min ms | max ms | GiB/s of file |", "|---|---|---|---|---|---|---|---|"]
    for r in sorted(records, key=lambda r: (r["pieces"], r["key_bytes"], r["variant"])):
        lines.append(f"| {r['pieces']} | {r['key_bytes']} | {r['variant']}: {what[r['variant']]} | {r['repeats']} | "
                     f"{r['median_ms']} | {r['min_ms']} | {r['max_ms']} | {r['gib_per_s']} |")
    with open(os.path.join(args.out, "FILE_PATH.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
