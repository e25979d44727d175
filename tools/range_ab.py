#!/usr/bin/env python3
"""Measure the ranged restore on one MI355X: medians of 5 repeats after a warm-up.

  python tools/range_ab.py [--out profiles/range] [--segments 1,8,256] [--ranges 1,16] [--repeats 5]

Writes <out>/range_ab.jsonl (one JSON record per measurement, with every run's time; appended per
segment count so a run may be split) and <out>/README.md (tables of whatever the jsonl holds).  No
threshold is fixed here.

For objects of 1, 8 and 256 segments of 32 MiB, without a cipher and with a 16-byte key, and ranges of
1 MiB and 16 MiB in the middle of the object (pinned fragments, DM_RESTORE_VERIFY_FRAGMENTS; host
clock around the synchronous call):
  present  dm_restore_range_buffer, every needed fragment given;
  rebuilt  the same with the first needed data fragment missing: rebuilt from four others;
  full     dm_restore_buffer / dm_restore_cipher_buffer of the same object in the same session (every
           data fragment given, fragment and segment checks on).  Its code is the parent commit's.
The expectation written beside them is DESIGN.md §4.2's 8 MiB chain, 122 ms, once per leaf launch: one
launch when every needed fragment is there, two when one is rebuilt (inputs, then the rebuilt one).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEGMENT = 32 << 20
PIECE = SEGMENT - 16
TOTAL, K = 12, 4
FRAG = SEGMENT // K
KEY = bytes((37 * i + 11 * 16 + 5) & 0xFF for i in range(16))
CHAIN_MS = 122.0   # one 8 MiB SHA-256 chain
NOTES_MARK = "<!-- notes: kept by tools/range_ab.py -->\n"


def runs_ms(call, repeats):
    def once():
        t = time.perf_counter()
        call()
        return (time.perf_counter() - t) * 1e3
    once()   # warm-up
    return [round(once(), 3) for _ in range(repeats)]


class Pinned:
    def __init__(self, L, nbytes):
        self.L, self.p = L, ctypes.c_void_p()
        rc = L.dm_host_alloc(nbytes, ctypes.byref(self.p))
        if rc != 0:
            raise RuntimeError(f"dm_host_alloc({nbytes}): {rc}")

    def free(self):
        self.L.dm_host_free(self.p)


def measure(ctx, nseg, args, emit):
    from deoss_amd.process import Processor
    p = Processor(ctx)
    L, h = ctx._L, p.enc._h
    src = Pinned(L, nseg * SEGMENT)
    # not constant: equal fragments would share a name and hide a mix-up
    pat = bytes((i * 131 + (i >> 8) * 31) & 0xFF for i in range(1 << 16))
    for o in range(0, nseg * SEGMENT, len(pat)):
        ctypes.memmove(src.p.value + o, pat, len(pat))
    for s in range(nseg):   # every segment different
        ctypes.memmove(src.p.value + s * SEGMENT + 5, s.to_bytes(8, "little"), 8)
        ctypes.memmove(src.p.value + s * PIECE + 77, s.to_bytes(8, "little"), 8)
        for j in range(K):   # and every data fragment
            ctypes.memmove(src.p.value + s * SEGMENT + j * FRAG + 123, (s * K + j + 1).to_bytes(8, "little"), 8)
    frags = Pinned(L, nseg * TOTAL * FRAG)
    out = Pinned(L, nseg * SEGMENT)
    seg = ctypes.create_string_buffer(32 * nseg)
    fragn = ctypes.create_string_buffer(32 * TOTAL * nseg)
    fid = ctypes.create_string_buffer(32)
    ok = ctypes.c_int(0)
    fst = ctypes.create_string_buffer(TOTAL * nseg)

    def check(rc):
        if rc != 0:
            raise RuntimeError((L.dm_last_error(None) or b"").decode())

    def pointers(skip=None, data_only=False):
        ptrs = (ctypes.c_void_p * (nseg * TOTAL))()
        for s in range(nseg):
            for j in range(K if data_only else TOTAL):
                if (s, j) != skip:
                    ptrs[s * TOTAL + j] = frags.p.value + (s * TOTAL + j) * FRAG
        return ptrs
    for key in (b"", KEY):
        piece = PIECE if key else SEGMENT
        size = nseg * piece
        if key:
            check(L.dm_process_cipher_buffer(h, src.p, size, SEGMENT, key, len(key), frags.p, seg, fragn, fid))
        else:
            check(L.dm_process_buffer(h, src.p, size, SEGMENT, frags.p, seg, fragn, fid))
        data = pointers(data_only=True)

        def full_call():
            if key:
                check(L.dm_restore_cipher_buffer(h, data, fragn, seg, None, nseg, size, SEGMENT, 3, key, len(key), out.p,
                                                 None, None, ctypes.byref(ok)))
            else:
                check(L.dm_restore_buffer(h, data, fragn, seg, None, nseg, size, SEGMENT, 3, out.p, None, None,
                                          ctypes.byref(ok)))
            assert ok.value == 1
        full = runs_ms(full_call, args.repeats)
        base = dict(segments=nseg, segment_bytes=SEGMENT, key_bytes=len(key), object_bytes=size)
        emit(dict(base, case="full", ms=round(statistics.median(full), 2), runs_ms=full))
        for mib in args.ranges:
            length = mib << 20
            off = size // 2 - length // 2
            seg0, nt, need, _ = p.range_plan(size, off, length, cipher=key)
            nneed = sum(map(sum, need))
            first = next(j for j in range(K) if need[0][j])
            for case, ptrs in (("present", pointers()), ("rebuilt", pointers(skip=(seg0, first)))):
                def range_call():
                    check(L.dm_restore_range_buffer(h, ptrs, fragn, nseg, size, SEGMENT, off, length, 1, key or None,
                                                    len(key), out.p, fst, None, ctypes.byref(ok)))
                    assert ok.value == 1
                runs = runs_ms(range_call, args.repeats)
                assert ctypes.string_at(out.p, 4096) == ctypes.string_at(src.p.value + off, 4096)
                assert ctypes.string_at(out.p.value + length - 4096, 4096) == ctypes.string_at(src.p.value + off + length - 4096, 4096)
                st = fst.raw
                assert st.count(b"\x04") == (1 if case == "rebuilt" else 0)
                ms = statistics.median(runs)
                launches = 2 if case == "rebuilt" else 1
                emit(dict(base, case=case, range_mib=mib, off=off, fragments_needed=nneed,
                          fragments_loaded=len(st) - st.count(b"\x00") - st.count(b"\x04"), ms=round(ms, 2), runs_ms=runs,
                          expected_chain_ms=CHAIN_MS * launches, full_ms=round(statistics.median(full), 2),
                          full_over_range=round(statistics.median(full) / ms, 2)))
    for b in (src, frags, out):
        b.free()
    p.close()


def write_readme(out_dir, records):
    lines = ["# Ranged restore measurements (tools/range_ab.py)", "",
             "One MI355X; medians of 5 repeats after a warm-up, host clock around the synchronous call; pinned",
             "fragments, fragment verification on.  Every run's time: range_ab.jsonl.  `full` is dm_restore_buffer /",
             "dm_restore_cipher_buffer of the same object in the same session (all data fragments given, fragment",
             "and segment checks on); its code is unchanged by the ranged restore.  `expected` is one 8 MiB chain",
             "(122 ms, DESIGN.md §4.2) per leaf launch: one launch with every needed fragment present, two when one",
             "is rebuilt.  No threshold is set.", ""]
    for kb in sorted({r["key_bytes"] for r in records}):
        lines += [f"## {'no cipher' if kb == 0 else '%d-byte key' % kb}", "",
                  "| segments | range MiB | case | fragments needed | loaded | ms | expected chain ms | full restore ms | full / ranged |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for r in records:
            if r["key_bytes"] != kb or r["case"] == "full":
                continue
            lines.append(f"| {r['segments']} | {r['range_mib']} | {r['case']} | {r['fragments_needed']} | "
                         f"{r['fragments_loaded']} | {r['ms']} | {r['expected_chain_ms']:.0f} | {r['full_ms']} | "
                         f"{r['full_over_range']} |")
        lines.append("")
    path = os.path.join(out_dir, "README.md")
    notes = ""   # whatever follows the marker is written by hand and kept
    if os.path.exists(path) and NOTES_MARK in open(path).read():
        notes = open(path).read().split(NOTES_MARK, 1)[1]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n" + NOTES_MARK + notes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range"))
    ap.add_argument("--segments", default="1,8,256")
    ap.add_argument("--ranges", default="1,16")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    args.segments = [int(x) for x in args.segments.split(",")]
    args.ranges = [int(x) for x in args.ranges.split(",")]
    import torch
    from deoss_amd import MerkleContext
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "range_ab.jsonl")
    records = []
    if os.path.exists(path):   # a split run: keep the other segment counts' records
        records = [json.loads(ln) for ln in open(path) if ln.strip()]
        records = [r for r in records if r["segments"] not in args.segments]

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)
        with open(path, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in records)
    with MerkleContext() as ctx:
        for nseg in args.segments:
            measure(ctx, nseg, args, emit)
    records.sort(key=lambda r: (r["key_bytes"], r["segments"], r.get("range_mib", 0), r["case"]))
    write_readme(args.out, records)


if __name__ == "__main__":
    main()
