#!/usr/bin/env python3
"""Measure the batched restore on one MI355X ("Many objects in one pass"): medians
of 5 rounds after a warm-up, the variants of a part interleaved round by round in one session, every
timed call's output compared with the original.

  python tools/restore_batch_ab.py [--out profiles/restore] [--parts kernel,mixed,downloads,batch]
                                   [--rounds 5] [--downloads 1,8,64]

Writes <out>/batch_ab.jsonl (one JSON record per figure; a split run keeps the other parts' records)
and <out>/BATCH.md (a table of whatever the jsonl holds; the headline benchmark's lines are kept).

  kernel     aes_cbc_decrypt_keyed_kernel against aes_cbc_decrypt_kernel over the same buffers: 256
             chains of 32 MiB, one key, each key length (HIP events).  Expected equal within the
             single-key kernel's min-max spread: both are bound by LDS lookups.  No threshold.
  mixed      3 x 16 chains of three key lengths: ONE keyed launch against three single-key launches
             back to back on one stream.  No threshold.
  downloads  THE GATE.  c concurrent verified restores of one 32 MiB segment each (2 data + 2 parity
             fragments supplied, DM_RESTORE_VERIFY_ALL, every second one encrypted under a key of its
             own), host clock from the start of all c threads until all are done.  A: through
             dm_batcher_restore (one batcher, 4 slots, 2 ms linger); B: c threads calling
             dm_restore_buffer / dm_restore_cipher_buffer on a four-lane context -- what the library
             could do before.  At the largest c, A's median must beat B's by more than B's min-max
             spread (exit status 1 if not).  At c = 1 A - B is reported: the linger and a pageable
             source make A slower there.
  batch      dm_restore_batch of 64 one-segment objects against ONE dm_restore_buffer of a 64-segment
             object made of the same segments: the same device work, so the difference is the batch
             bookkeeping's own cost, reported against the single call's spread.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEGMENT = 32 << 20
PIECE = SEGMENT - 16
K, M = 4, 8
FRAG = SEGMENT // K
KLENS = (16, 24, 32)
GIVEN = (1, 3, 5, 9)   # 2 data + 2 parity fragments of the 12: two data fragments are rebuilt
VALL = 7


def key_of(tag: int, klen: int) -> bytes:
    return bytes((tag * 29 + 37 * i + 11 * klen + 5) & 0xFF for i in range(klen))


def event_ms(torch, launch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    launch()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved(variants, rounds):
    """{name: [ms per round]}: one warm-up of every variant, then `rounds` rounds, each running
    every variant once in turn."""
    for fn in variants.values():
        fn()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(fn())
    return times


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3),
                spread_ms=round(max(ms) - min(ms), 3), rounds_ms=[round(x, 3) for x in ms])


def cell(s):
    return f"{s['median_ms']} ({s['min_ms']} .. {s['max_ms']})"


# ---- the decrypt kernels ---------------------------------------------------------------------------

def part_kernel(torch, ctx, args, emit):
    n = 256
    src = torch.empty(n * SEGMENT, dtype=torch.uint8, device="cuda")
    a = torch.empty(n * PIECE, dtype=torch.uint8, device="cuda")
    b = torch.empty(n * PIECE, dtype=torch.uint8, device="cuda")
    pa = torch.empty(n, dtype=torch.uint8, device="cuda")
    pb = torch.empty(n, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.fill_synthetic_async(src.data_ptr(), 0, src.numel(), 0xD1C0DE, stream)
    chains = [(src.data_ptr() + c * SEGMENT, b.data_ptr() + c * PIECE, 0) for c in range(n)]
    for klen in KLENS:
        key = key_of(1, klen)
        t = interleaved({
            "single": lambda: event_ms(torch, lambda: ctx.aes_cbc_decrypt_device_async(
                key, key[:16], src.data_ptr(), SEGMENT, SEGMENT, n, a.data_ptr(), PIECE, pa.data_ptr(), stream)),
            "keyed": lambda: event_ms(torch, lambda: ctx.aes_cbc_decrypt_keyed_device_async(
                [(key, key[:16])], chains, SEGMENT, pb.data_ptr(), stream)),
        }, args.rounds)
        assert torch.equal(a, b) and torch.equal(pa, pb), "the two kernels disagree"
        s, k = summary(t["single"]), summary(t["keyed"])
        diff = k["median_ms"] - s["median_ms"]
        emit(dict(part="kernel", chains=n, key_bytes=klen, chain_bytes=SEGMENT, single=s, keyed=k,
                  keyed_minus_single_ms=round(diff, 3), keyed_over_single=round(k["median_ms"] / s["median_ms"], 4),
                  within_single_spread=abs(diff) <= s["spread_ms"]))


def part_mixed(torch, ctx, args, emit):
    per = 16
    n = 3 * per
    src = torch.empty(n * SEGMENT, dtype=torch.uint8, device="cuda")
    a = torch.empty(n * PIECE, dtype=torch.uint8, device="cuda")
    b = torch.empty(n * PIECE, dtype=torch.uint8, device="cuda")
    pa = torch.empty(n, dtype=torch.uint8, device="cuda")
    pb = torch.empty(n, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.fill_synthetic_async(src.data_ptr(), 0, src.numel(), 0x5EED, stream)
    keys = [(key_of(10 + g, KLENS[g]), key_of(10 + g, 16)) for g in range(3)]
    # chain c belongs to group c // 16; the keyed launch gets them interleaved, as a batch would
    order = [g * per + i for i in range(per) for g in range(3)]
    chains = [(src.data_ptr() + c * SEGMENT, b.data_ptr() + c * PIECE, c // per) for c in order]

    def three_launches():
        for g in range(3):
            ctx.aes_cbc_decrypt_device_async(keys[g][0], keys[g][1], src.data_ptr() + g * per * SEGMENT, SEGMENT, SEGMENT,
                                             per, a.data_ptr() + g * per * PIECE, PIECE, pa.data_ptr() + g * per, stream)
    t = interleaved({
        "one_keyed_launch": lambda: event_ms(torch, lambda: ctx.aes_cbc_decrypt_keyed_device_async(
            keys, chains, SEGMENT, pb.data_ptr(), stream)),
        "three_single_key_launches": lambda: event_ms(torch, three_launches),
    }, args.rounds)
    assert torch.equal(a, b), "the two paths disagree"
    # the keyed launch writes verdict i for chain i of ITS list: undo the interleaving before comparing
    assert torch.equal(pa[torch.tensor(order, device="cuda")], pb), "the two paths disagree on a verdict"
    one, three = summary(t["one_keyed_launch"]), summary(t["three_single_key_launches"])
    emit(dict(part="mixed", chains_per_key_length=per, chain_bytes=SEGMENT, one_keyed_launch=one,
              three_single_key_launches=three, three_over_one=round(three["median_ms"] / one["median_ms"], 3)))


# ---- restores ----------------------------------------------------------------------------------------

class Download:
    """One object of one segment as a download handler holds it: 4 of its 12 fragments, its names."""

    def __init__(self, proc, body: bytes, cipher: bytes):
        self.body, self.cipher, self.size = body, cipher, len(body)
        segd, fragd, fid, frags = proc.process_buffer(body, want_frags=True, cipher=cipher)
        assert len(segd) == 32, "one segment per object"
        self.segd, self.fragd, self.fid = segd, fragd, fid
        self.frags = [frags[j * FRAG:(j + 1) * FRAG] if j in GIVEN else None for j in range(K + M)]

    def args(self):
        return dict(frags=self.frags, size=self.size, frag_names=self.fragd, seg_names=self.segd, fid=self.fid,
                    flags=VALL, cipher=self.cipher)


def body_of(i: int, n: int) -> bytes:
    import numpy as np
    return np.random.default_rng(7000 + i).integers(0, 256, n, dtype=np.uint8).tobytes()


def wall(c, one):
    """ms from the start of c threads until all are done, and what each returned."""
    res = [None] * c
    start = threading.Barrier(c + 1)

    def run(i):
        start.wait()
        res[i] = one(i)
    ts = [threading.Thread(target=run, args=(i,)) for i in range(c)]
    for t in ts:
        t.start()
    start.wait()
    t0 = time.perf_counter()
    for t in ts:
        t.join()
    return (time.perf_counter() - t0) * 1e3, res


def part_downloads(torch, ctx, args, emit):
    from deoss_amd import MerkleContext
    from deoss_amd.batcher import RESTORE, Batcher
    from deoss_amd.process import Processor
    cmax = max(args.downloads)
    lanes = MerkleContext(lanes=4)
    proc = Processor(lanes)
    # every second download is encrypted, each under a key of its own
    dl = [Download(proc, body_of(i, PIECE if i % 2 else SEGMENT), key_of(2000 + i, KLENS[(i // 2) % 3]) if i % 2 else b"")
          for i in range(cmax)]
    batcher = Batcher(RESTORE, SEGMENT, K, M, device=0, slots=4, linger_us=2000)
    gate = True

    def checked(c, res):
        for i in range(c):
            assert res[i][0] and res[i][1] == dl[i].body, f"download {i} did not give the original back"
    try:
        for c in args.downloads:
            def via_batcher():
                ms, res = wall(c, lambda i: batcher.restore(**dl[i].args()))
                checked(c, res)
                return ms

            def via_lanes():
                ms, res = wall(c, lambda i: proc.restore_buffer(**dl[i].args()))
                checked(c, res)
                return ms
            t = interleaved({"A_batcher": via_batcher, "B_four_lanes": via_lanes}, args.rounds)
            a, b = summary(t["A_batcher"]), summary(t["B_four_lanes"])
            rec = dict(part="downloads", downloads=c, segment_bytes=SEGMENT, A_batcher=a, B_four_lanes=b,
                       A_minus_B_ms=round(a["median_ms"] - b["median_ms"], 3),
                       B_over_A=round(b["median_ms"] / a["median_ms"], 2),
                       downloads_per_s_A=round(c / (a["median_ms"] / 1e3), 2),
                       downloads_per_s_B=round(c / (b["median_ms"] / 1e3), 2))
            if c == cmax and c > 1:
                rec["gate_A_beats_B_by_more_than_B_spread"] = gate = b["median_ms"] - a["median_ms"] > b["spread_ms"]
            emit(rec)
        requests, batches, largest = batcher.stats()
        emit(dict(part="downloads_batcher_stats", requests=requests, batches=batches, largest_batch=largest))
    finally:
        batcher.close()
        proc.close()
        lanes.close()
    return gate


def part_batch(torch, ctx, args, emit):
    from deoss_amd.process import Processor
    n = 64
    proc = Processor(ctx)
    dl = [Download(proc, body_of(100 + i, SEGMENT), b"") for i in range(n)]
    whole = b"".join(d.body for d in dl)
    fid = proc.process_buffer(whole, want_frags=False)[2]
    frags = [d.frags for d in dl]
    fragd, segd = b"".join(d.fragd for d in dl), b"".join(d.segd for d in dl)
    batch_args = [d.args() for d in dl]

    def batch():
        t0 = time.perf_counter()
        res = proc.restore_batch(batch_args)
        ms = (time.perf_counter() - t0) * 1e3
        assert all(r[0] and r[1] == d.body for r, d in zip(res, dl)), "the batch did not give the originals back"
        return ms

    def single():
        t0 = time.perf_counter()
        ok, data, _, _ = proc.restore_buffer(frags, len(whole), fragd, segd, fid, VALL)
        ms = (time.perf_counter() - t0) * 1e3
        assert ok and data == whole, "the single call did not give the original back"
        return ms
    try:
        t = interleaved({"batch_of_64": batch, "one_object_of_64_segments": single}, args.rounds)
        bt, sg = summary(t["batch_of_64"]), summary(t["one_object_of_64_segments"])
        diff = bt["median_ms"] - sg["median_ms"]
        emit(dict(part="batch", objects=n, segment_bytes=SEGMENT, batch_of_64=bt, one_object_of_64_segments=sg,
                  batch_minus_single_ms=round(diff, 3), within_single_spread=abs(diff) <= sg["spread_ms"]))
    finally:
        proc.close()


def write_table(out_dir, records):
    path = os.path.join(out_dir, "BATCH.md")
    keep = []   # the headline benchmark's section is written by hand from bench.py's lines: kept
    if os.path.exists(path):
        text = open(path).read()
        at = text.find("## The headline")
        if at >= 0:
            keep = [text[at:].rstrip("\n"), ""]
    lines = ["# Batched restore: measurements (tools/restore_batch_ab.py)", "",
             "One MI355X; medians of 5 rounds after a warm-up, the variants of a part interleaved round by round in",
             "one session, every timed call's output compared with the original.  Kernel times are HIP events,",
             "restore times the host clock.  Records: batch_ab.jsonl.", ""]
    ker = [r for r in records if r["part"] == "kernel"]
    if ker:
        lines += ["## aes_cbc_decrypt_keyed_kernel against aes_cbc_decrypt_kernel, 256 chains of 32 MiB, one key", "",
                  "| key bytes | single-key ms (min .. max) | keyed ms (min .. max) | keyed - single ms | within single's spread |",
                  "|---|---|---|---|---|"]
        lines += [f"| {r['key_bytes']} | {cell(r['single'])} | {cell(r['keyed'])} | {r['keyed_minus_single_ms']} | "
                  f"{'yes' if r['within_single_spread'] else 'no'} |" for r in ker]
        lines.append("")
    for r in (r for r in records if r["part"] == "mixed"):
        lines += ["## Mixed key lengths: 16 chains of 32 MiB per length", "", "| variant | ms (min .. max) |", "|---|---|",
                  f"| 48 chains, three key lengths, ONE keyed launch | {cell(r['one_keyed_launch'])} |",
                  f"| three single-key launches back to back | {cell(r['three_single_key_launches'])} |", "",
                  f"three / one = {r['three_over_one']}.", ""]
    dn = [r for r in records if r["part"] == "downloads"]
    if dn:
        lines += ["## Concurrent verified downloads of one 32 MiB segment (2 + 2 fragments, VERIFY_ALL, half encrypted): "
                  "wall time until all are done", "",
                  "| downloads | A: dm_batcher_restore ms (min .. max) | B: single calls, 4 lanes ms (min .. max) | A - B ms | B / A | downloads/s A | downloads/s B |",
                  "|---|---|---|---|---|---|---|"]
        lines += [f"| {r['downloads']} | {cell(r['A_batcher'])} | {cell(r['B_four_lanes'])} | {r['A_minus_B_ms']} | "
                  f"{r['B_over_A']} | {r['downloads_per_s_A']} | {r['downloads_per_s_B']} |" for r in dn]
        lines.append("")
        for r in dn:
            if "gate_A_beats_B_by_more_than_B_spread" in r:
                lines += [f"The gate at {r['downloads']} downloads: B - A = {-r['A_minus_B_ms']} ms against B's spread of "
                          f"{r['B_four_lanes']['spread_ms']} ms: it "
                          f"{'holds' if r['gate_A_beats_B_by_more_than_B_spread'] else 'FAILS'}.", ""]
        for r in (r for r in records if r["part"] == "downloads_batcher_stats"):
            lines += [f"The batcher over the whole part: {r['requests']} requests in {r['batches']} batches, the largest of "
                      f"{r['largest_batch']}.", ""]
    for r in (r for r in records if r["part"] == "batch"):
        lines += ["## dm_restore_batch of 64 one-segment objects against one dm_restore_buffer of 64 segments", "",
                  "| variant | ms (min .. max) |", "|---|---|",
                  f"| dm_restore_batch, 64 objects | {cell(r['batch_of_64'])} |",
                  f"| dm_restore_buffer, one object of 64 segments | {cell(r['one_object_of_64_segments'])} |", "",
                  f"batch - single = {r['batch_minus_single_ms']} ms against the single call's spread of "
                  f"{r['one_object_of_64_segments']['spread_ms']} ms"
                  f" ({'inside' if r['within_single_spread'] else 'outside'} it).", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines + keep))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "restore"))
    ap.add_argument("--parts", default="kernel,mixed,downloads,batch")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--downloads", default="1,8,64")
    args = ap.parse_args()
    args.downloads = [int(x) for x in args.downloads.split(",")]
    import torch
    from deoss_amd import MerkleContext
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "batch_ab.jsonl")
    parts = args.parts.split(",")
    records = []
    if os.path.exists(path):   # a split run: keep the other parts' records
        records = [json.loads(ln) for ln in open(path) if ln.strip()]
        records = [r for r in records if r["part"].split("_batcher_stats")[0] not in parts]

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)
        with open(path, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in records)
    gate = True
    with MerkleContext() as ctx:
        for part in parts:
            ok = {"kernel": part_kernel, "mixed": part_mixed, "downloads": part_downloads, "batch": part_batch}[part](
                torch, ctx, args, emit)
            if part == "downloads":
                gate = bool(ok)
            torch.cuda.empty_cache()
    write_table(args.out, records)
    return 0 if gate else 1


if __name__ == "__main__":
    sys.exit(main())
