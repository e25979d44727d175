#!/usr/bin/env python3
"""Measure the keyed AES-CBC launch (a key per chain) on one MI355X: medians of 5
rounds after a warm-up, the variants of a part interleaved round by round in one session.

  python tools/cipher_keyed_ab.py [--out profiles/cipher] [--parts kernel,mixed,uploads]
                                  [--rounds 5] [--uploads 1,8,64]

Writes <out>/keyed_ab.jsonl (one JSON record per figure; a split run keeps the other parts' records)
and <out>/KEYED.md (a table of whatever the jsonl holds).

  kernel   aes_cbc_encrypt_keyed_kernel against aes_cbc_encrypt_kernel over the same buffers: 1 and
           256 chains of 32 MiB, 16- and 32-byte keys (HIP events).  The chain body is the same
           function; the margin is the single-key kernel's own min-max spread over its rounds.
  mixed    A: 16 chains of each key length in ONE keyed launch; B: the 16 chains on 32-byte keys
           alone; C: three single-key launches back to back on one stream (what a batch of mixed
           keys costs without the keyed kernel).  The gate: A <= B + B's spread (exit status 1 if
           not: a wave then mixes round counts or the groups do not run side by side).  D, a control
           outside the gate: the same 48 chains all on 32-byte keys in one keyed launch.
  uploads  c concurrent encrypted uploads of 1 MiB with distinct keys, wall time until all are done:
           through dm_batcher_process_cipher (one PROCESS batcher) and from c threads calling
           dm_process_cipher_buffer on a four-lane context.  No threshold.
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
KLENS = (16, 24, 32)


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


def part_kernel(torch, ctx, args, emit):
    nmax = 256
    buf = torch.empty(nmax * SEGMENT, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.fill_synthetic_async(buf.data_ptr(), 0, buf.numel(), 0xC1F4E5, stream)
    for nchain in (1, 256):
        chains = [(buf.data_ptr() + c * SEGMENT, 0) for c in range(nchain)]
        for klen in (16, 32):
            key = key_of(1, klen)
            t = interleaved({
                "single": lambda: event_ms(torch, lambda: ctx.aes_cbc_encrypt_device_async(
                    key, key[:16], buf.data_ptr(), SEGMENT, PIECE, nchain, stream)),
                "keyed": lambda: event_ms(torch, lambda: ctx.aes_cbc_encrypt_keyed_device_async(
                    [(key, key[:16])], chains, PIECE, stream)),
            }, args.rounds)
            s, k = summary(t["single"]), summary(t["keyed"])
            diff = k["median_ms"] - s["median_ms"]
            emit(dict(part="kernel", chains=nchain, key_bytes=klen, chain_bytes=SEGMENT, single=s, keyed=k,
                      keyed_minus_single_ms=round(diff, 3), keyed_over_single=round(k["median_ms"] / s["median_ms"], 4),
                      within_single_spread=abs(diff) <= s["spread_ms"]))


def part_mixed(torch, ctx, args, emit):
    per = 16
    buf = torch.empty(3 * per * SEGMENT, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.fill_synthetic_async(buf.data_ptr(), 0, buf.numel(), 0x5EED, stream)
    # chain c: group c // 16 = key length 16 / 24 / 32, a key of its own
    keys = [(key_of(c, KLENS[c // per]), key_of(c, 16)) for c in range(3 * per)]
    # interleaved in the caller's order: the plan, not the caller, groups them by wave
    order = [g * per + i for i in range(per) for g in range(3)]
    chains_a = [(buf.data_ptr() + c * SEGMENT, c) for c in order]
    chains_b = [(buf.data_ptr() + c * SEGMENT, c) for c in range(2 * per, 3 * per)]
    one = [keys[g * per] for g in range(3)]

    def three_launches():
        for g in range(3):
            ctx.aes_cbc_encrypt_device_async(one[g][0], one[g][1], buf.data_ptr() + g * per * SEGMENT, SEGMENT, PIECE, per,
                                             stream)
    # D (a control, not part of the gate): the same 48 buffers all on 32-byte keys, so three waves of
    # the longest round count side by side -- what A costs if grouping by wave costs nothing
    keys_d = [(key_of(100 + c, 32), key_of(c, 16)) for c in range(3 * per)]
    chains_d = [(buf.data_ptr() + c * SEGMENT, c) for c in order]
    t = interleaved({
        "A_mixed_one_keyed_launch": lambda: event_ms(torch, lambda: ctx.aes_cbc_encrypt_keyed_device_async(
            keys, chains_a, PIECE, stream)),
        "B_32_byte_keys_alone": lambda: event_ms(torch, lambda: ctx.aes_cbc_encrypt_keyed_device_async(
            keys, chains_b, PIECE, stream)),
        "C_three_single_key_launches": lambda: event_ms(torch, three_launches),
        "D_48_chains_32_byte_keys": lambda: event_ms(torch, lambda: ctx.aes_cbc_encrypt_keyed_device_async(
            keys_d, chains_d, PIECE, stream)),
    }, args.rounds)
    a, b, c = (summary(t[k]) for k in ("A_mixed_one_keyed_launch", "B_32_byte_keys_alone", "C_three_single_key_launches"))
    ok = a["median_ms"] <= b["median_ms"] + b["spread_ms"]
    emit(dict(part="mixed", chains_per_key_length=per, chain_bytes=SEGMENT, A=a, B=b, C=c,
              D=summary(t["D_48_chains_32_byte_keys"]),
              A_minus_B_ms=round(a["median_ms"] - b["median_ms"], 3), C_over_A=round(c["median_ms"] / a["median_ms"], 3),
              gate_A_within_B_spread=ok))
    return ok


def part_uploads(torch, ctx, args, emit):
    from deoss_amd import MerkleContext
    from deoss_amd.batcher import PROCESS, Batcher
    from deoss_amd.process import Processor
    size = 1 << 20
    cmax = max(args.uploads)
    bodies = [bytes([(7 * i + 3) & 0xFF]) * size for i in range(cmax)]
    keys = [key_of(1000 + i, KLENS[i % 3]) for i in range(cmax)]
    lanes = MerkleContext(lanes=4)
    proc = Processor(lanes)
    batcher = Batcher(PROCESS, SEGMENT, 4, 8, device=0, linger_us=2000)

    def wall(c, one):
        fids = [None] * c
        start = threading.Barrier(c + 1)

        def run(i):
            start.wait()
            fids[i] = one(i)
        ts = [threading.Thread(target=run, args=(i,)) for i in range(c)]
        for t in ts:
            t.start()
        start.wait()
        t0 = time.perf_counter()
        for t in ts:
            t.join()
        return (time.perf_counter() - t0) * 1e3, fids
    try:
        for c in args.uploads:
            seen = {}

            def via_batcher():
                ms, fids = wall(c, lambda i: batcher.process(bodies[i], False, keys[i])[2])
                seen["batcher"] = fids
                return ms

            def via_lanes():
                ms, fids = wall(c, lambda i: proc.process_buffer(bodies[i], False, keys[i])[2])
                seen["lanes"] = fids
                return ms
            t = interleaved({"batcher": via_batcher, "lanes": via_lanes}, args.rounds)
            assert seen["batcher"] == seen["lanes"], "the two paths disagree on a fid"
            b, ln = summary(t["batcher"]), summary(t["lanes"])
            emit(dict(part="uploads", uploads=c, upload_bytes=size, batcher=b, four_lanes=ln,
                      lanes_over_batcher=round(ln["median_ms"] / b["median_ms"], 2),
                      uploads_per_s_batcher=round(c / (b["median_ms"] / 1e3), 2),
                      uploads_per_s_four_lanes=round(c / (ln["median_ms"] / 1e3), 2)))
    finally:
        batcher.close()
        proc.close()
        lanes.close()


def write_table(out_dir, records):
    lines = ["# Keyed AES-CBC launch: measurements (tools/cipher_keyed_ab.py)", "",
             "One MI355X; medians of 5 rounds after a warm-up, the variants of a part interleaved round by round in",
             "one session.  Kernel times are HIP events, upload times the host clock.  Records: keyed_ab.jsonl.", ""]
    ker = [r for r in records if r["part"] == "kernel"]
    if ker:
        lines += ["## aes_cbc_encrypt_keyed_kernel against aes_cbc_encrypt_kernel, 32 MiB chains", "",
                  "| chains | key bytes | single-key ms (min .. max) | keyed ms (min .. max) | keyed - single ms | within single's spread |",
                  "|---|---|---|---|---|---|"]
        lines += [f"| {r['chains']} | {r['key_bytes']} | {r['single']['median_ms']} ({r['single']['min_ms']} .. {r['single']['max_ms']}) | "
                  f"{r['keyed']['median_ms']} ({r['keyed']['min_ms']} .. {r['keyed']['max_ms']}) | {r['keyed_minus_single_ms']} | "
                  f"{'yes' if r['within_single_spread'] else 'no'} |" for r in ker]
        lines.append("")
    for r in (r for r in records if r["part"] == "mixed"):
        lines += ["## Mixed key lengths: 16 chains of 32 MiB per length" + (f" (session {r['session']})" if "session" in r else ""), "",
                  "| variant | ms (min .. max) |", "|---|---|",
                  f"| A: 48 chains, three key lengths, one keyed launch | {r['A']['median_ms']} ({r['A']['min_ms']} .. {r['A']['max_ms']}) |",
                  f"| B: the 16 chains on 32-byte keys alone | {r['B']['median_ms']} ({r['B']['min_ms']} .. {r['B']['max_ms']}) |",
                  f"| C: three single-key launches back to back | {r['C']['median_ms']} ({r['C']['min_ms']} .. {r['C']['max_ms']}) |",
                  *([f"| D (control): the 48 chains all on 32-byte keys, one keyed launch | {r['D']['median_ms']} ({r['D']['min_ms']} .. {r['D']['max_ms']}) |"]
                    if "D" in r else []),
                  "", f"A - B = {r['A_minus_B_ms']} ms against B's spread of {r['B']['spread_ms']} ms: the gate "
                  f"{'holds' if r['gate_A_within_B_spread'] else 'FAILS'}.  C / A = {r['C_over_A']}.", ""]
    up = [r for r in records if r["part"] == "uploads"]
    if up:
        lines += ["## Concurrent encrypted uploads of 1 MiB, distinct keys: wall time until all are done", "",
                  "| uploads | dm_batcher_process_cipher ms (min .. max) | dm_process_cipher_buffer, 4 lanes ms (min .. max) | lanes / batcher | uploads/s batcher | uploads/s lanes |",
                  "|---|---|---|---|---|---|"]
        lines += [f"| {r['uploads']} | {r['batcher']['median_ms']} ({r['batcher']['min_ms']} .. {r['batcher']['max_ms']}) | "
                  f"{r['four_lanes']['median_ms']} ({r['four_lanes']['min_ms']} .. {r['four_lanes']['max_ms']}) | "
                  f"{r['lanes_over_batcher']} | {r['uploads_per_s_batcher']} | {r['uploads_per_s_four_lanes']} |" for r in up]
        lines.append("")
    with open(os.path.join(out_dir, "KEYED.md"), "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cipher"))
    ap.add_argument("--parts", default="kernel,mixed,uploads")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--uploads", default="1,8,64")
    args = ap.parse_args()
    args.uploads = [int(x) for x in args.uploads.split(",")]
    import torch
    from deoss_amd import MerkleContext
    assert torch.cuda.is_available(), "needs an MI355X"
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "keyed_ab.jsonl")
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
    gate = True
    with MerkleContext() as ctx:
        for part in parts:
            ok = {"kernel": part_kernel, "mixed": part_mixed, "uploads": part_uploads}[part](torch, ctx, args, emit)
            if part == "mixed":
                gate = bool(ok)
            torch.cuda.empty_cache()
    write_table(args.out, records)
    return 0 if gate else 1


if __name__ == "__main__":
    sys.exit(main())
