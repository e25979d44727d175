#!/usr/bin/env python3
"""A/B of the restore path on the MI355X (DESIGN.md "Restore"): needs a GPU, fails without one.

  python tools/restore_ab.py [--segments 256] [--repeats 5] [--out FILE]

1. Kernel A/B on device-resident data: `--segments` segments of 32 MiB, 4 + 8, two data fragments
   of every segment missing (a seeded choice per segment).
     batched : ONE dm_rs_restore_device_async over all segments
     loop    : one dm_rs_reconstruct_device_async per segment (the path before this one)
   HIP events around the calls, interleaved repeats, the object compared with the original after
   every timed call.  Both against the HBM traffic the pass needs -- 4 reads + 2 writes per 16-byte
   unit -- and against the read rate dm_read_probe_async reaches on the same buffer in the same run.
2. Cost of the two verification phases of dm_restore_buffer (host clock around the synchronous
   call, fragments in pinned host memory) at 1, 8 and `--segments` segments: flags 0, fragments
   only, everything.
3. One CPU core on one segment with the CPU oracle (rs_oracle.c + merkle_oracle.c, the test
   checker: a stand-in for klauspost + crypto/sha256, whose SIMD coder is faster): Reconstruct of
   two data fragments plus SHA-256 of the four fragments used and of the segment.
Prints one JSON line per measurement and a summary line; --out also writes them to a file.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SEG = 32 << 20
K, M = 4, 8
TOTAL = K + M
FRAG = SEG // K


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("restore_ab: no GPU visible", file=sys.stderr)
        return 2
    from deoss_amd import MerkleContext
    from deoss_amd.process import Processor

    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    n = args.segments
    ctx = MerkleContext()
    proc = Processor(ctx)
    enc = proc.enc
    stream = torch.cuda.current_stream().cuda_stream
    obj = torch.empty(n * SEG, dtype=torch.uint8, device="cuda")
    par = torch.empty(n * M * FRAG, dtype=torch.uint8, device="cuda")
    segd = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    fragd = torch.empty(n * TOTAL * 32, dtype=torch.uint8, device="cuda")
    fid = torch.empty(32, dtype=torch.uint8, device="cuda")
    ctx.fill_synthetic_async(obj.data_ptr(), 0, n * SEG, 0xDE055AB, stream)
    proc.process_device_async(obj.data_ptr(), n * SEG, par.data_ptr(), segd.data_ptr(), fragd.data_ptr(),
                              fid.data_ptr(), stream)
    torch.cuda.synchronize()
    ref = obj.clone()
    rng = random.Random(2)
    lost = [sorted(rng.sample(range(K), 2)) for _ in range(n)]

    def erase():
        for s in range(n):
            for j in lost[s]:
                obj[s * SEG + j * FRAG:s * SEG + (j + 1) * FRAG].fill_(0x5A)

    ptrs_a, shards_b, present_b = [], [], []
    for s in range(n):
        row = [obj.data_ptr() + s * SEG + j * FRAG for j in range(K)] + \
              [par.data_ptr() + (s * M + i) * FRAG for i in range(M)]
        shards_b.append(row)
        present_b.append([j not in lost[s] for j in range(TOTAL)])
        ptrs_a += [0 if j in lost[s] else row[j] for j in range(TOTAL)]

    def batched():
        enc.restore_device_async(ptrs_a, n, SEG, obj.data_ptr(), stream)

    def loop():
        for s in range(n):
            enc.reconstruct_device_async(shards_b[s], present_b[s], FRAG, stream)

    def timed(fn):
        erase()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        assert torch.equal(obj, ref), "restored object differs from the original"
        return e0.elapsed_time(e1), wall

    def read_probe():
        x = torch.zeros(8, dtype=torch.uint8, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx.read_probe_async(obj.data_ptr(), n * SEG, x.data_ptr(), stream)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for fn in (batched, loop):   # warm-up: code objects, scratch, tables
        timed(fn)
    read_probe()
    ta, tb, wa, wb, tr = [], [], [], [], []
    for _ in range(args.repeats):   # interleaved
        a, w = timed(batched)
        ta.append(a)
        wa.append(w)
        b, w = timed(loop)
        tb.append(b)
        wb.append(w)
        tr.append(read_probe())
    traffic = n * FRAG * 6            # 4 fragment reads + 2 fragment writes per segment
    ma, mb, mr = statistics.median(ta), statistics.median(tb), statistics.median(tr)
    read_rate = n * SEG / (mr * 1e-3)
    emit(what="kernel_ab", segments=n, repeats=args.repeats, batched_event_ms=ta, loop_event_ms=tb,
         batched_wall_ms=wa, loop_wall_ms=wb, read_probe_ms=tr,
         batched_median_ms=ma, loop_median_ms=mb, speedup=mb / ma, traffic_bytes=traffic,
         batched_TBps=traffic / (ma * 1e-3) / 1e12, loop_TBps=traffic / (mb * 1e-3) / 1e12,
         read_peak_TBps=read_rate / 1e12, batched_fraction_of_read_peak=traffic / (ma * 1e-3) / read_rate)

    # ---- verification phases of dm_restore_buffer ---------------------------------------------
    L = ctx._L
    segd_h, fragd_h = bytes(segd.cpu().numpy()), bytes(fragd.cpu().numpy())
    hobj = torch.empty(n * SEG, dtype=torch.uint8).pin_memory()
    hobj.copy_(ref)
    hpar = torch.empty(n * 2 * FRAG, dtype=torch.uint8).pin_memory()     # parity fragments 0 and 1 of every segment
    for s in range(n):
        hpar[s * 2 * FRAG:(s + 1) * 2 * FRAG].copy_(par[s * M * FRAG:s * M * FRAG + 2 * FRAG])
    hout = torch.empty(n * SEG, dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()
    del ref, par
    torch.cuda.empty_cache()
    fptr = (ctypes.c_void_p * (n * TOTAL))()
    for s in range(n):
        for j in range(K):
            if j not in lost[s]:
                fptr[s * TOTAL + j] = hobj.data_ptr() + s * SEG + j * FRAG
        for i in range(2):
            fptr[s * TOTAL + K + i] = hpar.data_ptr() + (s * 2 + i) * FRAG
    phases = {}
    for ns in sorted({1, 8, n}):
        if ns > n:
            continue
        fid_ns = ctx.tree_root(segd_h[:32 * ns])
        size = ns * SEG - 12345
        res = {}
        for name, flags in (("none", 0), ("fragments", 1), ("all", 7)):
            ts = []
            for rep in range(min(args.repeats, 3) + 1):   # the first one warms up
                ok = ctypes.c_int(0)
                hout[:64].zero_()
                t0 = time.perf_counter()
                rc = L.dm_restore_buffer(enc._h, fptr, fragd_h, segd_h, fid_ns, ns, size, SEG, flags,
                                         ctypes.c_void_p(hout.data_ptr()), None, None, ctypes.byref(ok))
                dt = (time.perf_counter() - t0) * 1e3
                assert rc == 0 and ok.value == 1, (rc, ok.value, L.dm_last_error(None))
                assert torch.equal(hout[:size], hobj[:size])
                if rep:
                    ts.append(dt)
            res[name] = ts
        med = {k: statistics.median(v) for k, v in res.items()}
        phases[ns] = med
        emit(what="restore_buffer", segments=ns, ms=res, median_ms=med,
             fragment_phase_ms=med["fragments"] - med["none"], segment_and_fid_phase_ms=med["all"] - med["fragments"])

    # ---- one CPU core, one segment (the oracle as a stand-in for the SDK's restore) ------------
    import subprocess
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    from oracle import Oracle
    orc = Oracle()
    host = bytes(hobj[:SEG].numpy())
    data = [host[j * FRAG:(j + 1) * FRAG] for j in range(K)]
    parity = orc.rs_encode(data, M)
    shards = [None if j in lost[0] else data[j] for j in range(K)] + parity[:2] + [None] * (M - 2)
    cpu = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = orc.rs_reconstruct(K, M, shards, FRAG)
        for x in (shards[0] or got[0], shards[1] or got[1], parity[0], parity[1]):
            orc.sha256(x)
        orc.sha256(b"".join(got[:K]))
        cpu.append((time.perf_counter() - t0) * 1e3)
        assert got[:K] == data
    cpu_ms = statistics.median(cpu)
    emit(what="cpu_one_core_one_segment", backend=orc.backend(), ms=cpu, median_ms=cpu_ms)
    # smallest measured segment count at which the verified GPU restore takes less than the CPU's n x one segment
    beats = [ns for ns in sorted(phases) if phases[ns]["all"] < ns * cpu_ms]
    emit(what="summary", speedup_batched_over_loop=mb / ma, batched_ms=ma, loop_ms=mb,
         batched_fraction_of_read_peak=traffic / (ma * 1e-3) / read_rate,
         gpu_verified_ms={str(k): v["all"] for k, v in phases.items()}, cpu_ms_per_segment=cpu_ms,
         gpu_beats_one_core_from_segments=(beats[0] if beats else None))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    proc.close()
    ctx.close()
    if ma > mb:
        print("restore_ab: the batched call was slower than the loop", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
