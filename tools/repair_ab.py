#!/usr/bin/env python3
"""A/B of the repair path on the MI355X: needs a GPU, fails without one.

  python tools/repair_ab.py [--segments 256] [--repeats 5] [--file-segments 1,8,256] [--out FILE]

1. Kernel A/B on device-resident data: `--segments` segments of 32 MiB, 4 + 8, all 12 fragments of
   every segment in HBM.  Three cases: 2 fragments of every segment missing (the launch picks
   rs_restore_kernel), 8 missing (rs_repair_kernel), and a seeded mix of 1-8.
     repair : ONE dm_rs_repair_device_async over all segments
     loop   : one dm_rs_reconstruct_device_async per segment (the only way before this call)
   HIP events around the calls, interleaved repeats after a warm-up, every fragment compared with
   the original after every timed call.  Both against the HBM traffic the pass needs -- 4 fragment
   reads + nout fragment writes per segment -- and against the read rate dm_read_probe_async reaches
   on the same buffer in the same run.
2. Call level: dm_repair_files on the fragment directory of a 1-, 8- and 256-segment object with one
   seeded fragment file of every segment deleted, against dm_full_processing of the same object into
   a fresh directory (what the tracker's reFullProcessing does today).  Host clock around the
   synchronous calls, 3 repeats after a warm-up; every rebuilt file compared with the deleted one.
   The files were just written and read: they are on the page cache, and the numbers say so.
Prints one JSON line per measurement; --out also appends them to a file.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEG = 32 << 20
K, M = 4, 8
TOTAL = K + M
FRAG = SEG // K


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--file-segments", default="1,8,256")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("repair_ab: no GPU visible", file=sys.stderr)
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
    fid = torch.empty(32, dtype=torch.uint8, device="cuda")
    ctx.fill_synthetic_async(obj.data_ptr(), 0, n * SEG, 0xDE055AC, stream)
    proc.process_device_async(obj.data_ptr(), n * SEG, par.data_ptr(), 0, 0, fid.data_ptr(), stream)
    torch.cuda.synchronize()
    ref_obj, ref_par = obj.clone(), par.clone()

    def addr(s, j):
        return obj.data_ptr() + s * SEG + j * FRAG if j < K else par.data_ptr() + (s * M + j - K) * FRAG

    def view(s, j):
        return obj[s * SEG + j * FRAG:s * SEG + (j + 1) * FRAG] if j < K else \
            par[(s * M + j - K) * FRAG:(s * M + j - K + 1) * FRAG]

    def read_probe():
        x = torch.zeros(8, dtype=torch.uint8, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx.read_probe_async(obj.data_ptr(), n * SEG, x.data_ptr(), stream)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    rng = random.Random(15)
    cases = {
        "2_missing": [sorted(rng.sample(range(TOTAL), 2)) for _ in range(n)],
        "8_missing": [sorted(rng.sample(range(TOTAL), 8)) for _ in range(n)],
        "mix_1_to_8": [sorted(rng.sample(range(TOTAL), rng.randint(1, 8))) for _ in range(n)],
    }
    slower = False
    for name, lost in cases.items():
        ptrs = [addr(s, j) for s in range(n) for j in range(TOTAL)]
        present = [j not in lost[s] for s in range(n) for j in range(TOTAL)]
        rows = [[addr(s, j) for j in range(TOTAL)] for s in range(n)]
        pres_rows = [[j not in lost[s] for j in range(TOTAL)] for s in range(n)]

        def repair():
            enc.repair_device_async(ptrs, present, n, FRAG, stream)

        def loop():
            for s in range(n):
                enc.reconstruct_device_async(rows[s], pres_rows[s], FRAG, stream)

        def timed(fn):
            for s in range(n):
                for j in lost[s]:
                    view(s, j).fill_(0x5A)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            assert torch.equal(obj, ref_obj) and torch.equal(par, ref_par), "a repaired fragment differs from the original"
            return e0.elapsed_time(e1), wall

        for fn in (repair, loop):   # warm-up: code objects, scratch, tables
            timed(fn)
        read_probe()
        ta, tb, wa, wb, tr = [], [], [], [], []
        for _ in range(args.repeats):   # interleaved
            a, w = timed(repair)
            ta.append(a)
            wa.append(w)
            b, w = timed(loop)
            tb.append(b)
            wb.append(w)
            tr.append(read_probe())
        nout = sum(len(x) for x in lost)
        traffic = (n * K + nout) * FRAG            # k fragment reads + nout fragment writes per segment
        ma, mb, mr = statistics.median(ta), statistics.median(tb), statistics.median(tr)
        read_rate = n * SEG / (mr * 1e-3)
        wide = any(len(x) > K for x in lost)
        emit(what="kernel_ab", case=name, kernel="rs_repair_kernel" if wide else "rs_restore_kernel", segments=n,
             outputs=nout, repeats=args.repeats, repair_event_ms=ta, loop_event_ms=tb, repair_wall_ms=wa, loop_wall_ms=wb,
             read_probe_ms=tr, repair_median_ms=ma, loop_median_ms=mb, repair_range_ms=[min(ta), max(ta)],
             loop_range_ms=[min(tb), max(tb)], speedup=mb / ma, traffic_bytes=traffic,
             repair_TBps=traffic / (ma * 1e-3) / 1e12, loop_TBps=traffic / (mb * 1e-3) / 1e12,
             read_peak_TBps=read_rate / 1e12, repair_fraction_of_read_peak=traffic / (ma * 1e-3) / read_rate)
        slower |= ma > mb

    # ---- call level: dm_repair_files against dm_full_processing ---------------------------------
    host = torch.empty(n * SEG, dtype=torch.uint8)
    host.copy_(ref_obj)
    del ref_obj, ref_par, obj, par
    torch.cuda.empty_cache()
    work = tempfile.mkdtemp(prefix="repair_ab_", dir=args.workdir or None)
    try:
        for ns in [int(x) for x in args.file_segments.split(",") if x]:
            need = ns * SEG * 8            # the object, two fragment directories (3 x the object each) and slack
            if ns > n or shutil.disk_usage(work).free < need:
                emit(what="repair_files", segments=ns, result="not measured",
                     reason="more segments than --segments" if ns > n else "not enough free space in the work directory")
                continue
            src = os.path.join(work, "object%d" % ns)
            with open(src, "wb") as f:
                f.write(host[:ns * SEG - 12345].numpy().tobytes())
            have = os.path.join(work, "have%d" % ns)
            segd, fragd, _ = proc.full_processing_file(src, have, segment_files=False)
            rng = random.Random(ns)
            t_rep, t_full = [], []
            for rep in range(min(args.repeats, 3) + 1):   # the first one warms up
                gone = {}
                for s in range(ns):
                    j = rng.randrange(TOTAL)
                    name = fragd[32 * (s * TOTAL + j):32 * (s * TOTAL + j + 1)].hex()
                    path = os.path.join(have, name)
                    if name not in gone:
                        with open(path, "rb") as f:
                            gone[name] = f.read()
                        os.unlink(path)
                t0 = time.perf_counter()
                ok, nre, fst, sst = proc.repair_files(have, fragd)
                dt = (time.perf_counter() - t0) * 1e3
                assert ok and nre == len(gone), (ok, nre, len(gone))
                for name, data in gone.items():
                    with open(os.path.join(have, name), "rb") as f:
                        assert f.read() == data, "a rebuilt fragment file differs from the deleted one"
                fresh = os.path.join(work, "fresh%d" % ns)
                t0 = time.perf_counter()
                segd2, fragd2, _ = proc.full_processing_file(src, fresh, segment_files=False)
                df = (time.perf_counter() - t0) * 1e3
                assert fragd2 == fragd and segd2 == segd
                shutil.rmtree(fresh)
                if rep:
                    t_rep.append(dt)
                    t_full.append(df)
            mr, mf = statistics.median(t_rep), statistics.median(t_full)
            emit(what="repair_files", segments=ns, files_deleted_per_call=len(gone), page_cache=True,
                 repair_ms=t_rep, full_processing_ms=t_full, repair_median_ms=mr, full_processing_median_ms=mf,
                 repair_range_ms=[min(t_rep), max(t_rep)], full_processing_range_ms=[min(t_full), max(t_full)],
                 speedup=mf / mr)
            shutil.rmtree(have)
            os.unlink(src)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    proc.close()
    ctx.close()
    if slower:
        print("repair_ab: the batched call was slower than the loop", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
