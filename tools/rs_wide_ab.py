#!/usr/bin/env python3
"""Throughput of the wide Reed-Solomon coder on the MI355X: needs a GPU, fails
without one.

  python tools/rs_wide_ab.py [--shard-mib 8] [--repeats 5] [--out FILE]

Device-resident shards, HIP events around dm_rs_encode_device_async, a warm-up, then `--repeats`
rounds; a round times, one after the other, the geometry under test, 4 + 8 through rs_code_kernel
(the yardstick every round shares) and dm_read_probe_async over the geometry's data shards, so the
three medians of one geometry come from the same minutes of the machine.  Geometries: 4 + 8 through
rs_code_kernel, 4 + 8 forced through rs_code_wide_kernel (DEOSS_RS_FORCE_WIDE, read by
dm_rs_create_wide: measurement only; its parity is compared with rs_code_kernel's), then 10 + 4,
17 + 3, 16 + 16, 64 + 32, 128 + 128, 255 + 1 and 1 + 255.  Each geometry codes enough segments for
about 1 GiB of data shards, fewer where data + parity would pass 12 GiB.

Per geometry one JSON line: GiB/s of data coded; bytes moved per second -- nin x ceil(nout / 8)
shard reads + nout shard writes per segment -- and that as a fraction of the read rate the probe
reached; and the time relative to 4 + 8 through rs_code_kernel in the same rounds.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOMETRIES = [(4, 8, "rs_code_kernel"), (4, 8, "rs_code_wide_kernel"), (10, 4, None), (17, 3, None), (16, 16, None),
              (64, 32, None), (128, 128, None), (255, 1, None), (1, 255, None)]
DATA_TARGET = 1 << 30
MEMORY_CAP = 12 << 30
WINDOW_MS = 60.0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shard-mib", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    os.environ["DEOSS_RS_FORCE_WIDE"] = "1"   # before the library's first dm_rs_create_wide call
    import torch
    if not torch.cuda.is_available():
        print("rs_wide_ab: no GPU visible", file=sys.stderr)
        return 2
    from deoss_amd import MerkleContext
    from deoss_amd.reedsolomon import Encoder

    shard = args.shard_mib << 20
    ctx = MerkleContext()
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def reps_for(fn):
        fn()
        torch.cuda.synchronize()           # code object, tables
        once = timed(fn, 1)
        return max(1, min(50, int(WINDOW_MS / max(once, 1e-3))))

    class Case:
        def __init__(self, k, m, wide):
            self.k, self.m = k, m
            self.nseg = max(1, min(-(-DATA_TARGET // (k * shard)), MEMORY_CAP // ((k + m) * shard)))
            self.enc = Encoder(ctx, k, m, wide=wide)
            self.data = torch.empty(self.nseg * k * shard, dtype=torch.uint8, device="cuda")
            self.par = torch.empty(self.nseg * m * shard, dtype=torch.uint8, device="cuda")
            ctx.fill_synthetic_async(self.data.data_ptr(), 0, self.data.numel(), 0xDE055 + 1000 * k + m, stream)
            torch.cuda.synchronize()

        def encode(self):
            self.enc.encode_device_async(self.data.data_ptr(), self.k * shard, self.par.data_ptr(), self.m * shard, shard,
                                         self.nseg, stream)

        def close(self):
            self.enc.close()
            del self.data, self.par
            torch.cuda.empty_cache()

    xor8 = torch.zeros(8, dtype=torch.uint8, device="cuda")
    base = Case(4, 8, wide=False)
    base_reps = reps_for(base.encode)
    base.encode()
    torch.cuda.synchronize()
    base_parity = base.par.clone()
    for k, m, kernel in GEOMETRIES:
        wide = kernel != "rs_code_kernel"
        case = Case(k, m, wide=wide)

        def probe():
            ctx.read_probe_async(case.data.data_ptr(), case.data.numel(), xor8.data_ptr(), stream)

        reps, probe_reps = reps_for(case.encode), reps_for(probe)
        if (k, m) == (4, 8):
            case.data.copy_(base.data)
            case.encode()
            torch.cuda.synchronize()
            assert torch.equal(case.par, base_parity), "4 + 8: the two kernels' parity differs"
        t_case, t_base, t_probe = [], [], []
        for _ in range(args.repeats):      # interleaved
            t_case.append(timed(case.encode, reps))
            t_base.append(timed(base.encode, base_reps))
            t_probe.append(timed(probe, probe_reps))
        mc, mb, mp = statistics.median(t_case), statistics.median(t_base), statistics.median(t_probe)
        data_bytes = case.nseg * k * shard
        moved = case.nseg * (k * -(-m // 8) + m) * shard
        read_rate = data_bytes / (mp * 1e-3)
        emit(what="rs_wide_ab", data=k, parity=m, kernel=kernel or "rs_code_wide_kernel", shard_bytes=shard,
             segments=case.nseg, calls_per_window=reps, repeats=args.repeats, ms=t_case, median_ms=mc,
             range_ms=[min(t_case), max(t_case)], data_GiBps=data_bytes / (mc * 1e-3) / 2**30, moved_bytes=moved,
             moved_TBps=moved / (mc * 1e-3) / 1e12, read_probe_ms=t_probe, read_peak_TBps=read_rate / 1e12,
             moved_fraction_of_read_peak=moved / (mc * 1e-3) / read_rate, base_4_8_ms=t_base, base_4_8_median_ms=mb,
             base_4_8_GiBps=base.nseg * 4 * shard / (mb * 1e-3) / 2**30)
        case.close()
    narrow = [ln for ln in lines if ln["kernel"] == "rs_code_kernel"][0]
    forced = [ln for ln in lines if (ln["data"], ln["parity"], ln["kernel"]) == (4, 8, "rs_code_wide_kernel")][0]
    emit(what="rs_wide_ab_ratio_4_8", wide_over_existing=forced["median_ms"] / forced["base_4_8_median_ms"],
         existing_median_ms=forced["base_4_8_median_ms"], wide_median_ms=forced["median_ms"],
         existing_against_itself=narrow["median_ms"] / narrow["base_4_8_median_ms"])
    base.close()
    ctx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
