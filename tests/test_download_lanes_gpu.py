"""The download, repair and cipher paths on concurrent call lanes: restore (plain and with a cipher),
repair, ranged restore, the file forms of the three, FullProcessing with a cipher and the device-level
rs / AES-CBC entry points, called the way a gateway calls them -- many threads on one context with
several lanes, callers' own streams, and calls queued behind work that has not run yet.

What is under test is the runtime around the kernels (merkle_capi.hip and its *_capi.inl): per-lane
scratch (Dev::data, aes_win, htab and the leaf tables; RsLane::work, rst_desc, rst_tab, dec_tab through
rs_ln), begin_call's wait on the lane's tail event, tables_begin's wait on ev_htab before the pinned
bounce buffer is refilled, DevBuf::ensure handing a grown block to the reaper, and choose_lane's
routing past lanes whose tail has not finished.  The kernels themselves have their single-call tests
(test_restore_gpu.py, test_repair_gpu.py, test_range_gpu.py, test_cipher_gpu.py).

Every comparison is bit-exact and no expected byte comes from the code under test: plain objects,
their fragments and names are oracle_lib.full_processing's (the Coded class of test_restore_gpu.py),
ciphered ones tests/cipher_ref.py's (scheme_full_processing, cbc_encrypt_many, decrypt_blocks).
Expected statuses follow the rules the single-call tests state (each cited where it is applied).
All references are computed before any thread starts or any blocker is queued: the reference AES is
plain Python and would serialise the threads on the interpreter lock.

Shapes: 4 + 8, segment 4,096 (16,384 for the file paths), 1 to 9 segments per object, fragments of
16 bytes to 1 KiB at the device level.  The largest allocation is the blockers' 64 MiB buffer.
"""
from __future__ import annotations

import ctypes
import itertools
import os
import random
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cipher_ref as R  # noqa: E402
from test_repair_gpu import FILL, REBUILT  # noqa: E402
from test_restore_gpu import ABSENT, BAD, SPARE, USED, VALL, Coded, _flip  # noqa: E402

SEG_BAD_PADDING = 3                       # kSegBadPadding, rs_plan.hpp:167
SEG, K, M, TOTAL = 4096, 4, 8, 12
FRAG, P = SEG // K, SEG - 16
FSEG = 16384
FFRAG = FSEG // K
SENTINEL = 0xEE
MIX_SEED = 0xD0A1
KLENS = (16, 24, 32)
BLOCKER_BYTES, BLOCKER_CHUNK = 64 << 20, 32 << 20   # two serial 32 MiB chains side by side: about 0.5 s

KINDS = ("restore", "restore_cipher", "repair", "range", "range_cipher", "process_cipher", "retrieve_file",
         "retrieve_range", "repair_files", "dev_aes", "dev_restore", "dev_repair", "dev_windows")
CIPHER_KINDS = ("restore_cipher", "range_cipher", "process_cipher", "dev_aes", "dev_windows")
# the virtual-device run: 4 threads x 2 iterations, the kinds that index RsLane scratch through rs_ln
VIRTUAL_KINDS = ("restore_cipher", "repair", "range_cipher", "retrieve_file", "repair_files", "dev_restore",
                 "dev_repair", "dev_windows")


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---- the seeded mix (pure Python: test_drawn_mix_shape checks it without a GPU) --------------------

def _size(rng, piece, lo=1, tail_from=1):
    """1 .. 9 pieces, the last one never full (a padded last segment)."""
    nseg = rng.randint(lo, 9)
    return (nseg - 1) * piece + rng.randint(tail_from, piece - 1), nseg


def _draw_restore(rng, c, piece):
    """Two data fragments dropped per segment, the other two and 3 .. 6 parity fragments kept, one of the
    first four kept (the ones a restore would use) corrupted at a random byte."""
    c["size"], nseg = _size(rng, piece)
    c["kept"], c["hit"] = [], []
    for _ in range(nseg):
        drop = rng.sample(range(K), 2)
        row = sorted([j for j in range(K) if j not in drop] + rng.sample(range(K, TOTAL), rng.randint(3, 6)))
        c["kept"].append(row)
        c["hit"].append((row[rng.randrange(K)], rng.randrange(FRAG)))


def _draw_repair(rng, c, wide):
    """1 .. 4 fragments missing per segment (rs_restore_kernel); wide: one segment misses 5 .. 8, so the
    call launches rs_repair_kernel."""
    c["size"], nseg = _size(rng, SEG)
    miss = [rng.randint(1, K) for _ in range(nseg)]
    if wide:
        miss[rng.randrange(nseg)] = rng.randint(K + 1, M)
    c["kept"] = [sorted(rng.sample(range(TOTAL), TOTAL - n)) for n in miss]


def _draw_range(rng, c, piece, frag, tail_from=1):
    """A range that starts and ends in the middle of an AES block and spans segments; every segment
    keeps 5 .. 12 fragments, then the first touched segment loses the data fragment that holds the
    range's first byte (needed whatever the plan adds), so the rebuild round runs."""
    c["size"], nseg = _size(rng, piece, lo=2, tail_from=tail_from)
    while True:
        off = rng.randrange(c["size"] - 1)
        length = rng.randint(2, min(c["size"] - off, 3 * piece))
        if off % 16 and (off + length) % 16 and (off + length - 1) // piece > off // piece:
            break
    kept = [sorted(rng.sample(range(TOTAL), rng.randint(K + 1, TOTAL))) for _ in range(nseg)]
    first, j = off // piece, (off % piece) // frag
    kept[first] = [x for x in kept[first] if x != j]
    c.update(off=off, length=length, kept=kept, lost=(first, j))


def _draw_files(rng, c):
    """A file object whose last segment is padded but reaches its fourth data fragment, so no two
    fragments are equal and every name is a file of its own."""
    c["size"], nseg = _size(rng, FSEG, tail_from=3 * FFRAG + 1)
    return nseg


def _draw_retrieve_file(rng, c):
    nseg = _draw_files(rng, c)
    c["kept"] = [sorted(rng.sample(range(TOTAL), rng.randint(K, 7))) for _ in range(nseg)]


def _draw_repair_files(rng, c):
    nseg = _draw_files(rng, c)
    miss = [rng.choice([0, 1, 2, 3, 4, 5, 8]) for _ in range(nseg)]
    miss[rng.randrange(nseg)] = rng.randint(1, M)
    c["kept"] = [sorted(rng.sample(range(TOTAL), TOTAL - n)) for n in miss]


def _draw_dev_aes(rng, c):
    c.update(plain=16 * rng.randint(1, 16), nseg=rng.randint(1, 9), iv=bytes(rng.randrange(256) for _ in range(16)))


def _draw_dev_rs(rng, c, repair):
    """Patterns for dm_rs_restore_device_async (in_place: data fragments already at their final
    address) or dm_rs_repair_device_async (want: which missing fragments are asked for)."""
    c.update(frag=16 * rng.choice([1, 2, 5, 17, 64]), nseg=rng.randint(1, 9))
    c["present"] = [sorted(rng.sample(range(TOTAL), rng.randint(K, TOTAL))) for _ in range(c["nseg"])]
    if repair:
        c["want"] = [[j for j in range(TOTAL) if j not in p and rng.random() < 0.8] for p in c["present"]]
    else:
        c["in_place"] = [[j for j in p if j < K and rng.random() < 0.3] for p in c["present"]]


WIN_NB = 64          # ciphertext blocks the windows of one case read from


def _draw_dev_windows(rng, c):
    """(first block, blocks, predecessor: 0 the IV / 1 the block before / 2 a block elsewhere, check_pad)"""
    c["iv"] = bytes(rng.randrange(256) for _ in range(16))
    c["wins"] = []
    for _ in range(rng.randint(20, 60)):
        n = rng.randint(1, 3)
        c["wins"].append((rng.randint(1, WIN_NB - 3), n, rng.randrange(3), int(n >= 2 and rng.random() < 0.3)))


def draw_mix(nthreads=12, niter=3, seed=MIX_SEED):
    """The cases of tests 1 and 2: thread t's iteration i is case niter * t + i and takes the kinds in
    turn.  Every thread has its own cipher; the key lengths rotate so that the cases the barrier
    releases together (iteration 0) hold all three."""
    rng = random.Random(seed)
    cases, repairs = [], 0
    for t in range(nthreads):
        klen = KLENS[(t + t // 3) % 3]
        key = bytes(rng.randrange(256) for _ in range(klen))
        for i in range(niter):
            kind = KINDS[(niter * t + i) % len(KINDS)]
            c = dict(t=t, i=i, kind=kind, key=key, seed=rng.randrange(1 << 30))
            if kind in ("restore", "restore_cipher"):
                _draw_restore(rng, c, P if kind == "restore_cipher" else SEG)
            elif kind == "repair":
                _draw_repair(rng, c, wide=repairs % 2 == 1)
                repairs += 1
            elif kind in ("range", "range_cipher"):
                _draw_range(rng, c, P if kind == "range_cipher" else SEG, FRAG)
            elif kind == "process_cipher":
                c["size"], _ = _size(rng, P)
            elif kind == "retrieve_file":
                _draw_retrieve_file(rng, c)
            elif kind == "retrieve_range":
                _draw_range(rng, c, FSEG, FFRAG, tail_from=3 * FFRAG + 1)
            elif kind == "repair_files":
                _draw_repair_files(rng, c)
            elif kind == "dev_aes":
                _draw_dev_aes(rng, c)
            elif kind in ("dev_restore", "dev_repair"):
                _draw_dev_rs(rng, c, kind == "dev_repair")
            else:
                _draw_dev_windows(rng, c)
            cases.append(c)
    return cases


def pick(cases, kind, n):
    """The n-th case of a kind, wrapping around."""
    of = [c for c in cases if c["kind"] == kind]
    return of[n % len(of)]


# ---- expected statuses, from the rules the single-call tests state ---------------------------------

def restore_rows(c):
    """dm_restore_buffer hashes every fragment given: one that fails its name is BAD, the first k good
    ones in index order are USED, the other good ones SPARE (rt_select, rs_plan.hpp:169-188;
    test_restore_gpu.py::test_restore_buffer, "5 of 12, one used fragment corrupted")."""
    rows = []
    for row, (j, _) in zip(c["kept"], c["hit"]):
        st = [ABSENT] * TOTAL
        st[j] = BAD
        for n, x in enumerate(x for x in row if x != j):
            st[x] = USED if n < K else SPARE
        rows.append(st)
    return rows


def repair_rows(c):
    """Every missing fragment is REBUILT, the first k kept are the inputs (USED), a kept fragment beyond
    them is not read (ABSENT): test_repair_gpu.py::test_repair_buffer and ::test_repair_files_deleted_
    and_truncated; a segment with nothing missing is not read at all."""
    rows = []
    for row in c["kept"]:
        if len(row) == TOTAL:
            rows.append([ABSENT] * TOTAL)
            continue
        st = [REBUILT] * TOTAL
        for n, x in enumerate(row):
            st[x] = USED if n < K else ABSENT
        rows.append(st)
    return rows


def first_k_rows(c):
    """dm_retrieve_file reads only as many files as it needs: the first k that exist are USED, the rest
    stay ABSENT (test_restore_gpu.py::test_retrieve_file_wrong_length_and_corrupt_fragments)."""
    return [[USED if x in row[:K] else ABSENT for x in range(TOTAL)] for row in c["kept"]]


def range_rows(c, nseg, segment, cipher):
    """Untouched segments are never looked at; a touched one whose needed fragments are all given has
    USED exactly where dm_range_plan needs a fragment; one that lost a needed fragment uses the first k
    given and rebuilds only the lost needed ones (range_capi.inl:181;
    test_range_gpu.py::test_range_fuzz_200_cases).  dm_range_plan is host code (range_plan.hpp),
    checked against a brute-force model in tests/test_range_plan.py."""
    from deoss_amd.merkle import range_plan
    seg0, nt, need, _ = range_plan(c["size"], nseg, segment, K, c["off"], c["length"], cipher, 0)
    rows = [[ABSENT] * TOTAL for _ in range(nseg)]
    for t in range(nt):
        s = seg0 + t
        lost = [j for j in range(K) if need[t][j] and j not in c["kept"][s]]
        if not lost:
            rows[s][:K] = need[t]
            continue
        for j in c["kept"][s][:K]:
            rows[s][j] = USED
        for j in lost:
            rows[s][j] = REBUILT
    return rows


def _flat(rows):
    return bytes(x for row in rows for x in row)


# ---- references (CPU only), one per case, never changed afterwards ---------------------------------

class PlainObj:
    def __init__(self, oracle_lib, size, seed, segment):
        self.buf = _bytes(size, seed)
        c = Coded(oracle_lib, self.buf, segment, K, M)
        self.nseg, self.segd, self.fragd, self.fid, self.frags = c.nseg, c.segd, c.fragd, c.fid, c.frags
        self.padded = c.padded


class CipherObj:
    """tests/cipher_ref.py's scheme_full_processing of the object: names, fid and fragments of the
    ciphertext (one plain-Python CBC encryption per object)."""

    def __init__(self, size, seed, key):
        self.buf = _bytes(size, seed)
        segs, fragh, self.fid, self.frags = R.scheme_full_processing(self.buf, key, SEG)
        self.nseg = len(segs)
        self.segd = b"".join(segs)
        self.fragd = b"".join(h for row in fragh for h in row)
        self.raw = b"".join(f for row in self.frags for f in row)


def _given(o, c):
    """Fragment rows of a restore / repair / range case: kept ones, the hit one with a flipped bit."""
    rows = [[f if j in c["kept"][s] else None for j, f in enumerate(row)] for s, row in enumerate(o.frags)]
    for s, (j, at) in enumerate(c.get("hit", [])):
        rows[s][j] = _flip(rows[s][j], at)
    return rows


def _win_expect(wins, C, D, iv, X):
    """Expected output and verdicts of a window list.  Window w owns nblk + 1 output blocks (the last
    one a sentinel); block u of a window starting at ciphertext block b is D[b + u] ^ its predecessor;
    a check_pad window does not store its last block, whose verdict (sixteen 0x10 bytes) goes to
    pad_ok[w]; other verdicts stay as they were (7).  Returns (out blocks, verdicts, block offsets)."""
    b0, n, prev, pad = (np.array(x, dtype=np.int64) for x in zip(*wins))
    offs = np.concatenate([[0], np.cumsum(n + 1)])[:-1]
    out = np.full((int((n + 1).sum()), 16), SENTINEL, dtype=np.uint8)
    verdict = np.full(len(wins), 7, dtype=np.uint8)
    ivb = np.frombuffer(iv, dtype=np.uint8)
    for u in range(int(n.max())):
        m = np.nonzero(n > u)[0]
        idx = b0[m] + u
        pv = np.array(C[idx - 1])
        if u == 0:
            pv[prev[m] == 0] = ivb
            pv[prev[m] == 2] = X
        blk = D[idx] ^ pv
        last_pad = (pad[m] == 1) & (n[m] - 1 == u)
        out[(offs[m] + u)[~last_pad]] = blk[~last_pad]
        verdict[m[last_pad]] = (blk[last_pad] == 0x10).all(axis=1)
    return out, verdict, offs


def _win_blocks(key, seed):
    """(random ciphertext blocks C, their bare inverse cipher D, a predecessor block X kept elsewhere)"""
    rng = np.random.default_rng(seed)
    C = rng.integers(0, 256, size=(WIN_NB, 16), dtype=np.uint8)
    X = rng.integers(0, 256, size=16, dtype=np.uint8)
    return C, R.decrypt_blocks(R.expand_key(key), C), X


def _rs_object(oracle_lib, c):
    """nseg segments of 4 x frag bytes, the last one zero-padded: (truth (nseg, total, frag), padded object)."""
    segment = K * c["frag"]
    size = c["nseg"] * segment - segment // 3
    o = Coded(oracle_lib, _bytes(size, c["seed"]), segment, K, M)
    return np.array(np.frombuffer(o.raw, dtype=np.uint8)).reshape(c["nseg"], TOTAL, c["frag"]), \
        np.array(np.frombuffer(o.padded, dtype=np.uint8))


def build_ref(oracle_lib, c):
    kind, key = c["kind"], c["key"]
    r = {}
    if kind == "restore":
        o = r["o"] = PlainObj(oracle_lib, c["size"], c["seed"], SEG)
        r.update(frags=_given(o, c), fst=_flat(restore_rows(c)))
    elif kind == "restore_cipher":
        o = r["o"] = CipherObj(c["size"], c["seed"], key)
        r.update(frags=_given(o, c), fst=_flat(restore_rows(c)), wrong=bytes(b ^ 0x55 for b in key))
    elif kind == "repair":
        o = r["o"] = PlainObj(oracle_lib, c["size"], c["seed"], SEG)
        r.update(frags=_given(o, c), fst=_flat(repair_rows(c)))
    elif kind == "range":
        o = r["o"] = PlainObj(oracle_lib, c["size"], c["seed"], SEG)
        r.update(frags=_given(o, c), fst=_flat(range_rows(c, o.nseg, SEG, False)))
    elif kind == "range_cipher":
        o = r["o"] = CipherObj(c["size"], c["seed"], key)
        r.update(frags=_given(o, c), fst=_flat(range_rows(c, o.nseg, SEG, True)))
    elif kind == "process_cipher":
        r["o"] = CipherObj(c["size"], c["seed"], key)
    elif kind in ("retrieve_file", "retrieve_range", "repair_files"):
        o = r["o"] = PlainObj(oracle_lib, c["size"], c["seed"], FSEG)
        names = [o.fragd[32 * i:32 * i + 32].hex() for i in range(o.nseg * TOTAL)]
        assert len(set(names)) == len(names)
        r["files"] = {names[s * TOTAL + j]: o.frags[s][j] for s in range(o.nseg) for j in range(TOTAL)}
        r["have"] = [names[s * TOTAL + j] for s in range(o.nseg) for j in c["kept"][s]]
        rows = {"retrieve_file": first_k_rows, "repair_files": repair_rows}.get(kind)
        r["fst"] = _flat(rows(c) if rows else range_rows(c, o.nseg, FSEG, False))
    elif kind == "dev_aes":
        n, nseg = c["plain"], c["nseg"]
        plain = np.random.default_rng(c["seed"]).integers(0, 256, size=(nseg, n), dtype=np.uint8)
        padded = np.concatenate([plain, np.full((nseg, 16), 16, dtype=np.uint8)], axis=1)
        host = np.full((nseg, n + 16 + 48), SENTINEL, dtype=np.uint8)   # the bytes beyond plain + 16 must stay
        host[:, :n] = plain
        r.update(plain=plain, ct=R.cbc_encrypt_many(key, c["iv"], padded), host=host)
    elif kind == "dev_restore":
        truth, padded = _rs_object(oracle_lib, c)
        obj = np.full(c["nseg"] * K * c["frag"], 0xA5, dtype=np.uint8)
        for s, js in enumerate(c["in_place"]):
            for j in js:
                at = (s * K + j) * c["frag"]
                obj[at:at + c["frag"]] = truth[s, j]
        r.update(pool=truth, obj=obj, want=padded)
    elif kind == "dev_repair":
        truth, _ = _rs_object(oracle_lib, c)
        pres = np.zeros((c["nseg"], TOTAL), dtype=bool)
        tgt = np.zeros((c["nseg"], TOTAL), dtype=bool)
        for s in range(c["nseg"]):
            pres[s, c["present"][s]] = True
            tgt[s, c["want"][s]] = True
        work = np.full(truth.shape, FILL, dtype=np.uint8)
        work[pres] = truth[pres]
        want = work.copy()
        want[tgt] = truth[tgt]
        r.update(work=work, want=want, pres=pres, given=pres | tgt)
    elif kind == "dev_windows":
        C, D, X = _win_blocks(key, c["seed"])
        out, verdict, offs = _win_expect(c["wins"], C, D, c["iv"], X)
        r.update(C=C, X=X, out=out, verdict=verdict, offs=offs)
    return r


def prepare(c, r, where):
    """What a run of the case changes or writes: a fragment directory of its own."""
    if c["kind"] not in ("retrieve_file", "retrieve_range", "repair_files"):
        return None
    fd = where / "frags"
    fd.mkdir(parents=True)
    for name in r["have"]:
        (fd / name).write_bytes(r["files"][name])
    return where


# ---- one call of each kind, checked; returns what was wrong -----------------------------------------

class Env:
    def __init__(self, ctx, proc, settle=False):
        import copy
        self.torch, self.ctx, self.p, self.enc = _torch(), ctx, proc, proc.enc
        # settle: a kind that makes two asynchronous calls synchronises its stream between them.  Routing
        # counts a lane whose last call has not finished on the GPU as busy, so the second call may be sent
        # to another lane than the first; test 2 places calls by lane and cannot have that.
        self.settle = settle
        self.pf = copy.copy(proc)              # the same coder at the file paths' segment size
        self.pf.segment, self.pf.frag = FSEG, FFRAG


def _status(bad, what, got, want):
    if got != want:
        bad.append("%s: got %s, want %s" % (what, list(got), list(want)))


def _run_restore(env, c, r, prep, st, note):
    o, bad = r["o"], []
    key = c["key"] if c["kind"] == "restore_cipher" else b""
    ok, out, fst, sst = env.p.restore_buffer(r["frags"], c["size"], o.fragd, o.segd, o.fid, VALL, cipher=key)
    note()
    if not (ok and out == o.buf):
        bad.append("restored bytes differ (ok = %s)" % ok)
    _status(bad, "fragment statuses", fst, r["fst"])
    _status(bad, "segment statuses", sst, bytes(o.nseg))
    if key:   # the right names with a wrong cipher: every padding is bad, nothing leaves the device
        dst = ctypes.create_string_buffer(bytes([0x5A]) * c["size"], c["size"])
        ok, out, fst, sst = env.p.restore_buffer(r["frags"], c["size"], o.fragd, o.segd, o.fid, VALL, out=dst,
                                                 cipher=r["wrong"])
        note()
        if ok or out is not None or dst.raw != bytes([0x5A]) * c["size"]:
            bad.append("a wrong cipher released bytes")
        _status(bad, "segment statuses with a wrong cipher", sst, bytes([SEG_BAD_PADDING]) * o.nseg)
    return bad


def _run_repair(env, c, r, prep, st, note):
    o, bad = r["o"], []
    outs = [ctypes.create_string_buffer(bytes([FILL]) * FRAG, FRAG) for _ in range(o.nseg * TOTAL)]
    ok, got, fst, sst = env.p.repair_buffer(r["frags"], o.fragd, out=outs)
    note()
    if not ok:
        bad.append("not ok")
    _status(bad, "fragment statuses", fst, r["fst"])
    _status(bad, "segment statuses", sst, bytes(o.nseg))
    for i, b in enumerate(outs):   # a delivered fragment is the oracle's, every other buffer untouched
        s, j = divmod(i, TOTAL)
        if b.raw != (o.frags[s][j] if r["fst"][i] == REBUILT else bytes([FILL]) * FRAG):
            bad.append("out buffer of fragment (%d, %d)" % (s, j))
    return bad


def _run_range(env, c, r, prep, st, note):
    o, bad = r["o"], []
    key = c["key"] if c["kind"] == "range_cipher" else b""
    ok, out, fst, sst = env.p.restore_range(r["frags"], c["size"], c["off"], c["length"], o.fragd, cipher=key)
    note()
    if not (ok and out == o.buf[c["off"]:c["off"] + c["length"]]):
        bad.append("range bytes differ (ok = %s)" % ok)
    _status(bad, "fragment statuses", fst, r["fst"])
    _status(bad, "segment statuses", sst, bytes(o.nseg))
    return bad


def _run_process_cipher(env, c, r, prep, st, note):
    o = r["o"]
    got = env.p.process_buffer(o.buf, want_frags=True, cipher=c["key"])
    note()
    return [] if got == (o.segd, o.fragd, o.fid, o.raw) else ["digests, fid or fragments differ"]


def _run_retrieve_file(env, c, r, prep, st, note):
    o, bad = r["o"], []
    ok, fst, sst = env.pf.retrieve_file(str(prep / "frags"), o.fragd, c["size"], str(prep / "object"), o.segd, o.fid)
    note()
    if not (ok and (prep / "object").read_bytes() == o.buf):
        bad.append("restored file differs (ok = %s)" % ok)
    _status(bad, "fragment statuses", fst, r["fst"])
    _status(bad, "segment statuses", sst, bytes(o.nseg))
    return bad


def _run_retrieve_range(env, c, r, prep, st, note):
    o, bad = r["o"], []
    ok, out, fst, sst = env.pf.retrieve_range(str(prep / "frags"), o.fragd, c["size"], c["off"], c["length"])
    note()
    if not (ok and out == o.buf[c["off"]:c["off"] + c["length"]]):
        bad.append("range bytes differ (ok = %s)" % ok)
    _status(bad, "fragment statuses", fst, r["fst"])
    _status(bad, "segment statuses", sst, bytes(o.nseg))
    return bad


def _run_repair_files(env, c, r, prep, st, note):
    o, bad = r["o"], []
    ok, n, fst, sst = env.pf.repair_files(str(prep / "frags"), o.fragd)
    note()
    if not ok or n != len(r["files"]) - len(r["have"]):
        bad.append("ok = %s, %d files rebuilt of %d missing" % (ok, n, len(r["files"]) - len(r["have"])))
    _status(bad, "fragment statuses", fst, r["fst"])
    _status(bad, "segment statuses", sst, bytes(o.nseg))
    if sorted(os.listdir(prep / "frags")) != sorted(r["files"]):
        bad.append("the directory is not whole")
    else:
        bad += ["file " + name for name, b in r["files"].items() if (prep / "frags" / name).read_bytes() != b]
    return bad


def _run_dev_aes(env, c, r, prep, st, note):
    torch, n, nseg = env.torch, c["plain"], c["nseg"]
    stride = n + 16 + 48
    with torch.cuda.stream(st):
        buf = torch.from_numpy(r["host"]).cuda()
        out = torch.full((nseg * n + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        okd = torch.full((nseg + 16,), 7, dtype=torch.uint8, device="cuda")
        env.ctx.aes_cbc_encrypt_device_async(c["key"], c["iv"], buf.data_ptr(), stride, n, nseg, st.cuda_stream)
        note()
        if env.settle:
            st.synchronize()
        env.ctx.aes_cbc_decrypt_device_async(c["key"], c["iv"], buf.data_ptr(), stride, n + 16, nseg, out.data_ptr(), n,
                                             okd.data_ptr(), st.cuda_stream)
        note()
        st.synchronize()
        got, plain, okh = buf.cpu().numpy(), out.cpu().numpy(), okd.cpu().numpy()
    bad = []
    if not ((got[:, :n + 16] == r["ct"]).all() and (got[:, n + 16:] == SENTINEL).all()):
        bad.append("ciphertext differs or bytes beyond it changed")
    if not ((plain[:nseg * n].reshape(nseg, n) == r["plain"]).all() and (plain[nseg * n:] == SENTINEL).all()):
        bad.append("decrypted plaintext differs")
    if not ((okh[:nseg] == 1).all() and (okh[nseg:] == 7).all()):
        bad.append("padding verdicts %s" % okh.tolist())
    return bad


def _run_dev_restore(env, c, r, prep, st, note):
    torch, frag, nseg = env.torch, c["frag"], c["nseg"]
    with torch.cuda.stream(st):
        pool = torch.from_numpy(r["pool"]).cuda()
        obj = torch.from_numpy(r["obj"]).cuda()
        ptrs = [0] * (nseg * TOTAL)
        for s in range(nseg):
            for j in c["present"][s]:
                if j in c["in_place"][s]:
                    ptrs[s * TOTAL + j] = obj.data_ptr() + (s * K + j) * frag
                else:
                    ptrs[s * TOTAL + j] = pool.data_ptr() + (s * TOTAL + j) * frag
        env.enc.restore_device_async(ptrs, nseg, K * frag, obj.data_ptr(), st.cuda_stream)
        note()
        st.synchronize()
        got = obj.cpu().numpy()
    diff = np.nonzero(got != r["want"])[0]
    return ["first differing byte %d" % diff[0]] if diff.size else []


def _run_dev_repair(env, c, r, prep, st, note):
    torch, frag, nseg = env.torch, c["frag"], c["nseg"]
    with torch.cuda.stream(st):
        work = torch.from_numpy(r["work"]).cuda()
        given = r["given"].reshape(-1)
        ptrs = [work.data_ptr() + i * frag if given[i] else 0 for i in range(nseg * TOTAL)]
        env.enc.repair_device_async(ptrs, r["pres"].reshape(-1).tolist(), nseg, frag, st.cuda_stream)
        note()
        st.synchronize()
        got = work.cpu().numpy()
    diff = np.nonzero((got != r["want"]).reshape(-1))[0]   # wanted: the oracle's; held or neither: unchanged
    return ["first differing byte %d (fragment %d)" % (diff[0], diff[0] // frag)] if diff.size else []


def _windows(wins, offs, dC, dX, dout):
    return [(dC + 16 * b0, 0 if prev == 0 else dC + 16 * (b0 - 1) if prev == 1 else dX, dout + 16 * int(o), n, pad)
            for (b0, n, prev, pad), o in zip(wins, offs)]


def _run_dev_windows(env, c, r, prep, st, note):
    torch = env.torch
    with torch.cuda.stream(st):
        dC, dX = torch.from_numpy(r["C"]).cuda(), torch.from_numpy(r["X"]).cuda()
        out = torch.full((r["out"].size,), SENTINEL, dtype=torch.uint8, device="cuda")
        verdict = torch.full((len(c["wins"]),), 7, dtype=torch.uint8, device="cuda")
        wins = _windows(c["wins"], r["offs"], dC.data_ptr(), dX.data_ptr(), out.data_ptr())
        env.ctx.aes_cbc_decrypt_windows_device_async(c["key"], c["iv"], wins, verdict.data_ptr(), st.cuda_stream)
        note()
        st.synchronize()
        got, gv = out.cpu().numpy().reshape(-1, 16), verdict.cpu().numpy()
    bad = []
    diff = np.nonzero((got != r["out"]).any(axis=1))[0]
    if diff.size:
        bad.append("first differing output block %d" % diff[0])
    if not (gv == r["verdict"]).all():
        bad.append("padding verdicts differ")
    return bad


RUN = {"restore": _run_restore, "restore_cipher": _run_restore, "repair": _run_repair, "range": _run_range,
       "range_cipher": _run_range, "process_cipher": _run_process_cipher, "retrieve_file": _run_retrieve_file,
       "retrieve_range": _run_retrieve_range, "repair_files": _run_repair_files, "dev_aes": _run_dev_aes,
       "dev_restore": _run_dev_restore, "dev_repair": _run_dev_repair, "dev_windows": _run_dev_windows}


@pytest.fixture(scope="module")
def mix(oracle_lib):
    """[(case, reference)] of draw_mix(), computed once for tests 1 and 2 and left unchanged."""
    return [(c, build_ref(oracle_lib, c)) for c in draw_mix()]


def _small_slots(monkeypatch):
    """Pinned file slots of 3 fragments (read per call): slots are reused within a call, and a lane's
    first file call does not pin 4 x 64 MiB while a blocker runs."""
    monkeypatch.setenv("DEOSS_FP_SLOT_BYTES", str(3 * FFRAG))


# ---- 1. concurrent callers ---------------------------------------------------------------------------

def _concurrent(env, plans, tmp_path):
    """plans[t]: the (case, reference) list of thread t.  Every thread has its own stream, waits at the
    barrier and runs its cases in turn.  Returns (failures, [(kind, devices, lane)] of every call)."""
    todo = [[(c, r, prepare(c, r, tmp_path / ("t%d_%d" % (t, i)))) for i, (c, r) in enumerate(plan)]
            for t, plan in enumerate(plans)]
    streams = [env.torch.cuda.Stream() for _ in plans]
    barrier = threading.Barrier(len(plans))
    failures, where = [], []

    def worker(t):
        barrier.wait()
        for i, (c, r, prep) in enumerate(todo[t]):
            def note():
                devs, _, lane = env.ctx.last_call_devices()
                where.append((c["kind"], tuple(devs), lane))
            try:
                bad = RUN[c["kind"]](env, c, r, prep, streams[t], note)
            except Exception as e:   # an exception is a failure of that call
                bad = [repr(e)]
            failures.extend((t, i, c["kind"], b) for b in bad)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(len(plans))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    env.torch.cuda.synchronize()
    return failures, where


@pytest.mark.gpu
def test_concurrent_callers_on_three_lanes(mix, tmp_path, monkeypatch):
    """Twelve threads, three iterations each, on one MerkleContext(lanes=3), one Processor and its
    coder: every result is the reference's, and the calls did not all run on one lane.

    Catches: scratch shared between lanes that should be per lane -- e.g. rs_ln() (rs_capi.inl:48)
    returning r->ln[0] for every lane, or Dev::aes_win / Dev::htab made context-wide: two lanes'
    calls then upload descriptors and tables into one block while the other's kernel reads it."""
    from deoss_amd import MerkleContext
    from deoss_amd.process import Processor
    _small_slots(monkeypatch)
    ctx = MerkleContext(lanes=3)
    try:
        assert (ctx.device_count, ctx.lane_count) == (1, 3)
        proc = Processor(ctx, K, M, SEG)
        try:
            failures, where = _concurrent(Env(ctx, proc), [mix[3 * t:3 * t + 3] for t in range(12)], tmp_path)
        finally:
            proc.close()
    finally:
        ctx.close()
    assert failures == []
    lanes = sorted({lane for _, _, lane in where})
    print("lanes seen:", lanes, "calls:", len(where))
    assert {kind for kind, _, _ in where} == set(KINDS)
    assert set(lanes) <= {0, 1, 2} and len(lanes) >= 2, lanes   # not serialised on one lane (test 2 covers each)


class _Blockers:
    """The 64 MiB object every blocker hashes (a root at 32 MiB chunks: two serial chains side by side,
    about 0.5 s), the roots, and the stream of the device-level calls under test."""

    def __init__(self, torch):
        self.torch = torch
        self.blk = torch.zeros(BLOCKER_BYTES, dtype=torch.uint8, device="cuda")
        self.roots = torch.zeros((2, 32), dtype=torch.uint8, device="cuda")
        # another priority than the blockers' side streams: ordinary streams of one priority share a few
        # hardware queues (init_device's note), and a call that shared a blocker's would wait for it
        self.st = torch.cuda.Stream(priority=-1)


def _beside_blockers(env, bl, nb, items, seen):
    """Queue nb blockers on side streams -- routing gives them lanes 0 .. nb - 1 -- then run the items,
    each of which must run on lane nb of the first GPU and give the reference's result; afterwards the
    blockers must still be running, else the calls did not run beside them.  Returns the failures."""
    torch, ctx, failures = bl.torch, env.ctx, []
    torch.cuda.synchronize()
    side = [torch.cuda.Stream() for _ in range(nb)]
    try:
        for b, s in enumerate(side):
            ctx.root_device_async(bl.blk.data_ptr(), BLOCKER_BYTES, BLOCKER_CHUNK, bl.roots[b].data_ptr(), 0, s.cuda_stream)
            assert ctx.last_call_devices()[2] == b, "blocker %d did not take lane %d" % (b, b)
        for c, r, prep in items:
            def note():
                devs, _, lane = ctx.last_call_devices()
                seen.add((c["kind"], lane))
                if (devs, lane) != ([0], nb):
                    failures.append((nb, c["kind"], "ran on device(s) %s, lane %d" % (devs, lane)))
            try:
                bad = RUN[c["kind"]](env, c, r, prep, bl.st, note)
            except Exception as e:
                bad = [repr(e)]
            failures.extend((nb, c["kind"], b) for b in bad)
        running = [not s.query() for s in side]
    finally:
        torch.cuda.synchronize()
    assert all(running), ("with %d blocker(s): one had finished before the last call returned, so the calls did "
                          "not run beside it and the run proved nothing" % nb)
    return failures


@pytest.mark.gpu
def test_concurrent_callers_on_virtual_devices(mix, tmp_path, monkeypatch):
    """The same body, four threads with two iterations, on a context of two virtual devices with two
    lanes each (DEOSS_VIRTUAL_DEVICES=2 at creation, lanes=2): nphys is 2, devs is lane-major
    [lane 0 of GPU 0, lane 0 of GPU 1, lane 1 of GPU 0, lane 1 of GPU 1], the coder lives on the first
    GPU, so its calls run on devs[0] or devs[2] and rs_ln() must divide that index by nphys.  Every call
    must report device 0 and lane 0 or 1.  Then, as in test 2 and without threads: with a blocker on
    lane 0 every kind must run on lane 1 (devs[2]) and be exact.

    Catches: rs_ln (rs_capi.inl:48-49) or note_call (merkle_capi.hip:440-441) taking the lane without
    the division by nphys, and choose_lane's lane-major index l * nphys + p (merkle_capi.hip:587): each
    is the identity on a one-GPU context and goes wrong only with nphys > 1."""
    from deoss_amd import MerkleContext
    from deoss_amd.process import Processor
    _small_slots(monkeypatch)
    monkeypatch.setenv("DEOSS_VIRTUAL_DEVICES", "2")   # read at dm_create
    ctx = MerkleContext(lanes=2)
    monkeypatch.delenv("DEOSS_VIRTUAL_DEVICES")
    seen = set()
    try:
        assert (ctx.device_count, ctx.lane_count) == (2, 2)
        proc = Processor(ctx, K, M, SEG)
        try:
            cases = [next((c, r) for c, r in mix if c["kind"] == kind) for kind in VIRTUAL_KINDS]
            failures, where = _concurrent(Env(ctx, proc), [cases[2 * t:2 * t + 2] for t in range(4)], tmp_path)
            items = [(c, r, prepare(c, r, tmp_path / ("b1_" + c["kind"]))) for c, r in cases]
            placed = _beside_blockers(Env(ctx, proc, settle=True), _Blockers(_torch()), 1, items, seen)
        finally:
            proc.close()
    finally:
        ctx.close()
    assert failures == [] and placed == []
    assert {kind for kind, _, _ in where} == set(VIRTUAL_KINDS)
    assert {devs for _, devs, _ in where} == {(0,)} and {lane for _, _, lane in where} <= {0, 1}, where
    assert seen == {(kind, 1) for kind in VIRTUAL_KINDS}, seen


# ---- 2. every lane runs every path while the other lanes still have work ------------------------------

@pytest.mark.gpu
def test_every_lane_runs_every_kind_beside_running_lanes(mix, tmp_path, monkeypatch):
    """choose_lane (merkle_capi.hip:581) counts a lane whose tail event has not completed as busy and
    takes the lowest lane otherwise.  So with no blocker a call runs on lane 0, with a blocker (a 64 MiB
    root at 32 MiB chunks on a side stream) on lane 0 it runs on lane 1, with blockers on lanes 0 and 1
    on lane 2 -- where each scratch buffer is then allocated for the first time while another lane's
    kernels run.  Every kind runs once in each situation and is checked bit-exact.

    Catches: a lane index taken with the wrong divisor or offset (rs_ln, rs_capi.inl:48-49, or
    note_call's g / nphys, merkle_capi.hip:441): lanes 1 and 2 then share lane 0's RsLane, or the call
    reports another lane than routing chose; and choose_lane's hipEventQuery(ev_tail) line
    (merkle_capi.hip:588), without which every call here lands on lane 0 behind the blocker."""
    from deoss_amd import MerkleContext
    from deoss_amd.process import Processor
    torch = _torch()
    _small_slots(monkeypatch)
    cases = [c for c, _ in mix]
    refs = {id(c): r for c, r in mix}
    todo = [[(c, refs[id(c)], prepare(c, refs[id(c)], tmp_path / ("b%d_%s" % (nb, c["kind"]))))
             for c in [pick(cases, kind, nb) for kind in KINDS]] for nb in range(3)]
    ctx = MerkleContext(lanes=3)
    seen, failures = set(), []
    try:
        proc = Processor(ctx, K, M, SEG)
        try:
            env, bl = Env(ctx, proc, settle=True), _Blockers(torch)
            for nb in range(3):
                failures += _beside_blockers(env, bl, nb, todo[nb], seen)
            # the blockers computed something: both roots are of the same bytes
            assert bytes(bl.roots[0].cpu().numpy()) == bytes(bl.roots[1].cpu().numpy()) != bytes(32)
        finally:
            proc.close()
    finally:
        ctx.close()
    assert failures == []
    table = {kind: sorted(lane for k, lane in seen if k == kind) for kind in KINDS}
    print("(kind, lane):", table)
    assert seen == {(kind, lane) for kind in KINDS for lane in range(3)}, table


# ---- 3. one lane, two streams, no host synchronisation in between ------------------------------------
#
# Scratch capacities: DevBuf::ensure (merkle_capi.hip:181) rounds a block up to 2 MiB = 2,097,152 bytes.
#   rst_tab   one coding table is k x 256 x 8 = 8,192 bytes (rs_table, rs_plan.hpp:113), one per distinct
#             pattern: X1's few patterns fit the first 2 MiB block (256 tables); all 495 patterns need
#             495 x 8,192 = 4,055,040 bytes, so X2 grows rst_tab from 2 MiB to 4 MiB.
#   rst_desc  sizeof(dm::RsRestoreDesc) = 8 x 8 + 8 x 8 + 4 + 4 = 136 bytes (rs_plan.hpp:27): 495 of them
#             are 67,320 bytes and stay within the first 2 MiB block; it is refilled, not regrown.
#   aes_win   sizeof(dm::AesWindow) = 3 x 8 + 8 + 4 + 4 = 40 bytes (aes_kernels.hpp:214): 2 MiB hold 52,428
#             windows; X2's 60,000 need 2,400,000 bytes, so it grows aes_win from 2 MiB to 4 MiB.
#   dec_tab   k x 256 x 8 = 8,192 bytes for any pattern (k <= 8: at most 16 KiB): it can never outgrow its
#             first block, so for reconstruct X2 refills it with another pattern's table, no regrowth.
#   htab      the pinned bounce buffer starts at 1 MiB (tables_begin, merkle_capi.hip:739): X2's tables
#             of 3.9 MiB (rs) and 2.3 MiB (windows) regrow it as well.
NWIN_BIG = 60000
assert NWIN_BIG * 40 > 2 << 20 and 495 * 8192 > 2 << 20


class _RsJob:
    """Device buffers and the expected result of one repair / restore / reconstruct call."""

    def __init__(self, torch, oracle_lib, frag, present, seed, restore=False, want_all=False):
        nseg = len(present)
        c = dict(frag=frag, nseg=nseg, seed=seed)
        truth, padded = _rs_object(oracle_lib, c)
        self.frag, self.nseg = frag, nseg
        self.pres = np.zeros((nseg, TOTAL), dtype=bool)
        for s, p in enumerate(present):
            self.pres[s, list(p)] = True
        if restore:     # fragments elsewhere, the object buffer starts as 0xA5
            self.pool = torch.from_numpy(truth).cuda()
            self.buf = torch.full((nseg * K * frag,), 0xA5, dtype=torch.uint8, device="cuda")
            self.want = padded
            base = self.pool.data_ptr()
        else:           # held fragments in place, every other slot FILL; unless want_all, a missing parity
            work = np.full(truth.shape, FILL, dtype=np.uint8)   # fragment of an odd segment is neither held nor wanted
            work[self.pres] = truth[self.pres]
            self.skip = np.zeros_like(self.pres)
            if not want_all:
                self.skip[1::2, K:] = ~self.pres[1::2, K:]
            self.want = work.copy()
            tgt = ~self.pres & ~self.skip
            self.want[tgt] = truth[tgt]
            self.buf = torch.from_numpy(work).cuda()
            base = self.buf.data_ptr()
        give = self.pres if restore else ~self.skip
        self.ptrs = [base + i * frag if g else 0 for i, g in enumerate(give.reshape(-1))]

    def check(self, tag):
        got = self.buf.cpu().numpy().reshape(-1)
        diff = np.nonzero(got != self.want.reshape(-1))[0]
        assert diff.size == 0, (tag, "first differing byte", int(diff[0]), "fragment", int(diff[0]) // self.frag)


class _WinJob:
    """Windows of one and two blocks (a few with check_pad) over one small ciphertext, each writing to
    output blocks of its own; the reference decrypts the ciphertext once and is sliced (_win_expect)."""

    def __init__(self, torch, key, iv, nwin, seed):
        from deoss_amd._lib import AesWindow
        rng = random.Random(seed)
        wins = []
        for _ in range(nwin):
            n = rng.randint(1, 2)
            wins.append((rng.randint(1, WIN_NB - 3), n, rng.randrange(3), int(n == 2 and rng.random() < 0.1)))
        C, D, X = _win_blocks(key, seed)
        self.key, self.iv, self.nwin = key, iv, nwin
        self.want, self.verdict, offs = _win_expect(wins, C, D, iv, X)
        self.dC, self.dX = torch.from_numpy(C).cuda(), torch.from_numpy(X).cuda()
        self.out = torch.full((self.want.size,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.pad = torch.full((nwin,), 7, dtype=torch.uint8, device="cuda")
        # the descriptor array is built here, not inside the call, so that X2 reaches tables_begin
        # while the blocker still runs
        self.arr = (AesWindow * nwin)(*[AesWindow(i, p or None, o, n, pad) for i, p, o, n, pad in _windows(
            wins, offs, self.dC.data_ptr(), self.dX.data_ptr(), self.out.data_ptr())])

    def call(self, ctx, stream):
        ctx._check(ctx._L.dm_aes_cbc_decrypt_windows_device_async(
            ctx._h, self.key, len(self.key), self.iv, self.arr, self.nwin, ctypes.c_void_p(self.pad.data_ptr()),
            ctypes.c_void_p(stream)), "dm_aes_cbc_decrypt_windows_device_async")

    def check(self, tag):
        diff = np.nonzero((self.out.cpu().numpy().reshape(-1, 16) != self.want).any(axis=1))[0]
        assert diff.size == 0, (tag, "first differing output block", int(diff[0]))
        assert (self.pad.cpu().numpy() == self.verdict).all(), (tag, "padding verdicts")


class _AesJob:
    """aes_cbc_encrypt_device_async then aes_cbc_decrypt_device_async of nseg chains: everything travels
    in kernel arguments (round keys included), nothing in lane scratch."""

    def __init__(self, torch, key, iv, blocks, nseg, seed):
        n = 16 * blocks
        self.key, self.iv, self.n, self.nseg = key, iv, n, nseg
        self.plain = np.random.default_rng(seed).integers(0, 256, size=(nseg, n), dtype=np.uint8)
        self.ct = R.cbc_encrypt_many(key, iv, np.concatenate([self.plain, np.full((nseg, 16), 16, dtype=np.uint8)], axis=1))
        self.buf = torch.zeros((nseg, n + 16), dtype=torch.uint8, device="cuda")
        self.buf[:, :n] = torch.from_numpy(self.plain).cuda()
        self.out = torch.full((nseg, n), SENTINEL, dtype=torch.uint8, device="cuda")
        self.ok = torch.full((nseg,), 7, dtype=torch.uint8, device="cuda")

    def call(self, ctx, stream):
        n, nseg = self.n, self.nseg
        ctx.aes_cbc_encrypt_device_async(self.key, self.iv, self.buf.data_ptr(), n + 16, n, nseg, stream)
        ctx.aes_cbc_decrypt_device_async(self.key, self.iv, self.buf.data_ptr(), n + 16, n + 16, nseg, self.out.data_ptr(),
                                         n, self.ok.data_ptr(), stream)

    def check(self, tag):
        assert (self.buf.cpu().numpy() == self.ct).all(), (tag, "ciphertext")
        assert (self.out.cpu().numpy() == self.plain).all() and self.ok.cpu().tolist() == [1] * self.nseg, (tag, "plaintext")


ALL_495 = [list(p) for p in itertools.combinations(range(TOTAL), K)]


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["reconstruct", "restore", "repair", "windows", "aes"])
def test_one_lane_two_streams_no_host_sync(oracle_lib, entry):
    """On a one-lane context: X1 on stream A queued behind a blocker (another context's 64 MiB root on
    A), X2 on stream B with other inputs and tables larger than the scratch X1 sized, X3 on A again;
    one device synchronisation, then X1, X2 and X3 each equal the reference and every slot that was
    neither held nor wanted kept its sentinel.

    Catches: tables_begin's hipEventSynchronize(d.ev_htab) (merkle_capi.hip:738), without which X2
    overwrites the pinned bounce buffer before X1's upload was copied out of it (X1 then runs with
    X2's descriptors); begin_call's hipStreamWaitEvent on ev_tail (merkle_capi.hip:716), without which
    X2's upload on B lands in rst_desc / rst_tab / dec_tab / aes_win before X1's kernel on A has read
    them; and DevBuf::ensure's reaper_put (merkle_capi.hip:172): a block freed and reused at once
    while X1's queued kernel still reads it.  "aes": the plain encrypt / decrypt pair keeps nothing in
    lane scratch; two keys of different length interleaved on A and B pin that down."""
    from deoss_amd import MerkleContext
    from deoss_amd.reedsolomon import New
    torch = _torch()
    a, b = MerkleContext(lanes=1), MerkleContext(lanes=1)
    try:
        enc = New(a, K, M)
        A, B = torch.cuda.Stream(), torch.cuda.Stream(priority=-1)   # B never shares A's hardware queue
        blk = torch.zeros(BLOCKER_BYTES, dtype=torch.uint8, device="cuda")
        root = torch.zeros(32, dtype=torch.uint8, device="cuda")
        rng = random.Random(len(entry))
        small = [sorted(rng.sample(range(TOTAL), rng.randint(K, TOTAL - 1))) for _ in range(6)]
        if entry == "reconstruct":   # one segment per call, three different erasure patterns (dec_tab)
            jobs = [_RsJob(torch, oracle_lib, 16 * n, [p], 31 + n) for n, p in ((5, [0, 5, 6, 11]), (64, [2, 3, 7, 9, 10]),
                                                                                (5, [1, 4, 8, 9]))]

            def call(j, s):   # reconstruct rebuilds every missing shard: all twelve slots are given
                enc.reconstruct_device_async([j.buf.data_ptr() + i * j.frag for i in range(TOTAL)], j.pres[0].tolist(),
                                             j.frag, s)
        elif entry == "restore":     # X2: all 495 patterns, nothing in place (rst_tab 2 MiB -> 4 MiB)
            jobs = [_RsJob(torch, oracle_lib, 32, small[:3], 41, restore=True),
                    _RsJob(torch, oracle_lib, 16, ALL_495, 42, restore=True),
                    _RsJob(torch, oracle_lib, 32, small[3:], 43, restore=True)]

            def call(j, s):
                enc.restore_device_async(j.ptrs, j.nseg, K * j.frag, j.buf.data_ptr(), s)
        elif entry == "repair":      # X2: all 495 patterns with 8 outputs each (rst_tab 2 MiB -> 4 MiB)
            jobs = [_RsJob(torch, oracle_lib, 32, small[:3], 51), _RsJob(torch, oracle_lib, 16, ALL_495, 52, want_all=True),
                    _RsJob(torch, oracle_lib, 32, small[3:], 53)]

            def call(j, s):
                enc.repair_device_async(j.ptrs, j.pres.reshape(-1).tolist(), j.nseg, j.frag, s)
        elif entry == "windows":     # X2: 60,000 windows (aes_win 2 MiB -> 4 MiB), another key length
            keys = [bytes(rng.randrange(256) for _ in range(n)) for n in (16, 32, 24)]
            ivs = [bytes(rng.randrange(256) for _ in range(16)) for _ in range(3)]
            jobs = [_WinJob(torch, keys[0], ivs[0], 40, 61), _WinJob(torch, keys[1], ivs[1], NWIN_BIG, 62),
                    _WinJob(torch, keys[2], ivs[2], 40, 63)]

            def call(j, s):
                j.call(a, s)
        else:
            keys = [bytes(rng.randrange(256) for _ in range(n)) for n in (16, 32, 24)]
            ivs = [bytes(rng.randrange(256) for _ in range(16)) for _ in range(3)]
            jobs = [_AesJob(torch, keys[0], ivs[0], 9, 5, 71), _AesJob(torch, keys[1], ivs[1], 17, 3, 72),
                    _AesJob(torch, keys[2], ivs[2], 9, 5, 73)]

            def call(j, s):
                j.call(a, s)
        x1, x2, x3 = jobs
        torch.cuda.synchronize()
        try:
            b.root_device_async(blk.data_ptr(), BLOCKER_BYTES, BLOCKER_CHUNK, root.data_ptr(), 0, A.cuda_stream)
            call(x1, A.cuda_stream)
            queued = not A.query()
            call(x2, B.cuda_stream)
            call(x3, A.cuda_stream)
        finally:
            torch.cuda.synchronize()
        assert queued, "X1 returned after the blocker had finished: nothing was queued, the run proved nothing"
        for tag, j in (("X1", x1), ("X2", x2), ("X3", x3)):
            j.check((entry, tag))
        enc.close()
    finally:
        torch.cuda.synchronize()
        a.close()
        b.close()


# ---- 4. the drawn mix, checked on the CPU -------------------------------------------------------------

def test_drawn_mix_shape():
    """The seeded mix of tests 1 and 2 covers what they claim (no GPU, no library: the draw is pure)."""
    cases = draw_mix()
    assert len(cases) == 36 and cases == draw_mix()              # seeded: the same every time
    assert {c["kind"] for c in cases} == set(KINDS) and set(VIRTUAL_KINDS) <= set(KINDS)
    # three key lengths, a different cipher per thread, all three lengths among the cases the barrier
    # releases together
    ciphered = [c for c in cases if c["kind"] in CIPHER_KINDS]
    assert {len(c["key"]) for c in ciphered} == set(KLENS)
    assert len({c["key"] for c in cases}) == 12
    assert {len(c["key"]) for c in ciphered if c["i"] == 0} == set(KLENS)
    # repair: calls with at most 4 missing everywhere (rs_restore_kernel) and with more (rs_repair_kernel)
    miss = [max(TOTAL - len(row) for row in c["kept"]) for c in cases if c["kind"] == "repair"]
    assert any(n <= K for n in miss) and any(n > K for n in miss) and min(miss) >= 1
    assert all(1 <= TOTAL - len(row) <= M for c in cases if c["kind"] == "repair" for row in c["kept"])
    for kind in ("restore", "restore_cipher"):
        of = [c for c in cases if c["kind"] == kind]
        assert of
        for c in of:   # two data fragments dropped, one of the first four kept corrupted, a good one left to replace it
            for row, (j, at) in zip(c["kept"], c["hit"]):
                assert sum(1 for x in range(K) if x not in row) == 2 and j in row[:K] and 0 <= at < FRAG
                assert len(row) - 1 >= K
    for kind, piece, frag in (("range", SEG, FRAG), ("range_cipher", P, FRAG), ("retrieve_range", FSEG, FFRAG)):
        of = [c for c in cases if c["kind"] == kind]
        assert of
        for c in of:
            off, end = c["off"], c["off"] + c["length"]
            assert 0 <= off < end <= c["size"] and off % 16 and end % 16
            assert (end - 1) // piece > off // piece              # crosses a segment boundary
            s, j = c["lost"]
            assert s == off // piece and j == off % piece // frag and j not in c["kept"][s]
    # every case expected to succeed keeps k good fragments in every segment: the reference alone predicts ok
    for c in cases:
        if "kept" in c:
            nseg = -(-c["size"] // {"restore_cipher": P, "range_cipher": P, "retrieve_file": FSEG, "retrieve_range": FSEG,
                                    "repair_files": FSEG}.get(c["kind"], SEG))
            assert len(c["kept"]) == nseg and 1 <= nseg <= 9
            bad = dict(enumerate(j for j, _ in c.get("hit", [])))
            for s, row in enumerate(c["kept"]):
                assert len(set(row)) == len(row) and set(row) <= set(range(TOTAL))
                assert len([x for x in row if x != bad.get(s)]) >= K, (c["kind"], s)
        if c["kind"] in ("dev_restore", "dev_repair"):
            assert 16 <= c["frag"] <= 1024 and all(len(p) >= K for p in c["present"])
        if c["kind"] == "dev_aes":
            assert 16 <= c["plain"] <= 1024
    files = [c for c in cases if c["kind"] in ("retrieve_file", "retrieve_range", "repair_files")]
    assert all(c["size"] % FSEG > 3 * FFRAG for c in files)        # no two fragments equal: one file per name
