"""Python mirror of the klauspost/reedsolomon Encoder DeOSS fragments use (``dm_rs_*``).

cess-go-sdk (go.mod:8) codes every 32 MiB segment into ``chain.DataShards = 4`` data and
``chain.ParShards = 8`` parity fragments (``node/tracker.go:250,369``,
``node/fileHandler.go:250``) with ``github.com/klauspost/reedsolomon v1.12.4`` (``go.mod:65``).
:func:`New` mirrors ``reedsolomon.New(dataShards, parityShards)``; the returned
:class:`Encoder` has ``Split``, ``Encode``, ``Reconstruct`` and ``Verify`` with the same
argument meaning (a list of shards, ``None`` / empty for a missing one) and the same errors
(too few shards, short data), over klauspost's whole range ``data + parity <= 256``.  Every byte is
coded on the GPU (``rs_code_kernel``; beyond 8 + 8 ``rs_code_wide_kernel``); there is no CPU
fallback.  Device-resident forms take raw device pointers and a HIP stream handle.  A coder
beyond 8 + 8 is the standalone Encoder only: FullProcessing, restore and repair refuse it.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

from ._lib import DM_ERR_EMPTY, DeossMerkleError
from .merkle import MerkleContext

DATA_SHARDS = 4     # chain.DataShards
PAR_SHARDS = 8      # chain.ParShards


class ErrTooFewShards(DeossMerkleError):
    pass


class Encoder:
    def __init__(self, ctx: MerkleContext, data_shards: int, parity_shards: int, wide: bool = False):
        self._ctx = ctx
        self._L = ctx._L
        h = ctypes.c_void_p()
        what = "dm_rs_create_wide" if wide else "dm_rs_create"
        rc = getattr(self._L, what)(ctx._h, data_shards, parity_shards, ctypes.byref(h))
        ctx._check(rc, what)
        self._h = h
        ctx._children.add(self)   # the context destroys this coder before itself
        self.data_shards = data_shards
        self.parity_shards = parity_shards
        self.total_shards = data_shards + parity_shards

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.dm_rs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str) -> None:
        if rc == 0:
            return
        detail = (self._L.dm_last_error(self._ctx._h) or b"").decode()
        if "too few shards" in detail:
            raise ErrTooFewShards(rc, "too few shards given")
        if rc == DM_ERR_EMPTY:
            raise DeossMerkleError(rc, "not enough data to fill the number of requested shards")
        raise DeossMerkleError(rc, f"{what}: {self._L.dm_strerror(rc).decode()}: {detail}")

    def matrix(self) -> List[List[int]]:
        k, t = self.data_shards, self.total_shards
        out = ctypes.create_string_buffer(t * k)
        self._check(self._L.dm_rs_matrix(self._h, out), "dm_rs_matrix")
        return [list(out.raw[r * k:(r + 1) * k]) for r in range(t)]

    # -- klauspost Encoder API (host shards) ---------------------------------------------------
    def Split(self, data: bytes) -> List[bytes]:
        """Equal-size data shards (ceil(len / data)), the last zero-padded, plus empty parity."""
        if len(data) == 0:
            raise DeossMerkleError(DM_ERR_EMPTY, "not enough data to fill the number of requested shards")
        per = (len(data) + self.data_shards - 1) // self.data_shards
        b = bytes(data) + bytes(per * self.data_shards - len(data))
        return [b[i * per:(i + 1) * per] for i in range(self.data_shards)] + \
            [bytes(per) for _ in range(self.parity_shards)]

    def Encode(self, shards: List[bytes]) -> List[bytes]:
        """Fill shards[data:] with parity; returns the (new) shard list."""
        k, m = self.data_shards, self.parity_shards
        if len(shards) != self.total_shards:
            raise DeossMerkleError(-2, "too few shards given")
        n = len(shards[0])
        if any(len(s) != n for s in shards[:k]) or n == 0:
            raise DeossMerkleError(-2, "shard sizes do not match")
        ins = [ctypes.create_string_buffer(bytes(s), n) for s in shards[:k]]
        outs = [ctypes.create_string_buffer(n) for _ in range(m)]
        dp = (ctypes.c_void_p * k)(*[ctypes.addressof(b) for b in ins])
        pp = (ctypes.c_void_p * m)(*[ctypes.addressof(b) for b in outs])
        self._check(self._L.dm_rs_encode(self._h, dp, pp, n), "dm_rs_encode")
        return list(shards[:k]) + [b.raw for b in outs]

    def EncodeBuffer(self, data: bytes) -> List[bytes]:
        """Split + Encode of one segment in one call (dm_rs_encode_buffer)."""
        k, t = self.data_shards, self.total_shards
        if len(data) == 0:
            raise DeossMerkleError(DM_ERR_EMPTY, "not enough data to fill the number of requested shards")
        per = (len(data) + k - 1) // k
        out = ctypes.create_string_buffer(per * t)
        got = ctypes.c_uint64()
        src = ctypes.create_string_buffer(bytes(data), len(data))
        self._check(self._L.dm_rs_encode_buffer(self._h, src, len(data), out, ctypes.byref(got)),
                    "dm_rs_encode_buffer")
        assert got.value == per
        raw = out.raw
        return [raw[i * per:(i + 1) * per] for i in range(t)]

    def Reconstruct(self, shards: Sequence[Optional[bytes]]) -> List[bytes]:
        """Rebuild missing shards (None or empty); returns the complete list."""
        t = self.total_shards
        if len(shards) != t:
            raise DeossMerkleError(-2, "too few shards given")
        sizes = {len(s) for s in shards if s}
        if len(sizes) != 1:
            if not sizes:
                raise ErrTooFewShards(-2, "too few shards given")
            raise DeossMerkleError(-2, "shard sizes do not match")
        n = sizes.pop()
        bufs = [ctypes.create_string_buffer(bytes(s) if s else bytes(n), n) for s in shards]
        present = bytes(int(bool(s)) for s in shards)
        ptrs = (ctypes.c_void_p * t)(*[ctypes.addressof(b) for b in bufs])
        self._check(self._L.dm_rs_reconstruct(self._h, ptrs, present, n), "dm_rs_reconstruct")
        return [b.raw for b in bufs]

    def Verify(self, shards: Sequence[bytes]) -> bool:
        t = self.total_shards
        if len(shards) != t:
            raise DeossMerkleError(-2, "too few shards given")
        n = len(shards[0])
        bufs = [ctypes.create_string_buffer(bytes(s), max(n, 1)) for s in shards]
        ptrs = (ctypes.c_void_p * t)(*[ctypes.addressof(b) for b in bufs])
        ok = ctypes.c_int()
        self._check(self._L.dm_rs_verify(self._h, ptrs, n, ctypes.byref(ok)), "dm_rs_verify")
        return bool(ok.value)

    # -- device-resident forms -----------------------------------------------------------------
    def encode_device_async(self, data_ptr: int, data_stride: int, parity_ptr: int, parity_stride: int, shard: int,
                            nseg: int = 1, stream: int = 0) -> None:
        self._check(self._L.dm_rs_encode_device_async(self._h, data_ptr, data_stride, parity_ptr, parity_stride,
                                                       shard, nseg, stream), "dm_rs_encode_device_async")

    def reconstruct_device_async(self, shard_ptrs: Sequence[int], present: Sequence[bool], shard: int,
                                 stream: int = 0) -> None:
        t = self.total_shards
        ptrs = (ctypes.c_void_p * t)(*shard_ptrs)
        pres = bytes(int(bool(p)) for p in present)
        self._check(self._L.dm_rs_reconstruct_device_async(self._h, ptrs, pres, shard, stream),
                    "dm_rs_reconstruct_device_async")


    def restore_device_async(self, frag_ptrs: Sequence[int], nseg: int, segment: int, obj_ptr: int,
                             stream: int = 0) -> None:
        """``dm_rs_restore_device_async``: ``nseg`` segments, each with its own erasure pattern, in one
        kernel launch.  ``frag_ptrs``: nseg x total device addresses (0 / None = absent); afterwards
        ``obj_ptr`` holds every segment's data fragments in order."""
        n = nseg * self.total_shards
        if len(frag_ptrs) != n:
            raise DeossMerkleError(-2, "need one pointer per fragment of every segment")
        ptrs = (ctypes.c_void_p * n)(*[p or None for p in frag_ptrs])
        self._check(self._L.dm_rs_restore_device_async(self._h, ptrs, nseg, segment, obj_ptr, stream),
                    "dm_rs_restore_device_async")


    def repair_device_async(self, frag_ptrs: Sequence[int], present: Sequence[bool], nseg: int, frag: int,
                            stream: int = 0) -> None:
        """``dm_rs_repair_device_async``: ``nseg`` segments, each with its own pattern, in one kernel
        launch.  ``frag_ptrs``: nseg x total device addresses of ``frag`` bytes each; ``present``
        truthy: holds the fragment; falsy with an address: wanted, written; 0 / None: absent and
        not wanted."""
        n = nseg * self.total_shards
        if len(frag_ptrs) != n or len(present) != n:
            raise DeossMerkleError(-2, "need one pointer and one flag per fragment of every segment")
        ptrs = (ctypes.c_void_p * n)(*[p or None for p in frag_ptrs])
        pres = bytes(int(bool(p)) for p in present)
        self._check(self._L.dm_rs_repair_device_async(self._h, ptrs, pres, nseg, frag, stream),
                    "dm_rs_repair_device_async")


def repair_plan(present: Sequence[bool], want: Optional[Sequence[bool]] = None,
                data_shards: int = DATA_SHARDS, parity_shards: int = PAR_SHARDS
                ) -> Tuple[List[int], List[int], List[List[int]]]:
    """``dm_rs_repair_plan`` (pure host function, no GPU): for one pattern the fragments read (the
    first ``data_shards`` present in index order), the fragments written -- every one that is
    wanted (default: all) and not present, data or parity -- and one coding row per output.
    Raises :class:`ErrTooFewShards`."""
    from ._lib import load_library
    L = load_library()
    k, t = data_shards, data_shards + parity_shards
    if len(present) != t or (want is not None and len(want) != t):
        raise DeossMerkleError(-2, "present and want need data + parity entries")
    ins, outs = (ctypes.c_int * k)(), (ctypes.c_int * parity_shards)()
    rows = ctypes.create_string_buffer(parity_shards * k)
    nout = ctypes.c_int()
    pres = bytes(int(bool(p)) for p in present)
    wnt = bytes(int(bool(p)) for p in want) if want is not None else None
    rc = L.dm_rs_repair_plan(k, parity_shards, pres, wnt, ins, outs, rows, ctypes.byref(nout))
    if rc != 0:
        detail = (L.dm_last_error(None) or b"").decode()
        if "too few shards" in detail:
            raise ErrTooFewShards(rc, detail)
        raise DeossMerkleError(rc, detail)
    n = nout.value
    return list(ins), list(outs[:n]), [list(rows.raw[i * k:(i + 1) * k]) for i in range(n)]


def restore_plan(present: Sequence[bool], in_place: Optional[Sequence[bool]] = None,
                 data_shards: int = DATA_SHARDS, parity_shards: int = PAR_SHARDS
                 ) -> Tuple[List[int], List[int], List[List[int]]]:
    """``dm_rs_restore_plan`` (pure host function, no GPU): for one erasure pattern the fragments
    read (the first ``data_shards`` present in index order), the data fragments written (missing
    or not ``in_place``) and one coding row per output.  Raises :class:`ErrTooFewShards`."""
    from ._lib import load_library
    L = load_library()
    k, t = data_shards, data_shards + parity_shards
    if len(present) != t or (in_place is not None and len(in_place) != k):
        raise DeossMerkleError(-2, "present needs data + parity entries, in_place data entries")
    ins, outs = (ctypes.c_int * k)(), (ctypes.c_int * k)()
    rows = ctypes.create_string_buffer(k * k)
    nout = ctypes.c_int()
    pres = bytes(int(bool(p)) for p in present)
    inp = bytes(int(bool(p)) for p in in_place) if in_place is not None else None
    rc = L.dm_rs_restore_plan(k, parity_shards, pres, inp, ins, outs, rows, ctypes.byref(nout))
    if rc != 0:
        detail = (L.dm_last_error(None) or b"").decode()
        if "too few shards" in detail:
            raise ErrTooFewShards(rc, detail)
        raise DeossMerkleError(rc, detail)
    n = nout.value
    return list(ins), list(outs[:n]), [list(rows.raw[i * k:(i + 1) * k]) for i in range(n)]


def New(ctx: MerkleContext, data_shards: int = DATA_SHARDS, parity_shards: int = PAR_SHARDS) -> Encoder:
    """reedsolomon.New(dataShards, parityShards) on the context's first GPU: up to 8 + 8 the fragment
    coder every path takes (``dm_rs_create``), beyond that the wide one (``dm_rs_create_wide``)."""
    return Encoder(ctx, data_shards, parity_shards, wide=data_shards > 8 or parity_shards > 8)
