"""Python mirror of cess-go-sdk ``process.FullProcessing`` backed by the GPU pipeline (``dm_process_*``).

DeOSS computes every file id ("fid") and fragment name with
``process.FullProcessing(file, cipher, savedir) ([]chain.SegmentDataInfo, fid string, error)``
from cess-go-sdk (``go.mod:8``; not vendored): ``node/objectHandler.go:168``,
``node/fileHandler.go:771``, ``node/filesHandler.go:201``, ``node/resumeHandler.go:326``,
``node/tracker.go:767-769`` and the fragment download path ``node/fileHandler.go:964,997``.
:func:`FullProcessing` keeps that signature and result shape:

* the file is cut into ``SEGMENT_SIZE`` (chain.SegmentSize, 32 MiB) segments, the last one
  zero-padded;
* each segment becomes ``DATA_SHARDS + PAR_SHARDS`` fragments of ``FRAGMENT_SIZE`` (8 MiB) with
  the klauspost Reed-Solomon coder, written to ``savedir/<hex SHA-256 of the fragment>``;
* ``SegmentDataInfo.SegmentHash`` is ``savedir/<hex SHA-256 of the segment>`` and
  ``SegmentDataInfo.FragmentHash`` the fragment paths, data fragments first (the handlers open
  them by path and match ``filepath.Base`` against a requested hash, ``node/fileHandler.go:967-969``);
* the fid is the hex ``common/hashtree`` root over the segments.

Coding, hashing and the tree run on the GPU; there is no CPU fallback.  Segment files are written
too (the zero-padded segment = its data fragments in order), so every returned path exists.
:meth:`Processor.FullProcessing` is one ``dm_full_processing`` call: the library reads the file,
and fragment writes overlap the reads and the GPU's hashing.
With a non-empty ``cipher`` the object is AES-CBC encrypted on the GPU first (``dm_full_processing_cipher``,
the same one call) and everything is named by ciphertext; :meth:`Processor.RestoreFile` with the
same cipher gives the object back.  The scheme is recalled from the SDK, not pinned against it
(DESIGN.md §6.14): parity-unpinned, and the Go shim still routes a cipher to the SDK.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

from ._lib import DM_ERR_EMPTY, DM_ERR_INVALID, DM_ERR_IO, DeossMerkleError, RestoreObj, restore_obj_fields
from .merkle import RANGE_NO_PADDING_CHECK, MerkleContext, range_plan  # noqa: F401
from .reedsolomon import DATA_SHARDS, PAR_SHARDS, Encoder

SEGMENT_SIZE = 32 << 20                       # chain.SegmentSize
FRAGMENT_SIZE = SEGMENT_SIZE // DATA_SHARDS   # chain.FragmentSize (8 MiB; node/tracker.go:250 "96M")
RESTORE_VERIFY_FRAGMENTS, RESTORE_VERIFY_SEGMENTS, RESTORE_VERIFY_FID, RESTORE_VERIFY_ALL = 1, 2, 4, 7   # DM_RESTORE_*
REPAIR_SCRUB = 1                              # DM_REPAIR_SCRUB
FRAG_REBUILT = 4                              # frag_status of the repair calls: rebuilt, verified and delivered
CIPHER_BLOCK = 16                           # a piece of segment - 16 plaintext bytes + its PKCS#7 block = one segment
SEG_BAD_PADDING = 3                           # seg_status of dm_restore_cipher_buffer: what a wrong cipher looks like
WINDOW_SEGMENTS = 8                           # segments per GPU call (256 MiB of file + 768 MiB of fragments; the Go shim bounds the segments in flight by DEOSS_PROCESS_MEM_GIB)


def _cipher_bytes(cipher) -> bytes:
    """The key bytes of a cipher given as str (a Go string's bytes: UTF-8) or bytes."""
    return cipher.encode() if isinstance(cipher, str) else bytes(cipher or b"")


def _write_segments() -> bool:
    """Segment files are written unless DEOSS_SKIP_SEGMENT_FILES=1 (as in the Go shim: DeOSS itself
    only opens fragment paths, node/fileHandler.go:967-969)."""
    return os.environ.get("DEOSS_SKIP_SEGMENT_FILES") != "1"


@dataclass
class SegmentDataInfo:
    """chain.SegmentDataInfo: the segment's path name and its fragments' path names."""
    SegmentHash: str = ""
    FragmentHash: List[str] = field(default_factory=list)


@dataclass
class RestoreObject:
    """One object of :meth:`Processor.restore_batch`: ``restore_buffer``'s arguments and a cipher."""
    frags: list
    size: int
    frag_names: Optional[bytes] = None
    seg_names: Optional[bytes] = None
    fid: Optional[bytes] = None
    flags: int = RESTORE_VERIFY_ALL
    cipher: bytes = b""


class Processor:
    """One GPU pipeline (``dm_rs`` coder + context) for FullProcessing calls."""

    def __init__(self, ctx: Optional[MerkleContext] = None, data_shards: int = DATA_SHARDS,
                 parity_shards: int = PAR_SHARDS, segment: int = SEGMENT_SIZE):
        self.ctx = ctx or MerkleContext()
        self.enc = Encoder(self.ctx, data_shards, parity_shards)
        self.segment = segment
        self.k, self.m = data_shards, parity_shards
        self.frag = segment // data_shards

    def close(self) -> None:
        self.enc.close()

    def _check(self, rc: int, what: str) -> None:
        if rc == DM_ERR_EMPTY:
            raise DeossMerkleError(rc, "Empty data")
        self.enc._check(rc, what)

    # -- raw pipeline ----------------------------------------------------------------------------
    def process_buffer(self, buf, want_frags: bool = True, cipher=b"") -> Tuple[bytes, bytes, bytes, Optional[bytes]]:
        """One ``dm_process_buffer`` call: (segment digests, fragment digests, fid, fragments).  With
        a ``cipher`` (16, 24 or 32 bytes) one ``dm_process_cipher_buffer`` call: the same over the
        ceil(len / (segment - 16)) segments of ciphertext."""
        n = len(buf)
        key = _cipher_bytes(cipher)
        piece = self.segment - CIPHER_BLOCK if key else self.segment
        nseg = (n + piece - 1) // piece if n else 0
        total = self.k + self.m
        seg = ctypes.create_string_buffer(max(32 * nseg, 32))
        frag = ctypes.create_string_buffer(max(32 * nseg * total, 32))
        fid = ctypes.create_string_buffer(32)
        frags = ctypes.create_string_buffer(nseg * total * self.frag) if (want_frags and nseg) else None
        src = buf if isinstance(buf, ctypes.Array) else ctypes.create_string_buffer(bytes(buf), max(n, 1))
        L = self.ctx._L
        if key:
            self._check(L.dm_process_cipher_buffer(self.enc._h, src, n, self.segment, key, len(key), frags, seg,
                                                   frag, fid), "dm_process_cipher_buffer")
        else:
            self._check(L.dm_process_buffer(self.enc._h, src, n, self.segment, frags, seg, frag, fid),
                        "dm_process_buffer")
        return seg.raw[:32 * nseg], frag.raw[:32 * nseg * total], fid.raw, (frags.raw if frags is not None else None)

    def process_batch(self, bufs, want_frags: bool = False, ciphers=None):
        """``dm_process_batch``: many objects in one pass; list of (seg digests, frag digests, fid,
        fragments or None) per object.  With ``ciphers`` (one per object; empty or None = a plain
        object) ``dm_process_cipher_batch``: the encrypted objects' pieces are encrypted in one
        keyed launch, whatever the mix of keys, and every object is coded and named in the same pass."""
        n = len(bufs)
        if n == 0:
            return []
        if ciphers is not None and len(ciphers) != n:
            raise DeossMerkleError(DM_ERR_INVALID, "process_batch: one cipher per object")
        keys = [_cipher_bytes(c) for c in ciphers] if ciphers is not None else [b""] * n
        total = self.k + self.m
        srcs, segs, frs, fragss, nsegs = [], [], [], [], []
        ptrs = (ctypes.c_void_p * n)()
        lens = (ctypes.c_uint64 * n)()
        sp = (ctypes.c_void_p * n)()
        fp = (ctypes.c_void_p * n)()
        gp = (ctypes.c_void_p * n)()
        for i, b in enumerate(bufs):
            piece = self.segment - CIPHER_BLOCK if keys[i] else self.segment
            nseg = (len(b) + piece - 1) // piece
            nsegs.append(nseg)
            src = ctypes.create_string_buffer(bytes(b), max(len(b), 1))
            srcs.append(src)
            ptrs[i] = ctypes.addressof(src)
            lens[i] = len(b)
            segs.append(ctypes.create_string_buffer(max(32 * nseg, 32)))
            frs.append(ctypes.create_string_buffer(max(32 * nseg * total, 32)))
            sp[i] = ctypes.addressof(segs[-1])
            fp[i] = ctypes.addressof(frs[-1])
            if want_frags and nseg:
                fragss.append(ctypes.create_string_buffer(nseg * total * self.frag))
                gp[i] = ctypes.addressof(fragss[-1])
            else:
                fragss.append(None)
                gp[i] = None
        fids = ctypes.create_string_buffer(32 * n)
        if ciphers is None:
            self._check(self.ctx._L.dm_process_batch(self.enc._h, ptrs, lens, n, self.segment, gp, sp, fp, fids),
                        "dm_process_batch")
        else:
            kbufs = [ctypes.create_string_buffer(k, max(len(k), 1)) for k in keys]
            kp = (ctypes.c_void_p * n)(*[ctypes.addressof(k) for k in kbufs])
            kl = (ctypes.c_uint64 * n)(*[len(k) for k in keys])
            self._check(self.ctx._L.dm_process_cipher_batch(self.enc._h, ptrs, lens, kp, kl, n, self.segment, gp, sp,
                                                            fp, fids), "dm_process_cipher_batch")
        out = []
        for i in range(n):
            nseg = nsegs[i]
            out.append((segs[i].raw[:32 * nseg], frs[i].raw[:32 * nseg * total], fids.raw[32 * i:32 * i + 32],
                        fragss[i].raw if fragss[i] is not None else None))
        return out

    def process_device_async(self, obj_ptr: int, length: int, parity_ptr: int, seg_hash_ptr: int,
                             frag_hash_ptr: int, fid_ptr: int, stream: int = 0) -> None:
        """``dm_process_device_async``: object already in HBM (room for whole segments)."""
        self._check(self.ctx._L.dm_process_device_async(self.enc._h, obj_ptr, length, self.segment, parity_ptr,
                                                        seg_hash_ptr or None, frag_hash_ptr or None, fid_ptr,
                                                        stream), "dm_process_device_async")

    # -- FullProcessing ----------------------------------------------------------------------------
    def full_processing_file(self, file: str, savedir: str, segment_files: Optional[bool] = None, cipher=b""
                             ) -> Tuple[bytes, bytes, bytes]:
        """One ``dm_full_processing`` call: the library reads ``file``, writes every fragment (and
        segment) to ``savedir/<hex SHA-256>`` and returns (segment digests, fragment digests, fid).
        With a ``cipher`` (16, 24 or 32 bytes) one ``dm_full_processing_cipher`` call: the same over
        the ceil(size / (segment - 16)) segments of ciphertext."""
        L = self.ctx._L
        key = _cipher_bytes(cipher)
        piece = self.segment - CIPHER_BLOCK if key else self.segment
        if segment_files is None:
            segment_files = _write_segments()
        try:
            size = os.stat(file).st_size
        except OSError:
            size = 0
        cap = max(1, (size + piece - 1) // piece)
        total = self.k + self.m
        for _ in range(2):   # a FIFO / a file that grew: retry once with the count the library saw
            seg = ctypes.create_string_buffer(32 * cap)
            frag = ctypes.create_string_buffer(32 * cap * total)
            fid = ctypes.create_string_buffer(32)
            nseg = ctypes.c_uint64(0)
            rc = L.dm_full_processing_cipher(self.enc._h, os.fsencode(file), os.fsencode(savedir), self.segment,
                                             key, len(key), 1 if segment_files else 0, seg, frag, cap,
                                             ctypes.byref(nseg), fid)
            if rc == DM_ERR_INVALID and nseg.value > cap:
                cap = nseg.value
                continue
            if rc == DM_ERR_IO:   # file errors keep Go's text ("open <path>: no such file or directory")
                raise DeossMerkleError(rc, (L.dm_last_error(None) or b"").decode())
            self._check(rc, "dm_full_processing")
            n = nseg.value
            return seg.raw[:32 * n], frag.raw[:32 * n * total], fid.raw
        raise DeossMerkleError(DM_ERR_INVALID, "dm_full_processing: file size changed during the call")

    def fragment_lookup(self, file: str, fragment_hash: str, want_bytes: bool = True
                        ) -> Optional[Tuple[int, int, Optional[bytes]]]:
        """``dm_fragment_lookup``: the fragment of ``file`` named ``fragment_hash`` (hex SHA-256), as
        the download handler finds it (node/fileHandler.go:962-979) -- without writing any file.
        Returns (segment index, fragment index, fragment bytes or None), or None when no fragment of
        the file has that name."""
        L = self.ctx._L
        want = bytes.fromhex(fragment_hash)
        if len(want) != 32:
            raise ValueError("fragment hash must be 32 bytes of hex")
        out = ctypes.create_string_buffer(self.frag) if want_bytes else None
        found, seg_i, frag_i = ctypes.c_int(0), ctypes.c_uint64(0), ctypes.c_int(0)
        rc = L.dm_fragment_lookup(self.enc._h, os.fsencode(file), self.segment, want, out, self.frag if out else 0,
                                  ctypes.byref(found), ctypes.byref(seg_i), ctypes.byref(frag_i))
        if rc == DM_ERR_IO:
            raise DeossMerkleError(rc, (L.dm_last_error(None) or b"").decode())
        self._check(rc, "dm_fragment_lookup")
        if not found.value:
            return None
        return seg_i.value, frag_i.value, (out.raw if out is not None else None)

    # -- restore (the download side) ---------------------------------------------------------------
    def restore_buffer(self, frags, size: int, frag_names: Optional[bytes] = None,
                       seg_names: Optional[bytes] = None, fid: Optional[bytes] = None,
                       flags: int = RESTORE_VERIFY_ALL, out=None, cipher=b""
                       ) -> Tuple[bool, Optional[bytes], bytes, bytes]:
        """``dm_restore_buffer``: the object from fragments in memory.  ``frags``: nseg x (data +
        parity) fragments, flat or one list per segment, ``None`` = not downloaded.  Returns (ok,
        the object's ``size`` bytes or None, fragment statuses, segment statuses); a failed check is
        ``ok = False``, not an exception.  ``out``: a ctypes buffer of ``size`` bytes to fill instead
        (left untouched unless ok).  With a ``cipher`` (``dm_restore_cipher_buffer``) the names are
        of ciphertext, ``size`` is the plaintext size, and a segment whose padding block is bad after
        decryption -- a wrong cipher -- has status ``SEG_BAD_PADDING`` with ``ok = False``."""
        total = self.k + self.m
        key = _cipher_bytes(cipher)
        flat = [f for seg in frags for f in seg] if frags and isinstance(frags[0], (list, tuple)) else list(frags)
        if len(flat) % total:
            raise DeossMerkleError(DM_ERR_INVALID, "need data + parity entries per segment")
        nseg = len(flat) // total
        keep = [ctypes.create_string_buffer(bytes(f), len(f)) if f is not None else None for f in flat]
        for b in keep:
            if b is not None and len(b) != self.frag:
                raise DeossMerkleError(DM_ERR_INVALID, "fragment sizes do not match")
        ptrs = (ctypes.c_void_p * max(len(flat), 1))(*[ctypes.addressof(b) if b is not None else None for b in keep])
        dst = out if out is not None else ctypes.create_string_buffer(max(size, 1))
        fst = ctypes.create_string_buffer(max(nseg * total, 1))
        sst = ctypes.create_string_buffer(max(nseg, 1))
        ok = ctypes.c_int(0)
        if key:
            self._check(self.ctx._L.dm_restore_cipher_buffer(self.enc._h, ptrs, frag_names, seg_names, fid, nseg, size,
                                                             self.segment, flags, key, len(key), dst, fst, sst,
                                                             ctypes.byref(ok)), "dm_restore_cipher_buffer")
        else:
            self._check(self.ctx._L.dm_restore_buffer(self.enc._h, ptrs, frag_names, seg_names, fid, nseg, size,
                                                      self.segment, flags, dst, fst, sst, ctypes.byref(ok)),
                        "dm_restore_buffer")
        data = dst.raw[:size] if (ok.value and out is None) else None
        return bool(ok.value), data, fst.raw[:nseg * total], sst.raw[:nseg]

    def restore_batch(self, objects) -> List[Tuple[bool, Optional[bytes], bytes, bytes]]:
        """``dm_restore_batch``: many objects restored and verified in one pass.  ``objects``:
        :class:`RestoreObject` items or dicts with ``restore_buffer``'s arguments (``frags``, ``size``,
        ``frag_names``, ``seg_names``, ``fid``, ``flags``) and a ``cipher`` each.  Returns one (ok,
        data or None, fragment statuses, segment statuses) per object, each what ``restore_buffer``
        gives for that object alone; an argument error raises, naming the object."""
        objs = [RestoreObject(**o) if isinstance(o, dict) else o for o in objects]
        n = len(objs)
        if n == 0:
            return []
        total = self.k + self.m
        arr = (RestoreObj * n)()
        parts = []
        for i, o in enumerate(objs):
            f = restore_obj_fields(o.frags, o.size, o.frag_names, o.seg_names, o.fid, o.flags, _cipher_bytes(o.cipher),
                                    total, self.frag)
            arr[i] = f[0]
            parts.append(f)
        ok = (ctypes.c_int * n)()
        self._check(self.ctx._L.dm_restore_batch(self.enc._h, arr, n, self.segment, ok), "dm_restore_batch")
        res = []
        for i, (_o, nseg, out, fst, sst, _keep) in enumerate(parts):
            res.append((bool(ok[i]), out.raw[:objs[i].size] if ok[i] else None, fst.raw[:nseg * total], sst.raw[:nseg]))
        return res

    def retrieve_file(self, fragdir: str, frag_names: bytes, size: int, out_path: str,
                      seg_names: Optional[bytes] = None, fid: Optional[bytes] = None,
                      flags: int = RESTORE_VERIFY_ALL) -> Tuple[bool, bytes, bytes]:
        """``dm_retrieve_file``: the object from the fragment files ``fragdir/<hex name>`` into
        ``out_path`` (written only when everything asked for held).  Returns (ok, fragment statuses,
        segment statuses)."""
        total = self.k + self.m
        nseg = len(frag_names) // (32 * total)
        fst = ctypes.create_string_buffer(max(nseg * total, 1))
        sst = ctypes.create_string_buffer(max(nseg, 1))
        ok = ctypes.c_int(0)
        L = self.ctx._L
        rc = L.dm_retrieve_file(self.enc._h, os.fsencode(fragdir), frag_names, seg_names, fid, nseg, size,
                                self.segment, flags, os.fsencode(out_path), fst, sst, ctypes.byref(ok))
        if rc == DM_ERR_IO:   # file errors keep Go's text
            raise DeossMerkleError(rc, (L.dm_last_error(None) or b"").decode())
        self._check(rc, "dm_retrieve_file")
        return bool(ok.value), fst.raw[:nseg * total], sst.raw[:nseg]

    def _restore_file_cipher(self, fragdir: str, fragn: bytes, segn: bytes, size: int, out_path: str, key: bytes
                             ) -> Tuple[bool, bytes, bytes]:
        """RestoreFile with a cipher: the fragment files that exist (of the right length) are read
        into memory and restored by one ``dm_restore_cipher_buffer`` call; ``out_path`` is written
        under a temporary name and renamed only when everything held."""
        frags = []
        for i in range(len(fragn) // 32):
            p = os.path.join(fragdir, fragn[32 * i:32 * i + 32].hex())
            try:
                data = open(p, "rb").read() if os.path.getsize(p) == self.frag else None
            except FileNotFoundError:
                data = None
            frags.append(data)
        ok, data, fst, sst = self.restore_buffer(frags, size, frag_names=fragn, seg_names=segn, cipher=key,
                                                 flags=RESTORE_VERIFY_FRAGMENTS | RESTORE_VERIFY_SEGMENTS)
        if ok:
            tmp = os.path.join(os.path.dirname(out_path), ".dm-rt-%d-%s" % (os.getpid(), os.path.basename(out_path)))
            try:
                with open(tmp, "wb") as f:
                    f.write(data)
                os.replace(tmp, out_path)
            except OSError:
                if os.path.exists(tmp):
                    os.unlink(tmp)
                raise
        return ok, fst, sst

    def RestoreFile(self, fragdir: str, segments: List[SegmentDataInfo], size: int, out_path: str, cipher=""
                    ) -> Tuple[bool, Optional[Exception]]:
        """The RSRestore / join / truncate part of process.Retrievefile: ``segments`` is what
        FullProcessing returned (names = base names of its paths), the fragments are whichever of
        them lie in ``fragdir``.  Every fragment used and every restored segment is checked against
        its name.  With the ``cipher`` the object was processed with, the segments are decrypted
        after that and ``size`` is the plaintext size.  (True, None), or (False, error)."""
        total = self.k + self.m
        key = _cipher_bytes(cipher)
        try:
            segn = b"".join(bytes.fromhex(os.path.basename(s.SegmentHash)) for s in segments)
            fragn = b"".join(bytes.fromhex(os.path.basename(f)) for s in segments for f in s.FragmentHash)
            if len(segn) != 32 * len(segments) or len(fragn) != 32 * total * len(segments):
                raise ValueError("segment and fragment names must be hex SHA-256")
            if key:
                ok, fst, sst = self._restore_file_cipher(fragdir, fragn, segn, size, out_path, key)
            else:
                ok, fst, sst = self.retrieve_file(fragdir, fragn, size, out_path, seg_names=segn,
                                                  flags=RESTORE_VERIFY_FRAGMENTS | RESTORE_VERIFY_SEGMENTS)
        except (OSError, ValueError, DeossMerkleError) as e:
            return False, e
        if not ok and any(st == SEG_BAD_PADDING for st in sst):
            return False, DeossMerkleError(DM_ERR_INVALID, "restore failed: bad padding after decryption "
                                           "(wrong cipher?)")
        if not ok:
            bad = [s for s in range(len(sst)) if sst[s]]
            return False, DeossMerkleError(DM_ERR_INVALID, "restore failed: segment(s) %s could not be rebuilt "
                                           "from verified fragments" % ", ".join(map(str, bad)))
        return True, None

    # -- ranged restore (the HTTP Range of GET /file/open) -------------------------------------------
    def _nseg_of(self, size: int, key: bytes) -> int:
        piece = self.segment - CIPHER_BLOCK if key else self.segment
        return (size + piece - 1) // piece

    def range_plan(self, size: int, off: int, length: int, cipher=b"", padding_check: bool = True):
        """``dm_range_plan`` for this pipeline's shape: (seg0, ntouched, need, windows) of bytes
        [off, off + length) -- what a gateway fetches before :meth:`restore_range`."""
        key = _cipher_bytes(cipher)
        return range_plan(size, self._nseg_of(size, key), self.segment, self.k, off, length, bool(key),
                          0 if padding_check else RANGE_NO_PADDING_CHECK)

    def restore_range(self, frags, size: int, off: int, length: int, frag_names: Optional[bytes] = None,
                      cipher=b"", padding_check: bool = True, flags: int = RESTORE_VERIFY_FRAGMENTS, out=None
                      ) -> Tuple[bool, Optional[bytes], bytes, bytes]:
        """``dm_restore_range_buffer``: bytes [off, off + length) of the object from just the fragments
        that cover them.  ``frags`` and ``frag_names`` are shaped as :meth:`restore_buffer`'s, over
        the whole object; fragments outside :meth:`range_plan`'s ``need`` may be ``None`` and are never
        looked at unless a needed one is missing or bad.  Segment names and the fid are not checked
        (they name whole segments).  Returns (ok, the bytes or None, fragment statuses, segment
        statuses); with a ``cipher`` the first touched segment's padding block is checked too unless
        ``padding_check`` is off (a wrong cipher: ``SEG_BAD_PADDING``, ``ok = False``)."""
        total = self.k + self.m
        key = _cipher_bytes(cipher)
        flat = [f for seg in frags for f in seg] if frags and isinstance(frags[0], (list, tuple)) else list(frags)
        if len(flat) % total:
            raise DeossMerkleError(DM_ERR_INVALID, "need data + parity entries per segment")
        nseg = len(flat) // total
        keep = [ctypes.create_string_buffer(bytes(f), len(f)) if f is not None else None for f in flat]
        for b in keep:
            if b is not None and len(b) != self.frag:
                raise DeossMerkleError(DM_ERR_INVALID, "fragment sizes do not match")
        ptrs = (ctypes.c_void_p * max(len(flat), 1))(*[ctypes.addressof(b) if b is not None else None for b in keep])
        dst = out if out is not None else ctypes.create_string_buffer(max(length, 1))
        fst = ctypes.create_string_buffer(max(nseg * total, 1))
        sst = ctypes.create_string_buffer(max(nseg, 1))
        ok = ctypes.c_int(0)
        if not padding_check:
            flags |= RANGE_NO_PADDING_CHECK
        self._check(self.ctx._L.dm_restore_range_buffer(self.enc._h, ptrs, frag_names, nseg, size, self.segment, off,
                                                        length, flags, key or None, len(key), dst, fst, sst,
                                                        ctypes.byref(ok)), "dm_restore_range_buffer")
        data = dst.raw[:length] if (ok.value and out is None) else None
        return bool(ok.value), data, fst.raw[:nseg * total], sst.raw[:nseg]

    def retrieve_range(self, fragdir: str, frag_names: bytes, size: int, off: int, length: int, cipher=b"",
                       padding_check: bool = True, flags: int = RESTORE_VERIFY_FRAGMENTS, out=None
                       ) -> Tuple[bool, Optional[bytes], bytes, bytes]:
        """``dm_retrieve_range``: the same from the fragment files ``fragdir/<hex name>``; no file is
        written.  Returns as :meth:`restore_range`."""
        total = self.k + self.m
        key = _cipher_bytes(cipher)
        nseg = len(frag_names) // (32 * total)
        dst = out if out is not None else ctypes.create_string_buffer(max(length, 1))
        fst = ctypes.create_string_buffer(max(nseg * total, 1))
        sst = ctypes.create_string_buffer(max(nseg, 1))
        ok = ctypes.c_int(0)
        if not padding_check:
            flags |= RANGE_NO_PADDING_CHECK
        L = self.ctx._L
        rc = L.dm_retrieve_range(self.enc._h, os.fsencode(fragdir), frag_names, nseg, size, self.segment, off, length,
                                 flags, key or None, len(key), dst, fst, sst, ctypes.byref(ok))
        if rc == DM_ERR_IO:   # file errors keep Go's text
            raise DeossMerkleError(rc, (L.dm_last_error(None) or b"").decode())
        self._check(rc, "dm_retrieve_range")
        data = dst.raw[:length] if (ok.value and out is None) else None
        return bool(ok.value), data, fst.raw[:nseg * total], sst.raw[:nseg]

    def RestoreRange(self, fragdir: str, segments: List[SegmentDataInfo], size: int, off: int, length: int, cipher=""
                     ) -> Tuple[Optional[bytes], Optional[Exception]]:
        """Bytes [off, off + length) of the object ``segments`` describes (what FullProcessing
        returned) from whichever of its fragments lie in ``fragdir``: only the fragments the range
        needs are read, each checked against its name, a lost one rebuilt and checked.  (bytes, None),
        or (None, error)."""
        total = self.k + self.m
        try:
            fragn = b"".join(bytes.fromhex(os.path.basename(f)) for s in segments for f in s.FragmentHash)
            if len(fragn) != 32 * total * len(segments):
                raise ValueError("fragment names must be hex SHA-256")
            ok, data, fst, sst = self.retrieve_range(fragdir, fragn, size, off, length, cipher=cipher)
        except (OSError, ValueError, DeossMerkleError) as e:
            return None, e
        if not ok and any(st == SEG_BAD_PADDING for st in sst):
            return None, DeossMerkleError(DM_ERR_INVALID, "restore failed: bad padding after decryption "
                                          "(wrong cipher?)")
        if not ok:
            bad = [s for s in range(len(sst)) if sst[s]]
            return None, DeossMerkleError(DM_ERR_INVALID, "restore failed: segment(s) %s could not be rebuilt "
                                          "from verified fragments" % ", ".join(map(str, bad)))
        return data, None

    # -- repair (the storage side) -------------------------------------------------------------------
    def repair_buffer(self, frags, frag_names: bytes, want=None, out=None
                      ) -> Tuple[bool, List[Optional[bytes]], bytes, bytes]:
        """``dm_repair_buffer``: the missing fragments of every segment from the ones given.
        ``frags``: nseg x (data + parity) fragments, flat or one list per segment, ``None`` =
        missing.  ``want`` (same shape, truthy = wanted; default: every missing fragment): a wanted
        fragment that is given is checked against its name and rebuilt if it fails.  Returns (ok,
        per fragment the rebuilt bytes or None, fragment statuses, segment statuses); a rebuilt
        fragment is returned only when its SHA-256 equals its name.  ``out``: one ctypes buffer of a
        fragment's size per fragment (flat) to receive the wanted ones instead; the library leaves
        the buffer of a fragment it does not deliver untouched."""
        total = self.k + self.m
        flat = [f for seg in frags for f in seg] if frags and isinstance(frags[0], (list, tuple)) else list(frags)
        if len(flat) % total:
            raise DeossMerkleError(DM_ERR_INVALID, "need data + parity entries per segment")
        if want is None:
            wflat = [f is None for f in flat]
        else:
            wflat = [w for seg in want for w in seg] if want and isinstance(want[0], (list, tuple)) else list(want)
        if len(wflat) != len(flat):
            raise DeossMerkleError(DM_ERR_INVALID, "want needs one entry per fragment")
        nseg = len(flat) // total
        keep = [ctypes.create_string_buffer(bytes(f), len(f)) if f is not None else None for f in flat]
        for b in keep:
            if b is not None and len(b) != self.frag:
                raise DeossMerkleError(DM_ERR_INVALID, "fragment sizes do not match")
        if out is not None:
            outs = [o if w else None for o, w in zip(out, wflat)]
        else:
            outs = [ctypes.create_string_buffer(self.frag) if w else None for w in wflat]
        n = max(len(flat), 1)
        ptrs = (ctypes.c_void_p * n)(*[ctypes.addressof(b) if b is not None else None for b in keep])
        optrs = (ctypes.c_void_p * n)(*[ctypes.addressof(b) if b is not None else None for b in outs])
        fst = ctypes.create_string_buffer(max(nseg * total, 1))
        sst = ctypes.create_string_buffer(max(nseg, 1))
        ok = ctypes.c_int(0)
        self._check(self.ctx._L.dm_repair_buffer(self.enc._h, ptrs, optrs, frag_names, nseg, self.segment, fst, sst,
                                                 ctypes.byref(ok)), "dm_repair_buffer")
        st = fst.raw[:nseg * total]
        got = [o.raw if (o is not None and st[i] == 4) else None for i, o in enumerate(outs)]
        return bool(ok.value), got, st, sst.raw[:nseg]

    def repair_files(self, fragdir: str, frag_names: bytes, scrub: bool = False) -> Tuple[bool, int, bytes, bytes]:
        """``dm_repair_files``: make the fragment directory ``fragdir/<hex name>`` whole again.  A
        file that is missing or has the wrong length is rebuilt from its segment's other fragments;
        with ``scrub`` every existing file is read and checked too and a bad one is replaced.
        Returns (ok, files rebuilt, fragment statuses, segment statuses)."""
        total = self.k + self.m
        nseg = len(frag_names) // (32 * total)
        fst = ctypes.create_string_buffer(max(nseg * total, 1))
        sst = ctypes.create_string_buffer(max(nseg, 1))
        ok, nre = ctypes.c_int(0), ctypes.c_uint64(0)
        L = self.ctx._L
        rc = L.dm_repair_files(self.enc._h, os.fsencode(fragdir), frag_names, nseg, self.segment,
                               REPAIR_SCRUB if scrub else 0, fst, sst, ctypes.byref(nre), ctypes.byref(ok))
        if rc == DM_ERR_IO:   # file errors keep Go's text
            raise DeossMerkleError(rc, (L.dm_last_error(None) or b"").decode())
        self._check(rc, "dm_repair_files")
        return bool(ok.value), nre.value, fst.raw[:nseg * total], sst.raw[:nseg]

    def RepairFragments(self, fragdir: str, segments: List[SegmentDataInfo], scrub: bool = False
                        ) -> Tuple[int, Optional[Exception]]:
        """process.RepairFragments (go/process/repair_hip.go): ``segments`` is what FullProcessing
        returned; every fragment file of theirs that is missing from ``fragdir`` (with ``scrub``:
        or does not equal its name) is rebuilt from the segment's other fragments.  Needs neither
        the object nor the cipher.  (files rebuilt, None), or (files rebuilt, error) when some
        segment has too few good fragments left."""
        total = self.k + self.m
        try:
            fragn = b"".join(bytes.fromhex(os.path.basename(f)) for s in segments for f in s.FragmentHash)
            if len(fragn) != 32 * total * len(segments):
                raise ValueError("fragment names must be hex SHA-256")
            ok, n, _, sst = self.repair_files(fragdir, fragn, scrub)
        except (OSError, ValueError, DeossMerkleError) as e:
            return 0, e
        if not ok:
            bad = [s for s in range(len(sst)) if sst[s]]
            return n, DeossMerkleError(DM_ERR_INVALID, "repair failed: segment(s) %s could not be rebuilt from "
                                       "verified fragments" % ", ".join(map(str, bad)))
        return n, None

    def FullProcessing(self, file: str, cipher: str, savedir: str
                       ) -> Tuple[Optional[List[SegmentDataInfo]], str, Optional[Exception]]:
        """FullProcessing in one library call (``dm_full_processing``: reads, coding, hashing and
        fragment writes overlapped; with a cipher ``dm_full_processing_cipher``, the same windows
        over AES-CBC ciphertext, every file written by the library)."""
        try:
            segd, fragd, fid = self.full_processing_file(file, savedir, cipher=cipher)
        except (OSError, DeossMerkleError) as e:
            return None, "", e
        total = self.k + self.m
        info = []
        for s in range(len(segd) // 32):
            names = [os.path.join(savedir, fragd[32 * (s * total + j):32 * (s * total + j + 1)].hex())
                     for j in range(total)]
            info.append(SegmentDataInfo(os.path.join(savedir, segd[32 * s:32 * s + 32].hex()), names))
        return info, fid.hex(), None

    def NewProcessingStream(self, savedir: str, segment_files: Optional[bool] = None) -> "ProcessingStream":
        """FullProcessing while the body arrives: write() the pieces, close() -> (info, fid)."""
        return ProcessingStream(self, savedir, segment_files)

    def FullProcessingWindows(self, file: str, cipher: str, savedir: str
                              ) -> Tuple[Optional[List[SegmentDataInfo]], str, Optional[Exception]]:
        """The window path (the Go shim's shape before dm_full_processing): read a window of
        ``WINDOW_SEGMENTS`` segments, one ``dm_process_buffer`` call, write its fragments, repeat.
        Kept as the A/B baseline of ``bench.py --workload fullprocessing``.  With a cipher a window
        is ``WINDOW_SEGMENTS`` pieces of ``segment - 16`` plaintext bytes (segments are independent
        CBC chains, so windows carry no state) and the fid is the tree over all segment digests."""
        key = _cipher_bytes(cipher)
        try:
            size = os.path.getsize(file)
        except OSError as e:
            return None, "", e
        if size == 0:
            return None, "", DeossMerkleError(-1, "Empty data")
        os.makedirs(savedir, exist_ok=True)
        info: List[SegmentDataInfo] = []
        seg_digests = []
        window = WINDOW_SEGMENTS * (self.segment - CIPHER_BLOCK if key else self.segment)
        total = self.k + self.m
        try:
            with open(file, "rb") as f:
                while True:
                    buf = f.read(window)
                    if not buf:
                        break
                    segd, fragd, fid, frags = self.process_buffer(buf, want_frags=True, cipher=key)
                    for s in range(len(segd) // 32):
                        seg_digests.append(segd[32 * s:32 * s + 32])
                        names = []
                        for j in range(total):
                            t = s * total + j
                            path = os.path.join(savedir, fragd[32 * t:32 * t + 32].hex())
                            if not os.path.exists(path):
                                with open(path, "wb") as out:
                                    out.write(frags[t * self.frag:(t + 1) * self.frag])
                            names.append(path)
                        seg_path = os.path.join(savedir, segd[32 * s:32 * s + 32].hex())
                        if not os.path.exists(seg_path):   # data fragments in order = the padded segment
                            with open(seg_path, "wb") as out:
                                out.write(frags[s * total * self.frag:(s * total + self.k) * self.frag])
                        info.append(SegmentDataInfo(seg_path, names))
                    if len(buf) < window:
                        break
        except (OSError, DeossMerkleError) as e:
            return None, "", e
        if len(seg_digests) > WINDOW_SEGMENTS:   # several windows: tree over all segments
            fid = self.ctx.tree_root(b"".join(seg_digests))
        return info, fid.hex(), None


class ProcessingStream:
    """FullProcessing while the upload body arrives (``dm_pstream_*``): ``write()`` pieces of any
    size beside the handler's own file write, ``close()`` -> (SegmentDataInfo list, hex fid) with
    every fragment and segment file in ``savedir`` -- the same results as
    ``FullProcessing(file, "", savedir)`` on the same bytes, without reading the file again."""

    def __init__(self, proc: "Processor", savedir: str, segment_files: Optional[bool] = None):
        self._p = proc
        self._L = proc.ctx._L
        self.savedir = savedir
        self.written = 0
        self.device_bytes = self.peak_device_bytes = 0
        h = ctypes.c_void_p()
        if segment_files is None:
            segment_files = _write_segments()
        rc = self._L.dm_pstream_open(proc.enc._h, proc.segment, os.fsencode(savedir), 1 if segment_files else 0,
                                     ctypes.byref(h))
        self._raise(rc, "dm_pstream_open")
        self._h = h

    def _raise(self, rc: int, what: str) -> None:
        if rc == 0:
            return
        detail = (self._L.dm_last_error(None) or b"").decode()
        if rc == DM_ERR_EMPTY:
            raise DeossMerkleError(rc, "Empty data")
        if rc == DM_ERR_IO:
            raise DeossMerkleError(rc, detail)
        raise DeossMerkleError(rc, f"{what}: {self._L.dm_strerror(rc).decode()}: {detail}")

    def write(self, data) -> int:
        """One piece: bytes-like, or (address, length) of host memory."""
        if self._h is None:
            raise DeossMerkleError(DM_ERR_INVALID, "stream is closed")
        if isinstance(data, tuple):
            addr, n = data
            ptr = ctypes.c_void_p(addr)
        elif isinstance(data, bytes):
            n, ptr = len(data), ctypes.c_char_p(data)   # no copy
        else:
            mv = memoryview(data).cast("B")
            n = mv.nbytes
            ptr = ctypes.c_char_p(mv.tobytes()) if (mv.readonly or n == 0) else (ctypes.c_char * n).from_buffer(mv)
        rc = self._L.dm_pstream_write(self._h, ptr, n)
        if rc != 0:
            self.abort()
            self._raise(rc, "dm_pstream_write")
        self.written += n
        return n

    def close(self) -> Tuple[List[SegmentDataInfo], str]:
        if self._h is None:
            raise DeossMerkleError(DM_ERR_INVALID, "stream is closed")
        p = self._p
        total = p.k + p.m
        cap = max(1, (self.written + p.segment - 1) // p.segment)
        seg = ctypes.create_string_buffer(32 * cap)
        frag = ctypes.create_string_buffer(32 * cap * total)
        fid = ctypes.create_string_buffer(32)
        nseg = ctypes.c_uint64(0)
        self.device_bytes, self.peak_device_bytes = self.stats()
        h, self._h = self._h, None
        self._raise(self._L.dm_pstream_close(h, seg, frag, cap, ctypes.byref(nseg), fid), "dm_pstream_close")
        n = nseg.value
        info = []
        for s in range(n):
            names = [os.path.join(self.savedir, frag.raw[32 * (s * total + j):32 * (s * total + j + 1)].hex())
                     for j in range(total)]
            info.append(SegmentDataInfo(os.path.join(self.savedir, seg.raw[32 * s:32 * s + 32].hex()), names))
        self.segment_digests = seg.raw[:32 * n]
        self.fragment_digests = frag.raw[:32 * n * total]
        return info, fid.raw.hex()

    def stats(self) -> Tuple[int, int]:
        """(device bytes the stream holds now, the most it has held): chunk buffers in use or spare,
        bounded by DEOSS_PS_DEVICE_CAP (default 16 GiB), not by the body size."""
        if self._h is None:
            return self.device_bytes, self.peak_device_bytes
        cur, peak = ctypes.c_uint64(), ctypes.c_uint64()
        self._raise(self._L.dm_pstream_stats(self._h, ctypes.byref(cur), ctypes.byref(peak)), "dm_pstream_stats")
        return cur.value, peak.value

    def abort(self) -> None:
        if self._h is not None:
            self._L.dm_pstream_abort(self._h)
            self._h = None

    def __del__(self):
        try:
            self.abort()
        except Exception:
            pass


_default: Optional[Processor] = None


def FullProcessing(file: str, cipher: str, savedir: str
                   ) -> Tuple[Optional[List[SegmentDataInfo]], str, Optional[Exception]]:
    """process.FullProcessing(file, cipher, savedir) on the default GPU pipeline."""
    global _default
    if _default is None:
        try:
            _default = Processor()
        except DeossMerkleError as e:   # no GPU: the Go shape (nil, "", err), as gpu() fails in Go
            return None, "", e
    return _default.FullProcessing(file, cipher, savedir)


def RestoreFile(fragdir: str, segments: List[SegmentDataInfo], size: int, out_path: str, cipher=""
                ) -> Tuple[bool, Optional[Exception]]:
    """The restore part of process.Retrievefile on the default GPU pipeline (Processor.RestoreFile)."""
    global _default
    if _default is None:
        try:
            _default = Processor()
        except DeossMerkleError as e:   # no GPU: fails the Go way, as FullProcessing
            return False, e
    return _default.RestoreFile(fragdir, segments, size, out_path, cipher)


def RestoreRange(fragdir: str, segments: List[SegmentDataInfo], size: int, off: int, length: int, cipher=""
                 ) -> Tuple[Optional[bytes], Optional[Exception]]:
    """A byte range of an object on the default GPU pipeline (Processor.RestoreRange)."""
    global _default
    if _default is None:
        try:
            _default = Processor()
        except DeossMerkleError as e:   # no GPU: fails the Go way, as FullProcessing
            return None, e
    return _default.RestoreRange(fragdir, segments, size, off, length, cipher)


def RepairFragments(fragdir: str, segments: List[SegmentDataInfo], scrub: bool = False
                    ) -> Tuple[int, Optional[Exception]]:
    """process.RepairFragments on the default GPU pipeline (Processor.RepairFragments)."""
    global _default
    if _default is None:
        try:
            _default = Processor()
        except DeossMerkleError as e:   # no GPU: fails the Go way, as FullProcessing
            return 0, e
    return _default.RepairFragments(fragdir, segments, scrub)


def FindFragment(fpath: str, fragment_hash: str) -> Tuple[Optional[bytes], Optional[Exception]]:
    """process.FindFragment (go/process/process_hip.go) on the default GPU pipeline: the fragment
    of ``fpath`` named ``fragment_hash``, or (None, None) when the file has no such fragment."""
    global _default
    # file names are lower-case hex SHA-256 (node/fileHandler.go:968): any other spelling names no
    # fragment, as the handler's string comparison would find none
    try:
        ok = len(fragment_hash) == 64 and bytes.fromhex(fragment_hash).hex() == fragment_hash
    except ValueError:
        ok = False
    if not ok:
        return None, None
    try:
        if _default is None:
            _default = Processor()
        hit = _default.fragment_lookup(fpath, fragment_hash)
    except (DeossMerkleError, ValueError) as e:
        return None, e
    return (hit[2] if hit else None), None


def FullProcessingFiles(files: List[str], cipher: str, savedir: str
                        ) -> Tuple[List[Optional[List[SegmentDataInfo]]], List[str], List[Optional[Exception]]]:
    """process.FullProcessingFiles (go/process/process_hip.go; the batch upload PUT /files,
    node/filesHandler.go:197-207): every file's FullProcessing at once, results in file order; an
    empty path is skipped (None, "", None)."""
    from concurrent.futures import ThreadPoolExecutor
    n = len(files)
    infos: List[Optional[List[SegmentDataInfo]]] = [None] * n
    fids, errs = [""] * n, [None] * n

    def one(i):
        infos[i], fids[i], errs[i] = FullProcessing(files[i], cipher, savedir)

    global _default
    todo = [i for i in range(n) if files[i]]
    if todo and _default is None:   # the default pipeline, made once before the calls start
        try:
            _default = Processor()
        except DeossMerkleError as e:   # no GPU: every call fails the Go way
            return [None] * n, [""] * n, [e if files[i] else None for i in range(n)]
    with ThreadPoolExecutor(max(1, min(16, len(todo)))) as ex:
        list(ex.map(one, todo))
    return infos, fids, errs
