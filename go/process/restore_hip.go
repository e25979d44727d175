//go:build hip

// Restore: the download side of the package.  cess-go-sdk process.Retrievefile(chainer, fmeta, fid,
// dir, cipher) (called at node/fileHandler.go:519, :600 and :990) fetches, per segment, any
// chain.DataShards of its fragments from miners, rebuilds the missing data fragments
// (erasure.RSRestore), joins the segments and cuts the zero padding off at the file size.  The SDK
// goes on fetching; RestoreFile / RestoreFragments replace the rest with one GPU pass that also
// checks every fragment it uses against its name (its SHA-256) -- falling back to another fragment
// when one fails -- and every rebuilt segment against the segment name (include/deoss_merkle.h:
// dm_retrieve_file, dm_restore_buffer).  Downloads with cipher != "" stay with the SDK.
package process

/*
#cgo pkg-config: deoss_merkle
#include <stdlib.h>
#include "deoss_merkle.h"
*/
import "C"

import (
	"encoding/hex"
	"errors"
	"fmt"
	"path/filepath"
	"runtime"
	"sync"
	"unsafe"

	"github.com/CESSProject/cess-go-sdk/chain"
)

// ErrRestore: the fragments at hand do not give the object back (too few verified fragments of
// some segment, or a rebuilt segment that is not the one its name promises).
var ErrRestore = errors.New("restore: too few verified fragments or a segment mismatch")

// names decodes the base names of FullProcessing's paths (hex SHA-256) into digests.
func names(segs []chain.SegmentDataInfo) (segn, fragn []byte, err error) {
	total := chain.DataShards + chain.ParShards
	segn = make([]byte, 0, 32*len(segs))
	fragn = make([]byte, 0, 32*len(segs)*total)
	for _, s := range segs {
		if len(s.FragmentHash) != total {
			return nil, nil, fmt.Errorf("restore: segment with %d fragment names, want %d", len(s.FragmentHash), total)
		}
		d, e := hex.DecodeString(filepath.Base(s.SegmentHash))
		if e != nil || len(d) != 32 {
			return nil, nil, errors.New("restore: segment name is not a hex SHA-256")
		}
		segn = append(segn, d...)
		for _, f := range s.FragmentHash {
			d, e := hex.DecodeString(filepath.Base(f))
			if e != nil || len(d) != 32 {
				return nil, nil, errors.New("restore: fragment name is not a hex SHA-256")
			}
			fragn = append(fragn, d...)
		}
	}
	return segn, fragn, nil
}

// restoreError must run on the OS thread that made the call (dm_last_error is thread-local).
func restoreError(rc C.int) error {
	if rc == C.DM_ERR_EMPTY {
		return errors.New("Empty data")
	}
	if msg := C.GoString(C.dm_last_error(nil)); msg != "" {
		return errors.New(msg)
	}
	return errors.New(C.GoString(C.dm_strerror(rc)))
}

// RestoreFile rebuilds the file of size bytes at outPath from whichever fragments of segs (what
// FullProcessing returned, or the same names taken from the chain's file metadata) lie in
// fragDir/<name>.  Per segment the first chain.DataShards fragment files that exist are read;
// further ones only when one fails its check.  outPath appears only when every segment held.
func RestoreFile(fragDir string, segs []chain.SegmentDataInfo, size uint64, outPath string) error {
	if err := gpu(); err != nil {
		return err
	}
	if len(segs) == 0 {
		return errors.New("Empty data")
	}
	segn, fragn, err := names(segs)
	if err != nil {
		return err
	}
	rs := <-pipes
	defer func() { pipes <- rs }()
	cdir, cout := C.CString(fragDir), C.CString(outPath)
	defer C.free(unsafe.Pointer(cdir))
	defer C.free(unsafe.Pointer(cout))
	var ok C.int
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	rc := C.dm_retrieve_file(rs, cdir, (*C.uint8_t)(unsafe.Pointer(&fragn[0])), (*C.uint8_t)(unsafe.Pointer(&segn[0])), nil,
		C.uint64_t(len(segs)), C.uint64_t(size), C.uint64_t(chain.SegmentSize),
		C.int(C.DM_RESTORE_VERIFY_FRAGMENTS|C.DM_RESTORE_VERIFY_SEGMENTS), cout, nil, nil, &ok)
	if rc != C.DM_OK {
		return restoreError(rc)
	}
	if ok == 0 {
		return ErrRestore
	}
	return nil
}

// restoreArgs is an in-memory restore as the C calls take it: the decoded names and the table of
// fragment pointers.  The table lives in C memory (cgo forbids Go pointers to Go pointers); the
// fragments themselves stay pinned until release.
type restoreArgs struct {
	segn, fragn []byte
	table       *[1 << 28]unsafe.Pointer
	pin         runtime.Pinner
}

func (a *restoreArgs) release() {
	a.pin.Unpin()
	C.free(unsafe.Pointer(a.table))
}

// restoreInputs checks frags[s][j] (fragment j of segment s, nil = not fetched) against segs and
// builds the arguments; the caller defers release() when err is nil.
func restoreInputs(frags [][][]byte, segs []chain.SegmentDataInfo, size uint64) (*restoreArgs, error) {
	total := chain.DataShards + chain.ParShards
	frag := int(chain.SegmentSize) / chain.DataShards
	if len(segs) == 0 || len(frags) != len(segs) || size == 0 {
		return nil, errors.New("Empty data")
	}
	segn, fragn, err := names(segs)
	if err != nil {
		return nil, err
	}
	n := len(segs) * total
	table := (*[1 << 28]unsafe.Pointer)(C.calloc(C.size_t(n), C.size_t(unsafe.Sizeof(uintptr(0)))))
	if table == nil {
		return nil, errors.New("restore: out of memory")
	}
	a := &restoreArgs{segn: segn, fragn: fragn, table: table}
	for s := range frags {
		if len(frags[s]) != total {
			a.release()
			return nil, fmt.Errorf("restore: segment %d has %d fragment slots, want %d", s, len(frags[s]), total)
		}
		for j, f := range frags[s] {
			if f == nil {
				continue
			}
			if len(f) != frag {
				a.release()
				return nil, fmt.Errorf("restore: fragment %d of segment %d has %d bytes, want %d", j, s, len(f), frag)
			}
			a.pin.Pin(&f[0])
			table[s*total+j] = unsafe.Pointer(&f[0])
		}
	}
	return a, nil
}

// RestoreFragments is RestoreFile for bytes already in memory: frags[s][j] is fragment j of segment
// s (data fragments first) or nil when it was not fetched.  Returns the file's size bytes.
func RestoreFragments(frags [][][]byte, segs []chain.SegmentDataInfo, size uint64) ([]byte, error) {
	if err := gpu(); err != nil {
		return nil, err
	}
	in, err := restoreInputs(frags, segs, size)
	if err != nil {
		return nil, err
	}
	defer in.release()
	out := make([]byte, size)
	rs := <-pipes
	defer func() { pipes <- rs }()
	var ok C.int
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	rc := C.dm_restore_buffer(rs, (*unsafe.Pointer)(unsafe.Pointer(in.table)), (*C.uint8_t)(unsafe.Pointer(&in.fragn[0])),
		(*C.uint8_t)(unsafe.Pointer(&in.segn[0])), nil, C.uint64_t(len(segs)), C.uint64_t(size),
		C.uint64_t(chain.SegmentSize), C.int(C.DM_RESTORE_VERIFY_FRAGMENTS|C.DM_RESTORE_VERIFY_SEGMENTS),
		unsafe.Pointer(&out[0]), nil, nil, &ok)
	if rc != C.DM_OK {
		return nil, restoreError(rc)
	}
	if ok == 0 {
		return nil, ErrRestore
	}
	return out, nil
}

var (
	restoreOnce    sync.Once
	restoreBatcher *C.dm_batcher // in-memory restores from every goroutine
	restoreInitErr error
)

// restoreQueue makes the process-wide DM_BATCH_RESTORE batcher on first use: every visible GPU, 4
// worker slots each, 2 ms linger, as the upload side's batcher (DESIGN.md §6.9, §6.13).
func restoreQueue() error {
	if err := gpu(); err != nil {
		return err
	}
	restoreOnce.Do(func() {
		runtime.LockOSThread()
		defer runtime.UnlockOSThread()
		if rc := C.dm_batcher_create(nil, 0, C.DM_BATCH_RESTORE, C.uint64_t(chain.SegmentSize), C.int(chain.DataShards),
			C.int(chain.ParShards), 0, 0, 0, 2000, &restoreBatcher); rc != C.DM_OK {
			restoreInitErr = errors.New(C.GoString(C.dm_batcher_last_error()))
		}
	})
	return restoreInitErr
}

// RestoreBuffers is RestoreFragments through the process-wide restore batcher: download handlers
// (GET /file/download, GET /file/open) run one goroutine per request, and whatever they have queued
// becomes ONE verified GPU pass (dm_batcher_restore -> dm_restore_batch): many small downloads
// share one pass (measured: DESIGN.md §6.13).  frags, segs and size as RestoreFragments; cipher == "" is a plain
// object, otherwise the object is decrypted on the GPU after its checks (the scheme is recalled,
// not pinned: DESIGN.md §6.14) and size counts plaintext bytes.  A request that fails its checks
// returns ErrRestore and changes nothing for the requests that shared its pass.
func RestoreBuffers(frags [][][]byte, segs []chain.SegmentDataInfo, size uint64, cipher string) ([]byte, error) {
	if err := restoreQueue(); err != nil {
		return nil, err
	}
	in, err := restoreInputs(frags, segs, size)
	if err != nil {
		return nil, err
	}
	defer in.release()
	var ckey unsafe.Pointer
	if cipher != "" {
		ckey = C.CBytes([]byte(cipher))
		defer C.free(ckey)
	}
	out := make([]byte, size)
	var ok C.int
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	rc := C.dm_batcher_restore(restoreBatcher, (*unsafe.Pointer)(unsafe.Pointer(in.table)), (*C.uint8_t)(unsafe.Pointer(&in.fragn[0])),
		(*C.uint8_t)(unsafe.Pointer(&in.segn[0])), nil, C.uint64_t(len(segs)), C.uint64_t(size),
		C.int(C.DM_RESTORE_VERIFY_FRAGMENTS|C.DM_RESTORE_VERIFY_SEGMENTS), ckey, C.uint64_t(len(cipher)),
		unsafe.Pointer(&out[0]), nil, nil, &ok)
	if rc != C.DM_OK {
		return nil, batcherError(rc)
	}
	if ok == 0 {
		return nil, ErrRestore
	}
	return out, nil
}
