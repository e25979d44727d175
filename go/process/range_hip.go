//go:build hip

// Ranged restore: the HTTP Range of GET /file/open (node/fileHandler.go:399-545).  On a cache miss
// the handler calls process.Retrievefile for the whole object (:519) and only then hands a byte
// range to ReturnFileRangeStream (node/common.go:410-466): a 1 MiB seek into an 8 GiB object pays
// for 8 GiB of fragments.  RangePlan says which data fragments of which segments a range needs (so
// only those are fetched from miners), RestoreRange gives the range's bytes from whichever of the
// object's fragments lie in fragDir: the needed ones are read and checked against their names, a
// lost one is rebuilt from any chain.DataShards others and must equal its name
// (include/deoss_merkle.h: dm_range_plan, dm_retrieve_range).  Segment names and the fid are not
// checked: they name whole segments, which a ranged restore never has.  The whole-object restore can
// run afterwards to fill the cache.  Downloads with cipher != "" stay with the SDK: the cipher scheme
// is recalled, not pinned (DESIGN.md §6.14).
package process

/*
#cgo pkg-config: deoss_merkle
#include <stdlib.h>
#include "deoss_merkle.h"
*/
import "C"

import (
	"errors"
	"runtime"
	"unsafe"

	"github.com/CESSProject/cess-go-sdk/chain"
)

// ErrRangeCipher: a ranged restore of an encrypted object is not served here; restore the whole
// object with the SDK's Retrievefile and cut the range from it, as the handler does today.
var ErrRangeCipher = errors.New("restore: a byte range of an encrypted object stays with the SDK (whole-object Retrievefile)")

// RangeNeed is what bytes [off, off+length) of an object need: Need[t][j] is true when data fragment
// j of segment Seg0+t holds bytes of the range.
type RangeNeed struct {
	Seg0 uint64
	Need [][]bool
}

// RangePlan is the host-only plan (no GPU is touched): size is the object's size in bytes.
func RangePlan(size, off, length int64) (RangeNeed, error) {
	var plan RangeNeed
	if size <= 0 || off < 0 || length <= 0 {
		return plan, errors.New("restore: empty or negative range")
	}
	seg := int64(chain.SegmentSize)
	nseg := (size + seg - 1) / seg
	var seg0, ntouched, nwin C.uint64_t
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	rc := C.dm_range_plan(C.uint64_t(size), C.uint64_t(nseg), C.uint64_t(chain.SegmentSize), C.int(chain.DataShards),
		C.int(0), C.uint64_t(off), C.uint64_t(length), C.int(0), &seg0, &ntouched, nil, C.uint64_t(0), nil,
		C.uint64_t(0), &nwin)
	if rc != C.DM_OK {
		return plan, restoreError(rc)
	}
	need := make([]byte, int(ntouched)*chain.DataShards)
	rc = C.dm_range_plan(C.uint64_t(size), C.uint64_t(nseg), C.uint64_t(chain.SegmentSize), C.int(chain.DataShards),
		C.int(0), C.uint64_t(off), C.uint64_t(length), C.int(0), &seg0, &ntouched, (*C.uint8_t)(unsafe.Pointer(&need[0])),
		C.uint64_t(len(need)), nil, C.uint64_t(0), &nwin)
	if rc != C.DM_OK {
		return plan, restoreError(rc)
	}
	plan.Seg0 = uint64(seg0)
	plan.Need = make([][]bool, int(ntouched))
	for t := range plan.Need {
		plan.Need[t] = make([]bool, chain.DataShards)
		for j := range plan.Need[t] {
			plan.Need[t][j] = need[t*chain.DataShards+j] != 0
		}
	}
	return plan, nil
}

// RestoreRange returns bytes [off, off+length) of the object of size bytes that segments describes
// (what FullProcessing returned, or the same names from the chain's file metadata), from whichever
// of its fragments lie in fragdir/<name>.  Only the fragments RangePlan names are read -- or, where
// one is missing or fails its name, the first chain.DataShards that exist of that segment.  No file
// is written.
func RestoreRange(fragdir string, segments []chain.SegmentDataInfo, size, off, length int64, cipher string) ([]byte, error) {
	if cipher != "" { // the scheme is unpinned: encrypted downloads stay with the SDK
		return nil, ErrRangeCipher
	}
	if err := gpu(); err != nil {
		return nil, err
	}
	if len(segments) == 0 {
		return nil, errors.New("Empty data")
	}
	if size <= 0 || off < 0 || length <= 0 {
		return nil, errors.New("restore: empty or negative range")
	}
	_, fragn, err := names(segments)
	if err != nil {
		return nil, err
	}
	out := make([]byte, length)
	rs := <-pipes
	defer func() { pipes <- rs }()
	cdir := C.CString(fragdir)
	defer C.free(unsafe.Pointer(cdir))
	var ok C.int
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	rc := C.dm_retrieve_range(rs, cdir, (*C.uint8_t)(unsafe.Pointer(&fragn[0])), C.uint64_t(len(segments)), C.uint64_t(size),
		C.uint64_t(chain.SegmentSize), C.uint64_t(off), C.uint64_t(length), C.int(C.DM_RESTORE_VERIFY_FRAGMENTS), nil,
		C.uint64_t(0), unsafe.Pointer(&out[0]), nil, nil, &ok)
	if rc != C.DM_OK {
		return nil, restoreError(rc)
	}
	if ok == 0 {
		return nil, ErrRestore
	}
	return out, nil
}
