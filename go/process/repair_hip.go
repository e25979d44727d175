//go:build hip

// Repair: the storage side of the package.  DeOSS's tracker (node/tracker.go:320-355,
// checkFileState) stats every fragment file of an upload and, when one is missing, calls
// reFullProcessing: the whole object is read again, processed again -- with the client's cipher,
// when it had one -- and all 12 fragments of every segment are rewritten.  None of that is needed
// to get a fragment back: any chain.DataShards of a segment's fragments determine the others,
// fragments are ciphertext already, and every fragment is named by its own SHA-256, so a rebuilt one
// proves itself.  RepairFragments makes the fragment directory whole again from the fragment files
// that are left (include/deoss_merkle.h: dm_repair_files); it needs neither the object nor the
// cipher, so it serves encrypted uploads too.
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

// ErrRepair: the fragments left do not give the missing ones back (too few verified fragments of
// some segment, or a rebuilt fragment that is not the one its name promises).  Whatever could be
// rebuilt has been; the caller falls back to reFullProcessing.
var ErrRepair = errors.New("repair: too few verified fragments or a fragment mismatch")

// RepairFragments rebuilds every fragment file of segs (what FullProcessing returned, or the same
// names from the chain's file metadata) that is missing from fragDir, or has the wrong length,
// from the other fragments of its segment.  Per segment that misses a file the first
// chain.DataShards files that exist are read and checked against their names; a segment with all its
// files is not read.  With scrub every existing file is read and checked too, and one that does not
// equal its name is replaced.  A rebuilt file appears under its name only after its SHA-256 matched.
// rebuilt counts the files written, also when err is ErrRepair.
func RepairFragments(fragDir string, segs []chain.SegmentDataInfo, scrub bool) (rebuilt int, err error) {
	if err := gpu(); err != nil {
		return 0, err
	}
	if len(segs) == 0 {
		return 0, errors.New("Empty data")
	}
	_, fragn, err := names(segs)
	if err != nil {
		return 0, err
	}
	rs := <-pipes
	defer func() { pipes <- rs }()
	cdir := C.CString(fragDir)
	defer C.free(unsafe.Pointer(cdir))
	flags := C.int(0)
	if scrub {
		flags = C.int(C.DM_REPAIR_SCRUB)
	}
	var ok C.int
	var n C.uint64_t
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	rc := C.dm_repair_files(rs, cdir, (*C.uint8_t)(unsafe.Pointer(&fragn[0])), C.uint64_t(len(segs)),
		C.uint64_t(chain.SegmentSize), flags, nil, nil, &n, &ok)
	if rc != C.DM_OK {
		return int(n), restoreError(rc)
	}
	if ok == 0 {
		return int(n), ErrRepair
	}
	return int(n), nil
}
