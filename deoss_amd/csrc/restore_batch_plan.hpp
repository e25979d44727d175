// restore_batch_plan.hpp -- what a batched restore decides before it touches the GPU; plain
// C++17, no HIP.
//
// dm_restore_batch (restore_capi.inl) restores many objects, each with its own fragments, names,
// flags and cipher, in one pass.  Everything of that pass that is arithmetic lives here, so that it
// can be stepped on a CPU (tests/cpp/test_restore_batch_plan.cpp):
//   check   restore_check's conditions per object, every failure naming the object;
//   plan    per object: its first segment in the batch-wide segment run, its place in the object
//           buffer, its packed parity slots (only the parity fragments given take room) and, with a
//           cipher, the place of its joined plaintext pieces and of its padding verdicts;
//           per batch: the two device buffers' sizes, the fid slots, and the key table, in which
//           objects with identical cipher bytes share one entry (as batch_keys has it for uploads);
//   chains  the keyed decrypt launch over exactly the segments of the encrypted objects that passed
//           every check so far.
// Two buffers: the object buffer (every object's nseg x segment ciphertext or plain bytes, data
// fragments land in their final place) and the scratch,
//   [parity slots, packed][plaintext pieces of the encrypted objects, joined per object]
//   [padding verdicts, one byte per encrypted segment][fids, 32 bytes per object].
// All offsets are multiples of 16 but the verdict bytes', whose region is.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "cipher_scheme.hpp"

namespace dm_restore_plan {

constexpr uint64_t kRegionAlign = 256;   // start of each scratch region and slack of the object buffer

enum Code { kOk = 0, kEmpty = 1, kInvalid = 2 };

struct Error {
    Code code = kOk;
    uint64_t obj = 0;   // the object named (meaningless for a batch-wide error)
    std::string msg;
    explicit operator bool() const { return code != kOk; }
};

// One object as its caller describes it.  frags: nseg x total pointers, null = not downloaded (only
// tested for null here).  cipher == null or cipher_len == 0: a plain object.
struct Obj {
    const void* const* frags = nullptr;
    uint64_t nseg = 0, size = 0;
    const void* cipher = nullptr;
    uint64_t cipher_len = 0;
    const void* out = nullptr;   // only tested for null
    bool encrypted() const { return cipher != nullptr && cipher_len != 0; }
};

struct ObjPlan {
    uint64_t seg0 = 0;        // its first segment in the batch-wide run of segments
    uint64_t obj_off = 0;     // object buffer: seg0 * segment
    uint64_t npar = 0;        // parity fragments given
    uint64_t par_off = 0;     // scratch: npar slots of one fragment each, in (segment, index) order
    int32_t key = -1;         // key table entry, -1 = plain
    uint64_t plain_off = 0;   // scratch (cipher): nseg pieces of segment - 16 bytes, joined
    uint64_t pad_off = 0;     // scratch (cipher): nseg verdict bytes reserved
    uint64_t fid_off = 0;     // scratch: 32 bytes
};

struct KeyRef {   // the bytes of one distinct cipher (the first object that brought it)
    const uint8_t* bytes;
    uint64_t len;
};

struct Plan {
    uint64_t segment = 0, frag = 0, piece = 0;
    int k = 0, total = 0;
    std::vector<ObjPlan> obj;
    std::vector<KeyRef> keys;
    uint64_t nseg = 0;       // segments of all objects
    uint64_t npar = 0;       // parity fragments given, all objects
    uint64_t enc_nseg = 0;   // segments of encrypted objects
    uint64_t plain_base = 0, pad_base = 0, fid_base = 0;   // scratch regions
    uint64_t data_bytes = 0, work_bytes = 0;
    uint64_t device_bytes() const { return data_bytes + work_bytes; }
};

// One chain of the keyed decrypt launch: segment `seg` of object `obj`; ciphertext at in_off of the
// object buffer, plaintext to out_off of the scratch.  Chain i's verdict is byte pad_base + i.
struct Chain {
    uint64_t obj, seg;
    uint64_t in_off, out_off;
    uint32_t key;
};

inline uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

inline Error err(Code c, uint64_t o, const std::string& m) {
    Error e;
    e.code = c;
    e.obj = o;
    e.msg = m;
    return e;
}

// The segment size against the coder: what process_check asks (batch-wide, names no object).
inline Error check_segment(uint64_t segment, int k) {
    if (k < 1 || segment == 0 || segment % (16ull * (uint64_t)k))
        return err(kInvalid, 0, "segment size " + std::to_string(segment) + " must be a non-zero multiple of 16 x " +
                                    std::to_string(k) + " data shards");
    return Error();
}

// restore_check's conditions for object o, in its order: nseg >= 1; with a cipher, segment_ok and
// the key length; the size ends in the last piece (cipher) or segment.  Null frags or out first.
inline Error check_obj(const Obj& x, uint64_t o, uint64_t segment) {
    const std::string who = "object " + std::to_string(o) + ": ";
    if (!x.frags || !x.out) return err(kInvalid, o, who + "null argument");
    if (x.nseg == 0) return err(kEmpty, o, "Empty data (object " + std::to_string(o) + " has no segments)");
    uint64_t piece = segment;
    const bool enc = x.encrypted();
    if (enc) {
        if (!dm_cipher::segment_ok(segment))
            return err(kInvalid, o, who + "segment size " + std::to_string(segment) +
                                        " has no room for a block and its padding block");
        if (!dm_cipher::key_len_ok(x.cipher_len)) return err(kInvalid, o, who + dm_cipher::kKeyLenError);
        piece = segment - dm_cipher::kBlock;
    }
    if (x.size <= (x.nseg - 1) * piece || x.size > x.nseg * piece)
        return err(kInvalid, o, who + "size " + std::to_string(x.size) + " does not end in the last of " +
                                    std::to_string(x.nseg) + (enc ? " pieces of " : " segments of ") +
                                    std::to_string(piece) + " bytes");
    return Error();
}

// Every check of a batch, before anything runs: the first failure in object order.
inline Error check(const Obj* objs, uint64_t nobj, uint64_t segment, int k) {
    if (Error e = check_segment(segment, k)) return e;
    for (uint64_t o = 0; o < nobj; o++)
        if (Error e = check_obj(objs[o], o, segment)) return e;
    return Error();
}

// The plan of a checked batch over a coder of k data and m parity shards.
inline Plan plan(const Obj* objs, uint64_t nobj, uint64_t segment, int k, int m) {
    Plan p;
    p.segment = segment;
    p.k = k;
    p.total = k + m;
    p.frag = segment / (uint64_t)k;
    p.piece = segment - dm_cipher::kBlock;
    p.obj.resize(nobj);
    for (uint64_t o = 0; o < nobj; o++) {
        const Obj& x = objs[o];
        ObjPlan& q = p.obj[o];
        q.seg0 = p.nseg;
        q.obj_off = p.nseg * segment;
        for (uint64_t t = 0; t < x.nseg; t++)
            for (int j = k; j < p.total; j++) q.npar += x.frags[t * (uint64_t)p.total + j] != nullptr;
        q.par_off = p.npar * p.frag;
        p.npar += q.npar;
        p.nseg += x.nseg;
        if (!x.encrypted()) continue;
        const uint8_t* bytes = static_cast<const uint8_t*>(x.cipher);
        size_t e = 0;
        while (e < p.keys.size() && (p.keys[e].len != x.cipher_len || memcmp(p.keys[e].bytes, bytes, x.cipher_len) != 0)) e++;
        if (e == p.keys.size()) p.keys.push_back(KeyRef{bytes, x.cipher_len});
        q.key = (int32_t)e;
        q.plain_off = p.enc_nseg;   // in segments for now: the region's base is not known yet
        q.pad_off = p.enc_nseg;
        p.enc_nseg += x.nseg;
    }
    p.plain_base = round_up(p.npar * p.frag + 16, kRegionAlign);
    p.pad_base = round_up(p.plain_base + p.enc_nseg * p.piece, kRegionAlign);
    p.fid_base = round_up(p.pad_base + p.enc_nseg, kRegionAlign);
    for (uint64_t o = 0; o < nobj; o++) {
        ObjPlan& q = p.obj[o];
        q.fid_off = p.fid_base + 32 * o;
        if (q.key < 0) continue;
        q.plain_off = p.plain_base + q.plain_off * p.piece;
        q.pad_off = p.pad_base + q.pad_off;
    }
    p.data_bytes = p.nseg * segment + kRegionAlign;
    p.work_bytes = p.fid_base + 32 * nobj + 16;
    return p;
}

// The keyed decrypt launch: every segment of every encrypted object with alive[o] != 0, in object
// order.  chain0 (nullable) gets, per object, the index of its first chain (only meaningful for the
// objects in the list).
inline std::vector<Chain> decrypt_chains(const Plan& p, const Obj* objs, const uint8_t* alive,
                                         std::vector<uint64_t>* chain0 = nullptr) {
    std::vector<Chain> ch;
    if (chain0) chain0->assign(p.obj.size(), 0);
    for (uint64_t o = 0; o < p.obj.size(); o++) {
        const ObjPlan& q = p.obj[o];
        if (q.key < 0 || !alive[o]) continue;
        if (chain0) (*chain0)[o] = ch.size();
        for (uint64_t t = 0; t < objs[o].nseg; t++)
            ch.push_back(Chain{o, t, q.obj_off + t * p.segment, q.plain_off + t * p.piece, (uint32_t)q.key});
    }
    return ch;
}

}  // namespace dm_restore_plan
