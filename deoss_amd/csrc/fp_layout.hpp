// fp_layout.hpp -- where the segments, fragments and digests of a FullProcessing pass live (pure
// host code, no HIP).
//
// Shared by every path built on the FullProcessing pass (process_capi.inl -- process_staged with a
// cipher or without --, fullproc_capi.inl, process_stream.inl, fragment_capi.inl, and the windows
// of restore_capi.inl) and by the host tests
// (tests/cpp/test_fp_layout.cpp, plain and ASan/UBSan, no GPU).
//
// A segment of `seg` bytes is k data fragments of frag = seg / k bytes -- slices of the segment
// itself -- and m parity fragments, which sit beside each other in a block of pbytes = m * frag per
// segment.  A pass hashes segments and fragments in one leaf launch and names every file it writes
// after its digest; the orders below say which digest belongs to which file.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace dm_fp {

struct FpLayout {
    int k = 0, m = 0, total = 0;          // data, parity, all fragments of a segment
    uint64_t seg = 0, frag = 0, pbytes = 0;   // bytes: segment, fragment, a segment's parity
    FpLayout() = default;
    FpLayout(int data, int parity, uint64_t segment)
        : k(data), m(parity), total(data + parity), seg(segment), frag(segment / (uint64_t)data),
          pbytes((uint64_t)parity * (segment / (uint64_t)data)) {}

    // Fragment j of segment t of a run whose segments start at `data` and whose parity at `parity`.
    template <class B>
    B* frag_ptr(B* data, B* parity, uint64_t t, int j) const {
        return j < k ? data + t * seg + (uint64_t)j * frag : parity + (t * (uint64_t)m + (uint64_t)(j - k)) * frag;
    }

    // Digest order of a one-pass leaf launch over ns segments: segment t at t, then fragment (t, j).
    uint64_t leaves(uint64_t ns) const { return ns * (1 + (uint64_t)total); }
    uint64_t seg_slot(uint64_t t) const { return t; }
    uint64_t frag_slot(uint64_t ns, uint64_t t, int j) const { return ns + t * (uint64_t)total + (uint64_t)j; }
    // Digest order of the striped pass: the segments, then one row of ns digests per data fragment
    // index, then the parity fragments segment by segment.
    uint64_t striped_frag_slot(uint64_t ns, uint64_t t, int j) const {
        return j < k ? ns * (1 + (uint64_t)j) + t : ns * (1 + (uint64_t)k) + t * (uint64_t)m + (uint64_t)(j - k);
    }
    // Striped digests `lv` (32 * leaves(ns) bytes) into the one-pass order: segd gets the ns segment
    // digests, fragd the ns * total fragment digests.
    void striped_to_one_pass(uint64_t ns, const uint8_t* lv, uint8_t* segd, uint8_t* fragd) const {
        std::memcpy(segd, lv, 32 * ns);
        for (uint64_t t = 0; t < ns; t++)
            for (int j = 0; j < total; j++)
                std::memcpy(fragd + 32 * (frag_slot(ns, t, j) - ns), lv + 32 * striped_frag_slot(ns, t, j), 32);
    }

    // Fragment j of the object's segment gs, counted over the whole object (names its temporary).
    uint64_t frag_id(uint64_t gs, int j) const { return gs * (uint64_t)total + (uint64_t)j; }
};

// One run of ns segments at `data` with its parity at `parity`.
struct FpPiece {
    const uint8_t* data;
    const uint8_t* parity;
    uint64_t ns;
};

// The leaf table of a list of pieces: every segment of every piece first (their chains are the
// longest: they start first; left out when !segments), then every fragment in (piece, t, j) order.
// addr and lens hold the leaf count, which is returned.
inline uint64_t leaf_table(const FpLayout& L, const FpPiece* pieces, size_t npieces, bool segments, uint64_t* addr,
                           uint64_t* lens) {
    uint64_t i = 0;
    for (size_t p = 0; segments && p < npieces; p++)
        for (uint64_t t = 0; t < pieces[p].ns; t++, i++) {
            addr[i] = reinterpret_cast<uint64_t>(pieces[p].data + t * L.seg);
            lens[i] = L.seg;
        }
    for (size_t p = 0; p < npieces; p++)
        for (uint64_t t = 0; t < pieces[p].ns; t++)
            for (int j = 0; j < L.total; j++, i++) {
                addr[i] = reinterpret_cast<uint64_t>(L.frag_ptr(pieces[p].data, pieces[p].parity, t, j));
                lens[i] = L.frag;
            }
    return i;
}

// A pending output file is tagged with the digest that names it: a fragment's byte offset into the
// fragment digests (32 * frag_id), or the complement of a segment's offset into the segment digests
// (top bit set: digest arrays stay far below 2^63 bytes).
inline uint64_t frag_tag(uint64_t frag_id) { return 32 * frag_id; }
inline uint64_t seg_tag(uint64_t gs) { return ~(32 * gs); }
inline bool tag_is_seg(uint64_t tag) { return (tag >> 63) != 0; }
inline uint64_t tag_offset(uint64_t tag) { return tag_is_seg(tag) ? ~tag : tag; }
inline const uint8_t* tag_digest(const uint8_t* segd, const uint8_t* fragd, uint64_t tag) {
    return (tag_is_seg(tag) ? segd : fragd) + tag_offset(tag);
}

// Pinned-slot geometry: whole segments per slot on the way in, whole parity sets on the way out
// (at least one of each, however small the slot).
struct FpSlots {
    uint64_t spd, spp, cap;   // segments per data slot, per parity slot; bytes a slot must hold
};
inline FpSlots fp_slots(const FpLayout& L, uint64_t slot_bytes) {
    const uint64_t spd = std::max<uint64_t>(1, slot_bytes / L.seg), spp = std::max<uint64_t>(1, slot_bytes / L.pbytes);
    return {spd, spp, std::max(spd * L.seg, spp * L.pbytes)};
}

// Stripe schedule of the streamed paths (host buffers, files): W bytes of every leaf per step at
// full width, but the stripes start at W/16 and grow by 1/8 per step.  The first stripe's transfer
// overlaps nothing (the GPU waits for it), and each later one must finish within the previous
// stripe's hashing (transfers run ~1.2x the chain-bound hash rate at 256 x 32 MiB).  Offsets and
// widths are multiples of 64 (whole blocks).  Measured on the files path: 15.45 -> 15.70 GiB/s
// (profiles/r02/LOGS.md#r02x_files.log).
inline void stripe_schedule(uint64_t W, uint64_t len, std::vector<uint64_t>& so, std::vector<uint64_t>& sw) {
    so.clear();
    sw.clear();
    for (uint64_t off = 0, w = std::max<uint64_t>(64, (W / 16) / 64 * 64); off < len;) {
        so.push_back(off);
        sw.push_back(w);
        off += w;
        w = std::min(W, std::max(w + 64, (w + w / 8) / 64 * 64));
    }
}

// The striped FullProcessing pass over a window of ns segments: the slot's row pitch, and the
// stripes [so[j], so[j] + sw[j]) of the segment -- stripe_schedule cut at the segment's end and at
// every fragment boundary, so each stripe lies in one data fragment.  frag % 64 == 0.
inline uint64_t fp_stripe_pitch(uint64_t slot_cap, uint64_t ns) { return std::max<uint64_t>(64, (slot_cap / ns) / 64 * 64); }
inline void fp_stripe_plan(const FpLayout& L, uint64_t W, std::vector<uint64_t>& so, std::vector<uint64_t>& sw) {
    std::vector<uint64_t> so0, sw0;
    stripe_schedule(W, L.seg, so0, sw0);
    so.clear();
    sw.clear();
    for (size_t j = 0; j < so0.size(); j++)
        for (uint64_t o = so0[j], e = std::min(L.seg, so0[j] + sw0[j]); o < e;) {
            const uint64_t b = std::min(e, (o / L.frag + 1) * L.frag);
            so.push_back(o);
            sw.push_back(b - o);
            o = b;
        }
}

}  // namespace dm_fp
