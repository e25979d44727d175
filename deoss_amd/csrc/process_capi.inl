// process_capi.inl -- FullProcessing on the GPU (dm_process_*, include/deoss_merkle.h).
// Part of merkle_capi.hip (included after rs_capi.inl; shares dm_ctx, Dev, dm_rs and the helpers).
//
// Replaces cess-go-sdk process.FullProcessing(file, cipher = "", savedir) (go.mod:8), which every
// upload handler runs to get the fid and the fragment names (node/objectHandler.go:168,
// node/fileHandler.go:771, node/filesHandler.go:201, node/resumeHandler.go:326,
// node/tracker.go:767-769) and the fragment download path re-runs (node/fileHandler.go:964,997).
// One call, all on the device:
//   1. zero the last segment's padding in place (hipMemsetAsync);
//   2. rs_code_kernel codes every segment into its parity fragments (one launch, all segments);
//   3. ONE table-mode leaf-kernel launch hashes the nseg segments (32 MiB leaves, listed first so
//      they start first) and the nseg x (data + parity) fragments (8 MiB leaves) together: the
//      segment chains set the time, the fragment chains run beside them on otherwise idle SIMDs;
//   4. the segment digests reduce to the fid (K2 / finish).
// Oracle: oracle/process_oracle.c (restated composition; parity of the composition unpinned).

namespace {

// nseg segments at `obj` (segment-contiguous, padding already zeroed) belonging to objects whose
// segments start at first[o] (first.size() == nobj + 1): RS coding, one leaf launch over every
// segment and fragment, one fid per object into fids (nobj x 32, device).  Digests land in
// d.leaves in the one-pass order (FpLayout::seg_slot, frag_slot).  after_rs (nullable) is
// recorded once the parity is written, so a caller can copy it out while the leaf kernel runs.
int process_segments(dm_rs* r, Dev& d, hipStream_t s, uint8_t* obj, uint64_t segment, uint8_t* parity,
                     const std::vector<uint64_t>& first, uint8_t* fids, hipEvent_t after_rs = nullptr) {
    dm_ctx* c = r->c;
    const FpLayout L(r->k, r->m, segment);
    const uint64_t nseg = first.back(), nobj = first.size() - 1;
    HIP_TRY(launch_rs(d, s, L.k, rs_encode_args(r, obj, L.seg, parity, L.pbytes, L.frag, nseg)));
    if (after_rs) HIP_TRY(hipEventRecord(after_rs, s));
    // leaf table: segments first (their chains are the longest: they start first), then fragments
    const uint64_t T = L.leaves(nseg);
    std::vector<uint64_t> addr(T), lens(T);
    const FpPiece all{obj, parity, nseg};
    leaf_table(L, &all, 1, true, addr.data(), lens.data());
    dm::LeafArgs la;
    RC_TRY(table_args(c, d, s, addr.data(), lens.data(), T, (nobj + 1) * 12 + 2048, &la));
    hipEvent_t* tr = timing_record(c, d);
    if (tr) HIP_TRY(hipEventRecord(tr[0], s));
    RC_TRY(launch_leaves(c, d, s, la, true, true, pick_leaf_kernel(c, d, T)));
    if (tr) HIP_TRY(hipEventRecord(tr[1], s));
    if (nobj == 1) RC_TRY(finish(c, d, s, d.leaves.u8(), nseg, true, fids));
    else RC_TRY(batch_roots_from_leaves(c, d, s, d.leaves.u8(), first, fids));
    if (tr) HIP_TRY(hipEventRecord(tr[2], s));
    return DM_OK;
}

// The fid from segment digests held on the host (several windows, a stream's batches, a restore):
// hashtree root over n digests -> root (host), in d's scratch; synchronises s.
int rt_fid(dm_ctx* c, Dev& d, hipStream_t s, const uint8_t* segd, uint64_t n, uint8_t root[32]) {
    HIP_TRY(d.leaves.ensure(32 * n));
    HIP_TRY(d.root.ensure(32));
    HIP_TRY(hipMemcpyAsync(d.leaves.p, segd, 32 * n, hipMemcpyHostToDevice, s));
    RC_TRY(finish(c, d, s, d.leaves.u8(), n, true, d.root.u8()));
    HIP_TRY(hipMemcpyAsync(root, d.root.p, 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return DM_OK;
}

int process_dev(dm_rs* r, Dev& d, hipStream_t s, uint8_t* obj, uint64_t len, uint64_t segment, uint8_t* parity,
                uint8_t* seg_hashes, uint8_t* frag_hashes, uint8_t* fid) {
    dm_ctx* c = r->c;
    const int total = r->k + r->m;
    const uint64_t nseg = ceil_div(len, segment);
    RC_TRY(begin_call(c, d, s));
    if (nseg * segment > len) HIP_TRY(hipMemsetAsync(obj + len, 0, nseg * segment - len, s));
    RC_TRY(process_segments(r, d, s, obj, segment, parity, {0, nseg}, fid));
    if (seg_hashes) HIP_TRY(hipMemcpyAsync(seg_hashes, d.leaves.p, nseg * 32, hipMemcpyDeviceToDevice, s));
    if (frag_hashes)
        HIP_TRY(hipMemcpyAsync(frag_hashes, d.leaves.u8() + nseg * 32, nseg * total * 32, hipMemcpyDeviceToDevice, s));
    return DM_OK;
}

int process_staged(dm_rs* r, Dev& d, const std::vector<uint64_t>& first, uint64_t segment, void* const* frags_out,
                   uint8_t* const* seg_hashes, uint8_t* const* frag_hashes, uint8_t* fids);

// Host objects -> device (segment-aligned, zero-padded) -> process_segments -> host outputs.
// Per-object outputs are nullable (frags_out / seg_hashes / frag_hashes may be NULL arrays or hold
// NULL entries); fids (nobj x 32) is required.  Runs on d.stream, synchronous.
int process_host(dm_rs* r, Dev& d, const void* const* objs, const uint64_t* lens, uint64_t nobj, uint64_t segment,
                 void* const* frags_out, uint8_t* const* seg_hashes, uint8_t* const* frag_hashes, uint8_t* fids) {
    dm_ctx* c = r->c;
    hipStream_t s = d.stream;
    RC_TRY(begin_call(c, d, s));
    std::vector<uint64_t> first(nobj + 1, 0), off(nobj);
    for (uint64_t o = 0; o < nobj; o++) {
        first[o + 1] = first[o] + ceil_div(lens[o], segment);
        off[o] = first[o] * segment;
    }
    const uint64_t S = first[nobj];
    HIP_TRY(d.data.ensure(S * segment + kAlign));
    RC_TRY(h2d_at(c, d, objs, lens, nobj, off));
    for (uint64_t o = 0; o < nobj; o++) {
        const uint64_t pad = (first[o + 1] - first[o]) * segment - lens[o];
        if (pad) HIP_TRY(hipMemsetAsync(d.data.u8() + off[o] + lens[o], 0, pad, s));
    }
    return process_staged(r, d, first, segment, frags_out, seg_hashes, frag_hashes, fids);
}

// The part of process_host after staging: first.back() whole segments lie at d.data (padding zeroed
// or, with a cipher, already ciphertext), queued on d.stream.
int process_staged(dm_rs* r, Dev& d, const std::vector<uint64_t>& first, uint64_t segment, void* const* frags_out,
                   uint8_t* const* seg_hashes, uint8_t* const* frag_hashes, uint8_t* fids) {
    dm_ctx* c = r->c;
    hipStream_t s = d.stream;
    const FpLayout L(r->k, r->m, segment);
    const uint64_t nobj = first.size() - 1, S = first[nobj];
    DevBuf& work = rs_ln(r, d).work;
    HIP_TRY(work.ensure(S * L.pbytes + nobj * 32));
    uint8_t* parity = work.u8();
    uint8_t* dfid = parity + S * L.pbytes;
    RC_TRY(process_segments(r, d, s, d.data.u8(), segment, parity, first, dfid));
    HIP_TRY(hipMemcpyAsync(fids, dfid, nobj * 32, hipMemcpyDeviceToHost, s));
    const uint64_t set = (uint64_t)L.total * L.frag;   // a segment's fragments in frags_out: data, then parity
    for (uint64_t o = 0; o < nobj; o++) {
        const uint64_t f0 = first[o], ns = first[o + 1] - first[o];
        if (seg_hashes && seg_hashes[o])
            HIP_TRY(hipMemcpyAsync(seg_hashes[o], d.leaves.u8() + 32 * L.seg_slot(f0), ns * 32, hipMemcpyDeviceToHost, s));
        if (frag_hashes && frag_hashes[o])
            HIP_TRY(hipMemcpyAsync(frag_hashes[o], d.leaves.u8() + 32 * L.frag_slot(S, f0, 0), ns * L.total * 32,
                                   hipMemcpyDeviceToHost, s));
        if (frags_out && frags_out[o]) {
            uint8_t* out = static_cast<uint8_t*>(frags_out[o]);
            for (uint64_t i = 0; i < ns; i++) {
                HIP_TRY(hipMemcpyAsync(out + i * set, L.frag_ptr(d.data.u8(), parity, f0 + i, 0), L.seg,
                                       hipMemcpyDeviceToHost, s));
                HIP_TRY(hipMemcpyAsync(out + i * set + L.seg, L.frag_ptr(d.data.u8(), parity, f0 + i, L.k), L.pbytes,
                                       hipMemcpyDeviceToHost, s));
            }
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    return DM_OK;
}

// process_host for one object with a cipher (cipher_scheme.hpp): the object's P = segment - 16 byte
// pieces go to the device at stride `segment` (one 2-D copy with source pitch P), the last piece's
// tail is zeroed, the encrypt kernel turns every piece into one segment of ciphertext in place, and
// from there process_staged runs as for a plain object of nseg whole segments.
int process_cipher_host(dm_rs* r, Dev& d, const CipherKey& key, const uint8_t* host, uint64_t len, uint64_t segment,
                        void* frags_out, uint8_t* seg_hashes, uint8_t* frag_hashes, uint8_t* fid) {
    dm_ctx* c = r->c;
    hipStream_t s = d.stream;
    RC_TRY(begin_call(c, d, s));
    const dm_cipher::Geometry g = dm_cipher::geometry(len, segment);
    HIP_TRY(d.data.ensure(g.nseg * segment + kAlign));
    const uint64_t full = len / g.piece, rem = len - full * g.piece;
    if (full)
        HIP_TRY(hipMemcpy2DAsync(d.data.p, segment, host, g.piece, g.piece, full, hipMemcpyHostToDevice, s));
    if (rem) {
        uint8_t* last = d.data.u8() + full * segment;
        HIP_TRY(hipMemcpyAsync(last, host + full * g.piece, rem, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(last + rem, 0, g.piece - rem, s));
    }
    HIP_TRY(launch_aes_encrypt(s, key, d.data.u8(), segment, g.piece, g.nseg));
    return process_staged(r, d, {0, g.nseg}, segment, &frags_out, &seg_hashes, &frag_hashes, fid);
}

// The keys of a batch whose objects carry a cipher each: key_of[o] indexes keys, -1 = a plain
// object.  Objects with identical cipher bytes share an entry.
struct BatchKeys {
    std::vector<CipherKey> keys;
    std::vector<int32_t> key_of;
    bool any() const { return !keys.empty(); }
};

// Fills bk for nobj objects (ciphers / cipher_lens nullable: all plain).  A bad length fails naming
// the object; nothing else is checked here.
int batch_keys(dm_ctx* c, const void* const* ciphers, const uint64_t* cipher_lens, uint64_t nobj, BatchKeys& bk) {
    bk.keys.clear();
    bk.key_of.assign(nobj, -1);
    if (!ciphers || !cipher_lens) return DM_OK;
    std::vector<uint64_t> owner;   // the first object of each key entry
    for (uint64_t o = 0; o < nobj; o++) {
        if (!ciphers[o] || cipher_lens[o] == 0) continue;
        if (!dm_cipher::key_len_ok(cipher_lens[o]))
            return fail(c, DM_ERR_INVALID, "object %llu: %s", (unsigned long long)o, dm_cipher::kKeyLenError);
        size_t e = 0;
        while (e < owner.size() && (cipher_lens[owner[e]] != cipher_lens[o] ||
                                    std::memcmp(ciphers[owner[e]], ciphers[o], cipher_lens[o]) != 0))
            e++;
        if (e == owner.size()) {
            CipherKey k;
            RC_TRY(cipher_key(c, ciphers[o], cipher_lens[o], k));
            bk.keys.push_back(k);
            owner.push_back(o);
        }
        bk.key_of[o] = (int32_t)e;
    }
    return DM_OK;
}

// process_host for objects with a cipher each (bk.key_of[o] < 0: a plain object of the same batch).
// One staging pass: plain objects as process_host puts them down, encrypted ones as
// process_cipher_host does (P = segment - 16 byte pieces at stride `segment`, the last piece zeroed
// up to P); ONE keyed launch encrypts every encrypted object's pieces in place, whatever the mix
// of keys; from there process_staged runs once over all segments.
int process_cipher_batch_host(dm_rs* r, Dev& d, const BatchKeys& bk, const void* const* objs, const uint64_t* lens,
                              uint64_t nobj, uint64_t segment, void* const* frags_out, uint8_t* const* seg_hashes,
                              uint8_t* const* frag_hashes, uint8_t* fids) {
    dm_ctx* c = r->c;
    hipStream_t s = d.stream;
    RC_TRY(begin_call(c, d, s));
    const uint64_t piece = segment - dm_cipher::kBlock;
    std::vector<uint64_t> first(nobj + 1, 0);
    for (uint64_t o = 0; o < nobj; o++)
        first[o + 1] = first[o] + (bk.key_of[o] < 0 ? ceil_div(lens[o], segment) : dm_cipher::geometry(lens[o], segment).nseg);
    const uint64_t S = first[nobj];
    HIP_TRY(d.data.ensure(S * segment + kAlign));
    std::vector<const void*> pptr;
    std::vector<uint64_t> plen, poff;
    for (uint64_t o = 0; o < nobj; o++)
        if (bk.key_of[o] < 0) {
            pptr.push_back(objs[o]);
            plen.push_back(lens[o]);
            poff.push_back(first[o] * segment);
        }
    if (!pptr.empty()) RC_TRY(h2d_at(c, d, pptr.data(), plen.data(), pptr.size(), poff));
    std::vector<KeyedChain> chains;
    for (uint64_t o = 0; o < nobj; o++) {
        uint8_t* base = d.data.u8() + first[o] * segment;
        const uint64_t ns = first[o + 1] - first[o];
        if (bk.key_of[o] < 0) {
            const uint64_t pad = ns * segment - lens[o];
            if (pad) HIP_TRY(hipMemsetAsync(base + lens[o], 0, pad, s));
            continue;
        }
        const uint8_t* host = static_cast<const uint8_t*>(objs[o]);
        const uint64_t full = lens[o] / piece, rem = lens[o] - full * piece;
        if (full) HIP_TRY(hipMemcpy2DAsync(base, segment, host, piece, piece, full, hipMemcpyHostToDevice, s));
        if (rem) {
            uint8_t* last = base + full * segment;
            HIP_TRY(hipMemcpyAsync(last, host + full * piece, rem, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemsetAsync(last + rem, 0, piece - rem, s));
        }
        for (uint64_t t = 0; t < ns; t++) chains.push_back(KeyedChain{base + t * segment, (uint32_t)bk.key_of[o]});
    }
    RC_TRY(launch_aes_encrypt_keyed(c, d, s, bk.keys, chains, piece));
    return process_staged(r, d, first, segment, frags_out, seg_hashes, frag_hashes, fids);
}

int process_check(dm_rs* r, uint64_t len, uint64_t segment) {
    dm_ctx* c = r->c;
    if (len == 0) return fail(c, DM_ERR_EMPTY, "Empty data");
    if (segment == 0 || segment % (16ull * (uint64_t)r->k))
        return fail(c, DM_ERR_INVALID, "segment size %llu must be a non-zero multiple of 16 x %d data shards",
                    (unsigned long long)segment, r->k);
    return DM_OK;
}

}  // namespace

extern "C" {

int dm_process_device_async(dm_rs* r, void* dev_obj, uint64_t len, uint64_t segment, void* dev_parity,
                            void* dev_seg_hashes, void* dev_frag_hashes, void* dev_fid, void* stream) {
    if (!r) return bad_arg();
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    RC_TRY(rs_narrow(r, "dm_process_device_async"));
    RC_TRY(process_check(r, len, segment));
    if (!dev_obj || !dev_parity || !dev_fid || !is_aligned16(dev_obj) || !is_aligned16(dev_parity))
        return fail(c, DM_ERR_INVALID, "dm_process_device_async: need 16-byte aligned object and parity buffers");
    Dev& d = c->devs[g];
    return process_dev(r, d, pick_stream(d, stream), static_cast<uint8_t*>(dev_obj), len, segment,
                       static_cast<uint8_t*>(dev_parity), static_cast<uint8_t*>(dev_seg_hashes),
                       static_cast<uint8_t*>(dev_frag_hashes), static_cast<uint8_t*>(dev_fid));
}

int dm_process_buffer(dm_rs* r, const void* host, uint64_t len, uint64_t segment, void* frags_out,
                      uint8_t* seg_hashes, uint8_t* frag_hashes, uint8_t fid[32]) {
    if (!r) return bad_arg();
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    RC_TRY(rs_narrow(r, "dm_process_buffer"));
    if (!fid || (!host && len)) return fail(c, DM_ERR_INVALID, "dm_process_buffer: null argument");
    RC_TRY(process_check(r, len, segment));
    return process_host(r, c->devs[g], &host, &len, 1, segment, &frags_out, &seg_hashes, &frag_hashes, fid);
}

int dm_process_cipher_buffer(dm_rs* r, const void* host, uint64_t len, uint64_t segment, const void* cipher,
                             uint64_t cipher_len, void* frags_out, uint8_t* seg_hashes, uint8_t* frag_hashes,
                             uint8_t fid[32]) {
    if (!r) return bad_arg();
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    RC_TRY(rs_narrow(r, "dm_process_cipher_buffer"));
    if (!fid || (!host && len)) return fail(c, DM_ERR_INVALID, "dm_process_cipher_buffer: null argument");
    RC_TRY(process_check(r, len, segment));
    if (!dm_cipher::segment_ok(segment))
        return fail(c, DM_ERR_INVALID, "segment size %llu has no room for a block and its padding block",
                    (unsigned long long)segment);
    CipherKey key;
    RC_TRY(cipher_key(c, cipher, cipher_len, key));
    Dev& d = c->devs[g];
    const int rc = process_cipher_host(r, d, key, static_cast<const uint8_t*>(host), len, segment, frags_out,
                                       seg_hashes, frag_hashes, fid);
    if (rc != DM_OK) (void)hipStreamSynchronize(d.stream);   // no copy from the caller's memory stays queued
    return rc;
}

int dm_process_batch(dm_rs* r, const void* const* objs, const uint64_t* lens, uint64_t nobj, uint64_t segment,
                     void* const* frags_out, uint8_t* const* seg_hashes, uint8_t* const* frag_hashes, uint8_t* fids) {
    if (!r) return bad_arg();
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    RC_TRY(rs_narrow(r, "dm_process_batch"));
    if (nobj == 0) return DM_OK;
    if (!objs || !lens || !fids) return fail(c, DM_ERR_INVALID, "dm_process_batch: null argument");
    for (uint64_t o = 0; o < nobj; o++) {
        if (lens[o] == 0) return fail(c, DM_ERR_EMPTY, "Empty data (object %llu has no bytes)", (unsigned long long)o);
        if (!objs[o]) return fail(c, DM_ERR_INVALID, "object %llu: NULL pointer", (unsigned long long)o);
    }
    RC_TRY(process_check(r, lens[0], segment));
    return process_host(r, c->devs[g], objs, lens, nobj, segment, frags_out, seg_hashes, frag_hashes, fids);
}

int dm_process_cipher_batch(dm_rs* r, const void* const* objs, const uint64_t* lens, const void* const* ciphers,
                            const uint64_t* cipher_lens, uint64_t nobj, uint64_t segment, void* const* frags_out,
                            uint8_t* const* seg_hashes, uint8_t* const* frag_hashes, uint8_t* fids) {
    if (!r) return bad_arg();
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    RC_TRY(rs_narrow(r, "dm_process_cipher_batch"));
    if (nobj == 0) return DM_OK;
    if (!objs || !lens || !fids) return fail(c, DM_ERR_INVALID, "dm_process_cipher_batch: null argument");
    for (uint64_t o = 0; o < nobj; o++) {
        if (lens[o] == 0) return fail(c, DM_ERR_EMPTY, "Empty data (object %llu has no bytes)", (unsigned long long)o);
        if (!objs[o]) return fail(c, DM_ERR_INVALID, "object %llu: NULL pointer", (unsigned long long)o);
    }
    BatchKeys bk;
    RC_TRY(batch_keys(c, ciphers, cipher_lens, nobj, bk));
    RC_TRY(process_check(r, lens[0], segment));
    if (bk.any() && !dm_cipher::segment_ok(segment))
        return fail(c, DM_ERR_INVALID, "segment size %llu has no room for a block and its padding block",
                    (unsigned long long)segment);
    Dev& d = c->devs[g];
    const int rc = process_cipher_batch_host(r, d, bk, objs, lens, nobj, segment, frags_out, seg_hashes, frag_hashes, fids);
    if (rc != DM_OK) (void)hipStreamSynchronize(d.stream);   // no copy from the caller's memory stays queued
    return rc;
}

}  // extern "C"
