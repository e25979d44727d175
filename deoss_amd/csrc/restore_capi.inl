// restore_capi.inl -- the download side on the GPU (dm_rs_restore_*, dm_restore_buffer,
// dm_retrieve_file; include/deoss_merkle.h).  Part of merkle_capi.hip (after fullproc_capi.inl;
// shares dm_ctx, Dev, dm_rs and the leaf launches).  Plans, statuses and a launch's descriptors are
// rs_plan.hpp; the fragment reads and the output writes are fp_files.hpp (read_files, pwrite_all).
//
// Replaces the RSRestore / join / truncate part of cess-go-sdk process.Retrievefile(chainer, fmeta,
// fid, dir, cipher = "") (node/fileHandler.go:519,600,990): for every segment any chain.DataShards
// of its fragments rebuild the data fragments, the segments are joined and the zero padding is cut
// off at the file size.  Here, per call (or per window of segments):
//   1. fragments go to HBM: data fragments straight to their final place in the object, parity
//      fragments to scratch;
//   2. (DM_RESTORE_VERIFY_FRAGMENTS) ONE table-mode leaf launch hashes every fragment given; a
//      fragment whose SHA-256 is not its name is bad and the next good one takes its place;
//   3. ONE rs_restore_kernel launch rebuilds every segment, each with its own erasure pattern
//      (one coding table per distinct pattern, uploaded once);
//   4. (DM_RESTORE_VERIFY_SEGMENTS / _FID) one leaf launch hashes the restored segments, the
//      digests reduce to the fid;
//   5. the object's bytes leave the device only when everything asked for held.
// Steps 2 - 4 are rt_check_frags and rt_rebuild for both paths; they take addresses, and each path
// keeps its own layout of the parity fragments and its own policy after a failed check.

#include "restore_batch_plan.hpp"

namespace {

constexpr uint64_t kRtWindowBytes = 1ull << 30;   // dm_retrieve_file: segment bytes per GPU pass (+ 2x parity scratch)
constexpr int kRtReaders = 8;                      // fragment files read at once into a pinned slot

int rs_desc_launch(dm_rs* r, Dev& d, hipStream_t s, const RsBatch& b, uint64_t units) {
    dm_ctx* c = r->c;
    if (!b.any_out) return DM_OK;
    RsLane& L = rs_ln(r, d);
    const uint64_t dbytes = b.desc.size() * sizeof(dm::RsRestoreDesc), tbytes = b.tabs.size() * 8;
    RC_TRY(tables_begin(c, d, dbytes + tbytes + 1024));
    RC_TRY(upload(c, d, s, L.rst_desc, b.desc.data(), dbytes));
    RC_TRY(upload(c, d, s, L.rst_tab, b.tabs.data(), tbytes));
    const dm::RsRestoreArgs a{static_cast<const dm::RsRestoreDesc*>(L.rst_desc.p), static_cast<const uint2*>(L.rst_tab.p),
                              units, b.desc.size()};
    const dim3 grid = rs_grid(d, units, a.nseg), block(dm::kRsThreads);
    if (b.any_wide)   // a repair with more than k outputs somewhere; else the narrower kernel does it
        rs_for_k(r->k, [&](auto K) { hipLaunchKernelGGL(dm::rs_repair_kernel<decltype(K)::value>, grid, block, 0, s, a); });
    else
        rs_for_k(r->k, [&](auto K) { hipLaunchKernelGGL(dm::rs_restore_kernel<decltype(K)::value>, grid, block, 0, s, a); });
    HIP_TRY(hipGetLastError());
    return DM_OK;
}

// SHA-256 of `addrs.size()` device ranges of `len` bytes each (16-byte aligned), one table-mode leaf
// launch; the digests stay in d.leaves and are copied to `dig` (synchronises s).
int rt_hash(dm_ctx* c, Dev& d, hipStream_t s, const std::vector<uint64_t>& addrs, uint64_t len,
            std::vector<uint8_t>& dig) {
    const uint64_t T = addrs.size();
    dig.resize(32 * T);
    if (T == 0) return DM_OK;
    const std::vector<uint64_t> lens(T, len);
    dm::LeafArgs la;
    RC_TRY(table_args(c, d, s, addrs.data(), lens.data(), T, 1024, &la));
    RC_TRY(launch_leaves(c, d, s, la, true, true, pick_leaf_kernel(c, d, T)));
    HIP_TRY(hipMemcpyAsync(dig.data(), d.leaves.p, 32 * T, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return DM_OK;
}

// The fragments of a run of segments, [ns * total]: where one that is on the device and passed its
// check lies, else null.
using RtFrags = std::vector<const uint8_t*>;

struct RtLoad {     // one fragment brought to the device
    uint64_t idx;   // t * total + j within the run
    uint8_t* to;
};

// One loaded fragment against its name (dig, name: 32 bytes each; null name: taken as given): a good
// one is entered in f at l.idx, another is kFragBad there.  The rule of the single-object calls and
// of the batch alike.
void rt_enter_frag(const RtLoad& l, const uint8_t* dig, const uint8_t* name, RtFrags& f, uint8_t* fst) {
    if (name && std::memcmp(dig, name, 32) != 0) {
        fst[l.idx] = kFragBad;
        return;
    }
    f[l.idx] = l.to;
}

// ns segment digests against their names: a segment that differs is kSegMismatch; true when all match.
bool rt_match_segs(const uint8_t* segd, const uint8_t* seg_names, uint64_t ns, uint8_t* sst) {
    bool all = true;
    for (uint64_t t = 0; t < ns; t++)
        if (std::memcmp(segd + 32 * t, seg_names + 32 * t, 32) != 0) {
            sst[t] = kSegMismatch;
            all = false;
        }
    return all;
}

// 2. The fragments just loaded against their names (names + 32 * idx; null: taken as given), hashed
// in one leaf launch: a good one is entered in f, another is kFragBad.
int rt_check_frags(dm_ctx* c, Dev& d, hipStream_t s, const std::vector<RtLoad>& loads, uint64_t frag,
                   const uint8_t* names, RtFrags& f, uint8_t* fst) {
    std::vector<uint8_t> dig;
    if (names) {
        std::vector<uint64_t> addrs(loads.size());
        for (size_t q = 0; q < loads.size(); q++) addrs[q] = reinterpret_cast<uint64_t>(loads[q].to);
        RC_TRY(rt_hash(c, d, s, addrs, frag, dig));
    }
    for (size_t q = 0; q < loads.size(); q++)
        rt_enter_frag(loads[q], names ? dig.data() + 32 * q : nullptr, names ? names + 32 * loads[q].idx : nullptr, f, fst);
    return DM_OK;
}

enum class Rebuild { kDone, kTooFew, kMismatch };

// 3 + 4. ns segments at `base` from the good fragments, wherever those lie: statuses (kTooFew:
// nothing is launched), ONE restore launch; then, with seg_names or want_segd, one leaf launch over
// the segments, whose digests go to segd and are compared with seg_names (nullable; kMismatch).
int rt_rebuild(dm_rs* r, Dev& d, hipStream_t s, const RtFrags& f, uint64_t ns, uint8_t* base, uint64_t segment,
               uint8_t* fst, uint8_t* sst, const uint8_t* seg_names, bool want_segd, std::vector<uint8_t>& segd,
               Rebuild& res) {
    dm_ctx* c = r->c;
    const int k = r->k, total = r->k + r->m;
    const uint64_t frag = segment / (uint64_t)k;
    res = Rebuild::kTooFew;
    if (!rt_select(k, total, ns, f.data(), fst, sst)) return DM_OK;
    RestoreBatch b{r->mat.data(), k, r->m};
    for (uint64_t t = 0; t < ns; t++)
        RC_TRY(plan_status(c, restore_add(b, f.data() + t * total, base + t * segment, frag), k));
    RC_TRY(rs_desc_launch(r, d, s, b, frag / 16));
    res = Rebuild::kDone;
    if (!seg_names && !want_segd) return DM_OK;
    std::vector<uint64_t> sa(ns);
    for (uint64_t t = 0; t < ns; t++) sa[t] = reinterpret_cast<uint64_t>(base + t * segment);
    RC_TRY(rt_hash(c, d, s, sa, segment, segd));
    if (seg_names && !rt_match_segs(segd.data(), seg_names, ns, sst)) res = Rebuild::kMismatch;
    return DM_OK;
}

// The arguments every restore entry point shares.  key (nullable): the call has a cipher, which is
// parsed into it; the object then ends in the last of nseg pieces of segment - 16 bytes.
int restore_check(dm_rs* r, uint64_t nseg, uint64_t size, uint64_t segment, CipherKey* key = nullptr,
                  const void* cipher = nullptr, uint64_t cipher_len = 0) {
    dm_ctx* c = r->c;
    if (nseg == 0) return fail(c, DM_ERR_EMPTY, "Empty data");
    RC_TRY(process_check(r, size ? size : 1, segment));
    uint64_t piece = segment;
    if (key) {
        if (!dm_cipher::segment_ok(segment))
            return fail(c, DM_ERR_INVALID, "segment size %llu has no room for a block and its padding block",
                        (unsigned long long)segment);
        RC_TRY(cipher_key(c, cipher, cipher_len, *key));
        piece = segment - dm_cipher::kBlock;
    }
    if (size <= (nseg - 1) * piece || size > nseg * piece)
        return fail(c, DM_ERR_INVALID, "size %llu does not end in the last of %llu %s of %llu bytes",
                    (unsigned long long)size, (unsigned long long)nseg, key ? "pieces" : "segments",
                    (unsigned long long)piece);
    return DM_OK;
}

// The fragment and segment statuses of a call, copied to the caller however the call ends.
struct RtStatus {
    std::vector<uint8_t> fst, sst;
    RtStatus(const dm_rs* r, uint64_t nseg) : fst(nseg * (uint64_t)(r->k + r->m), 0), sst(nseg, 0) {}
    void copy_out(uint8_t* frag_status, uint8_t* seg_status) const {
        if (frag_status) std::memcpy(frag_status, fst.data(), fst.size());
        if (seg_status) std::memcpy(seg_status, sst.data(), sst.size());
    }
};

// key (nullable): the object was uploaded with a cipher (cipher_scheme.hpp).  Every name and the
// fid are of ciphertext, so steps 1-4 run as without one; then the segments are decrypted into
// scratch, and `size` counts plaintext bytes.  A padding block that is not sixteen 0x10 bytes (what
// a wrong cipher looks like) is kSegBadPadding and *ok stays 0: a result, not an error.
int restore_buffer(dm_rs* r, Dev& d, const void* const* frags, const uint8_t* frag_names, const uint8_t* seg_names,
                   const uint8_t* fid, uint64_t nseg, uint64_t size, uint64_t segment, int flags, void* out,
                   uint8_t* fst, uint8_t* sst, int* ok, const CipherKey* key = nullptr) {
    dm_ctx* c = r->c;
    hipStream_t s = d.stream;
    RC_TRY(begin_call(c, d, s));
    const int k = r->k, total = r->k + r->m;
    const uint64_t frag = segment / (uint64_t)k, NF = nseg * (uint64_t)total;
    // 1. data fragments to their final place, parity fragments to scratch
    uint64_t npar = 0;
    for (uint64_t t = 0; t < nseg; t++)
        for (int j = k; j < total; j++) npar += frags[t * total + j] != nullptr;
    HIP_TRY(d.data.ensure(nseg * segment + kAlign));
    DevBuf& work = rs_ln(r, d).work;
    // with a cipher: the plaintext pieces and the padding verdicts follow the parity fragments
    const uint64_t piece = segment - dm_cipher::kBlock, plain_off = round_up(npar * frag + 16, kAlign);
    HIP_TRY(work.ensure(key ? plain_off + nseg * piece + nseg : npar * frag + 16));
    RtFrags have(NF, nullptr);
    std::vector<RtLoad> loads;
    uint64_t slot = 0;   // parity fragments are packed: only those given take room
    for (uint64_t t = 0; t < nseg; t++)
        for (int j = 0; j < total; j++) {
            const uint64_t i = t * total + j;
            if (!frags[i]) continue;
            uint8_t* to = j < k ? d.data.u8() + t * segment + (uint64_t)j * frag : work.u8() + (slot++) * frag;
            HIP_TRY(hipMemcpyAsync(to, frags[i], frag, hipMemcpyHostToDevice, s));
            loads.push_back({i, to});
        }
    // 2. every supplied fragment against its name
    const bool vfrag = (flags & DM_RESTORE_VERIFY_FRAGMENTS) && frag_names;
    RC_TRY(rt_check_frags(c, d, s, loads, frag, vfrag ? frag_names : nullptr, have, fst));
    // 3 + 4. one restore launch; the restored segments against their names, their tree against the fid
    const bool vseg = (flags & DM_RESTORE_VERIFY_SEGMENTS) && seg_names, vfid = (flags & DM_RESTORE_VERIFY_FID) && fid;
    std::vector<uint8_t> segd;
    Rebuild res;
    RC_TRY(rt_rebuild(r, d, s, have, nseg, d.data.u8(), segment, fst, sst, vseg ? seg_names : nullptr, vfid, segd, res));
    if (res != Rebuild::kDone) return DM_OK;
    if (vfid) {
        uint8_t root[32];
        RC_TRY(rt_fid(c, d, s, segd.data(), nseg, root));
        if (std::memcmp(root, fid, 32) != 0) return DM_OK;
    }
    const void* obj = d.data.p;
    if (key) {   // 4b. ciphertext -> the joined plaintext pieces, every padding block checked
        bool all = true;
        uint8_t* plain = work.u8() + plain_off;
        uint8_t* pad_ok = plain + nseg * piece;
        HIP_TRY(launch_aes_decrypt(d, s, *key, d.data.u8(), segment, segment, nseg, plain, piece, pad_ok));
        std::vector<uint8_t> pad(nseg);
        HIP_TRY(hipMemcpyAsync(pad.data(), pad_ok, nseg, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint64_t t = 0; t < nseg; t++)
            if (pad[t] != 1) {
                sst[t] = kSegBadPadding;
                all = false;
            }
        if (!all) return DM_OK;
        obj = plain;
    }
    // 5. everything held: the object's bytes, without the padding
    HIP_TRY(hipMemcpyAsync(out, obj, size, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *ok = 1;
    return DM_OK;
}

std::atomic<uint64_t> g_rt_seq{0};

// Fragment files -> pinned slots (parallel preads) -> HBM, slot by slot; synchronises d.copy.
int rt_load(dm_rs* r, Dev& d, const std::vector<RtLoad>& loads, const std::vector<std::string>& paths, uint64_t frag,
            uint64_t slot_cap, FpEvents& ev, uint64_t& next_slot) {
    dm_ctx* c = r->c;
    RsLane& L = rs_ln(r, d);
    const uint64_t per = std::max<uint64_t>(1, slot_cap / frag);
    for (size_t g0 = 0; g0 < loads.size(); g0 += per) {
        const size_t n = std::min<size_t>(per, loads.size() - g0);
        const int sl = (int)(next_slot++ % kFpSlots);
        HIP_TRY(hipEventSynchronize(ev.slot[sl]));   // the slot's previous copies have left it
        uint8_t* buf = L.fp_slot[sl].u8();
        const std::string err = read_files(paths.data() + g0, n, frag, buf, kRtReaders);
        if (!err.empty()) return fail(c, DM_ERR_IO, "%s", err.c_str());
        for (size_t i = 0; i < n; i++)
            HIP_TRY(hipMemcpyAsync(loads[g0 + i].to, buf + i * frag, frag, hipMemcpyHostToDevice, d.copy));
        HIP_TRY(hipEventRecord(ev.slot[sl], d.copy));
    }
    HIP_TRY(hipStreamSynchronize(d.copy));
    return DM_OK;
}

// Everything of dm_retrieve_file but the temporary file's fate; *ok = 1 when the object was
// restored, verified as asked and written to out_fd.
int retrieve_windows(dm_rs* r, Dev& d, const std::string& dir, const uint8_t* frag_names, const uint8_t* seg_names,
                     const uint8_t* fid, uint64_t nseg, uint64_t size, uint64_t segment, int flags, int out_fd,
                     const std::string& out_name, uint8_t* fst, uint8_t* sst, int* ok) {
    dm_ctx* c = r->c;
    RsLane& L = rs_ln(r, d);
    hipStream_t s = d.stream;
    RC_TRY(begin_call(c, d, s));
    const FpLayout lay(r->k, r->m, segment);   // parity fragments in L.work, laid out as FullProcessing's
    const int k = lay.k, total = lay.total;
    const uint64_t frag = lay.frag;
    // test hooks (env, read per call): small windows and slots exercise several windows and slot reuse
    const uint64_t win = std::max<uint64_t>(1, env_bytes("DEOSS_RT_WINDOW_BYTES", kRtWindowBytes) / segment);
    const uint64_t slot_cap = std::max(env_bytes("DEOSS_FP_SLOT_BYTES", kFpSlotBytes), frag);
    for (auto& b : L.fp_slot) HIP_TRY(b.ensure(slot_cap));
    FpEvents ev;
    for (auto& e : ev.slot) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    uint64_t next_slot = 0;
    const bool vfrag = (flags & DM_RESTORE_VERIFY_FRAGMENTS) != 0;
    const bool vseg = (flags & DM_RESTORE_VERIFY_SEGMENTS) && seg_names, vfid = (flags & DM_RESTORE_VERIFY_FID) && fid;
    std::vector<uint8_t> segd_all(vfid ? 32 * nseg : 0);
    bool all = true;
    for (uint64_t w0 = 0; w0 < nseg; w0 += win) {
        const uint64_t ns = std::min(win, nseg - w0);
        HIP_TRY(hipStreamSynchronize(s));   // the previous window's kernels are done with the object buffer
        HIP_TRY(d.data.ensure(ns * segment + kAlign));
        HIP_TRY(L.work.ensure(ns * lay.pbytes + 16));
        RtFrags have(ns * (uint64_t)total, nullptr);
        std::vector<int> cand(ns, 0), ngood(ns, 0);
        uint8_t* wf = fst + w0 * total;
        const uint8_t* wnames = frag_names + 32 * w0 * total;
        // 1 + 2. per segment the first k fragment files that exist; further ones while a check fails
        for (;;) {
            std::vector<RtLoad> loads;
            std::vector<std::string> paths;
            for (uint64_t t = 0; t < ns; t++) {
                int need = k - ngood[t];
                while (need > 0 && cand[t] < total) {
                    const int j = cand[t]++;
                    const uint64_t i = t * total + j;
                    const std::string p = dir + "/" + hex32(wnames + 32 * i);
                    struct stat st {};
                    if (::stat(p.c_str(), &st) != 0) {
                        if (errno == ENOENT || errno == ENOTDIR) continue;   // not downloaded: absent
                        return fail(c, DM_ERR_IO, "stat %s: %s", p.c_str(), go_errno(errno).c_str());
                    }
                    if (!S_ISREG(st.st_mode) || (uint64_t)st.st_size != frag) {
                        wf[i] = kFragBad;   // not a fragment of this object's shape
                        continue;
                    }
                    loads.push_back({i, lay.frag_ptr(d.data.u8(), L.work.u8(), t, j)});
                    paths.push_back(p);
                    need--;
                }
            }
            if (loads.empty()) break;
            RC_TRY(rt_load(r, d, loads, paths, frag, slot_cap, ev, next_slot));
            RC_TRY(rt_check_frags(c, d, s, loads, frag, vfrag ? wnames : nullptr, have, wf));
            for (const RtLoad& l : loads) ngood[l.idx / total] += have[l.idx] != nullptr;
        }
        // 3 + 4. one restore launch over the window, its segments against their names
        std::vector<uint8_t> segd;
        Rebuild res;
        RC_TRY(rt_rebuild(r, d, s, have, ns, d.data.u8(), segment, wf, sst + w0, vseg ? seg_names + 32 * w0 : nullptr, vfid,
                          segd, res));
        if (res != Rebuild::kDone) all = false;   // later windows still report their fragments
        else if (vfid) std::memcpy(segd_all.data() + 32 * w0, segd.data(), 32 * ns);
        if (!all) continue;
        // 5. the window's bytes through the pinned slots into the output file, cut at the file size
        const uint64_t wbeg = w0 * segment, wend = std::min(size, (w0 + ns) * segment);
        for (uint64_t o = wbeg; o < wend; o += slot_cap) {
            const uint64_t n = std::min(slot_cap, wend - o);
            const int sl = (int)(next_slot++ % kFpSlots);
            HIP_TRY(hipEventSynchronize(ev.slot[sl]));
            HIP_TRY(hipMemcpyAsync(L.fp_slot[sl].p, d.data.u8() + (o - wbeg), n, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            const std::string err = pwrite_all(out_fd, out_name, L.fp_slot[sl].u8(), n, o);
            if (!err.empty()) return fail(c, DM_ERR_IO, "%s", err.c_str());
        }
    }
    if (all && vfid) {
        uint8_t root[32];
        RC_TRY(rt_fid(c, d, s, segd_all.data(), nseg, root));
        if (std::memcmp(root, fid, 32) != 0) all = false;
    }
    *ok = all ? 1 : 0;
    return DM_OK;
}

// dm_restore_buffer and, with `key` (storage for the parsed cipher), dm_restore_cipher_buffer.
int restore_buffer_call(dm_rs* r, const char* fn, const void* const* frags, const uint8_t* frag_names,
                        const uint8_t* seg_names, const uint8_t* fid, uint64_t nseg, uint64_t size, uint64_t segment,
                        int flags, CipherKey* key, const void* cipher, uint64_t cipher_len, void* out,
                        uint8_t* frag_status, uint8_t* seg_status, int* ok) {
    if (!r || !ok) return bad_arg();
    *ok = 0;
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    RC_TRY(rs_narrow(r, fn));
    if (!frags || !out) return fail(c, DM_ERR_INVALID, "%s: null argument", fn);
    RC_TRY(restore_check(r, nseg, size, segment, key, cipher, cipher_len));
    RtStatus st(r, nseg);
    const int rc = restore_buffer(r, c->devs[g], frags, frag_names, seg_names, fid, nseg, size, segment, flags, out,
                                  st.fst.data(), st.sst.data(), ok, key);
    // no copy from the caller's memory stays queued, whichever way the call ends
    if (rc != DM_OK || !*ok) (void)hipStreamSynchronize(c->devs[g].stream);
    st.copy_out(frag_status, seg_status);
    return rc;
}

// ---- many objects in one pass (dm_restore_batch, the DM_BATCH_RESTORE batcher) ----

// The batch as restore_batch_plan.hpp takes it.
std::vector<dm_restore_plan::Obj> rb_objs(const dm_restore_obj* objs, uint64_t nobj) {
    std::vector<dm_restore_plan::Obj> po(nobj);
    for (uint64_t o = 0; o < nobj; o++) {
        po[o].frags = objs[o].frags;
        po[o].nseg = objs[o].nseg;
        po[o].size = objs[o].size;
        po[o].cipher = objs[o].cipher;
        po[o].cipher_len = objs[o].cipher_len;
        po[o].out = objs[o].out;
    }
    return po;
}

int rb_fail(dm_ctx* c, const dm_restore_plan::Error& e) {
    return fail(c, e.code == dm_restore_plan::kEmpty ? DM_ERR_EMPTY : DM_ERR_INVALID, "%s", e.msg.c_str());
}

// Statuses of every object of a batch, [plan.nseg * total] and [plan.nseg] in the batch-wide
// segment order; copied to the callers however the pass ends.
struct RbStatus {
    std::vector<uint8_t> fst, sst;
    RbStatus(const dm_restore_plan::Plan& p) : fst(p.nseg * (uint64_t)p.total, 0), sst(p.nseg, 0) {}
    void copy_out(const dm_restore_plan::Plan& p, const dm_restore_obj* objs) const {
        for (size_t o = 0; o < p.obj.size(); o++) {
            const uint64_t s0 = p.obj[o].seg0, ns = objs[o].nseg;
            if (objs[o].frag_status) std::memcpy(objs[o].frag_status, fst.data() + s0 * p.total, ns * p.total);
            if (objs[o].seg_status) std::memcpy(objs[o].seg_status, sst.data() + s0, ns);
        }
    }
};

// The pass of dm_restore_batch over a checked batch and its plan, on d.stream; synchronous.  The
// steps are restore_buffer's, each ONE launch over every object still alive: an object that fails a
// step keeps the statuses restore_buffer would give it and is left out of the steps after.
int restore_batch_host(dm_rs* r, Dev& d, const dm_restore_obj* objs, const std::vector<dm_restore_plan::Obj>& po,
                       const dm_restore_plan::Plan& p, RbStatus& st, int* ok) {
    dm_ctx* c = r->c;
    hipStream_t s = d.stream;
    RC_TRY(begin_call(c, d, s));
    const uint64_t nobj = p.obj.size(), segment = p.segment, frag = p.frag;
    const int k = p.k, total = p.total;
    DevBuf& work = rs_ln(r, d).work;
    // the whole batch must fit: no splitting, and no growth that fails half way through the staging
    {
        const bool gd = p.data_bytes > d.data.cap, gw = p.work_bytes > work.cap;   // a grown buffer's old block is freed first
        const uint64_t grow = (gd ? p.data_bytes : 0) + (gw ? p.work_bytes : 0);
        const uint64_t back = (gd ? d.data.cap : 0) + (gw ? work.cap : 0);
        size_t fr = 0, tot = 0;
        if (grow && free_on(d.id, &fr, &tot) && fr + back < grow + kMallocHeadroom)
            return fail(c, DM_ERR_NOMEM, "dm_restore_batch: the batch needs %llu bytes of device memory, %llu are free",
                        (unsigned long long)p.device_bytes(), (unsigned long long)fr);
    }
    HIP_TRY(d.data.ensure(p.data_bytes));
    HIP_TRY(work.ensure(p.work_bytes));
    std::vector<CipherKey> keys(p.keys.size());
    for (size_t e = 0; e < keys.size(); e++) RC_TRY(cipher_key(c, p.keys[e].bytes, p.keys[e].len, keys[e]));
    std::vector<uint8_t> alive(nobj, 1);
    // 1. one staging: data fragments to their final place, parity fragments packed into scratch
    RtFrags have(p.nseg * (uint64_t)total, nullptr);
    std::vector<RtLoad> loads;          // idx: batch-wide fragment index
    std::vector<uint64_t> load_obj;
    for (uint64_t o = 0; o < nobj; o++) {
        const dm_restore_plan::ObjPlan& q = p.obj[o];
        uint64_t slot = 0;
        for (uint64_t t = 0; t < objs[o].nseg; t++)
            for (int j = 0; j < total; j++) {
                const void* src = objs[o].frags[t * total + j];
                if (!src) continue;
                uint8_t* to = j < k ? d.data.u8() + q.obj_off + t * segment + (uint64_t)j * frag
                                    : work.u8() + q.par_off + (slot++) * frag;
                HIP_TRY(hipMemcpyAsync(to, src, frag, hipMemcpyHostToDevice, s));
                loads.push_back({(q.seg0 + t) * total + j, to});
                load_obj.push_back(o);
            }
    }
    // 2. one leaf launch over every fragment of the objects that asked for the fragment check
    {
        std::vector<uint64_t> addrs;
        std::vector<size_t> which;
        for (size_t i = 0; i < loads.size(); i++) {
            const dm_restore_obj& x = objs[load_obj[i]];
            if ((x.flags & DM_RESTORE_VERIFY_FRAGMENTS) && x.frag_names) {
                addrs.push_back(reinterpret_cast<uint64_t>(loads[i].to));
                which.push_back(i);
            } else {
                rt_enter_frag(loads[i], nullptr, nullptr, have, st.fst.data());
            }
        }
        std::vector<uint8_t> dig;
        RC_TRY(rt_hash(c, d, s, addrs, frag, dig));
        for (size_t a = 0; a < which.size(); a++) {
            const RtLoad& l = loads[which[a]];
            const uint64_t o = load_obj[which[a]], local = l.idx - p.obj[o].seg0 * total;
            rt_enter_frag(l, dig.data() + 32 * a, objs[o].frag_names + 32 * local, have, st.fst.data());
        }
    }
    // 3. statuses per object; one restore launch over every segment of the objects that can be rebuilt
    RestoreBatch b{r->mat.data(), k, r->m};
    for (uint64_t o = 0; o < nobj; o++) {
        const dm_restore_plan::ObjPlan& q = p.obj[o];
        const uint64_t f0 = q.seg0 * total;
        if (!rt_select(k, total, objs[o].nseg, have.data() + f0, st.fst.data() + f0, st.sst.data() + q.seg0)) {
            alive[o] = 0;
            continue;
        }
        for (uint64_t t = 0; t < objs[o].nseg; t++)
            RC_TRY(plan_status(c, restore_add(b, have.data() + f0 + t * total, d.data.u8() + q.obj_off + t * segment, frag), k));
    }
    RC_TRY(rs_desc_launch(r, d, s, b, frag / 16));
    // 4. one leaf launch over the segments of the objects that asked for segment or fid checks; the
    // fid objects come first, so that their digests are one run of d.leaves and reduce in place
    {
        std::vector<uint64_t> order, first(1, 0), sa;
        auto vseg = [&](uint64_t o) { return (objs[o].flags & DM_RESTORE_VERIFY_SEGMENTS) && objs[o].seg_names; };
        auto vfid = [&](uint64_t o) { return (objs[o].flags & DM_RESTORE_VERIFY_FID) && objs[o].fid; };
        for (uint64_t o = 0; o < nobj; o++)
            if (alive[o] && vfid(o)) {
                order.push_back(o);
                first.push_back(first.back() + objs[o].nseg);
            }
        const uint64_t nfid = order.size();
        for (uint64_t o = 0; o < nobj; o++)
            if (alive[o] && !vfid(o) && vseg(o)) order.push_back(o);
        for (uint64_t o : order)
            for (uint64_t t = 0; t < objs[o].nseg; t++)
                sa.push_back(reinterpret_cast<uint64_t>(d.data.u8() + p.obj[o].obj_off + t * segment));
        if (!sa.empty()) {
            const uint64_t T = sa.size();
            const std::vector<uint64_t> lens(T, segment);
            dm::LeafArgs la;
            RC_TRY(table_args(c, d, s, sa.data(), lens.data(), T, (nfid + 1) * 12 + 2048, &la));
            RC_TRY(launch_leaves(c, d, s, la, true, true, pick_leaf_kernel(c, d, T)));
            std::vector<uint8_t> segd(32 * T), roots(32 * nfid);
            HIP_TRY(hipMemcpyAsync(segd.data(), d.leaves.p, 32 * T, hipMemcpyDeviceToHost, s));
            if (nfid) {
                uint8_t* dfid = work.u8() + p.fid_base;
                RC_TRY(batch_roots_from_leaves(c, d, s, d.leaves.u8(), first, dfid));
                HIP_TRY(hipMemcpyAsync(roots.data(), dfid, 32 * nfid, hipMemcpyDeviceToHost, s));
            }
            HIP_TRY(hipStreamSynchronize(s));
            uint64_t at = 0;
            for (size_t i = 0; i < order.size(); i++) {
                const uint64_t o = order[i], ns = objs[o].nseg;
                if (vseg(o) && !rt_match_segs(segd.data() + 32 * at, objs[o].seg_names, ns, st.sst.data() + p.obj[o].seg0))
                    alive[o] = 0;
                if (alive[o] && i < nfid && std::memcmp(roots.data() + 32 * i, objs[o].fid, 32) != 0) alive[o] = 0;
                at += ns;
            }
        }
    }
    // 5. one keyed decrypt launch over the segments of the encrypted objects still alive
    {
        const std::vector<dm_restore_plan::Chain> ch = dm_restore_plan::decrypt_chains(p, po.data(), alive.data());
        if (!ch.empty()) {
            std::vector<KeyedDChain> kc(ch.size());
            for (size_t i = 0; i < ch.size(); i++)
                kc[i] = KeyedDChain{d.data.u8() + ch[i].in_off, work.u8() + ch[i].out_off, ch[i].key};
            uint8_t* pad_ok = work.u8() + p.pad_base;
            RC_TRY(launch_aes_decrypt_keyed(c, d, s, keys, kc, segment, pad_ok));
            // 6. the padding verdicts come back, and only then any bytes
            std::vector<uint8_t> pad(ch.size());
            HIP_TRY(hipMemcpyAsync(pad.data(), pad_ok, ch.size(), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            for (size_t i = 0; i < ch.size(); i++)
                if (pad[i] != 1) {
                    st.sst[p.obj[ch[i].obj].seg0 + ch[i].seg] = kSegBadPadding;
                    alive[ch[i].obj] = 0;
                }
        }
    }
    for (uint64_t o = 0; o < nobj; o++) {
        if (!alive[o]) continue;
        const dm_restore_plan::ObjPlan& q = p.obj[o];
        const uint8_t* src = q.key < 0 ? d.data.u8() + q.obj_off : work.u8() + q.plain_off;
        HIP_TRY(hipMemcpyAsync(objs[o].out, src, objs[o].size, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    for (uint64_t o = 0; o < nobj; o++) ok[o] = alive[o];
    return DM_OK;
}

// Plan, pass and statuses of a batch whose arguments have been checked; what dm_restore_batch and
// the batcher's workers both run (the caller holds the lane).
int restore_batch_run(dm_rs* r, Dev& d, const dm_restore_obj* objs, uint64_t nobj, uint64_t segment, int* ok) {
    for (uint64_t o = 0; o < nobj; o++) ok[o] = 0;
    const std::vector<dm_restore_plan::Obj> po = rb_objs(objs, nobj);
    const dm_restore_plan::Plan p = dm_restore_plan::plan(po.data(), nobj, segment, r->k, r->m);
    RbStatus st(p);
    const int rc = restore_batch_host(r, d, objs, po, p, st, ok);
    // no copy from or to a caller's memory stays queued, whichever way the pass ends
    if (rc != DM_OK) {
        (void)hipStreamSynchronize(d.stream);
        for (uint64_t o = 0; o < nobj; o++) ok[o] = 0;
    }
    st.copy_out(p, objs);
    if (d.data.cap > kFpKeepBytes) r->c->reaper.put(d.id, d.data);
    if (rs_ln(r, d).work.cap > kFpKeepBytes) r->c->reaper.put(d.id, rs_ln(r, d).work);
    return rc;
}

std::mutex g_plan_mu;
std::map<int, std::vector<uint8_t>> g_plan_mats;   // data * 16 + parity -> coding matrix

}  // namespace

extern "C" {

int dm_rs_restore_plan(int data, int parity, const uint8_t* present, const uint8_t* in_place, int* inputs,
                       int* outputs, uint8_t* rows, int* nout) {
    if (!present || !inputs || !outputs || !rows || !nout) return bad_arg();
    if (data < 1 || data > dm::kRsMaxIn || parity < 1 || parity > dm::kRsMaxOut)
        return fail(nullptr, DM_ERR_INVALID, "shard counts: 1 <= data <= %d, 1 <= parity <= %d", dm::kRsMaxIn,
                    dm::kRsMaxOut);
    std::vector<uint8_t> mat;
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        std::vector<uint8_t>& cached = g_plan_mats[data * 16 + parity];
        if (cached.empty() && !rs_build_matrix(data, parity, cached))
            return fail(nullptr, DM_ERR_INVALID, "singular Vandermonde top");
        mat = cached;
    }
    RsPlan p;
    RC_TRY(plan_status(nullptr, restore_plan(mat.data(), data, parity, present, in_place, p), data));
    std::memcpy(inputs, p.inputs, sizeof(int) * (size_t)data);
    std::memcpy(outputs, p.outputs, sizeof(int) * (size_t)p.nout);
    std::memcpy(rows, p.rows, (size_t)p.nout * (size_t)data);
    *nout = p.nout;
    return DM_OK;
}

int dm_rs_restore_device_async(dm_rs* r, const void* const* dev_frags, uint64_t nseg, uint64_t segment, void* dev_obj,
                               void* stream) {
    if (!r) return bad_arg();
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    RC_TRY(rs_narrow(r, "dm_rs_restore_device_async"));
    const int k = r->k, total = r->k + r->m;
    if (!dev_frags || !dev_obj || nseg == 0 || segment == 0 || segment % (16ull * (uint64_t)k) || !is_aligned16(dev_obj))
        return fail(c, DM_ERR_INVALID,
                    "dm_rs_restore_device_async: need a 16-byte aligned object and a segment size that is a "
                    "non-zero multiple of 16 x %d data shards", k);
    for (uint64_t i = 0; i < nseg * (uint64_t)total; i++)
        if (!is_aligned16(dev_frags[i]))
            return fail(c, DM_ERR_INVALID, "dm_rs_restore_device_async: fragment %llu of segment %llu not 16-byte aligned",
                        (unsigned long long)(i % total), (unsigned long long)(i / total));
    const uint64_t frag = segment / (uint64_t)k;
    RestoreBatch b{r->mat.data(), k, r->m};   // every plan first: a segment with too few fragments fails the call before any launch
    b.desc.reserve(nseg);
    for (uint64_t t = 0; t < nseg; t++)
        RC_TRY(plan_status(c, restore_add(b, reinterpret_cast<const uint8_t* const*>(dev_frags) + t * total,
                                          static_cast<uint8_t*>(dev_obj) + t * segment, frag), k));
    Dev& d = c->devs[g];
    hipStream_t s = pick_stream(d, stream);
    RC_TRY(begin_call(c, d, s));
    return rs_desc_launch(r, d, s, b, frag / 16);
}

int dm_restore_buffer(dm_rs* r, const void* const* frags, const uint8_t* frag_names, const uint8_t* seg_names,
                      const uint8_t* fid, uint64_t nseg, uint64_t size, uint64_t segment, int flags, void* out,
                      uint8_t* frag_status, uint8_t* seg_status, int* ok) {
    return restore_buffer_call(r, "dm_restore_buffer", frags, frag_names, seg_names, fid, nseg, size, segment, flags,
                               nullptr, nullptr, 0, out, frag_status, seg_status, ok);
}

int dm_restore_cipher_buffer(dm_rs* r, const void* const* frags, const uint8_t* frag_names, const uint8_t* seg_names,
                             const uint8_t* fid, uint64_t nseg, uint64_t size, uint64_t segment, int flags,
                             const void* cipher, uint64_t cipher_len, void* out, uint8_t* frag_status,
                             uint8_t* seg_status, int* ok) {
    CipherKey key;
    return restore_buffer_call(r, "dm_restore_cipher_buffer", frags, frag_names, seg_names, fid, nseg, size, segment,
                               flags, &key, cipher, cipher_len, out, frag_status, seg_status, ok);
}

int dm_restore_batch(dm_rs* r, const dm_restore_obj* objs, uint64_t nobj, uint64_t segment, int* ok) {
    if (!r) return bad_arg();
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    RC_TRY(rs_narrow(r, "dm_restore_batch"));
    if (nobj == 0) return DM_OK;
    if (!objs || !ok) return fail(c, DM_ERR_INVALID, "dm_restore_batch: null argument");
    if (const dm_restore_plan::Error e = dm_restore_plan::check(rb_objs(objs, nobj).data(), nobj, segment, r->k))
        return rb_fail(c, e);
    return restore_batch_run(r, c->devs[g], objs, nobj, segment, ok);
}

int dm_retrieve_file(dm_rs* r, const char* fragdir, const uint8_t* frag_names, const uint8_t* seg_names,
                     const uint8_t* fid, uint64_t nseg, uint64_t size, uint64_t segment, int flags, const char* out_path,
                     uint8_t* frag_status, uint8_t* seg_status, int* ok) {
    if (!r || !ok) return bad_arg();
    *ok = 0;
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    RC_TRY(rs_narrow(r, "dm_retrieve_file"));
    if (!fragdir || !frag_names || !out_path) return fail(c, DM_ERR_INVALID, "dm_retrieve_file: null argument");
    RC_TRY(restore_check(r, nseg, size, segment));
    std::string dir = fragdir;
    while (dir.size() > 1 && dir.back() == '/') dir.pop_back();
    const std::string outp = out_path;
    const size_t slash = outp.rfind('/');
    const std::string tmp = (slash == std::string::npos ? std::string() : outp.substr(0, slash + 1)) + ".dm-rt-" +
                            std::to_string((long long)::getpid()) + "-" +
                            std::to_string((unsigned long long)g_rt_seq++);
    FdGuard fd;
    fd.fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (fd.fd < 0) return fail(c, DM_ERR_IO, "open %s: %s", outp.c_str(), go_errno(errno).c_str());   // as os.Create(out_path)
    Dev& d = c->devs[g];
    RtStatus st(r, nseg);
    int rc = retrieve_windows(r, d, dir, frag_names, seg_names, fid, nseg, size, segment, flags, fd.fd, tmp,
                              st.fst.data(), st.sst.data(), ok);
    if (rc != DM_OK) {   // a failed call may leave copies queued: none may land in a slot the next call fills
        (void)hipStreamSynchronize(d.copy);
        (void)hipStreamSynchronize(d.stream);
    }
    if (d.data.cap > kFpKeepBytes) c->reaper.put(d.id, d.data);
    if (rs_ln(r, d).work.cap > kFpKeepBytes) c->reaper.put(d.id, rs_ln(r, d).work);
    if (rc == DM_OK && *ok) {
        if (::close(fd.fd) != 0) rc = fail(c, DM_ERR_IO, "close %s: %s", tmp.c_str(), go_errno(errno).c_str());
        fd.fd = -1;
        if (rc == DM_OK && ::rename(tmp.c_str(), outp.c_str()) != 0)
            rc = fail(c, DM_ERR_IO, "rename %s %s: %s", tmp.c_str(), outp.c_str(), go_errno(errno).c_str());
        if (rc != DM_OK) *ok = 0;
    }
    if (rc != DM_OK || !*ok) ::unlink(tmp.c_str());   // no temporary survives a failed call
    st.copy_out(frag_status, seg_status);
    return rc;
}

}  // extern "C"
