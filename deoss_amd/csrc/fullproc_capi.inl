// fullproc_capi.inl -- dm_full_processing: cess-go-sdk process.FullProcessing(file, "", savedir)
// (go.mod:8; called at node/objectHandler.go:168, node/fileHandler.go:771,
// node/filesHandler.go:201, node/resumeHandler.go:326, node/tracker.go:767-769) from the file path,
// in one call.  Part of merkle_capi.hip (after files_capi.inl, rs_capi.inl, process_capi.inl).
//
// Per window of segments (up to kFpWindowBytes of file; one window up to 32 GiB):
//   A. the file is pread into pinned slots (whole segments per slot, parallel readers) and each
//      slot is copied to HBM -- nothing else, so the leaf chains can start as soon as the reads
//      allow (the last segment's zero padding is filled in the slot);
//   B. one RS launch and one leaf launch over the window's segments and fragments
//      (process_segments, the same GPU pass as dm_process_buffer);
//   C. while the leaf kernel's serial chains run (~0.5 s for 32 MiB segments), the data fragments
//      and segment files -- plain file bytes -- are copied from the file by background writers
//      (copy_file_range, page cache to page cache), and the parity fragments come back through
//      the slots and are written to temporary files;
//   D. the digests come back and every temporary file is renamed to savedir/<hex SHA-256>.
// The fid is the hashtree root over all segment digests.  The Go shim's window path (read a
// window, one batched GPU call, then write its fragments) leaves the GPU idle during the writes
// and the writes idle during the hashing; here they overlap.
//
// dm_full_processing_cipher: the same with a cipher (cipher_scheme.hpp), through the same windows.
// A segment is then the AES-CBC ciphertext of a P = segment - 16 byte piece of the file: the pieces
// are read at the segment pitch and encrypted in place -- as whole chains, or with
// DEOSS_FP_STRIPES=1 per stripe in the striped pass (the range kernel, with the SHA-256 chains one
// stripe behind) -- and the data fragments and segment files, ciphertext, come back from HBM
// through the slots as the parity does.

namespace {

constexpr uint64_t kFpSlotBytes = 64ull << 20;         // pinned slot (whole segments / parity sets)
constexpr int kFpSlots = 4;                             // = dm_rs::fp_slot
constexpr size_t kFpDataWriters = 8;                    // jobs copying data fragments / segments from the file
constexpr int kFpReaders = 8;                           // pread threads per slot (phase A gates the leaf pass)

constexpr uint64_t kFpWindowBytes = 32ull << 30;        // file bytes per GPU pass (+ 2x parity in HBM)
constexpr uint64_t kFpStripeMinSegs = 4;                // windows of at least this many segments read in stripes

// DEOSS_FP_TRACE=1: phase times of each dm_full_processing window on stderr (diagnostics)
struct FpTrace {
    bool on = std::getenv("DEOSS_FP_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void mark(const char* what) const {
        if (on)
            std::fprintf(stderr, "[fp] %-28s %8.1f ms\n", what,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};

constexpr uint64_t kFpKeepBytes = 4ull << 30;   // window scratch kept between dm_full_processing calls

struct FpEvents {
    hipEvent_t slot[kFpSlots] = {}, enc[kFpSlots] = {}, rs = nullptr, copied = nullptr;
    ~FpEvents() {
        for (hipEvent_t e : slot)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : enc)
            if (e) (void)hipEventDestroy(e);
        if (rs) (void)hipEventDestroy(rs);
        if (copied) (void)hipEventDestroy(copied);
    }
};

// Striped pass over one window of ns segments (file bytes [fbeg, fend)): for every stripe [o, o + w)
// of the segment (stripe_schedule, split at fragment boundaries) the window's ns pieces are pread
// into one pinned slot, copied to HBM with one 2D copy (segment pitch), and two resumable leaf
// launches absorb them: the ns segment chains (kit->comp[0]) and the ns chains of the data fragment
// the stripe lies in (kit->comp[1]).  After the last stripe: RS over the window and one leaf launch
// over the parity fragments (on s), then the fid over the segment digests.  d.leaves: the striped
// order (FpLayout::striped_frag_slot).
// With a cipher (key) the window's pieces are fbeg + t * (seg - 16) of the file and a stripe brings
// their plaintext [o, min(o + w, seg - 16)) (dm_cipher::stripe_span); after the stripe's copy one
// range-encrypt launch on s -- idle until RS, which so follows the last encrypt -- makes it
// ciphertext in place, and the two leaf launches wait for that instead of the copy.
template <class TakeSlot>
int fp_striped_pass(dm_rs* r, Dev& d, hipStream_t s, StreamKit* kit, const FileSet& fs, uint64_t fbeg, uint64_t fend,
                    uint64_t ns, const FpLayout& L, uint64_t slot_cap, int readers, TakeSlot& take_slot,
                    bool (&busy)[kFpSlots], FpEvents& ev, uint8_t* parity, uint8_t* dfid, FpTrace& tr,
                    const CipherKey* key) {
    dm_ctx* c = r->c;
    const int k = L.k, m = L.m;
    const uint64_t seg = L.seg, frag = L.frag;
    const uint64_t pitch = key ? seg - dm_cipher::kBlock : seg;   // file bytes per segment
    const uint64_t W = fp_stripe_pitch(slot_cap, ns);             // slot row pitch
    std::vector<uint64_t> so, sw;
    fp_stripe_plan(L, W, so, sw);   // no stripe crosses a fragment boundary
    const uint64_t nsteps = so.size();
    uint32_t* seg_state = reinterpret_cast<uint32_t*>(dfid + 256);
    uint32_t* frag_state = seg_state + 8 * ns;
    // tables: row j = the ns segment pointers at stripe j's offset; lens = ns segments, ns fragments;
    // the parity launch: ns x m fragment pointers and lengths
    std::vector<uint64_t> addr(nsteps * ns), lens(2 * ns, seg), paddr(ns * m), plen(ns * m, frag);
    for (uint64_t t = 0; t < ns; t++) lens[ns + t] = frag;
    for (uint64_t j = 0; j < nsteps; j++)
        for (uint64_t t = 0; t < ns; t++) addr[j * ns + t] = reinterpret_cast<uint64_t>(d.data.u8() + t * seg + so[j]);
    for (uint64_t i = 0; i < ns * m; i++) paddr[i] = reinterpret_cast<uint64_t>(parity + i * frag);
    RC_TRY(tables_begin(c, d, (addr.size() + lens.size() + 2 * ns * m) * 8 + 4096));
    HIP_TRY(d.leaves.ensure(32 * L.leaves(ns)));
    RC_TRY(upload(c, d, s, d.tab_addr, addr.data(), addr.size() * 8));
    RC_TRY(upload(c, d, s, d.tab_len, lens.data(), lens.size() * 8));
    RC_TRY(upload(c, d, s, d.tab_first, paddr.data(), paddr.size() * 8));
    RC_TRY(upload(c, d, s, d.tab_ids, plen.data(), plen.size() * 8));
    HIP_TRY(hipEventRecord(ev.copied, s));   // the tables are on the device before any launch
    for (hipStream_t x : {kit->comp[0], kit->comp[1]}) HIP_TRY(hipStreamWaitEvent(x, ev.copied, 0));
    const int kind = pick_leaf_kernel(c, d, ns);
    for (uint64_t j = 0; j < nsteps; j++) {
        const uint64_t o = so[j], w = sw[j], q = o / frag;
        int sl;
        RC_TRY(take_slot(&sl));
        uint8_t* buf = rs_ln(r, d).fp_slot[sl].u8();
        const dm_cipher::StripeSpan sp = key ? dm_cipher::stripe_span(o, w, seg) : dm_cipher::StripeSpan{o, w, false};
        std::vector<FilePart> parts;
        for (uint64_t t = 0; t < ns; t++) {
            const uint64_t a = fbeg + t * pitch + o;
            const uint64_t have = a < fend ? std::min(sp.len, fend - a) : 0;
            if (have) parts.push_back({0, a, have, buf + t * W});
            if (have < sp.len) std::memset(buf + t * W + have, 0, sp.len - have);   // the last segment's zero padding
        }
        RC_TRY(read_parts(c, fs, parts, readers));
        HIP_TRY(hipMemcpy2DAsync(d.data.u8() + o, seg, buf, W, sp.len, ns, hipMemcpyHostToDevice, d.copy));
        HIP_TRY(hipEventRecord(ev.slot[sl], d.copy));
        busy[sl] = true;
        hipEvent_t landed = ev.slot[sl];   // what the stripe's chains wait for
        if (key) {
            HIP_TRY(hipStreamWaitEvent(s, ev.slot[sl], 0));
            HIP_TRY(launch_aes_encrypt_range(s, *key, d.data.u8(), seg, pitch, ns, sp.blk_lo(), sp.blk_hi()));
            HIP_TRY(hipEventRecord(ev.enc[sl], s));
            landed = ev.enc[sl];
        }
        dm::LeafArgs la{};
        la.addrs = static_cast<const uint64_t*>(d.tab_addr.p) + j * ns;
        la.nleaves = ns;
        la.byte_off = o;
        la.byte_end = o + w;
        la.state = seg_state;
        la.lens = static_cast<const uint64_t*>(d.tab_len.p);
        la.digests = d.leaves.u8();
        HIP_TRY(hipStreamWaitEvent(kit->comp[0], landed, 0));
        RC_TRY(launch_leaves(c, d, kit->comp[0], la, true, true, kind));
        la.byte_off = o - q * frag;
        la.byte_end = la.byte_off + w;
        la.state = frag_state;   // re-initialised where each fragment starts (byte_off 0)
        la.lens = static_cast<const uint64_t*>(d.tab_len.p) + ns;
        la.digests = d.leaves.u8() + 32 * L.striped_frag_slot(ns, 0, (int)q);
        HIP_TRY(hipStreamWaitEvent(kit->comp[1], landed, 0));
        RC_TRY(launch_leaves(c, d, kit->comp[1], la, true, true, kind));
    }
    tr.mark("A': stripes read, launched");
    // RS after the last copy, then the parity fragments' chains (8 MiB: shorter than the segments')
    HIP_TRY(hipEventRecord(ev.copied, d.copy));
    HIP_TRY(hipStreamWaitEvent(s, ev.copied, 0));
    HIP_TRY(launch_rs(d, s, k, rs_encode_args(r, d.data.u8(), seg, parity, L.pbytes, frag, ns)));
    HIP_TRY(hipEventRecord(ev.rs, s));
    const dm::LeafArgs pa =
        table_args(d.tab_first.p, d.tab_ids.p, ns * m, d.leaves.u8() + 32 * L.striped_frag_slot(ns, 0, k));
    RC_TRY(launch_leaves(c, d, s, pa, true, true, pick_leaf_kernel(c, d, ns * m)));
    // the fid once the segment chains are done
    HIP_TRY(hipEventRecord(kit->ev[0], kit->comp[0]));
    HIP_TRY(hipEventRecord(kit->ev[1], kit->comp[1]));
    HIP_TRY(hipStreamWaitEvent(s, kit->ev[0], 0));
    HIP_TRY(hipStreamWaitEvent(s, kit->ev[1], 0));
    RC_TRY(finish(c, d, s, d.leaves.u8(), ns, true, dfid));
    return DM_OK;
}

// Everything but the renames; `out` collects every file written under its temporary name.
// key: null, or the cipher (cipher_scheme.hpp) -- segment t of the object is then the ciphertext of
// the file's piece t, so every file written comes back from HBM, none from the file.
int full_processing_windows(dm_rs* r, Dev& d, const FileSet& fs, FpOutputs& out, uint64_t seg, int flags,
                            std::vector<uint8_t>& segd, std::vector<uint8_t>& fragd, uint8_t fid[32],
                            const CipherKey* key) {
    dm_ctx* c = r->c;
    const int g = (int)(&d - c->devs.data());   // the call's lane
    RsLane& L = rs_ln(r, d);
    hipStream_t s = d.stream;
    const FpLayout lay(r->k, r->m, seg);
    const int total = lay.total;
    const uint64_t frag = lay.frag, pbytes = lay.pbytes;   // parity bytes per segment
    const uint64_t pitch = key ? seg - dm_cipher::kBlock : seg;   // file bytes per segment
    const uint64_t size = fs.size[0], nseg = ceil_div(size, pitch);
    // test hooks (env, read per call): smaller slots / windows exercise slot reuse and multi-window fids
    const uint64_t window_bytes = env_bytes("DEOSS_FP_WINDOW_BYTES", kFpWindowBytes);
    const FpSlots slots = fp_slots(lay, env_bytes("DEOSS_FP_SLOT_BYTES", kFpSlotBytes));
    const uint64_t spd = slots.spd, spp = slots.spp, slot_cap = slots.cap;
    const uint64_t win = std::max<uint64_t>(spd, window_bytes / seg / spd * spd);   // segments per window
    const int readers = (int)std::min<uint64_t>(64, env_bytes("DEOSS_FP_READERS", kFpReaders));
    RC_TRY(begin_call(c, d, s));
    for (auto& b : L.fp_slot) HIP_TRY(b.ensure(slot_cap));
    FpEvents ev;
    for (auto& e : ev.slot) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : ev.enc) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ev.rs, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ev.copied, hipEventDisableTiming));
    // where data files are copied from: the open file (kernel copies) or, for a pipe, its bytes
    const uint8_t* mem = fs.mem[0].empty() ? nullptr : fs.mem[0].data();
    int in_fd = fs.fd[0];
    FdGuard own_fd;
    if (!key && !mem && in_fd < 0) {
        in_fd = own_fd.fd = ::open(fs.path[0].c_str(), O_RDONLY | O_CLOEXEC);
        if (in_fd < 0) return fail(c, DM_ERR_IO, "open %s: %s", fs.path[0].c_str(), go_errno(errno).c_str());
    }
    std::vector<uint8_t> tail;      // the zero-padded last segment (its data files are written from here)
    uint64_t tail_seg = ~0ull;
    SlotWrites wd;                  // data-fragment / segment-file writers (declared after their sources)
    SlotWrites wr[kFpSlots];
    bool busy[kFpSlots] = {false, false, false, false};
    uint64_t next = 0;   // slot round robin across both phases and windows
    auto take_slot = [&](int* out) -> int {
        const int sl = (int)(next++ % kFpSlots);
        if (busy[sl]) {
            HIP_TRY(hipEventSynchronize(ev.slot[sl]));
            const std::string e = wr[sl].wait();
            if (!e.empty()) return fail(c, DM_ERR_IO, "%s", e.c_str());
            busy[sl] = false;
        }
        *out = sl;
        return DM_OK;
    };
    // The window's data fragments and segment files -- plain file bytes -- are copied from the
    // file itself by background jobs (copy_file_range: page cache to page cache); the zero-padded
    // last segment's from `tail`.
    auto start_data_files = [&](uint64_t w0, uint64_t ns) {
        std::vector<FpFile> files;
        for (uint64_t gs = w0; gs < w0 + ns; gs++) {
            const uint8_t* src = gs == tail_seg ? tail.data() : mem ? mem + gs * seg : nullptr;
            out.data_files(lay, gs, src, in_fd, gs * seg, (flags & DM_FP_SEGMENT_FILES) != 0, files);
        }
        wd.start(std::move(files), (size_t)env_bytes("DEOSS_FP_DATA_WRITERS", kFpDataWriters));
    };
    const bool one_window = nseg <= win;
    const char* stripes_env = std::getenv("DEOSS_FP_STRIPES");
    const bool stripes_off = stripes_env != nullptr && stripes_env[0] == '0';
    // with a cipher the default is the other way round: at 257 x 32 MiB the striped pass measured
    // slower than encrypt-then-hash, so it runs only when DEOSS_FP_STRIPES asks for it
    const bool stripes_want = key ? stripes_env != nullptr && !stripes_off : !stripes_off;
    // two extra compute streams for the striped pass (segment and data-fragment chains side by side)
    StreamKit* kit = nullptr;
    RC_TRY(kit_acquire(c, g, &kit));
    struct KitBack {
        dm_ctx* c;
        int g;
        StreamKit* k;
        ~KitBack() {
            for (hipStream_t x : {k->comp[0], k->comp[1]}) (void)hipStreamSynchronize(x);
            kit_release(c, g, k);
        }
    } kit_back{c, g, kit};
    FpTrace tr;
    for (uint64_t w0 = 0; w0 < nseg; w0 += win) {
        const uint64_t ns = std::min(win, nseg - w0);
        const uint64_t fbeg = w0 * pitch, fend = std::min(size, (w0 + ns) * pitch);
        // striped (round 3): the window is read in stripes [o, o + w) of EVERY segment, so the segment
        // and data-fragment chains start with the first stripe instead of after the whole window
        // (the reads of an 8 GiB file took 236 ms before any chain started); needs whole 64-B blocks
        // per fragment.  DEOSS_FP_STRIPES=0 keeps the read-then-launch order (A/B); with a cipher
        // that order is the default and DEOSS_FP_STRIPES=1 asks for the stripes.
        const bool striped = ns >= kFpStripeMinSegs && frag % 64 == 0 && stripes_want;
        HIP_TRY(d.data.ensure(ns * seg + kAlign));
        HIP_TRY(L.work.ensure(ns * pbytes + 256 + 2 * ns * 32));
        uint8_t* parity = L.work.u8();
        uint8_t* dfid = parity + ns * pbytes;
        if (!striped) {
            // A: file -> slots -> HBM, nothing else, so the leaf chains start as early as the reads allow
            for (uint64_t t0 = 0; t0 < ns; t0 += spd) {
                const uint64_t nt = std::min(spd, ns - t0), len = nt * pitch, a = fbeg + t0 * pitch;
                int sl;
                RC_TRY(take_slot(&sl));
                uint8_t* buf = L.fp_slot[sl].u8();
                const uint64_t have = a < fend ? std::min(len, fend - a) : 0;
                std::vector<FilePart> parts;
                for (uint64_t q = 0; q < have; q += 8ull << 20)
                    parts.push_back({0, a + q, std::min<uint64_t>(8ull << 20, have - q), buf + q});
                RC_TRY(read_parts(c, fs, parts, readers));
                if (have < len) std::memset(buf + have, 0, len - have);
                if (key)   // pieces at the segment pitch; the encrypt kernel appends each one's padding block
                    HIP_TRY(hipMemcpy2DAsync(d.data.u8() + t0 * seg, seg, buf, pitch, pitch, nt, hipMemcpyHostToDevice,
                                             d.copy));
                else
                    HIP_TRY(hipMemcpyAsync(d.data.u8() + t0 * seg, buf, len, hipMemcpyHostToDevice, d.copy));
                HIP_TRY(hipEventRecord(ev.slot[sl], d.copy));
                busy[sl] = true;
                if (!key && t0 + nt == ns && have < len) {   // the file's last, zero-padded segment: keep a copy
                    tail.assign(buf + (nt - 1) * seg, buf + nt * seg);
                    tail_seg = w0 + t0 + nt - 1;
                }
            }
            tr.mark("A: reads + H2D enqueued");
            // B: RS + one leaf launch over segments and fragments, after the last H2D
            HIP_TRY(hipEventRecord(ev.copied, d.copy));
            HIP_TRY(hipStreamWaitEvent(s, ev.copied, 0));
            if (key) HIP_TRY(launch_aes_encrypt(s, *key, d.data.u8(), seg, pitch, ns));
            RC_TRY(process_segments(r, d, s, d.data.u8(), seg, parity, {0, ns}, dfid, ev.rs));
        } else {
            if (!key && fend - fbeg < ns * seg) {   // the file's last, zero-padded segment, for its data files
                tail.assign(seg, 0);
                const uint64_t a = fbeg + (ns - 1) * seg;
                RC_TRY(read_parts(c, fs, {{0, a, fend - a, tail.data()}}, readers));
                tail_seg = w0 + ns - 1;
            }
            // the data files need only the file: their copies run from the start, beside the reads
            if (!key) start_data_files(w0, ns);
            RC_TRY(fp_striped_pass(r, d, s, kit, fs, fbeg, fend, ns, lay, slot_cap, readers, take_slot, busy, ev,
                                   parity, dfid, tr, key));
        }
        // C: while the leaf chains run, the parity comes back through the slots and is written as
        // each set lands (the data fragments and segment files are already being copied)
        if (!striped && !key) start_data_files(w0, ns);
        HIP_TRY(hipStreamWaitEvent(d.copy, ev.rs, 0));
        tr.mark("B: launched, data copies started");
        // with a cipher the data fragments and segment files are ciphertext: they come back as the
        // parity does, whole segments per slot, once RS -- which follows the last encrypt -- has run
        for (uint64_t t0 = 0; key && t0 < ns; t0 += spd) {
            const uint64_t nt = std::min(spd, ns - t0);
            int sl;
            RC_TRY(take_slot(&sl));
            uint8_t* buf = L.fp_slot[sl].u8();
            HIP_TRY(hipMemcpyAsync(buf, d.data.u8() + t0 * seg, nt * seg, hipMemcpyDeviceToHost, d.copy));
            HIP_TRY(hipEventRecord(ev.slot[sl], d.copy));
            HIP_TRY(hipEventSynchronize(ev.slot[sl]));
            std::vector<FpFile> files;
            for (uint64_t u = 0; u < nt; u++)
                out.data_files(lay, w0 + t0 + u, buf + u * seg, -1, 0, (flags & DM_FP_SEGMENT_FILES) != 0, files);
            wr[sl].start(std::move(files));
            busy[sl] = true;
        }
        for (uint64_t t0 = 0; t0 < ns; t0 += spp) {
            const uint64_t nt = std::min(spp, ns - t0);
            int sl;
            RC_TRY(take_slot(&sl));
            uint8_t* buf = L.fp_slot[sl].u8();
            HIP_TRY(hipMemcpyAsync(buf, parity + t0 * pbytes, nt * pbytes, hipMemcpyDeviceToHost, d.copy));
            HIP_TRY(hipEventRecord(ev.slot[sl], d.copy));
            HIP_TRY(hipEventSynchronize(ev.slot[sl]));
            wr[sl].start(out.parity_files(lay, w0 + t0, nt, buf));
            busy[sl] = true;
        }
        tr.mark("C: parity back, writes queued");
        // D: digests.  One pass: d.leaves holds the segments, then the fragments (FpLayout::seg_slot,
        // frag_slot), as segd / fragd do; the striped order is brought into that one here
        std::vector<uint8_t> lv;
        if (striped) {
            lv.resize(32 * lay.leaves(ns));
            HIP_TRY(hipMemcpyAsync(lv.data(), d.leaves.p, lv.size(), hipMemcpyDeviceToHost, s));
        } else {
            HIP_TRY(hipMemcpyAsync(segd.data() + 32 * w0, d.leaves.p, 32 * ns, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(fragd.data() + 32 * w0 * total, d.leaves.u8() + 32 * ns, 32 * ns * total,
                                   hipMemcpyDeviceToHost, s));
        }
        if (one_window) HIP_TRY(hipMemcpyAsync(fid, dfid, 32, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (striped) lay.striped_to_one_pass(ns, lv.data(), segd.data() + 32 * w0, fragd.data() + 32 * w0 * total);
        HIP_TRY(hipStreamSynchronize(d.copy));   // this window's slots are in host memory: HBM reusable
        tr.mark("D: leaf pass done");
        const std::string e = wd.wait();
        tr.mark("data files written");   // the window's data files, before the next window reuses `tail`
        if (!e.empty()) return fail(c, DM_ERR_IO, "%s", e.c_str());
    }
    for (int sl = 0; sl < kFpSlots; sl++) {
        const std::string e = wr[sl].wait();
        if (!e.empty()) return fail(c, DM_ERR_IO, "%s", e.c_str());
    }
    tr.mark("parity files written");
    // several windows: the fid is the tree over every segment digest
    if (!one_window) RC_TRY(rt_fid(c, d, s, segd.data(), nseg, fid));
    return DM_OK;
}

// dm_full_processing (cipher_len == 0) and dm_full_processing_cipher.
int full_processing_call(dm_rs* r, const char* path, const char* savedir, uint64_t segment, const void* cipher,
                         uint64_t cipher_len, int flags, uint8_t* seg_hashes, uint8_t* frag_hashes, uint64_t cap,
                         uint64_t* nseg_out, uint8_t fid[32]) {
    if (!r || !path || !savedir || !fid) return bad_arg();
    dm_ctx* c = r->c;
    const int g = rs_lane(c);
    CallLock lk(c, g, kReserved);
    if (nseg_out) *nseg_out = 0;
    RC_TRY(rs_narrow(r, cipher_len ? "dm_full_processing_cipher" : "dm_full_processing"));
    CipherKey ck;
    const CipherKey* key = nullptr;
    if (cipher_len) {
        RC_TRY(cipher_key(c, cipher, cipher_len, ck));
        key = &ck;
    }
    FileSet fs;
    RC_TRY(open_files(c, &path, 1, fs));   // "open <path>: ..." first, as os.Open would fail
    const uint64_t size = fs.size[0];
    if (size == 0) return fail(c, DM_ERR_EMPTY, "Empty data");
    RC_TRY(process_check(r, size, segment));
    if (key && !dm_cipher::segment_ok(segment))
        return fail(c, DM_ERR_INVALID, "segment size %llu has no room for a block and its padding block",
                    (unsigned long long)segment);
    const uint64_t nseg = key ? dm_cipher::geometry(size, segment).nseg : ceil_div(size, segment);
    if (nseg_out) *nseg_out = nseg;
    if ((seg_hashes || frag_hashes) && cap < nseg)
        return fail(c, DM_ERR_INVALID, "dm_full_processing: %llu segments, digest arrays hold %llu",
                    (unsigned long long)nseg, (unsigned long long)cap);
    FpOutputs out;
    out.open(savedir, ".dm-fp-");
    const std::string me = mkdir_all(out.dir);
    if (!me.empty()) return fail(c, DM_ERR_IO, "%s", me.c_str());
    const int total = r->k + r->m;
    std::vector<uint8_t> segd(32 * nseg), fragd(32 * nseg * total);
    Dev& d = c->devs[g];
    int rc = full_processing_windows(r, d, fs, out, segment, flags, segd, fragd, fid, key);
    {
        if (rc != DM_OK) {   // a failed call may leave copies queued: none may land in a slot the next call fills
            (void)hipStreamSynchronize(d.copy);
            (void)hipStreamSynchronize(d.stream);
        }
        // the window buffers grow with the file (up to 32 GiB of segments + 64 GiB of parity): give
        // back what a large call took beyond kFpKeepBytes, so it does not stay resident beside
        // other work on this GPU; the call has synchronised its streams already
        if (d.data.cap > kFpKeepBytes) c->reaper.put(d.id, d.data);
        if (rs_ln(r, d).work.cap > kFpKeepBytes) c->reaper.put(d.id, rs_ln(r, d).work);
    }
    if (rc == DM_OK) {
        const std::string e = out.rename_all(segd.data(), fragd.data());
        if (!e.empty()) rc = fail(c, DM_ERR_IO, "%s", e.c_str());
    }
    if (rc != DM_OK) {   // no temporary survives a failed call
        out.unlink_pending();
        return rc;
    }
    if (seg_hashes) std::memcpy(seg_hashes, segd.data(), segd.size());
    if (frag_hashes) std::memcpy(frag_hashes, fragd.data(), fragd.size());
    return DM_OK;
}

}  // namespace

extern "C" {

int dm_full_processing(dm_rs* r, const char* path, const char* savedir, uint64_t segment, int flags,
                       uint8_t* seg_hashes, uint8_t* frag_hashes, uint64_t cap, uint64_t* nseg_out, uint8_t fid[32]) {
    return full_processing_call(r, path, savedir, segment, nullptr, 0, flags, seg_hashes, frag_hashes, cap, nseg_out, fid);
}

int dm_full_processing_cipher(dm_rs* r, const char* path, const char* savedir, uint64_t segment, const void* cipher,
                              uint64_t cipher_len, int flags, uint8_t* seg_hashes, uint8_t* frag_hashes, uint64_t cap,
                              uint64_t* nseg_out, uint8_t fid[32]) {
    return full_processing_call(r, path, savedir, segment, cipher, cipher_len, flags, seg_hashes, frag_hashes, cap,
                                nseg_out, fid);
}

}  // extern "C"
